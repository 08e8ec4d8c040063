// motion3.hip — MotionEstimate::motionEstimate for 8x8 and 16x16 PUs, "row team" kernel: FOUR PUs per wave.
//
// Same reference semantics and bit-exact outputs as motion.hip / motion2.hip (source/encoder/motion.cpp:739-1569 in mesearch.h).
// For small PUs a whole wave per PU wastes lanes: the team kernel of motion2.hip spends ~1200 VALU instructions per 8x8 PU
// with 4-20 useful lanes (profiles/r01_v2_pmc_sq.txt).  Here one PU is owned by one DPP ROW of 16 lanes, so a wave64
// carries four independent searches in SIMT fashion:
//   * every decision variable (bmv, bcost, dir ...) is an ordinary per-thread value, identical across the 16 lanes of a row;
//     the four rows of a wave diverge freely (the hardware exec mask handles it);
//   * a candidate costs each lane one packed quad load per 64 pixels of PU + v_sad_u8, then a 4-step `row_ror` DPP all-reduce
//     leaves the block sum in all 16 lanes — no readlane, no LDS, no barrier;
//   * lanes are tile-major (4 consecutive lanes = the 4 rows of one 4x4 tile), so the SATD's vertical Hadamard runs across
//     DPP quads (tiles.h idea) and its horizontal one in registers;
//   * every candidate, integer or sub-pel, is a block read from the pre-filtered quarter-pel planes
//     (x265hip_build_subpel_planes; plane 0 is the picture), so the serial chain contains no filtering.
#include "common.h"
#include <cstdlib>
#include "mesearch.h"
#include "filters.h"

namespace xh {

// packed 16-bit SATD helpers (s2v, Pk16) live in common.h
// dpp_all / row_allsum (16-lane DPP all-reduce) live in common.h

// sum over the team: a 16-lane row (DPP only) or the whole wave (row all-reduce + 4 readlanes; the wave is then one PU and
// its control flow is uniform)
template <int TEAM>
__device__ __forceinline__ int team_allsum(int v)
{
    if (TEAM == 8)
    {
        // eight lanes = half a DPP row: butterflies inside the quad, then the mirrored half (lane i <-> 7 - i sits in the other quad)
        v += dpp_all<0xB1>(v);          // quad_perm [1,0,3,2]
        v += dpp_all<0x4E>(v);          // quad_perm [2,3,0,1]
        v += dpp_all<0x141>(v);         // row_half_mirror
        return v;
    }
    v = row_allsum(v);
    if (TEAM == 64)
        v = __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
    return v;
}

template <typename P, int N, int TEAM, bool CHROMA = false>
struct RowTeam
{
    typedef typename Packed<P>::T Q;
    static constexpr int IPT = N * N / 4 / TEAM;       // quads per lane: 1 (8x8), 4 (16x16 on 16 lanes, 32x32 on 64), 16 (64x64 on 64)
    static constexpr int TX = N / 4;                   // tiles per row
    // Candidate blocks are addressed as (uniform base) + (32-bit unsigned byte offset): the loads then take the scalar-base form
    // (global_load v, voffset, s[base]) and the per-load 64-bit pointer arithmetic disappears.  The base is the plane pointer moved back
    // by kBias elements so that offsets of candidates above / left of the picture origin stay non-negative; nothing is read at the base.
    static constexpr uint32_t kBias = 1u << 22;
    const char* base;                                  // (const char*)(planes - kBias), the same for every lane
    uint32_t org;                                      // byte offset of phase plane 0 at the PU origin from `base`
    const char* costBase;                              // (const char*)(mvcost centre - kCostBias)
    static constexpr uint32_t kCostBias = 1u << 16;
    int64_t planeElems;
    bool smallPlane;                                   // planeElems < 2^24: the phase offset fits a 24-bit multiply
    int stride;
    const uint16_t* cost;
    Mv qmvp;
    int s;                                             // lane within the team (0..TEAM-1)
    int qoff[IPT];                                     // element offset of this lane's quads inside the PU (row * stride + col)
    Q fq[IPT];
    int fu[IPT][4];
    s2v fp[IPT][2];                                    // the same source samples as packed pairs (0,1) and (2,3)
    bool pk16;                                         // depth <= 10: packed 16-bit SATD
    // bChromaSATD (4:2:0): the chroma block is (N/2)^2 per plane = N*N/16 quads; a lane holds one quad per pass.  8x8 PUs put Cb in
    // lanes 0-3 and Cr in lanes 4-7 of one pass, 16x16 / 32x32 PUs take one pass per plane with every lane busy.
    static constexpr int CPASS = N == 8 ? 1 : 2;
    const P* cref[CPASS];                               // reference chroma plane at this lane's quad (mv (0,0))
    int strideC, depth;
    int fuc[CPASS][4];
    bool cact;                                          // lane takes part in the chroma term

    __device__ __forceinline__ uint16_t cost_at(int i) const { return *reinterpret_cast<const uint16_t*>(costBase + (size_t)(((uint32_t)i + kCostBias) * 2u)); }
    __device__ __forceinline__ int mvcost(int qx, int qy) const { return (int)(uint16_t)(cost_at(qx - qmvp.x) + cost_at(qy - qmvp.y)); }
    template <typename T> __device__ __forceinline__ T ld_off(uint32_t byteOff) const { return ld_unaligned<T>(base + (size_t)byteOff); }

    __device__ __forceinline__ uint32_t cand(Mv q) const
    {
        // full-rate 24-bit multiplies instead of v_mul_lo_u32 / v_mad_u64_u32 (quarter rate) on the candidate chain: the stride is below
        // 2^23 (checked at dispatch), the phase index is 0..15 and the plane size is below 2^24 elements up to 4K (smallPlane)
        const int ph = (q.y & 3) * 4 + (q.x & 3);
        const uint32_t po = smallPlane ? (uint32_t)__umul24(ph, (int)planeElems) : (uint32_t)ph * (uint32_t)planeElems;
        return org + (po + (uint32_t)(__mul24(q.y >> 2, stride) + (q.x >> 2))) * (uint32_t)sizeof(P);
    }
    // subpelCompare(..., sad) (motion.cpp:1571) / sad() of the block at quarter-pel vector q, WITHOUT mv cost
    __device__ __forceinline__ int sad_q(Mv q) const
    {
        const uint32_t r = cand(q);
        unsigned acc = 0;
#pragma unroll
        for (int j = 0; j < IPT; j++)
            acc = Packed<P>::sad(ld_off<Q>(r + (uint32_t)qoff[j]), fq[j], acc);
        return team_allsum<TEAM>((int)acc);
    }
    // subpelCompare(..., satd): 4x4 Hadamard tiles, rows of a tile in the 4 lanes of a DPP quad
    __device__ __forceinline__ int satd_q(Mv q) const
    {
        const uint32_t r = cand(q);
        const bool hi1 = s & 1, hi2 = s & 2;
        int acc = 0;
        if (sizeof(P) == 1 || pk16)                  // 8-bit: always (the 32-bit path below is not even compiled in)
        {
            const s2v one = { 1, 1 }, kh = { 1, -1 };
            const s2v k1 = hi1 ? -one : one, k2 = hi2 ? -one : one;
#pragma unroll
            for (int j = 0; j < IPT; j++)
            {
                s2v p01, p23;
                Pk16<P>::split(ld_off<Q>(r + (uint32_t)qoff[j]), p01, p23);
                const s2v d01 = fp[j][0] - p01, d23 = fp[j][1] - p23;
                const s2v A = d01 + d23, B = d01 - d23;                          // (d0+d2, d1+d3), (d0-d2, d1-d3)
                const s2v Ar = as_s2(__builtin_amdgcn_alignbit(as_u(A), as_u(A), 16)), Br = as_s2(__builtin_amdgcn_alignbit(as_u(B), as_u(B), 16));
                s2v m01 = Ar * kh + A, m23 = Br * kh + B;                        // (h0, -h1), (h2, -h3): signs do not matter below
                s2v pr = as_s2((uint32_t)__builtin_amdgcn_mov_dpp((int)as_u(m01), 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
                m01 = m01 * k1 + pr;
                pr = as_s2((uint32_t)__builtin_amdgcn_mov_dpp((int)as_u(m23), 0xB1, 0xF, 0xF, true));
                m23 = m23 * k1 + pr;
                pr = as_s2((uint32_t)__builtin_amdgcn_mov_dpp((int)as_u(m01), 0x4E, 0xF, 0xF, true));         // quad_perm [2,3,0,1]
                m01 = m01 * k2 + pr;
                pr = as_s2((uint32_t)__builtin_amdgcn_mov_dpp((int)as_u(m23), 0x4E, 0xF, 0xF, true));
                m23 = m23 * k2 + pr;
                acc = __builtin_amdgcn_sdot2(__builtin_elementwise_max(m01, -m01), one, acc, false);
                acc = __builtin_amdgcn_sdot2(__builtin_elementwise_max(m23, -m23), one, acc, false);
            }
            return team_allsum<TEAM>(acc) >> 1;
        }
#pragma unroll
        for (int j = 0; j < IPT; j++)
        {
            int p[4];
            Packed<P>::unpack(ld_off<Q>(r + (uint32_t)qoff[j]), p);
            const int d0 = fu[j][0] - p[0], d1 = fu[j][1] - p[1], d2 = fu[j][2] - p[2], d3 = fu[j][3] - p[3];
            const int s01 = d0 + d1, e01 = d0 - d1, s23 = d2 + d3, e23 = d2 - d3;
            int m[4] = { s01 + s23, s01 - s23, e01 + e23, e01 - e23 };
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                const int pr = __builtin_amdgcn_mov_dpp(m[i], 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
                m[i] = hi1 ? pr - m[i] : m[i] + pr;
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                const int pr = __builtin_amdgcn_mov_dpp(m[i], 0x4E, 0xF, 0xF, true);       // quad_perm [2,3,0,1]
                m[i] = hi2 ? pr - m[i] : m[i] + pr;
            }
            acc += iabs(m[0]) + iabs(m[1]) + iabs(m[2]) + iabs(m[3]);
        }
        // every tile's |H D H^T| sum is even (pixel.hip), so one >> 1 over the block equals the per-tile >> 1 of pixel.cpp:235
        return team_allsum<TEAM>(acc) >> 1;
    }
    // SATD of the Cb and Cr blocks predicted at quarter-pel luma vector q (= eighth-pel chroma), the chroma part of subpelCompare
    __device__ __forceinline__ int chroma_term(Mv q) const
    {
        const bool hi1 = s & 1, hi2 = s & 2;
        int acc = 0;
#pragma unroll
        for (int ps = 0; ps < CPASS; ps++)
        {
            int p[4];
            chroma_quad_hv(cref[ps], strideC, q.x, q.y, depth, p);
            const int d[4] = { fuc[ps][0] - p[0], fuc[ps][1] - p[1], fuc[ps][2] - p[2], fuc[ps][3] - p[3] };
            const int a = quad_row_hadamard_abs(d, hi1, hi2);
            acc += cact ? a : 0;
        }
        return team_allsum<TEAM>(acc) >> 1;                 // every 4x4 tile sum is even: one shift equals the per-tile >> 1 of satd_4x4
    }
    // MotionEstimate::subpelCompare: luma sad / satd + (bChromaSATD) the chroma SATD term
    __device__ __forceinline__ int sub_q(Mv q, int satd) const
    {
        const int v = satd ? satd_q(q) : sad_q(q);
        return CHROMA ? v + chroma_term(q) : v;
    }

    // mestar.h contract: K full-pel points measured together (all their loads in flight before the first reduction)
    template <int K>
    __device__ __forceinline__ void fullpel_costs(const int (&mx)[K], const int (&my)[K], int (&out)[K]) const
    {
        unsigned acc[K];
        int mvc[K];
#pragma unroll
        for (int k = 0; k < K; k++)
        {
            const uint32_t r = org + (uint32_t)(__mul24(my[k], stride) + mx[k]) * (uint32_t)sizeof(P);
            acc[k] = 0;
#pragma unroll
            for (int j = 0; j < IPT; j++)
                acc[k] = Packed<P>::sad(ld_off<Q>(r + (uint32_t)qoff[j]), fq[j], acc[k]);
            mvc[k] = mvcost(mx[k] * 4, my[k] * 4);
        }
#pragma unroll
        for (int k = 0; k < K; k++)
            out[k] = team_allsum<TEAM>((int)acc[k]) + mvc[k];
    }
    __device__ __forceinline__ int fullpel_cost(int mx, int my, int shift) const
    {
        return sad_q(Mv{ mx * 4, my * 4 }) + mvcost(mx << shift, my << shift);
    }

    // mesearch.h contract: every point measured on its own
    static constexpr int kSubpelGroup = 1;
    static constexpr int kFullGroup = 1;
    static constexpr bool kSea = false;
    __device__ __forceinline__ void opening(Mv pmv, Mv fp, bool fpOk, bool zeroOk, int (&out)[3]) const
    {
        out[0] = sub_q(pmv, 0);
        if (fpOk) out[1] = fullpel_cost(fp.x, fp.y, 2);
        if (zeroOk) out[2] = fullpel_cost(0, 0, 2);
    }
    template <int K>
    __device__ __forceinline__ void pattern(const Mv (&m)[K], int (&out)[K], int n = K) const
    {
#pragma unroll
        for (int k = 0; k < K; k++)
            if (k < n) out[k] = fullpel_cost(m[k].x, m[k].y, 2);
    }
    template <int K>
    __device__ __forceinline__ void subpels(const Mv (&q)[K], const bool (&ok)[K], int cmp, int (&out)[K]) const
    {
#pragma unroll
        for (int k = 0; k < K; k++)
            if (ok[k]) out[k] = sub_q(q[k], cmp) + mvcost(q[k].x, q[k].y);
    }
};

template <typename P, int N, int TEAM, bool CHROMA>
__global__ __launch_bounds__(256) void motion3_kernel(const P* __restrict__ fencPlane, int64_t strideF, int64_t strideR,
                                                      const int32_t* __restrict__ pu_xy, const int32_t* __restrict__ mvminA,
                                                      const int32_t* __restrict__ mvmaxA, const int32_t* __restrict__ qmvpA,
                                                      int numCand, const int32_t* __restrict__ mvcA, int merange, int method, int subme,
                                                      const uint16_t* __restrict__ mvcostTab, int n,
                                                      const P* __restrict__ planes, int64_t planeElems, DeriveRange dr,
                                                      int32_t* __restrict__ outMv, int32_t* __restrict__ outCost, ChromaPlanes cp, int depth)
{
    typedef RowTeam<P, N, TEAM, CHROMA> RT;
    typedef typename RT::Q Q;
    constexpr int TPB = 256 / TEAM;                         // PUs per workgroup
    RT c;
    c.s = threadIdx.x & (TEAM - 1);
    c.stride = (int)strideR;
    c.planeElems = planeElems;
    c.smallPlane = planeElems < (1 << 24);
    c.cost = mvcostTab;
    c.pk16 = depth <= 10;
    c.costBase = reinterpret_cast<const char*>(mvcostTab) - (size_t)RT::kCostBias * 2;
    c.base = reinterpret_cast<const char*>(planes) - (size_t)RT::kBias * sizeof(P);
    // XCD-aware block order (see motion2.hip): XCD x works on the x-th contiguous eighth of the raster-ordered PU list
    const int chunk = gridDim.x >> 3;
    const int lblock = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    const int pu = lblock * TPB + threadIdx.x / TEAM;
    if (pu >= n)
        return;                                             // whole rows leave together

    const int bx = pu_xy[2 * pu], by = pu_xy[2 * pu + 1];
    Mv mvmin, mvmax, qmvp;
    pu_range(dr, pu, bx, by, merange, qmvpA, mvminA, mvmaxA, c.s == 0, qmvp, mvmin, mvmax);
    c.qmvp = qmvp;
    c.org = (RT::kBias + (uint32_t)(by * (int)strideR + bx)) * (uint32_t)sizeof(P);
    {
        const P* f = fencPlane + (int64_t)by * strideF + bx;
#pragma unroll
        for (int j = 0; j < RT::IPT; j++)
        {
            const int t = j * (TEAM / 4) + (c.s >> 2), r = c.s & 3;     // tile-major: 4 consecutive lanes = the 4 rows of tile t
            const int row = (t / RT::TX) * 4 + r, col = (t % RT::TX) * 4;
            c.qoff[j] = (row * (int)strideR + col) * (int)sizeof(P);          // bytes
            c.fq[j] = ld_unaligned<Q>(f + (int64_t)row * strideF + col);
            Packed<P>::unpack(c.fq[j], c.fu[j]);
            c.fp[j][0] = s2v{ (short)c.fu[j][0], (short)c.fu[j][1] };
            c.fp[j][1] = s2v{ (short)c.fu[j][2], (short)c.fu[j][3] };
        }
    }
    if (CHROMA)
    {
        c.strideC = (int)cp.strideRC;
        c.depth = depth;
        constexpr int TXC = N / 8;                              // 4x4 tiles per row of the chroma block
        const int t = c.s >> 2, r = c.s & 3;
        const int cbx = bx >> 1, cby = by >> 1;
#pragma unroll
        for (int ps = 0; ps < RT::CPASS; ps++)
        {
            // 8x8 PU: tile 0 = Cb, tile 1 = Cr, tiles 2-3 idle; larger PUs: pass 0 = Cb, pass 1 = Cr, tile t of the plane
            const int plane = N == 8 ? (t & 1) : ps;
            const int tt = N == 8 ? 0 : t;
            const int row = (tt / TXC) * 4 + r, col = (tt % TXC) * 4;
            const P* fc = (const P*)(plane ? cp.fencCr : cp.fencCb) + (int64_t)(cby + row) * cp.strideFC + cbx + col;
            load4(fc, c.fuc[ps]);
            c.cref[ps] = (const P*)(plane ? cp.refCr : cp.refCb) + (int64_t)(cby + row) * cp.strideRC + cbx + col;
        }
        c.cact = N == 8 ? (t < 2) : true;
    }

    const MeBest best = me_search(c, qmvp, mvmin, mvmax, numCand, mvcA + (int64_t)pu * numCand * 2, merange, method, subme, N, N);
    if (c.s == 0)
    {
        outMv[2 * pu] = best.mv.x;
        outMv[2 * pu + 1] = best.mv.y;
        outCost[pu] = best.cost;
    }
    if (dr.predOut)
    {
        // Predict::predInterLumaPixel (predict.cpp:245-266) at the winner: copy / hpp / vpp / hvpp of the block == the block of phase plane
        // (y & 3) * 4 + (x & 3) at the full-pel part of the vector; each lane moves the quads it has been comparing all along
        const uint32_t r = c.cand(best.mv);
        P* pd = (P*)dr.predOut + (int64_t)by * dr.predStride + bx;
#pragma unroll
        for (int j = 0; j < RT::IPT; j++)
        {
            const int t = j * (TEAM / 4) + (c.s >> 2), rr = c.s & 3;
            const int row = (t / RT::TX) * 4 + rr, col = (t % RT::TX) * 4;
            st_unaligned<Q>(pd + (int64_t)row * dr.predStride + col, c.template ld_off<Q>(r + (uint32_t)c.qoff[j]));
        }
    }
}

// the row-team launch for the shapes me_kernel_for gives it (8x8 / 16x16 / 32x32 with planes); cp.enable adds the chroma SATD term
int launch_motion3(int depth, int size, const void* fencPlane, int64_t strideF, int64_t strideR, const int32_t* pu_xy, const int32_t* mvmin,
                   const int32_t* mvmax, const int32_t* qmvp, int numCand, const int32_t* mvc, int merange, int method, int subme,
                   const uint16_t* mvcost, int n, const void* planes, int64_t planeElems, const DeriveRange& dr, const ChromaPlanes& cp,
                   int32_t* outMv, int32_t* outCost, hipStream_t st)
{
    // 8x8: eight PUs per wave (8-lane teams, a lane = two quads: all per-candidate control and address work is shared by twice as many PUs as
    // with 16-lane teams); 16x16: four PUs per wave; 32x32: one wave per PU
    const int tpb = size == 8 ? 32 : (size == 16 ? 16 : 4);     // (16x16 on 8-lane teams measured slower: 35 vs 28 us)
    const int blocks = (((n + tpb - 1) / tpb) + 7) & ~7;
    dim3 grid(blocks), block(256);
    const bool chroma = cp.enable != 0;
#define M3C(P, N, TEAM, CH) hipLaunchKernelGGL((motion3_kernel<P, N, TEAM, CH>), grid, block, 0, st, (const P*)fencPlane, strideF, strideR, pu_xy, mvmin, mvmax, qmvp, \
                                    numCand, mvc, merange, method, subme, mvcost, n, (const P*)planes, planeElems, dr, outMv, outCost, cp, depth)
#define M3(P, N, TEAM) do { if (chroma) M3C(P, N, TEAM, true); else M3C(P, N, TEAM, false); } while (0)
    if (depth == 8)
    {
        if (size == 8) M3(uint8_t, 8, 8);
        else if (size == 16) M3(uint8_t, 16, 16);
        else M3(uint8_t, 32, 64);
    }
    else
    {
        if (size == 8) M3(uint16_t, 8, 8);
        else if (size == 16) M3(uint16_t, 16, 16);
        else M3(uint16_t, 32, 64);
    }
#undef M3C
#undef M3
    hipError_t e = hipGetLastError();
    if (dr.predOut && dr.predDone && e == hipSuccess)
        *dr.predDone = 1;
    return e == hipSuccess ? X265HIP_OK : check_hip(e, "motion3_kernel");
}

} // namespace xh
