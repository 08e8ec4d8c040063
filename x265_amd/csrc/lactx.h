// lactx.h — the lookahead kernels' block evaluator: one 8x8 block of the padded half-pel plane set per DPP row of 16 lanes, four
// candidate vectors measured side by side (Lowres::lowresMC / lowresQPelCost, reference source/common/lowres.h:67-120), and the
// single-word row handshake.  Shared by lookahead.hip (HEX at range 16, the non-HME launch) and lookahead_hme.hip (the two HME levels).
#pragma once
#include "common.h"
#include "internal.h"

namespace xh {

template <typename P> struct LaPk;
template <> struct LaPk<uint8_t>
{
    typedef uint32_t T;
    static __device__ __forceinline__ T avg(T a, T b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
    static __device__ __forceinline__ unsigned sad(T a, T b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }
    static __device__ __forceinline__ void unpack(T a, int v[4]) { v[0] = a & 255; v[1] = (a >> 8) & 255; v[2] = (a >> 16) & 255; v[3] = a >> 24; }
};
template <> struct LaPk<uint16_t>
{
    typedef uint2 T;
    static __device__ __forceinline__ uint32_t avg1(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7fff7fffu); }
    static __device__ __forceinline__ T avg(T a, T b) { return make_uint2(avg1(a.x, b.x), avg1(a.y, b.y)); }
    static __device__ __forceinline__ unsigned sad(T a, T b) { return __builtin_amdgcn_sad_u16(a.y, b.y, __builtin_amdgcn_sad_u16(a.x, b.x, 0u)); }
    static __device__ __forceinline__ void unpack(T a, int v[4]) { v[0] = a.x & 0xffff; v[1] = a.x >> 16; v[2] = a.y & 0xffff; v[3] = a.y >> 16; }
};

__device__ __forceinline__ int sfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <typename P>
struct LaCtx
{
    typedef typename LaPk<P>::T Q;
    const P* ref0;            // hpel plane 0 at this lane's quad of the current block
    int64_t planeElems;
    int stride;
    const uint16_t* cost;     // centred MVD cost row
    int px, py;               // mvp (scalar, quarter-pel)
    int slot;                 // candidate slot of this lane (0..3)
    int sel[4];               // sel[j] = slot == j ? ~0 : 0
    bool hi1, hi2;
    Q fq;
    int fu[4];

    // Lowres::lowresMC / lowresQPelCost block fetch (lowres.h:75-90, :102-118)
    __device__ __forceinline__ Q fetch(int qx, int qy) const
    {
        const int ia = (qy & 2) | ((qx & 2) >> 1);
        const int rx = qx + (qx & 1), ry = qy + (qy & 1);
        const int ib = (ry & 2) | ((rx & 2) >> 1);
        // 24-bit full-rate multiplies (lowres planes are far below 2^24 elements, strides below 2^23: checked at the entry point)
        const P* a = ref0 + (__umul24(ia, (int)planeElems) + __mul24(qy >> 2, stride) + (qx >> 2));
        const P* b = ref0 + (__umul24(ib, (int)planeElems) + __mul24(ry >> 2, stride) + (rx >> 2));
        return LaPk<P>::avg(ld_global_unaligned<Q>(a), ld_global_unaligned<Q>(b));
    }
    __device__ __forceinline__ int sad(int qx, int qy) const { return row_allsum((int)LaPk<P>::sad(fetch(qx, qy), fq)); }
    __device__ __forceinline__ int satd(int qx, int qy) const { return satd_of(fetch(qx, qy)); }
    // 8x8 SATD of the source block against a predicted block held one packed quad per lane
    __device__ __forceinline__ int satd_of(Q blk) const
    {
        int p[4];
        LaPk<P>::unpack(blk, p);
        const int d0 = fu[0] - p[0], d1 = fu[1] - p[1], d2 = fu[2] - p[2], d3 = fu[3] - p[3];
        const int s01 = d0 + d1, e01 = d0 - d1, s23 = d2 + d3, e23 = d2 - d3;
        int m[4] = { s01 + s23, s01 - s23, e01 + e23, e01 - e23 };
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const int pr = __builtin_amdgcn_mov_dpp(m[i], 0xB1, 0xF, 0xF, true);
            m[i] = hi1 ? pr - m[i] : m[i] + pr;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const int pr = __builtin_amdgcn_mov_dpp(m[i], 0x4E, 0xF, 0xF, true);
            m[i] = hi2 ? pr - m[i] : m[i] + pr;
        }
        return row_allsum(iabs(m[0]) + iabs(m[1]) + iabs(m[2]) + iabs(m[3])) >> 1;
    }
    __device__ __forceinline__ int mvcost(int qx, int qy) const { return (int)(uint16_t)(cost[qx - px] + cost[qy - py]); }

    // measure 4*K candidates (quarter-pel vectors, scalar arrays) side by side: slot j of round k takes candidate 4k + j.
    // dist[] = SAD or SATD, mvc[] = lambda * bits of the vector.
    template <int K>
    __device__ __forceinline__ void eval(const int (&cx)[4 * K], const int (&cy)[4 * K], bool useSatd, int (&dist)[4 * K], int (&mvc)[4 * K]) const
    {
        int vd[K], vm[K];
#pragma unroll
        for (int k = 0; k < K; k++)
        {
            // this lane's candidate out of four wave-uniform values: mask-and-or (branch-free; the ?: chain compiled to exec-mask branches)
            const int qx = (cx[4 * k] & sel[0]) | (cx[4 * k + 1] & sel[1]) | (cx[4 * k + 2] & sel[2]) | (cx[4 * k + 3] & sel[3]);
            const int qy = (cy[4 * k] & sel[0]) | (cy[4 * k + 1] & sel[1]) | (cy[4 * k + 2] & sel[2]) | (cy[4 * k + 3] & sel[3]);
            vd[k] = useSatd ? satd(qx, qy) : sad(qx, qy);
            vm[k] = mvcost(qx, qy);
        }
#pragma unroll
        for (int k = 0; k < K; k++)
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                dist[4 * k + j] = __builtin_amdgcn_readlane(vd[k], 16 * j);
                mvc[4 * k + j] = __builtin_amdgcn_readlane(vm[k], 16 * j);
            }
    }
};

__device__ __forceinline__ int la_clip(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint64_t la_load(const uint64_t* p) { return __hip_atomic_load((const XH_GLOBAL_AS uint64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void la_unpack(uint64_t w, int& x, int& y)
{
    x = sfl((int)(int16_t)(uint16_t)(w & 0xffff));
    y = sfl((int)(int16_t)(uint16_t)((w >> 16) & 0xffff));
}

__device__ __forceinline__ void la_add64(int64_t* p, int v) { atomicAdd((unsigned long long*)p, (unsigned long long)(long long)v); }

} // namespace xh
