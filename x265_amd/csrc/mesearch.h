// mesearch.h — MotionEstimate::motionEstimate (reference: source/encoder/motion.cpp:739-1569) written once for the three motion
// kernels (motion.hip: generic, motion2.hip: team, motion3.hip: row team), with the pieces they share: MV helpers, the packed-SAD trait,
// the workload and pattern tables, and the (qmvp, mvmin, mvmax) prologue of a PU.
//
// Sections of the reference: predictor, zero and candidate tests :761-812; DIA :831-852; HEX :855-944; UMH :946-1130 (meumh.h); STAR
// :1132-1240 (mestar.h); SEA :1242-1395 (the generic kernel's own); FULL :1397-1441; bestpre/bmv merge :1449-1455; sub-pel refine
// :1504-1561 driven by workload[] :48-58; COPY*_IF_LT tie-breaking (common.h:183-204), MV::clipped / checkRange (mv.h:88-100).
//
// The kernels differ only in how they measure a candidate, which an evaluator `C` provides (besides the mestar.h / meumh.h contract
// fullpel_cost, fullpel_costs<K>, mvcost):
//     void opening(Mv pmv, Mv fp, bool fpOk, bool zeroOk, int (&out)[3])
//         out[0] = subpelCompare(pmv, sad) WITHOUT the mv cost (the bprecost start value, :771); out[1] / out[2] = the full-pel cost of
//         fp / of (0, 0), read only when fpOk / zeroOk
//     void pattern<K>(const Mv (&m)[K], int (&out)[K], int n = K)
//         sad + mvcost(m << 2) of the full-pel points of a DIA / HEX / square / FULL step; only out[0..n) is read (FULL's row tail, where
//         m[n..K) repeat m[n - 1])
//     void subpels<K>(const Mv (&q)[K], const bool (&ok)[K], int cmp, int (&out)[K])
//         subpelCompare(q, cmp: 0 sad, 1 satd) + mvcost(q) (+ the chroma SATD term of bChromaSATD); out[k] is read only where ok[k]
//     static constexpr int kSubpelGroup    sub-pel directions measured side by side (1: one by one)
//     static constexpr int kFullGroup      FULL points of a row measured per step (1: one by one)
//     static constexpr bool kSea           the evaluator has sea_search (X265_SEA)
// A cost never depends on the running best, so each step measures its points — all at once or one by one, as the evaluator
// chooses — and then replays the reference's comparisons in reference order with strict '<': the result is the same bit for bit.
#pragma once
#include "common.h"
#include "searchrange.h"
#include "mestar.h"
#include "meumh.h"

namespace xh {

struct Mv { int x, y; };

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ Mv mv_clip(Mv v, Mv lo, Mv hi)
{
    Mv r = { v.x > hi.x ? hi.x : v.x, v.y > hi.y ? hi.y : v.y };
    r.x = r.x < lo.x ? lo.x : r.x;
    r.y = r.y < lo.y ? lo.y : r.y;
    return r;
}
__device__ __forceinline__ bool mv_in_range(Mv v, Mv lo, Mv hi) { return v.x >= lo.x && v.x <= hi.x && v.y >= lo.y && v.y <= hi.y; }
__device__ __forceinline__ int sext2(int v) { return (v & 2) ? (v | ~3) : v; }

// four packed pixels: SAD against another four, and the four values
template <typename P> struct Packed;
template <> struct Packed<uint8_t>
{
    typedef uint32_t T;
    static __device__ __forceinline__ unsigned sad(T a, T b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
    static __device__ __forceinline__ void unpack(T a, int v[4]) { v[0] = a & 255; v[1] = (a >> 8) & 255; v[2] = (a >> 16) & 255; v[3] = a >> 24; }
};
template <> struct Packed<uint16_t>
{
    typedef uint2 T;
    static __device__ __forceinline__ unsigned sad(T a, T b, unsigned acc)
    {
        acc = __builtin_amdgcn_sad_u16(a.x, b.x, acc);
        return __builtin_amdgcn_sad_u16(a.y, b.y, acc);
    }
    static __device__ __forceinline__ void unpack(T a, int v[4]) { v[0] = a.x & 0xffff; v[1] = a.x >> 16; v[2] = a.y & 0xffff; v[3] = a.y >> 16; }
};

// motion.cpp:48-58 workload[subme] = { hpel_iters, hpel_dirs, qpel_iters, qpel_dirs, hpel_satd }
__device__ __constant__ const uint8_t kWorkload[8][5] = { {1,4,0,4,0}, {1,4,1,4,0}, {1,4,1,4,1}, {2,4,1,4,1}, {2,4,2,4,1}, {1,8,1,8,1}, {2,8,1,8,1}, {2,8,2,8,1} };

// The search-pattern tables of motion.cpp:63-65 as packed nibbles (value + 8): a lookup is two VALU ops on a literal instead of
// a dependent constant-memory load sitting on the serial chain (per lane in the SIMT row-team kernel).
__device__ __forceinline__ int hex2x(int i) { return (int)((0x679A9767u >> (4 * i)) & 15) - 8; }      // {-1,-2,-1,1,2,1,-1,-2}
__device__ __forceinline__ int hex2y(int i) { return (int)((0x8668AA86u >> (4 * i)) & 15) - 8; }      // {-2,0,2,2,0,-2,-2,0}
__device__ __forceinline__ int mod6m1(int i) { return (int)((0x05432105u >> (4 * i)) & 15); }          // {5,0,1,2,3,4,5,0}
__device__ __forceinline__ int sq1x(int i) { return (int)((0x997797888ull >> (4 * i)) & 15) - 8; }     // {0,0,0,-1,1,-1,-1,1,1}
__device__ __forceinline__ int sq1y(int i) { return (int)((0x979788978ull >> (4 * i)) & 15) - 8; }     // {0,-1,1,0,0,-1,1,-1,1}

// (qmvp, mvmin, mvmax) of PU `pu`: the caller's arrays, or Search::setSearchRange fused into the launch (dr.enable, searchrange.h), in
// which case the thread with `writer` set also writes the arrays, so they hold what the separate entry point would produce
__device__ __forceinline__ void pu_range(const DeriveRange& dr, int pu, int bx, int by, int merange, const int32_t* qmvpA, const int32_t* mvminA,
                                         const int32_t* mvmaxA, bool writer, Mv& qmvp, Mv& mvmin, Mv& mvmax)
{
    if (dr.enable)
    {
        qmvp = Mv{ 0, 0 };
        if (dr.mvSrc && dr.srcIdx[pu] >= 0)
            qmvp = Mv{ dr.mvSrc[2 * dr.srcIdx[pu]], dr.mvSrc[2 * dr.srcIdx[pu] + 1] };
        const SearchRange sr = search_range(dr.picW, dr.picH, dr.maxCUSize, merange, dr.refLagPixels, bx, by, qmvp.x, qmvp.y);
        mvmin = Mv{ sr.minx, sr.miny };
        mvmax = Mv{ sr.maxx, sr.maxy };
        if (writer)
        {
            dr.qmvpO[2 * pu] = qmvp.x; dr.qmvpO[2 * pu + 1] = qmvp.y;
            dr.mvminO[2 * pu] = mvmin.x; dr.mvminO[2 * pu + 1] = mvmin.y;
            dr.mvmaxO[2 * pu] = mvmax.x; dr.mvmaxO[2 * pu + 1] = mvmax.y;
        }
    }
    else
    {
        mvmin = Mv{ mvminA[2 * pu], mvminA[2 * pu + 1] };
        mvmax = Mv{ mvmaxA[2 * pu], mvmaxA[2 * pu + 1] };
        qmvp = Mv{ qmvpA[2 * pu], qmvpA[2 * pu + 1] };
    }
}

template <class C>
__device__ __forceinline__ int subpel_one(C& c, Mv q, int cmp)
{
    const Mv qs[1] = { q };
    const bool ok[1] = { true };
    int v[1];
    c.template subpels<1>(qs, ok, cmp, v);
    return v[0];
}

// one iteration of the sub-pel square refine around bmv (motion.cpp:1514-1530, :1541-1557), directions 1..dirs of square1[] at `step`
// quarter-pels; returns the winning direction, 0 when none improves on bcost
template <class C>
__device__ __forceinline__ int subpel_refine_step(C& c, Mv bmv, int dirs, int step, int cmp, Mv qmvmin, Mv qmvmax, int& bcost)
{
    constexpr int G = C::kSubpelGroup;
    int bdir = 0;
    for (int d0 = 1; d0 <= dirs; d0 += G)
    {
        Mv q[G];
        bool ok[G];
        int cs[G];
#pragma unroll
        for (int k = 0; k < G; k++)
        {
            q[k] = Mv{ bmv.x + sq1x(d0 + k) * step, bmv.y + sq1y(d0 + k) * step };
            ok[k] = !((q[k].y < qmvmin.y) | (q[k].y > qmvmax.y));
        }
        c.template subpels<G>(q, ok, cmp, cs);
#pragma unroll
        for (int k = 0; k < G; k++)
            if (ok[k] && cs[k] < bcost) { bcost = cs[k]; bdir = d0 + k; }
    }
    return bdir;
}

struct MeBest { Mv mv; int cost; };

// The whole of motionEstimate for one PU: (qmvp, mvmin, mvmax) as Search::setSearchRange gives them, mvc = the PU's numCand raw
// candidates; returns the quarter-pel vector and its cost.  Every decision variable is the same in all threads of the PU's team.
template <class C>
__device__ __forceinline__ MeBest me_search(C& c, Mv qmvp, Mv mvmin, Mv mvmax, int numCand, const int32_t* __restrict__ mvc, int merange,
                                            int method, int subme, int w, int h)
{
#define YOK(yy) (((yy) >= mvmin.y) & ((yy) <= mvmax.y))
#define LT1(v) do { const int v_ = (v); if (v_ < bcost) bcost = v_; } while (0)
    const Mv qmvmin = { mvmin.x * 4, mvmin.y * 4 }, qmvmax = { mvmax.x * 4, mvmax.y * 4 };
    // ---- predictor, zero and candidates (motion.cpp:761-812)
    const Mv pmv = mv_clip(qmvp, qmvmin, qmvmax);
    Mv bestpre = pmv;
    Mv bmv = { (pmv.x + 2) >> 2, (pmv.y + 2) >> 2 };
    int open[3];
    c.opening(pmv, bmv, ((pmv.x & 3) | (pmv.y & 3)) != 0, (pmv.x | pmv.y) != 0, open);
    int bprecost = open[0];
    int bcost = bprecost;
    if ((pmv.x & 3) | (pmv.y & 3))
        bcost = open[1];
    if ((pmv.x | pmv.y) && open[2] < bcost)
    {
        bcost = open[2];
        bmv.x = 0;
        bmv.y = max(min(0, mvmax.y), mvmin.y);
    }
    for (int i = 0; i < numCand; i++)
    {
        const Mv m = mv_clip(Mv{ mvc[2 * i], mvc[2 * i + 1] }, qmvmin, qmvmax);
        if ((m.x | m.y) && !(m.x == pmv.x && m.y == pmv.y) && !(m.x == bestpre.x && m.y == bestpre.y))
        {
            const int cst = subpel_one(c, m, 0);
            if (cst < bprecost)
            {
                bprecost = cst;
                bestpre = m;
            }
        }
    }

    // X265_UMH_SEARCH (meumh.h) ends either for good or in the hexagon refine of X265_HEX_SEARCH (goto me_hex2, motion.cpp:1127)
    int meth = method, hexRange = merange;       // UMH scales the range the hexagon refine then runs with (motion.cpp:1039)
    if (meth == 2)
        meth = umh_search(c, mvmin.x, mvmin.y, mvmax.x, mvmax.y, hexRange, bmv.x, bmv.y, bcost, (pmv.x + 2) >> 2, (pmv.y + 2) >> 2, numCand,
                          mvc, qmvp.x, qmvp.y, w, h) ? 1 : -1;
    if (meth == 0)
    {
        // X265_DIA_SEARCH, motion.cpp:831-852
        bcost <<= 4;
        int i = merange;
        do
        {
            const Mv cd[4] = { { bmv.x, bmv.y - 1 }, { bmv.x, bmv.y + 1 }, { bmv.x - 1, bmv.y }, { bmv.x + 1, bmv.y } };
            int cs[4];
            c.template pattern<4>(cd, cs);
            if (YOK(bmv.y - 1)) LT1((cs[0] << 4) + 1);
            if (YOK(bmv.y + 1)) LT1((cs[1] << 4) + 3);
            LT1((cs[2] << 4) + 4);
            LT1((cs[3] << 4) + 12);
            if (!(bcost & 15))
                break;
            bmv.x -= sext2((bcost >> 2) & 3);
            bmv.y -= sext2(bcost & 3);
            bcost &= ~15;
        }
        while (--i && mv_in_range(bmv, mvmin, mvmax));
        bcost >>= 4;
    }
    else if (meth == 1)
    {
        // X265_HEX_SEARCH, motion.cpp:855-944
        {
            // the two sad_x3 calls of motion.cpp:857-873, replayed in order
            const Mv cd[6] = { { bmv.x - 2, bmv.y }, { bmv.x - 1, bmv.y + 2 }, { bmv.x + 1, bmv.y + 2 },
                               { bmv.x + 2, bmv.y }, { bmv.x + 1, bmv.y - 2 }, { bmv.x - 1, bmv.y - 2 } };
            int cs[6];
            c.template pattern<6>(cd, cs);
            bcost <<= 3;
            if (YOK(bmv.y)) LT1((cs[0] << 3) + 2);
            if (YOK(bmv.y + 2))
            {
                LT1((cs[1] << 3) + 3);
                LT1((cs[2] << 3) + 4);
            }
            if (YOK(bmv.y)) LT1((cs[3] << 3) + 5);
            if (YOK(bmv.y - 2))
            {
                LT1((cs[4] << 3) + 6);
                LT1((cs[5] << 3) + 7);
            }
        }
        if (bcost & 7)
        {
            int dir = (bcost & 7) - 2;
            if (YOK(bmv.y + hex2y(dir + 1)))
            {
                bmv.x += hex2x(dir + 1);
                bmv.y += hex2y(dir + 1);
                for (int i = (hexRange >> 1) - 1; i > 0 && mv_in_range(bmv, mvmin, mvmax); i--)
                {
                    const Mv cd[3] = { { bmv.x + hex2x(dir + 0), bmv.y + hex2y(dir + 0) },
                                       { bmv.x + hex2x(dir + 1), bmv.y + hex2y(dir + 1) },
                                       { bmv.x + hex2x(dir + 2), bmv.y + hex2y(dir + 2) } };
                    int cs[3];
                    c.template pattern<3>(cd, cs);
                    bcost &= ~7;
                    if (YOK(cd[0].y)) LT1((cs[0] << 3) + 1);
                    if (YOK(cd[1].y)) LT1((cs[1] << 3) + 2);
                    if (YOK(cd[2].y)) LT1((cs[2] << 3) + 3);
                    if (!(bcost & 7))
                        break;
                    dir += (bcost & 7) - 2;
                    dir = mod6m1(dir + 1);
                    bmv.x += hex2x(dir + 1);
                    bmv.y += hex2y(dir + 1);
                }
            }
        }
        bcost >>= 3;
        // square refine, motion.cpp:918-942: both sad_x4 calls are centred on the same bmv
        int dir = 0;
        {
            const Mv cd[8] = { { bmv.x, bmv.y - 1 }, { bmv.x, bmv.y + 1 }, { bmv.x - 1, bmv.y }, { bmv.x + 1, bmv.y },
                               { bmv.x - 1, bmv.y - 1 }, { bmv.x - 1, bmv.y + 1 }, { bmv.x + 1, bmv.y - 1 }, { bmv.x + 1, bmv.y + 1 } };
            int cs[8];
            c.template pattern<8>(cd, cs);
            if (YOK(bmv.y - 1) && cs[0] < bcost) { bcost = cs[0]; dir = 1; }
            if (YOK(bmv.y + 1) && cs[1] < bcost) { bcost = cs[1]; dir = 2; }
            if (cs[2] < bcost) { bcost = cs[2]; dir = 3; }
            if (cs[3] < bcost) { bcost = cs[3]; dir = 4; }
            if (YOK(bmv.y - 1) && cs[4] < bcost) { bcost = cs[4]; dir = 5; }
            if (YOK(bmv.y + 1) && cs[5] < bcost) { bcost = cs[5]; dir = 6; }
            if (YOK(bmv.y - 1) && cs[6] < bcost) { bcost = cs[6]; dir = 7; }
            if (YOK(bmv.y + 1) && cs[7] < bcost) { bcost = cs[7]; dir = 8; }
        }
        bmv.x += sq1x(dir);
        bmv.y += sq1y(dir);
    }
    else if (meth == 3)
        star_search(c, mvmin.x, mvmin.y, mvmax.x, mvmax.y, merange, bmv.x, bmv.y, bcost);  // X265_STAR_SEARCH (mestar.h)
    else if (meth == 4)
    {
        if constexpr (C::kSea)
            c.sea_search(mvmin, mvmax, merange, bmv, bcost);                             // X265_SEA (motion.hip)
    }
    else if (meth == 5)
    {
        // X265_FULL_SEARCH, motion.cpp:1397-1441: raster order, strict '<' keeps the first minimum; F points of a row per step
        constexpr int F = C::kFullGroup;
        for (int ty = mvmin.y; ty <= mvmax.y; ty++)
            for (int tx = mvmin.x; tx <= mvmax.x; tx += F)
            {
                const int K = min(F, mvmax.x - tx + 1);
                Mv cd[F];
#pragma unroll
                for (int k = 0; k < F; k++) cd[k] = Mv{ tx + min(k, K - 1), ty };
                int cs[F];
                c.template pattern<F>(cd, cs, K);
#pragma unroll
                for (int k = 0; k < F; k++)
                    if (k < K && cs[k] < bcost)
                    {
                        bcost = cs[k];
                        bmv.x = tx + k;
                        bmv.y = ty;
                    }
            }
    }

    // motion.cpp:1449-1455
    if (bprecost < bcost)
    {
        bmv = bestpre;
        bcost = bprecost;
    }
    else
    {
        bmv.x *= 4;
        bmv.y *= 4;
    }

    if (!bcost)
        bcost = c.mvcost(bmv.x, bmv.y);            // motion.cpp:1466-1471
    else
    {
        // motion.cpp:1504-1561
        const int hpelIters = kWorkload[subme][0], hpelDirs = kWorkload[subme][1];
        const int qpelIters = kWorkload[subme][2], qpelDirs = kWorkload[subme][3], hpelSatd = kWorkload[subme][4];
        int iters = hpelIters;
        if (hpelSatd)
        {
            bool fused = false;
            if constexpr (C::kSubpelGroup > 1)
            {
                if (hpelDirs == 4)
                {
                    // bcost = satd(bmv) (motion.cpp:1507) and the first half-pel iteration are independent: one 5-wide measurement
                    Mv q[5];
                    bool ok[5];
                    int cs[5];
                    q[0] = bmv; ok[0] = true;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                    {
                        q[k + 1] = Mv{ bmv.x + sq1x(1 + k) * 2, bmv.y + sq1y(1 + k) * 2 };
                        ok[k + 1] = !((q[k + 1].y < qmvmin.y) | (q[k + 1].y > qmvmax.y));
                    }
                    c.template subpels<5>(q, ok, 1, cs);
                    bcost = cs[0];
                    int bdir = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (ok[k + 1] && cs[k + 1] < bcost) { bcost = cs[k + 1]; bdir = 1 + k; }
                    bmv.x += sq1x(bdir) * 2;
                    bmv.y += sq1y(bdir) * 2;
                    iters = bdir ? hpelIters - 1 : 0;   // a first iteration that found nothing ends the half-pel refine
                    fused = true;
                }
            }
            if (!fused)
                bcost = subpel_one(c, bmv, 1);
        }
        for (int iter = 0; iter < iters; iter++)
        {
            const int bdir = subpel_refine_step(c, bmv, hpelDirs, 2, hpelSatd, qmvmin, qmvmax, bcost);
            if (!bdir)
                break;
            bmv.x += sq1x(bdir) * 2;
            bmv.y += sq1y(bdir) * 2;
        }
        if (!hpelSatd)
            bcost = subpel_one(c, bmv, 1);
        for (int iter = 0; iter < qpelIters; iter++)
        {
            const int bdir = subpel_refine_step(c, bmv, qpelDirs, 1, 1, qmvmin, qmvmax, bcost);
            if (!bdir)
                break;
            bmv.x += sq1x(bdir);
            bmv.y += sq1y(bdir);
        }
    }
#undef YOK
#undef LT1
    return MeBest{ bmv, bcost };
}

} // namespace xh
