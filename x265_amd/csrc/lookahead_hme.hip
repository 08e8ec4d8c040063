// lookahead_hme.hip — the two search levels of the lookahead under --hme (CostEstimateGroup::estimateCUCost(…, hme), reference
// source/encoder/slicetype.cpp:3216-3324; the per-level method and range of MotionEstimate::motionEstimate under ref->isHMELowres,
// motion.cpp:817, :3309) for batches of (frame, reference) pairs on gfx950.
//
// The mapping is lookahead.hip's: one wave per block row of one pair walking right to left, the rows of a pair on one XCD in dispatch
// order, a single-word {epoch, mv} handshake towards the row above, four candidate slots per wave.  What is general here:
//  * the plane set, its stride, the distance between its planes and the grid are launch arguments of a LEVEL: level 0 walks the
//    quarter-resolution planes over the 4x4 grid and leaves with vector and cost only, level 1 is the half-resolution pass;
//  * the search method is a compile-time parameter (DIA, HEX, UMH, STAR) and the range a launch argument; UMH and STAR are the shared
//    meumh.h / mestar.h over an adapter of the block evaluator;
//  * level 1 measures a fifth predictor, twice the level-0 vector of the block's quarter-resolution parent (slicetype.cpp:3281-3284).
// The levels are separate launches on one stream: no wave ever waits for another level.
#include "common.h"
#include "internal.h"
#include "lactx.h"
#include "mestar.h"
#include "meumh.h"

namespace xh {

typedef x265hip_lookahead_hme_pair HmePair;

// the mestar.h / meumh.h evaluator contract over LaCtx: full-pel offsets in, sad + lowres mvcost out, four points per round
template <typename P>
struct LaFullpel
{
    const LaCtx<P>& c;
    __device__ __forceinline__ int mvcost(int qx, int qy) const { return sfl(c.mvcost(qx, qy)); }
    template <int K>
    __device__ __forceinline__ void fullpel_costs(const int (&mx)[K], const int (&my)[K], int (&out)[K]) const
    {
        static_assert(K % 4 == 0, "four candidate slots per round");
        int cx[K], cy[K], d[K], m[K];
#pragma unroll
        for (int i = 0; i < K; i++) { cx[i] = mx[i] * 4; cy[i] = my[i] * 4; }
        c.template eval<K / 4>(cx, cy, false, d, m);
#pragma unroll
        for (int i = 0; i < K; i++) out[i] = d[i] + m[i];
    }
    __device__ __forceinline__ int fullpel_cost(int mx, int my, int shift) const
    {
        const int cx[4] = { mx * 4, mx * 4, mx * 4, mx * 4 }, cy[4] = { my * 4, my * 4, my * 4, my * 4 };
        int d[4], m[4];
        c.template eval<1>(cx, cy, false, d, m);
        return d[0] + mvcost(mx << shift, my << shift);
    }
};

// the index of the level-0 entry a level-1 block reads (slicetype.cpp:3228, evaluated as C evaluates it)
__host__ __device__ __forceinline__ int hme_lower_index(int cuX, int cuY, int widthInCU) { return cuX / 2 + (cuY / 2) * widthInCU / 2; }

template <typename P, int METHOD>
__global__ __launch_bounds__(64) void lookahead_hme_kernel(const HmePair* __restrict__ pairs, int nPairs, int64_t stride, int64_t planeElems, int W, int H,
                                                           int rowsPerSlice, int numSlices, int merange, int flags,
                                                           const uint16_t* __restrict__ costTab, uint32_t epoch, int64_t* __restrict__ est)
{
    typedef LaCtx<P> C;
    typedef typename C::Q Q;
    constexpr int N = 8;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int pairIdx = (k / H) * 8 + xcd;
    if (pairIdx >= nPairs)
        return;
    const int cuY = H - 1 - (k % H);
    const HmePair pr = pairs[pairIdx];
    const bool bidirList = pr.bidirList != 0;
    const bool level0 = flags & 1;
    const bool vecOnly = bidirList || level0;                    // level 0 returns at slicetype.cpp:3323
    const bool useLower = !level0 && (flags & 2) && pr.lowerMvs != nullptr && pr.lowerMvCosts != nullptr;
    if (pr.sliceGeom)
    {
        rowsPerSlice = pr.sliceGeom & 0xffff;
        numSlices = pr.sliceGeom >> 16;
    }
    int slice = cuY / rowsPerSlice;
    if (slice > numSlices - 1) slice = numSlices - 1;
    const int lastY = slice == numSlices - 1 ? H - 1 : rowsPerSlice * (slice + 1) - 1;
    const bool lastRow = cuY == lastY;

    const int lane = threadIdx.x, s = lane & 15;
    const int t = s >> 2, r = s & 3;
    const int qrow = (t >> 1) * 4 + r, qcol = (t & 1) * 4;       // tile-major: the 4 rows of a 4x4 tile in one DPP quad
    C c;
    c.slot = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; j++)
        c.sel[j] = c.slot == j ? -1 : 0;
    c.hi1 = s & 1;
    c.hi2 = s & 2;
    c.stride = (int)stride;
    c.planeElems = planeElems;
    c.cost = costTab;
    const LaFullpel<P> fp{ c };
    const P* fencRow = (const P*)pr.fenc + (int64_t)(cuY * N + qrow) * stride + qcol;
    const P* refRow = (const P*)pr.ref + (int64_t)(cuY * N + qrow) * stride + qcol;
    const uint64_t* below = pr.sync + (int64_t)(cuY + 1) * W;
    uint64_t* mine = pr.sync + (int64_t)cuY * W;

    const int mvminY = -cuY * N - 8, mvmaxY = (H - cuY - 1) * N + 8;
    int rowSum = 0, scoreSum = 0, scoreAq = 0, intraCnt = 0;
    int prevX = 0, prevY = 0;
    bool stuck = false;

#pragma unroll 1
    for (int cuX = W - 1; cuX >= 0; cuX--)
    {
        const int cuXY = cuY * W + cuX;
        c.fq = ld_global_unaligned<Q>(fencRow + cuX * N);
        LaPk<P>::unpack(c.fq, c.fu);
        c.ref0 = refRow + cuX * N;
        const int mvminX = -cuX * N - 8, mvmaxX = (W - cuX - 1) * N + 8;
        const int qminX = mvminX * 4, qmaxX = mvmaxX * 4, qminY = mvminY * 4, qmaxY = mvmaxY * 4;

        // ---- reverse-order MV prediction (slicetype.cpp:3271-3307): the neighbours as in lookahead.hip, then the level-0 vector ----
        int mx[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, my[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        int numc = 0;
        const bool hasRight = cuX < W - 1, hasLeft = cuX > 0;
        const int icLoad = vecOnly ? 0 : ld_global_unaligned<int>(pr.intraCost + cuXY);
        const int iqLoad = (!vecOnly && pr.invQscale) ? ld_global_unaligned<int>(pr.invQscale + cuXY) : 256;
        // the level-0 entry this block reads: written by the launch before this one on the same stream
        const int lowIdx = hme_lower_index(cuX, cuY, W);
        const bool fifth = useLower && lowIdx < pr.lowerCount;
        const int lowCost = fifth ? pr.lowerMvCosts[lowIdx] : 0;
        const int lowX = fifth ? pr.lowerMvs[2 * lowIdx] : 0, lowY = fifth ? pr.lowerMvs[2 * lowIdx + 1] : 0;
        if (!lastRow)
        {
            // the single-word handshake of lookahead.hip: each word validated on its own, bounded spin, sticky give-up reported through est[4 i + 3]
            const int lo = hasLeft ? cuX - 1 : cuX, hi = hasRight ? cuX + 1 : cuX;
            uint64_t w0 = 0, w1 = 0, w2 = 0;
            int spins = 0;
            for (;;)
            {
                w0 = la_load(below + cuX);
                w1 = la_load(below + lo);
                w2 = la_load(below + hi);
                const bool ok = (uint32_t)sfl((int)(w0 >> 32)) == epoch && (uint32_t)sfl((int)(w1 >> 32)) == epoch && (uint32_t)sfl((int)(w2 >> 32)) == epoch;
                if (ok || stuck)
                    break;
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1 << 22)) stuck = true;
            }
            int bx, by, lx, ly, rx, ry;
            la_unpack(w0, bx, by);
            la_unpack(w1, lx, ly);
            la_unpack(w2, rx, ry);
            if (hasRight)
            {
                mx[0] = prevX; my[0] = prevY;
                mx[1] = bx; my[1] = by;
                mx[2] = hasLeft ? lx : rx; my[2] = hasLeft ? ly : ry;
                mx[3] = rx; my[3] = ry;                               // only counted when hasLeft
                numc = hasLeft ? 4 : 3;
            }
            else
            {
                mx[0] = bx; my[0] = by;
                mx[1] = lx; my[1] = ly;                               // only counted when hasLeft
                numc = hasLeft ? 2 : 1;
            }
        }
        else if (hasRight)
        {
            mx[0] = prevX; my[0] = prevY;
            numc = 1;
        }
        if (fifth && sfl(lowCost) > 0)
        {
            // MVC(lowerResMvs * 2), placed behind the neighbours (wave-uniform selects: no dynamically indexed array)
            const int fx = sfl(lowX) * 2, fy = sfl(lowY) * 2;
#pragma unroll
            for (int i = 0; i < 5; i++)
                if (i == numc) { mx[i] = fx; my[i] = fy; }
            numc++;
        }
        int mvpX = 0, mvpY = 0, skipCost = 0x7fffffff;
        c.px = 0; c.py = 0;
        if (numc)
        {
            int d[8], m[8];
            if (numc > 4)
                c.template eval<2>(mx, my, true, d, m);
            else
            {
                const int ax[4] = { mx[0], mx[1], mx[2], mx[3] }, ay[4] = { my[0], my[1], my[2], my[3] };
                int d4[4], m4[4];
                c.template eval<1>(ax, ay, true, d4, m4);
#pragma unroll
                for (int i = 0; i < 4; i++) d[i] = d4[i];
                d[4] = 0;
            }
            int mvpcost = 1 << 28;                                // MotionEstimate::COST_MAX (motion.h:65)
#pragma unroll
            for (int i = 0; i < 5; i++)
                if (i < numc)
                {
                    if (d[i] < mvpcost) { mvpcost = d[i]; mvpX = mx[i]; mvpY = my[i]; }
                    if (bidirList && !(mvpX | mvpY))              // slicetype.cpp:3303-3305
                        skipCost = d[i];
                }
        }
        c.px = mvpX; c.py = mvpY;

        // ---- motionEstimate, lowres flavour (motion.cpp:761-795) ----
        const int pmvX = la_clip(mvpX, qminX, qmaxX), pmvY = la_clip(mvpY, qminY, qmaxY);
        int bmvX = (pmvX + 2) >> 2, bmvY = (pmvY + 2) >> 2;
        int bcost;
        int bprecost;
        {
            const int cx[4] = { pmvX, bmvX * 4, 0, 0 }, cy[4] = { pmvY, bmvY * 4, 0, 0 };
            int d[4], m[4];
            c.template eval<1>(cx, cy, false, d, m);
            bprecost = d[0];
            bcost = bprecost;
            if ((pmvX | pmvY) & 3)
                bcost = d[1] + m[1];
            if (pmvX | pmvY)
            {
                const int z = d[2] + m[2];
                if (z < bcost)
                {
                    bcost = z;
                    bmvX = 0;
                    bmvY = mvmaxY < 0 ? mvmaxY : 0;
                    if (bmvY < mvminY) bmvY = mvminY;
                }
            }
        }
#define YOK(yy) (((yy) >= mvminY) & ((yy) <= mvmaxY))
#define LT1(v) do { const int v_ = (v); if (v_ < bcost) bcost = v_; } while (0)
        // X265_UMH_SEARCH ends either for good or in the hexagon refine of X265_HEX_SEARCH (goto me_hex2, motion.cpp:1127).  The lowres
        // search passes no candidate list (numCandidates == 0), so UMH's adaptive range (:988-1040) never applies.
        bool hex = METHOD == X265HIP_ME_HEX;
        int hexRange = merange;
        if (METHOD == X265HIP_ME_UMH)
            hex = umh_search(fp, mvminX, mvminY, mvmaxX, mvmaxY, hexRange, bmvX, bmvY, bcost, (pmvX + 2) >> 2, (pmvY + 2) >> 2, 0, (const int32_t*)nullptr,
                             mvpX, mvpY, N, N);
        if (METHOD == X265HIP_ME_DIA)
        {
            // ---- diamond search, radius 1 (motion.cpp:820-843) ----
            bcost <<= 4;
            int i = merange;
            do
            {
                const int cx[4] = { bmvX * 4, bmvX * 4, (bmvX - 1) * 4, (bmvX + 1) * 4 }, cy[4] = { (bmvY - 1) * 4, (bmvY + 1) * 4, bmvY * 4, bmvY * 4 };
                int d[4], m[4];
                c.template eval<1>(cx, cy, false, d, m);
                if (YOK(bmvY - 1)) LT1(((d[0] + m[0]) << 4) + 1);
                if (YOK(bmvY + 1)) LT1(((d[1] + m[1]) << 4) + 3);
                LT1(((d[2] + m[2]) << 4) + 4);
                LT1(((d[3] + m[3]) << 4) + 12);
                if (!(bcost & 15))
                    break;
                bmvX -= (int)((uint32_t)bcost << 28) >> 30;
                bmvY -= (int)((uint32_t)bcost << 30) >> 30;
                bcost &= ~15;
            }
            while (--i && bmvX >= mvminX && bmvX <= mvmaxX && bmvY >= mvminY && bmvY <= mvmaxY);
            bcost >>= 4;
        }
        else if (hex)
        {
            // ---- hexagon search (motion.cpp:855-944) ----
            {
                const int cx[8] = { (bmvX - 2) * 4, (bmvX - 1) * 4, (bmvX + 1) * 4, (bmvX + 2) * 4, (bmvX + 1) * 4, (bmvX - 1) * 4, bmvX * 4, bmvX * 4 };
                const int cy[8] = { bmvY * 4, (bmvY + 2) * 4, (bmvY + 2) * 4, bmvY * 4, (bmvY - 2) * 4, (bmvY - 2) * 4, bmvY * 4, bmvY * 4 };
                int d[8], m[8];
                c.template eval<2>(cx, cy, false, d, m);
                bcost <<= 3;
                if (YOK(bmvY)) LT1(((d[0] + m[0]) << 3) + 2);
                if (YOK(bmvY + 2))
                {
                    LT1(((d[1] + m[1]) << 3) + 3);
                    LT1(((d[2] + m[2]) << 3) + 4);
                }
                if (YOK(bmvY)) LT1(((d[3] + m[3]) << 3) + 5);
                if (YOK(bmvY - 2))
                {
                    LT1(((d[4] + m[4]) << 3) + 6);
                    LT1(((d[5] + m[5]) << 3) + 7);
                }
            }
            if (bcost & 7)
            {
                // hex2[] = {-1,-2},{-2,0},{-1,2},{1,2},{2,0},{1,-2},{-1,-2},{-2,0}; mod6m1[] = 5,0,1,2,3,4,5,0 (motion.cpp:63-64)
                auto hx = [](int i) { return (int)((0x679A9767u >> (4 * i)) & 15) - 8; };
                auto hy = [](int i) { return (int)((0x8668AA86u >> (4 * i)) & 15) - 8; };
                auto m6 = [](int i) { return (int)((0x05432105u >> (4 * i)) & 15); };
                int dir = (bcost & 7) - 2;
                if (YOK(bmvY + hy(dir + 1)))
                {
                    bmvX += hx(dir + 1);
                    bmvY += hy(dir + 1);
#pragma unroll 1
                    for (int i = (hexRange >> 1) - 1; i > 0 && bmvX >= mvminX && bmvX <= mvmaxX && bmvY >= mvminY && bmvY <= mvmaxY; i--)
                    {
                        const int cx[4] = { (bmvX + hx(dir)) * 4, (bmvX + hx(dir + 1)) * 4, (bmvX + hx(dir + 2)) * 4, bmvX * 4 };
                        const int cy[4] = { (bmvY + hy(dir)) * 4, (bmvY + hy(dir + 1)) * 4, (bmvY + hy(dir + 2)) * 4, bmvY * 4 };
                        int d[4], m[4];
                        c.template eval<1>(cx, cy, false, d, m);
                        bcost &= ~7;
                        if (YOK(bmvY + hy(dir))) LT1(((d[0] + m[0]) << 3) + 1);
                        if (YOK(bmvY + hy(dir + 1))) LT1(((d[1] + m[1]) << 3) + 2);
                        if (YOK(bmvY + hy(dir + 2))) LT1(((d[2] + m[2]) << 3) + 3);
                        if (!(bcost & 7))
                            break;
                        dir += (bcost & 7) - 2;
                        dir = m6(dir + 1);
                        bmvX += hx(dir + 1);
                        bmvY += hy(dir + 1);
                    }
                }
            }
            bcost >>= 3;
            {
                // square refine (motion.cpp:924-942): square1[1..8] = (0,-1),(0,1),(-1,0),(1,0),(-1,-1),(-1,1),(1,-1),(1,1)
                const int cx[8] = { bmvX * 4, bmvX * 4, (bmvX - 1) * 4, (bmvX + 1) * 4, (bmvX - 1) * 4, (bmvX - 1) * 4, (bmvX + 1) * 4, (bmvX + 1) * 4 };
                const int cy[8] = { (bmvY - 1) * 4, (bmvY + 1) * 4, bmvY * 4, bmvY * 4, (bmvY - 1) * 4, (bmvY + 1) * 4, (bmvY - 1) * 4, (bmvY + 1) * 4 };
                int d[8], m[8];
                c.template eval<2>(cx, cy, false, d, m);
                int dir = -1;
                const bool up = YOK(bmvY - 1), dn = YOK(bmvY + 1);
                const bool ok[8] = { up, dn, true, true, up, dn, up, dn };
#pragma unroll
                for (int i = 0; i < 8; i++)
                {
                    const int v = d[i] + m[i];
                    if (ok[i] && v < bcost) { bcost = v; dir = i; }
                }
                if (dir >= 0)
                {
                    bmvX += (int)((0x99779788u >> (4 * dir)) & 15) - 8;   // x offsets {0,0,-1,1,-1,-1,1,1} + 8, one nibble each
                    bmvY += (int)((0x97978897u >> (4 * dir)) & 15) - 8;   // y offsets {-1,1,0,0,-1,1,-1,1} + 8
                }
            }
        }
        else if (METHOD == X265HIP_ME_STAR)
            star_search(fp, mvminX, mvminY, mvmaxX, mvmaxY, merange, bmvX, bmvY, bcost);
        // ---- motion.cpp:1448-1454 ----
        if (bprecost < bcost)
        {
            bmvX = pmvX; bmvY = pmvY;
            bcost = bprecost;
        }
        else
        {
            bmvX *= 4; bmvY *= 4;
        }
        // ---- lowres sub-pel refine (motion.cpp:1465-1503, workload[1]: 4 half-pel and 4 quarter-pel directions) ----
        if (!bcost)
        {
            const int cx[4] = { bmvX, bmvX, bmvX, bmvX }, cy[4] = { bmvY, bmvY, bmvY, bmvY };
            int d[4], m[4];
            c.template eval<1>(cx, cy, false, d, m);
            bcost = m[0];
        }
        else
        {
            {
                const int cx[4] = { bmvX, bmvX, bmvX - 2, bmvX + 2 }, cy[4] = { bmvY - 2, bmvY + 2, bmvY, bmvY };
                int d[4], m[4];
                c.template eval<1>(cx, cy, false, d, m);
                int bdir = -1;
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int v = d[i] + m[i];
                    if (cy[i] >= qminY && cy[i] <= qmaxY && v < bcost) { bcost = v; bdir = i; }
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (bdir == i) { const int nx = cx[i], ny = cy[i]; bmvX = nx; bmvY = ny; }
            }
            {
                const int cx[8] = { bmvX, bmvX, bmvX, bmvX - 1, bmvX + 1, bmvX, bmvX, bmvX }, cy[8] = { bmvY, bmvY - 1, bmvY + 1, bmvY, bmvY, bmvY, bmvY, bmvY };
                int d[8], m[8];
                c.template eval<2>(cx, cy, true, d, m);
                bcost = d[0] + m[0];
                int bdir = -1;
#pragma unroll
                for (int i = 1; i < 5; i++)
                {
                    const int v = d[i] + m[i];
                    if (cy[i] >= qminY && cy[i] <= qmaxY && v < bcost) { bcost = v; bdir = i; }
                }
#pragma unroll
                for (int i = 1; i < 5; i++)
                    if (bdir == i) { const int nx = cx[i], ny = cy[i]; bmvX = nx; bmvY = ny; }
            }
        }
#undef YOK
#undef LT1
        if (bidirList && skipCost < 64 && skipCost < bcost)      // slicetype.cpp:3316-3320
        {
            bcost = skipCost;
            bmvX = 0; bmvY = 0;
        }
        // ---- publish, then the block's bookkeeping (slicetype.cpp:3321-3387) ----
        if (lane == 0)
            __hip_atomic_store(mine + cuX, ((uint64_t)epoch << 32) | (uint32_t)(uint16_t)bmvX | ((uint32_t)(uint16_t)bmvY << 16),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        prevX = bmvX; prevY = bmvY;
        const int fencCost = bcost;
        if (vecOnly)
        {
            if (lane == 0)
            {
                pr.mvs[2 * cuXY] = bmvX;
                pr.mvs[2 * cuXY + 1] = bmvY;
                pr.mvCosts[cuXY] = fencCost;
            }
            continue;
        }
        int cuCost = fencCost + 4, listused = 1;
        const int ic = sfl(icLoad);
        if (ic < cuCost) { cuCost = ic; listused = 0; }
        const bool scored = (cuX > 0 && cuX < W - 1 && cuY > 0 && cuY < H - 1) || W <= 2 || H <= 2;
        int cuCostAq = cuCost;
        if (scored)
        {
            if (pr.invQscale)
                cuCostAq = (cuCost * sfl(iqLoad) + 128) >> 8;
            scoreSum += cuCost;
            scoreAq += cuCostAq;
            intraCnt += !listused;
        }
        rowSum += cuCostAq;
        if (lane == 0)
        {
            pr.mvs[2 * cuXY] = bmvX;
            pr.mvs[2 * cuXY + 1] = bmvY;
            pr.mvCosts[cuXY] = fencCost;
            pr.lowresCosts[cuXY] = (uint16_t)((cuCost < 16383 ? cuCost : 16383) | (listused << 14));
        }
    }
    if (lane == 0 && !vecOnly)
    {
        pr.rowSatds[cuY] = rowSum;
        la_add64(est + 4 * pairIdx, scoreSum);
        la_add64(est + 4 * pairIdx + 1, scoreAq);
        la_add64(est + 4 * pairIdx + 2, intraCnt);
    }
    if (lane == 0 && stuck)
        atomicOr((unsigned long long*)(est + 4 * pairIdx + 3), 1ull);
}

// How far, in pixels of its level, a measured block's top-left corner can lie outside the grid's own area [0, (W-1)*8] x [0, (H-1)*8]:
//    8  the search window (mvmin / mvmax, slicetype.cpp:3248-3251)
//  + 8  a neighbour's vector, taken from a window one block to the side or below, measured unclipped as a predictor (:3297-3302)
//  + 8  points the methods measure past the window: HEX leaves it by up to 2 in x and its square refine adds 1; UMH's unchecked
//       COST_MV_X4 steps chain up to 2 + 2 + 2; DIA 2; STAR checks every point; the sub-pel refine and the second half-pel plane of a
//       quarter-pel fetch add 1 more.  8 covers every method.
static constexpr int kReach = 24;
static constexpr int kVecSlack = 8;      // of that, what a block's FINAL vector can lie outside its own window (the third term)

template <typename P, int M>
static void launch_hme(dim3 grid, hipStream_t st, const HmePair* pairs, int nPairs, const x265hip_lookahead_hme_level& g, int flags, const uint16_t* mvcost,
                       uint32_t epoch, int64_t* est)
{
    hipLaunchKernelGGL((lookahead_hme_kernel<P, M>), grid, dim3(64), 0, st, pairs, nPairs, g.stride, g.planeElems, g.widthInCU, g.heightInCU, g.numRowsPerSlice,
                       g.numSlices, g.range, flags, mvcost, epoch, est);
}

static bool level_shape_ok(const x265hip_lookahead_hme_level* g)
{
    return g && g->widthInCU >= 1 && g->heightInCU >= 1 && g->widthInCU <= 512 && g->heightInCU <= 512 && g->stride >= 8 && g->stride < (1 << 23) &&
           g->planeElems > 0 && g->planeElems < (1 << 24) && g->padOffset >= 0 && g->padOffset < g->planeElems;
}

} // namespace xh

using namespace xh;

extern "C" int x265hip_lookahead_hme_slices_ok(int W8, int H8, int W4, int H4, int rows8, int numSlices)
{
    if (W8 < 1 || H8 < 1 || W4 < 1 || H4 < 1 || rows8 < 1 || numSlices < 1 || (long long)rows8 * (numSlices - 1) >= H8)
        return 0;
    // level-0 rows per slice, slicetype.cpp:3083-3086
    int rows4 = H4 / numSlices;
    rows4 = rows4 > 5 ? rows4 : 5;
    rows4 = rows4 < H4 ? rows4 : H4;
    if (numSlices > 1 && (long long)rows4 * (numSlices - 1) >= H4)
        return 0;                                   // a slice would start at or past the last level-0 row: the reference walks off the grid
    for (int cuY = 0; cuY < H8; cuY++)
    {
        int slice = cuY / rows8;
        if (slice > numSlices - 1) slice = numSlices - 1;
        const int first4 = rows4 * slice, last4 = slice == numSlices - 1 ? H4 - 1 : rows4 * (slice + 1) - 1;
        for (int cuX = 0; cuX < W8; cuX++)
        {
            const int k = hme_lower_index(cuX, cuY, W8);
            if (k >= W4 * H4) return 0;
            const int row = k / W4;
            if (row < first4 || row > last4) return 0;
        }
    }
    return 1;
}

extern "C" int x265hip_lookahead_cost_hme_batch(int depth, const x265hip_lookahead_hme_pair* pairs, int nPairs, int level,
                                                const x265hip_lookahead_hme_level* geom, const x265hip_lookahead_hme_level* lower,
                                                const uint16_t* mvcost, uint32_t epoch, int64_t* est, void* stream)
{
    XH_CHECK_DEV();
    if (!valid_depth(depth) || nPairs < 0 || (level != 0 && level != 1) || !level_shape_ok(geom) || (lower && !level_shape_ok(lower)) || epoch == 0 || !est ||
        !mvcost || geom->numSlices < 1 || geom->numRowsPerSlice < 1 || (long long)geom->numRowsPerSlice * (geom->numSlices - 1) >= geom->heightInCU)
        return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: depth %d pairs %d level %d epoch %u, or a level's geometry", depth, nPairs, level, epoch);
    const x265hip_lookahead_hme_level& g = *geom;
    if (g.method < X265HIP_ME_DIA || g.method > X265HIP_ME_STAR)
        return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: search method %d is not served (DIA, HEX, UMH, STAR are; FULL has an HME-only window rule, "
                         "SEA needs integral planes)", g.method);
    if (g.range < 1 || g.range > X265HIP_LA_HME_MAX_RANGE)
        return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: range %d outside 1..%d", g.range, X265HIP_LA_HME_MAX_RANGE);
    // ---- every measured block inside its plane's allocation -------------------------------------------------------------------
    // A block whose top-left corner is at (x, y) of a plane reads the elements origin + y * stride + x .. + 8 * stride + 8 (eight lines
    // of eight, one more line and column for the second half-pel plane's rounding).  With the origin padOffset elements into an
    // allocation of planeElems, every read stays inside when
    //        y_min * stride + x_min >= -padOffset      and      (y_max + 8) * stride + x_max + 8 < planeElems - padOffset.
    // Window, neighbour predictors and search points: x in [-kReach, (W - 1) * 8 + kReach], y in [-kReach, (H - 1) * 8 + kReach].
    {
        const int64_t lo = -(int64_t)kReach * g.stride - kReach;
        const int64_t hi = (int64_t)((g.heightInCU - 1) * 8 + kReach + 8) * g.stride + (g.widthInCU - 1) * 8 + kReach + 8;
        if (lo < -g.padOffset || hi >= g.planeElems - g.padOffset)
            return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: level %d planes (stride %lld, %lld elements, origin at %lld) do not hold a %dx%d grid with "
                             "%d pixels of search reach", level, (long long)g.stride, (long long)g.planeElems, (long long)g.padOffset, g.widthInCU, g.heightInCU, kReach);
    }
    // The fifth predictor of level-1 block (cuX, cuY) is twice the vector of level-0 block k = (kx, ky).  That vector lies in k's own
    // window widened by kVecSlack: vx in [-(kx * 8 + 8 + s), (W4 - kx - 1) * 8 + 8 + s], vy likewise, so the block measured is at
    //        x = cuX * 8 + 2 vx,  y = cuY * 8 + 2 vy
    // and the same two inequalities must hold for the extremes of every block (k need not be the block's parent: see hme_lower_index).
    if (level == 1 && lower)
    {
        const int W4 = lower->widthInCU, H4 = lower->heightInCU, s = kVecSlack;
        for (int cuY = 0; cuY < g.heightInCU; cuY++)
            for (int cuX = 0; cuX < g.widthInCU; cuX++)
            {
                const int k = hme_lower_index(cuX, cuY, g.widthInCU);
                if (k >= W4 * H4)
                    return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: block (%d, %d) reads level-0 entry %d of %d", cuX, cuY, k, W4 * H4);
                const int kx = k % W4, ky = k / W4;
                const int64_t xmin = cuX * 8 - 2 * (kx * 8 + 8 + s), xmax = cuX * 8 + 2 * ((W4 - kx - 1) * 8 + 8 + s);
                const int64_t ymin = cuY * 8 - 2 * (ky * 8 + 8 + s), ymax = cuY * 8 + 2 * ((H4 - ky - 1) * 8 + 8 + s);
                if (ymin * g.stride + xmin < -g.padOffset || (ymax + 8) * g.stride + xmax + 8 >= g.planeElems - g.padOffset)
                    return set_error(X265HIP_EINVAL, "lookahead_cost_hme_batch: the doubled level-0 vector of block (%d, %d) can leave the level-1 planes", cuX, cuY);
            }
    }
    if (nPairs == 0) return X265HIP_OK;
    int e = check_hip(hipMemsetAsync(est, 0, (size_t)nPairs * 4 * sizeof(int64_t), as_stream(stream)), "lookahead hme memset");
    if (e) return e;
    const int groups = (nPairs + 7) / 8;
    const dim3 grid((unsigned)(groups * g.heightInCU * 8));
    hipStream_t st = as_stream(stream);
    const int flags = (level == 0 ? 1 : 0) | (lower ? 2 : 0);       // without level 0's geometry the fifth predictor cannot be bounded: not taken
#define XH_HME(P) do { switch (g.method) { \
        case X265HIP_ME_DIA: launch_hme<P, X265HIP_ME_DIA>(grid, st, pairs, nPairs, g, flags, mvcost, epoch, est); break; \
        case X265HIP_ME_HEX: launch_hme<P, X265HIP_ME_HEX>(grid, st, pairs, nPairs, g, flags, mvcost, epoch, est); break; \
        case X265HIP_ME_UMH: launch_hme<P, X265HIP_ME_UMH>(grid, st, pairs, nPairs, g, flags, mvcost, epoch, est); break; \
        default: launch_hme<P, X265HIP_ME_STAR>(grid, st, pairs, nPairs, g, flags, mvcost, epoch, est); break; } } while (0)
    if (depth == 8) XH_HME(uint8_t); else XH_HME(uint16_t);
#undef XH_HME
    XH_LAUNCH_CHECK("lookahead_hme_kernel");
    return X265HIP_OK;
}
