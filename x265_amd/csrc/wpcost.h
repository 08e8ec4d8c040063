// wpcost.h — the arithmetic of the frame encoder's weighted-prediction analysis, stated once for the kernel (wpcost.hip), the binding's X265HIP_VERIFY
// path (x265_amd/host/x265_hip_weightp.cpp) and the CPU checker of the tests: what the reference's mcLuma, mcChroma and weightCost
// (source/encoder/weightPrediction.cpp:60-218) compute, with Lowres::lowresMC (source/common/lowres.h:67-92), the chroma interpolation filters
// (source/common/ipfilter.cpp:80-282), weight_pp_c (source/common/pixel.cpp:518-543) and the SATD of source/common/pixel.cpp:239-297.  Everything is
// integer; 8 / 10 / 12 bit; 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4.  P is the sample type (uint8_t at 8 bit, uint16_t above); plane pointers address sample (0, 0)
// of a plane with readable borders, strides are in samples, vectors are the reference's MV (two int32: x, y) in quarter-pels of the lowres picture.
//
// The quirks, kept to the letter:
//   * mcLuma walks `y < lines; y += 8` and `x < width; x += 8`, cu++ per block: a row of (width + 7) / 8 blocks; a partial last block is compensated whole
//   * mcChroma indexes the vectors with cu = y * lowresWidthInCU (y in chroma PIXEL rows), + 1 per block, and compensates a block only where
//     x < lowresWidthInCU && y < lowresHeightInCU with x, y in chroma PIXELS: the top-left corner of the plane; every other block is a plain copy
//   * mcChroma doubles the vector, shifts it by the chroma shifts, clips it to [(-x - 8) * 4, (width - x - 1 + 8) * 4], takes the position from mv >> 2
//     and the filter phases from mv & 7
//   * weight_pp passes the sample through int16_t after << (14 - depth)
//   * x265's 8x8 SATD is two 8x4 SATDs, each ((left 4x4 Hadamard sum) + (right one)) >> 1; 16x16 is eight of them
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XW_HD __host__ __device__ __forceinline__
#else
#define XW_HD inline
#endif

// what the compensation may read around a plane, in samples: the clipped vector reaches 8 before the plane and (extent - 1 + 8) after a block's origin
#define XW_LUMA_LO    8      /* columns / rows before sample (0, 0) of the four lowres planes */
#define XW_LUMA_HI    16     /* columns / rows after `width` / `lines`: 7 + an 8-wide block + 1 for the second plane of a quarter-pel average */
#define XW_CHROMA_LO  9      /* 8 + one filter tap */
#define XW_CHROMA_HI(b) ((b) + 10)   /* b = the block's extent (16 >> the chroma shift): 7 + the block + two filter taps + 1 */
#define XW_MAX_CANDS  16     /* candidates of one evaluation */

XW_HD int xw_clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }

// g_chromaFilter (source/common/constants.cpp), the HEVC chroma interpolation taps
XW_HD int xw_chroma_tap(int frac, int k)
{
    const int t[8][4] = { { 0, 64, 0, 0 }, { -2, 58, 10, -2 }, { -4, 54, 16, -2 }, { -6, 46, 28, -4 }, { -4, 36, 36, -4 }, { -4, 28, 46, -6 }, { -2, 16, 54, -4 },
                          { -2, 10, 58, -2 } };
    return t[frac][k];
}

// ---- mcLuma: sample (x, y) of the compensated lowres plane.  planes[4] = the reference's lowresPlane[0..3]; mvs = fenc.lowresMvs[list][diffPoc]
template <typename P>
XW_HD int xw_mc_luma(const P* const planes[4], int64_t stride, int width, int lines, const int32_t* mvs, int x, int y)
{
    const int bx = x & ~7, by = y & ~7, cu = (by >> 3) * ((width + 7) >> 3) + (bx >> 3);
    const int mx = xw_clip3((-bx - 8) * 4, (width - bx - 1 + 8) * 4, mvs[2 * cu]);
    const int my = xw_clip3((-by - 8) * 4, (lines - by - 1 + 8) * 4, mvs[2 * cu + 1]);
    const int64_t at = (int64_t)y * stride + x;
    const int hpelA = (my & 2) | ((mx & 2) >> 1);
    const int a = planes[hpelA][at + (mx >> 2) + (int64_t)(my >> 2) * stride];
    if (!((mx | my) & 1))
        return a;
    const int qx = mx + (mx & 1), qy = my + (my & 1);
    const int hpelB = (qy & 2) | ((qx & 2) >> 1);
    const int b = planes[hpelB][at + (qx >> 2) + (int64_t)(qy >> 2) * stride];
    return (a + b + 1) >> 1;                                                     // pixelavg_pp, weight 32
}
// which branch of lowresMC block (bx, by) takes: 0 a half-pel plane, 1 the rounded average; *clipped: bit 0 left, 1 right, 2 top, 3 bottom
XW_HD int xw_mc_luma_branch(int width, int lines, const int32_t* mvs, int bx, int by, int* clipped)
{
    const int cu = (by >> 3) * ((width + 7) >> 3) + (bx >> 3);
    const int vx = mvs[2 * cu], vy = mvs[2 * cu + 1];
    const int mx = xw_clip3((-bx - 8) * 4, (width - bx - 1 + 8) * 4, vx), my = xw_clip3((-by - 8) * 4, (lines - by - 1 + 8) * 4, vy);
    *clipped = (mx > vx ? 1 : 0) | (mx < vx ? 2 : 0) | (my > vy ? 4 : 0) | (my < vy ? 8 : 0);
    return ((mx | my) & 1) ? 1 : 0;
}

// ---- mcChroma: the vector of the block that holds (x, y), after doubling, shifting and clipping.  Returns 0 where the block is a plain copy
XW_HD int xw_mc_chroma_mv(int width, int height, const int32_t* mvs, int lowresWidthInCU, int lowresHeightInCU, int hshift, int vshift, int x, int y, int* mx,
                          int* my, int* clipped)
{
    const int bw = 16 >> hshift, bh = 16 >> vshift;
    const int bx = x - x % bw, by = y - y % bh;
    *mx = *my = *clipped = 0;
    if (!(bx < lowresWidthInCU && by < lowresHeightInCU))
        return 0;
    const int cu = by * lowresWidthInCU + bx / bw;
    const int vx = (mvs[2 * cu] * 2) >> hshift, vy = (mvs[2 * cu + 1] * 2) >> vshift;
    *mx = xw_clip3((-bx - 8) * 4, (width - bx - 1 + 8) * 4, vx);
    *my = xw_clip3((-by - 8) * 4, (height - by - 1 + 8) * 4, vy);
    *clipped = (*mx > vx ? 1 : 0) | (*mx < vx ? 2 : 0) | (*my > vy ? 4 : 0) | (*my < vy ? 8 : 0);
    return 1;
}
// the branch of mcChroma: 0 plain copy (outside the corner), 1 copy_pp at the vector, 2 filter_hpp, 3 filter_vpp, 4 filter_hps + filter_vsp
XW_HD int xw_mc_chroma_branch(int compensated, int mx, int my)
{
    const int xFrac = mx & 7, yFrac = my & 7;
    return !compensated ? 0 : (!(xFrac | yFrac) ? 1 : (!yFrac ? 2 : (!xFrac ? 3 : 4)));
}
// sample (x, y) of the compensated chroma plane; src = the reference's (border-extended) chroma plane
template <typename P>
XW_HD int xw_mc_chroma(const P* src, int64_t stride, int width, int height, const int32_t* mvs, int lowresWidthInCU, int lowresHeightInCU, int hshift, int vshift,
                       int depth, int x, int y)
{
    int mx, my, clipped;
    const int64_t at = (int64_t)y * stride + x;
    if (!xw_mc_chroma_mv(width, height, mvs, lowresWidthInCU, lowresHeightInCU, hshift, vshift, x, y, &mx, &my, &clipped))
        return src[at];
    const P* t = src + at + (int64_t)(my >> 2) * stride + (mx >> 2);
    const int xFrac = mx & 7, yFrac = my & 7, maxv = (1 << depth) - 1;
    if (!(xFrac | yFrac))
        return t[0];
    if (!yFrac || !xFrac)
    {
        // interp_horiz_pp_c<4> / interp_vert_pp_c<4>
        const int64_t step = !yFrac ? 1 : stride;
        const int frac = !yFrac ? xFrac : yFrac;
        int sum = 0;
        for (int k = 0; k < 4; k++)
            sum += (int)t[(k - 1) * step] * xw_chroma_tap(frac, k);
        const int16_t val = (int16_t)((sum + 32) >> 6);
        return xw_clip3(0, maxv, val);
    }
    // interp_horiz_ps_c<4> with isRowExt into the 16-bit intermediate, then interp_vert_sp_c<4> from row NTAPS_CHROMA / 2 - 1 of it
    const int headRoom = 14 - depth, shiftH = 6 - headRoom, offH = (int)((unsigned)-8192 << shiftH);
    const int shiftV = 6 + headRoom, offV = (1 << (shiftV - 1)) + (8192 << 6);
    int sum = 0;
    for (int r = 0; r < 4; r++)
    {
        int h = 0;
        for (int k = 0; k < 4; k++)
            h += (int)t[(int64_t)(r - 1) * stride + (k - 1)] * xw_chroma_tap(xFrac, k);
        const int16_t imm = (int16_t)((h + offH) >> shiftH);
        sum += imm * xw_chroma_tap(yFrac, r);
    }
    const int16_t val = (int16_t)((sum + offV) >> shiftV);
    return xw_clip3(0, maxv, val);
}

// ---- weightCost.  A candidate as weight_pp receives it (weightPrediction.cpp:182-189)
struct xw_cand { int32_t present, w0, round, shift, offset; };
XW_HD xw_cand xw_make_cand(int depth, int wtPresent, int inputWeight, int inputOffset, int log2WeightDenom)
{
    const int correction = 14 - depth;
    xw_cand c;
    c.present = wtPresent;
    c.w0 = inputWeight;
    c.round = (log2WeightDenom ? 1 << (log2WeightDenom - 1) : 0) << correction;
    c.shift = log2WeightDenom + correction;
    c.offset = inputOffset << (depth - 8);          // (a negative offset: an arithmetic shift, as the reference's compilers do it)
    return c;
}
// weight_pp_c on one sample
XW_HD int xw_weight(int v, const xw_cand& c, int depth)
{
    const int16_t val = (int16_t)(v << (14 - depth));
    return xw_clip3(0, (1 << depth) - 1, ((c.w0 * val + c.round) >> c.shift) + c.offset);
}
XW_HD int xw_abs(int v) { return v < 0 ? -v : v; }
// the sum of the absolute 4x4 Hadamard coefficients of d[0..3][x0..x0+3]
XW_HD int xw_had4(const int (*d)[8], int x0)
{
    int t[4][4];
    for (int i = 0; i < 4; i++)
    {
        const int s01 = d[i][x0] + d[i][x0 + 1], d01 = d[i][x0] - d[i][x0 + 1], s23 = d[i][x0 + 2] + d[i][x0 + 3], d23 = d[i][x0 + 2] - d[i][x0 + 3];
        t[i][0] = s01 + s23; t[i][1] = d01 + d23; t[i][2] = s01 - s23; t[i][3] = d01 - d23;
    }
    int sum = 0;
    for (int j = 0; j < 4; j++)
    {
        const int s01 = t[0][j] + t[1][j], d01 = t[0][j] - t[1][j], s23 = t[2][j] + t[3][j], d23 = t[2][j] - t[3][j];
        sum += xw_abs(s01 + s23) + xw_abs(d01 + d23) + xw_abs(s01 - s23) + xw_abs(d01 - d23);
    }
    return sum;
}
// satd_8x4 of the differences d[4][8] (reference minus source)
XW_HD int xw_satd_8x4(const int (*d)[8]) { return (xw_had4(d, 0) + xw_had4(d, 4)) >> 1; }

// the (weighted) SATD of one 8x8 block: ref / fenc address its top-left sample
template <typename P>
XW_HD int xw_satd_8x8(const P* ref, int64_t refStride, const P* fenc, int64_t fencStride, const xw_cand& c, int depth)
{
    int satd = 0;
    for (int half = 0; half < 2; half++)
    {
        int d[4][8];
        for (int j = 0; j < 4; j++)
            for (int i = 0; i < 8; i++)
            {
                int v = ref[(int64_t)(half * 4 + j) * refStride + i];
                if (c.present)
                    v = xw_weight(v, c, depth);
                d[j][i] = v - (int)fenc[(int64_t)(half * 4 + j) * fencStride + i];
            }
        satd += xw_satd_8x4(d);
    }
    return satd;
}
// one block of weightCost: luma = min(satd 8x8, intraCost[cu]); chroma = satd 8x8, or satd 16x16 (four 8x8) with bs == 16.  intra NULL: no minimum
template <typename P>
XW_HD uint32_t xw_block_cost(const P* ref, int64_t refStride, const P* fenc, int64_t fencStride, int bs, const int32_t* intra, const xw_cand& c, int depth)
{
    int cost = 0;
    for (int y = 0; y < bs; y += 8)
        for (int x = 0; x < bs; x += 8)
            cost += xw_satd_8x8(ref + (int64_t)y * refStride + x, refStride, fenc + (int64_t)y * fencStride + x, fencStride, c, depth);
    if (intra && *intra < cost)
        cost = *intra;
    return (uint32_t)cost;
}
// the blocks of a plane as weightCost walks them: luma rows of (width + 7) / 8 blocks; chroma width / bs
XW_HD int xw_blocks_x(int width, int bs) { return (width + bs - 1) / bs; }
XW_HD int xw_blocks_y(int height, int bs) { return (height + bs - 1) / bs; }
