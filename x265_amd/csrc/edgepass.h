// edgepass.h — the arithmetic of the edge pass (x265hip_edge_planes, include/x265hip.h), stated once for the kernel (edgepass.hip), the binding's
// doubt resolution (x265_amd/host/x265_hip_srcplanes.cpp) and the CPU checker (tests/support/edge_ref.cpp).
//
// It restates the reference's edgeFilter + computeEdge (source/encoder/slicetype.cpp:90-215), quirks included:
//   Gaussian   the 5x5 integer kernel / 159, applied where row >= 2 && col >= 2 && row != height-2 && col != width-2 (`!=`, not `<`: row height-1 and
//              column width-1 ARE filtered and read two rows / columns past the picture); everywhere else the Gaussian plane holds the source sample
//   Sobel      on the Gaussian plane, rows 1..height-2, columns 1..width-2; outside that range the edge plane keeps the SOURCE sample and the angle is 0
//   magnitude  sqrtf(h*h + v*v) >= T restated in integers: h*h + v*v >= T*T (|h|, |v| <= 16 * pmax = 65520 at 12 bit: 64-bit sum; near T every term
//              is below 2^24, exact in float, and sqrtf is monotone and exact at T*T)
//   angle      (pixel)theta, theta = float(atan2f(v, h)) * 180 / 3.14159265, + 180 when negative, compiled -ffast-math against the host's libm: no
//              formula here promises that truncation.  A pixel is sorted into one of three classes instead (xe_angle): a SPECIAL direction (value
//              from a table the caller made with the reference's own computeEdge), DOUBTFUL (within XE_DOUBT_BAND of a whole degree: provisional
//              value, listed for the caller to resolve with computeEdge), or plain (int)degrees.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define XE_HD __host__ __device__
#else
#define XE_HD
#endif

#define XE_SPECIALS   9
#define XE_PI_REF     3.14159265            /* slicetype.h:52 */
#define XE_DOUBT_BAND (1.0 / 1024)          /* degrees; the reference's float chain (atan2f, one rounding to float at <= 180) is off by < 1e-4 */

enum { XE_PLAIN = 0, XE_SPECIAL = 1, XE_DOUBTFUL = 2 };

XE_HD static inline int xe_threshold(int depth) { return depth == 8 ? 255 : 1023; }          /* (pixel)EDGE_THRESHOLD, slicetype.h:47-51 */

XE_HD static inline int xe_gauss_applies(int row, int col, int width, int height)
{
    return row >= 2 && col >= 2 && row != height - 2 && col != width - 2;
}

/* the 25 taps grouped by their six weights; p = the centre sample, `stride` in samples */
template <typename P>
XE_HD static inline int xe_gauss25(const P* p, int64_t stride)
{
    const P *r0 = p - 2 * stride, *r1 = p - stride, *r3 = p + stride, *r4 = p + 2 * stride;
    const int w2 = r0[-2] + r0[2] + r4[-2] + r4[2];
    const int w4 = r0[-1] + r0[1] + r1[-2] + r1[2] + r3[-2] + r3[2] + r4[-1] + r4[1];
    const int w5 = r0[0] + p[-2] + p[2] + r4[0];
    const int w9 = r1[-1] + r1[1] + r3[-1] + r3[1];
    const int w12 = r1[0] + p[-1] + p[1] + r3[0];
    return (2 * w2 + 4 * w4 + 5 * w5 + 9 * w9 + 12 * w12 + 15 * p[0]) / 159;
}

/* the Gaussian plane's sample at (col, row) of a width x height picture whose sample (0, 0) is src[0] */
template <typename P>
XE_HD static inline int xe_gauss_at(const P* src, int64_t stride, int col, int row, int width, int height)
{
    const P* p = src + (int64_t)row * stride + col;
    return xe_gauss_applies(row, col, width, height) ? xe_gauss25(p, stride) : (int)p[0];
}

XE_HD static inline int xe_sobel_applies(int row, int col, int width, int height)
{
    return row >= 1 && col >= 1 && row < height - 1 && col < width - 1;
}

/* g = the centre of a 3x3 neighbourhood of the Gaussian plane */
template <typename G>
XE_HD static inline void xe_sobel(const G* g, int64_t stride, int* h, int* v)
{
    const int tl = g[-stride - 1], tm = g[-stride], tr = g[-stride + 1], ml = g[-1], mr = g[1], bl = g[stride - 1], bm = g[stride], br = g[stride + 1];
    *h = 3 * (tr - tl + br - bl) + 10 * (mr - ml);
    *v = 3 * (bl - tl + br - tr) + 10 * (bm - tm);
}

XE_HD static inline int xe_is_edge(int h, int v, int threshold)
{
    return (int64_t)h * h + (int64_t)v * v >= (int64_t)threshold * threshold;
}

/* index into the specials table, or -1: v == 0, h == 0 or |h| == |v| by the signs of (v, h) */
XE_HD static inline int xe_special_index(int h, int v)
{
    const int ah = h < 0 ? -h : h, av = v < 0 ? -v : v;
    if (h && v && ah != av)
        return -1;
    return ((v > 0) - (v < 0) + 1) * 3 + (h > 0) - (h < 0) + 1;
}

/* class of the pixel; *value = the table's entry, the provisional or the final angle */
XE_HD static inline int xe_angle(int h, int v, const uint16_t* specials, int* value)
{
    const int s = xe_special_index(h, v);
    if (s >= 0)
    {
        *value = specials[s];
        return XE_SPECIAL;
    }
    double deg = atan2((double)v, (double)h) * 180.0 / XE_PI_REF;
    if (deg < 0)
        deg += 180.0;
    *value = (int)deg;
    return fabs(deg - floor(deg + 0.5)) < XE_DOUBT_BAND ? XE_DOUBTFUL : XE_PLAIN;
}

/* entries of the doubt list */
XE_HD static inline uint32_t xe_doubt_pack(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }
XE_HD static inline int xe_doubt_x(uint32_t d) { return (int)(d & 0xffff); }
XE_HD static inline int xe_doubt_y(uint32_t d) { return (int)(d >> 16); }
