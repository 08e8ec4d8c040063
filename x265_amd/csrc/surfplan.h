// surfplan.h — the integer rules of the SAD-surface builder (surfbuild.hip) and of the launch interface of its kernels (sadsurf.hip): which rows a
// launch takes and how large its grids are.  Plain ints in, plain ints out; no HIP types and no HIP includes, so that the CPU tier compiles and pins
// them on their own (tests/test_surfplan.py).
#pragma once

namespace xh {
namespace plan {

// every row of the padded reference picture (margin, picture, margin) is on the device
inline bool picture_complete(int uploaded, int marginY, int picH) { return uploaded >= marginY + picH + marginY; }

// CTU rows of a surface that `uploaded` rows of the padded reference picture allow: [rowsBuilt, returned value).  A CTU row needs its 64 picture
// lines and the S lines below them; a complete picture (its bottom margin is there) gives every row.
inline int rows_possible(int rowsBuilt, int ctuRows, int S, int uploaded, int marginY, int picH)
{
    const bool complete = picture_complete(uploaded, marginY, picH);
    const int finalPic = uploaded - marginY;           // picture rows [.., finalPic) are on the device
    int r1 = rowsBuilt;
    while (r1 < ctuRows && (complete || 64 * (r1 + 1) + S <= finalPic))
        r1++;
    return r1;
}

// Whole rounds.  148 KB of LDS = one workgroup per CU: a launch of rows x cols CTUs takes ceil(CTUs / free CUs) rounds of the same duration whatever the
// last round holds.  Rows of pictures that are still arriving — the ones no search is waiting for yet — are left out when they would only open a round
// that stays less than 3/4 full: taken from the last arriving item backwards, and only when the arriving items can give up the whole excess.
// Item: anything with `int take` (rows wanted; trimmed in place) and `bool arriving`.
template <typename Item>
inline void trim_to_rounds(Item* items, int n, int cols, int freeCUs)
{
    int rows = 0, spare = 0;
    for (int k = 0; k < n; k++) { rows += items[k].take; if (items[k].arriving) spare += items[k].take; }
    if (!(cols > 0 && cols <= freeCUs && rows * cols > freeCUs))
        return;
    const int rowsPerRound = freeCUs / cols;
    int excess = rows % rowsPerRound;
    if (!(excess * 4 < rowsPerRound * 3 && excess <= spare))
        return;
    for (int k = n; k-- > 0 && excess > 0;)
        if (items[k].arriving)
        {
            const int d = items[k].take < excess ? items[k].take : excess;
            items[k].take -= d; excess -= d;
        }
}

// the wide form's grid: as many workgroups as the device holds at once (one per free CU), bounded further by `cap` when it is positive, never more than
// the launch has CTUs
inline int wide_groups(int freeCUs, int cap, int total)
{
    int g = freeCUs;
    if (cap > 0 && cap < g) g = cap;
    if (total < g) g = total;
    return g;
}

// sub-pel SATD tables, first form (subpel_satd_kernel): jobs[l] = prefix sums of the (block, vector) jobs of levels 1..3; a wave runs four 16x16 jobs
// or one larger job at once, a workgroup is four waves; the grid is a multiple of 128 (the XCD order's chunks) of at most 4096 workgroups
inline int subpel_waves(const int jobs[4]) { return (jobs[1] + 3) / 4 + (jobs[2] - jobs[1]) + (jobs[3] - jobs[2]); }
inline int subpel_grid(int waves) { return ((waves / 4 + 1 < 4096 ? waves / 4 + 1 : 4096) + 127) & ~127; }

// second form (subpel_satd_kernel_lds): a workgroup per 32x32 quadrant of a 64x64 block, per 32x32 block, per four 16x16 blocks; a multiple of 128 of at
// most 16384 workgroups
inline int subpel_lds_groups(int blocks1, int blocks2, int blocks3) { return 4 * blocks3 + blocks2 + (blocks1 + 3) / 4; }
inline int subpel_lds_grid(int groups) { return ((groups < 16384 ? groups : 16384) + 127) & ~127; }

} // namespace plan
} // namespace xh
