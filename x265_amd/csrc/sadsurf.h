// sadsurf.h — what the SAD-surface builder (surfbuild.hip) and the kernels it launches (sadsurf.hip) share: the table layout, the kernels' argument
// structs and the launch interface, which is the only way the builder reaches a kernel.  Included by those two files only; not part of the C ABI.
#pragma once
#include "common.h"

namespace xh {

constexpr int kWin = X265HIP_SADSURF_WIN;

struct SurfLayout
{
    int blocksX[4], blocksY[4], per[4], entryBytes[4];
    int64_t originOff[4], tableOff[4];   // byte offsets inside a CTU row's chunk
    int64_t subpelOff[4];                 // sub-pel SATD tables (levels 1..3 when bit 4 of `levels` is set; 0 = not built)
    int64_t pitch;                        // bytes per CTU row
    int ctuCols, ctuRows;
};

// one surface's share of a launch: rows [row0, row0 + rows) of its table
struct SurfJob
{
    const uint8_t* ref; int64_t refStride;       // the job's reference pixel (0, 0): the surfaces of one launch may follow different reference pictures
    const uint8_t* src; int64_t srcPitch;
    char* out;                                    // device table buffer (chunk of CTU row 0 first)
    int S, lambda20, row0, rows;
    int level0;                                   // the 8x8 windows are wanted
};
constexpr int kMaxJobs = 16;

// one launch: rows of up to kMaxJobs surfaces that share the geometry and the table layout (same encoder, same levels) — of one reference picture or several
struct SurfArgs
{
    int picW, picH, marginX, marginY;
    int bufRows;                                  // rows of the padded picture in device memory (marginY above picture row 0)
    int64_t pitch;
    int64_t originOff[4], tableOff[4];
    int blocksX[4];
    int blocksY0;                                 // 8x8 blocks inside the picture, vertically
    int nJobs;
    int xcd;                                      // 1: XCD-aware CTU order (surf_ctu, sadsurf.hip)
    int64_t subpelOff3;                           // >= 0: the CTU's 49 sub-pel SATD entries of the 64x64 level are zeroed (subpel_satd_kernel_lds adds four quadrants into them)
    SurfJob job[kMaxJobs];
};

struct SubpelArgs
{
    const void* pic; const void* planes; int64_t stride, planeElems;        // reference: pixel (0, 0) of the picture / of plane 0; planes 1..15 follow
    const void* src; int64_t srcPitch;                                      // source luma, bytes per row
    char* out;                                                              // the surface's device chunks
    int64_t pitch, originOff[4], subpelOff[4];
    int blocksX[4], blocksY[4], per[4];
    int row0, rows;
    int jobs[4];                                                            // (block, vector) jobs of levels 1..3 in this launch: prefix sums
    int xcd;                                                                // 1: XCD-aware job order (the grid is a multiple of 128)
};

// ---- the launch interface (sadsurf.hip) --------------------------------------------------------------------------------------------------------

// the wide form (16-bit pictures above a range of 16): the surfaces of a launch live in a buffer of device memory that the builder lends it
bool surf16_wide(int depth, int S);

// The 64x64 level's sub-pel entries of these surfaces are SUMS over the block's four quadrants: subpel_satd_kernel_lds adds into them, so the window
// kernel in front of it must have zeroed them.  One value per launch (the surfaces of a launch share levels and depth) and both sides read it:
// SurfArgs::subpelOff3 is set from it, and launch_subpel takes the adding form only where it holds.  Where launch_subpel takes the first form after
// all (X265HIP_SUBPEL_LDS=0, strides that are no multiple of 4 bytes) or the builder skips the tables (a replica without planes), the entries are
// zeroed and then plainly stored or left alone, as they always were.
inline bool subpel_quadrant_sums(int levels, int depth) { return (levels & 16) && (depth == 8 || depth == 10); }

// the dynamic LDS limits of the three window kernels, raised once per device (the current one); false: the runtime refused
bool raise_lds_limits(int dev);

// the window kernel of `depth` for `rows` CTU rows of `cols` CTUs whose largest search range is maxS; wideBuf: wideGroups regions of 16 x (2 maxS)^2 u32
// when surf16_wide(depth, maxS).  False: the launch failed
bool launch_windows(const SurfArgs& a, int depth, int maxS, int cols, int rows, hipStream_t st, char* wideBuf, int wideGroups);

// the sub-pel SATD tables of one surface's rows; B = bytes per sample (the second form wants sa.stride and sa.planeElems to be whole dwords);
// quadrantSums = subpel_quadrant_sums() of the launch whose window kernel went in front.  False: the launch failed
bool launch_subpel(const SubpelArgs& sa, int depth, int B, bool quadrantSums, hipStream_t st);

} // namespace xh
