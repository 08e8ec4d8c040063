// x265_hip_weightp.cpp — the translation unit of the drop-in that serves the frame encoder's weighted-prediction analysis:
// x265::weightAnalyse (reference source/encoder/weightPrediction.cpp:222-505), which FrameEncoder::compressFrame calls for every P slice with --weightp and
// every B slice with --weightb before the frame's first CTU row may start.  On a picture whose brightness changed it makes, per plane, a motion-compensated
// copy of the reference and up to 46 whole-plane passes (weight_pp + SATD), on one thread.
//
// Every DECISION stays the reference's own compiled code: integration/Makefile compiles weightPrediction.cpp a second time (the reference's flags) with
// weightAnalyse renamed weightAnalyseWp and `primitives` renamed to the private table defined here, a copy of the process's table whose slots the body calls
// are shims.  The body runs as always — float guesses, early termination, the scale and offset loops with their break, the 0.998 test, the denominator
// reduction, the chroma matching, the memcpy into the slice, the border extension of the reference's chroma — and only what it MEASURES comes from the device:
//   compensation slots (cu[8x8].copy_pp, pu[8x8].pixelavg_pp, the five chroma[csp].pu[16x16] slots)   do nothing; they tell which list's reference is read
//   pu[8x8].satd / pu[16x16].satd    the block is found from the source pointer's offset in the frame's plane.  The first block of an unweighted pass opens
//                                    the plane: x265hip_wpcost_set_luma / set_chroma (upload + one compensation launch — for chroma after the body extended
//                                    the borders) and one evaluation; every call returns its block's entry
//   weight_pp                        names the candidate by its arguments; one x265hip_wpcost_eval covers it and the next four offsets of its scale (the body
//                                    walks consecutive offsets from the first one it asks for), so a scale costs one launch
// A call the shims cannot place (a pointer outside the planes, a candidate never evaluated, a refused geometry, a failed call) fails the run: the shims return
// zeros from there on, the result is discarded and the reference's untouched object (weightAnalyseRef, the process's own table) runs from the start.
// The state is thread-local: frame encoders analyse at the same time.  Only the product's encoders link this unit.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#define protected public
#define private public
#include "common.h"
#include "primitives.h"
#include "frame.h"
#include "picyuv.h"
#include "lowres.h"
#include "slice.h"
#include "mv.h"
#undef protected
#undef private

#include "x265hip.h"
#include "x265_hip_debug.h"
#include "../csrc/wpcost.h"

// weak: a library without the entry points leaves every analysis to the reference's body
extern "C" {
int x265hip_wpcost_begin(int depth, int csp, x265hip_wpcost** ctx) __attribute__((weak));
int x265hip_wpcost_set_luma(x265hip_wpcost* ctx, const void* fencPlane, const void* const refPlanes[4], int64_t stride, int width, int lines,
                            const int32_t* intraCost, const int32_t* mvs) __attribute__((weak));
int x265hip_wpcost_set_chroma(x265hip_wpcost* ctx, int plane, const void* fencPlane, const void* refPlane, int64_t stride, int width, int height,
                              const int32_t* mvs, int lowresWidthInCU, int lowresHeightInCU) __attribute__((weak));
int x265hip_wpcost_blocks(const x265hip_wpcost* ctx, int plane) __attribute__((weak));
int x265hip_wpcost_eval(x265hip_wpcost* ctx, int plane, const x265hip_weight_param* cand, int n, uint32_t* blockCosts, uint32_t* totals) __attribute__((weak));
void x265hip_wpcost_stats(const x265hip_wpcost* ctx, uint64_t* launches, uint64_t* deviceNs, uint64_t* uploadedBytes) __attribute__((weak));
}

namespace X265_NS {

void weightAnalyseRef(Slice& slice, Frame& frame, x265_param& param);     // weightPrediction_seam.o: the reference's object, its symbol renamed
void weightAnalyseWp(Slice& slice, Frame& frame, x265_param& param);      // weightPrediction_wp.o: the same source through the private table
EncoderPrimitives x265hip_wp_primitives;                                  // ... which is this one

namespace {

std::atomic<int> g_wpState(0);                       // 0 undecided, 1 asked for (X265HIP_WEIGHTP=1), 2 usable and left to the default, -1 off
std::atomic<uint64_t> g_served(0), g_evals(0), g_launches(0), g_deviceNs(0), g_early(0), g_host(0), g_servedNs(0), g_hostNs(0);
std::mutex g_wpLock;
std::once_flag g_tableOnce;
char g_hostWhy[96] = "";

inline uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void wp_report()
{
    const uint64_t s = g_served.load(), h = g_host.load();
    fprintf(stderr, "x265hip: weightp: %llu analyses served, %llu evaluations, %llu launches, %.3f ms on the device, %llu took the early exit, %llu left to the host%s%s"
            " (per analysis: %.3f ms served, %.3f ms on the host)\n", (unsigned long long)s, (unsigned long long)g_evals.load(),
            (unsigned long long)g_launches.load(), g_deviceNs.load() * 1e-6, (unsigned long long)g_early.load(), (unsigned long long)h, g_hostWhy[0] ? ": " : "",
            g_hostWhy, s ? g_servedNs.load() * 1e-6 / s : 0.0, h ? g_hostNs.load() * 1e-6 / h : 0.0);
}

void left_to_host(const char* why)
{
    std::lock_guard<std::mutex> g(g_wpLock);
    if (!g_hostWhy[0])
        snprintf(g_hostWhy, sizeof(g_hostWhy), "%s", why);
}

// X265HIP_WEIGHTP=1 switches the seam on, =0 off; unset: on in the 8-bit and Main10 builds, each by its own measurement (profiles/r16_v1_wpcost_ab.txt,
// DESIGN.md §8); the Main12 build was not measured and ships off
bool wp_on()
{
    int st = g_wpState.load(std::memory_order_acquire);
    if (!st)
    {
        std::lock_guard<std::mutex> g(g_wpLock);
        st = g_wpState.load();
        if (!st)
        {
            const char* env = getenv("X265HIP_WEIGHTP");
            const char* all = getenv("X265HIP");
            const bool usable = !(env && strcmp(env, "1")) && !(all && !strcmp(all, "0")) && x265hip_wpcost_begin && x265hip_wpcost_set_luma &&
                                x265hip_wpcost_set_chroma && x265hip_wpcost_blocks && x265hip_wpcost_eval && x265hip_wpcost_stats && x265hip_device_count() > 0;
            st = !usable ? -1 : (env ? 1 : 2);
            g_wpState.store(st, std::memory_order_release);
        }
    }
    return st == 1 || (st == 2 && (X265_DEPTH == 8 || X265_DEPTH == 10));
}

struct Range
{
    const pixel* lo; const pixel* hi;
    bool has(const void* p) const { return (const pixel*)p >= lo && (const pixel*)p < hi; }
};

// one analysis, on the thread that runs it
struct Run
{
    bool active = false, failed = false, verify = false;
    const char* why = "";
    Slice* slice = nullptr; Frame* frame = nullptr; x265_param* param = nullptr;
    x265hip_wpcost* ctx = nullptr;                   // kept between analyses of the thread
    int ctxCsp = -1;
    int planes = 1, lists = 1, hshift = 0, vshift = 0;
    const pixel* orig[3] = {};                       // the frame's planes as weightCost walks them
    Range fenc[3] = {};
    intptr_t stride[3] = {};
    int width[3] = {}, height[3] = {}, bs[3] = {}, blocksX[3] = {}, blocks[3] = {};
    Range ref[2][2] = {};                            // per list: the reference's lowres buffers, its chroma buffers (cb and cr each)
    Range refCr[2] = {};
    int curList = 0;                                 // the list whose reference the body read last
    bool mcSeen = false;                             // compensation slots ran since the last plane was opened
    int plane = -1, list = 0;                        // the plane that is open
    const int32_t* mvs = nullptr;                    // ... and its vectors
    Range weightTemp = {};                           // where the body's weight_pp writes: a SATD that reads there is a weighted one
    std::vector<uint32_t> unweighted, batch;
    int batchW = 0, batchD = 0, batchO = 0, batchN = 0;
    const uint32_t* cur = nullptr;                   // the block costs of the candidate the body is measuring
    uint64_t evals = 0, opened = 0;
    // X265HIP_VERIFY: the compensated plane on the host
    std::vector<pixel> mc;
};
thread_local Run t_run;

int fail(const char* why)
{
    Run& r = t_run;
    if (!r.failed)
    {
        r.failed = true;
        r.why = why;
    }
    return 0;
}

void touch(const void* p)
{
    Run& r = t_run;
    for (int l = 0; l < r.lists; l++)
        if (r.ref[l][0].has(p) || r.ref[l][1].has(p) || r.refCr[l].has(p))
            r.curList = l;
}

// weightAnalyse's own choice of vectors for a list (weightPrediction.cpp:323-344): integers only
const int32_t* vectors_of(const Run& r, int list)
{
    Frame* refFrame = r.slice->m_refFrameList[list][0];
    const int diffPoc = abs(r.slice->m_poc - refFrame->m_poc);
    if (diffPoc > r.param->bframes + 1)
        return nullptr;
    const MV* mvs = r.frame->m_lowres.lowresMvs[list][diffPoc];
    return mvs[0].x != 0x7FFF ? (const int32_t*)mvs : nullptr;
}

void verify_blocks(Run& r, const x265hip_weight_param* cand, int n, const uint32_t* got)
{
    const int k = r.plane, bs = r.bs[k], nb = r.blocks[k];
    const intptr_t st = r.stride[k];
    for (int i = 0; i < n; i++)
    {
        const xw_cand c = xw_make_cand(X265_DEPTH, cand[i].wtPresent, cand[i].inputWeight, cand[i].inputOffset, cand[i].log2WeightDenom);
        int b = 0;
        for (int y = 0; y < r.height[k]; y += bs)
            for (int x = 0; x < r.width[k]; x += bs, b++)
            {
                const uint32_t want = xw_block_cost<pixel>(r.mc.data() + (size_t)y * st + x, st, r.orig[k] + (size_t)y * st + x, st, bs,
                                                           k ? NULL : r.frame->m_lowres.intraCost + b, c, X265_DEPTH);
                if (want != got[(size_t)i * nb + b])
                {
                    fprintf(stderr, "x265hip: weightp: VERIFY FAILED: poc %d list %d plane %d block %d of candidate %d/%d%+d (present %d): %u, wpcost.h on the host %u\n",
                            r.slice->m_poc, r.list, k, b, cand[i].inputWeight, 1 << cand[i].log2WeightDenom, cand[i].inputOffset, cand[i].wtPresent,
                            got[(size_t)i * nb + b], want);
                    abort();
                }
            }
    }
}

bool evaluate(Run& r, const x265hip_weight_param* cand, int n, std::vector<uint32_t>& out)
{
    uint32_t totals[XW_MAX_CANDS];
    out.resize((size_t)n * r.blocks[r.plane]);
    if (x265hip_wpcost_eval(r.ctx, r.plane, cand, n, out.data(), totals))
    {
        g_wpState.store(-1);
        x265hip_device_failure("weightp", "x265hip_wpcost_eval");
        fail("a device failure");
        return false;
    }
    r.evals += n;
    if (r.verify)
        verify_blocks(r, cand, n, out.data());
    return true;
}

// the first block of an unweighted pass: upload the plane, compensate, evaluate
bool open_plane(Run& r, int k)
{
    const int list = r.curList;
    Frame* refFrame = r.slice->m_refFrameList[list][0];
    Lowres& fenc = r.frame->m_lowres;
    Lowres& refLowres = refFrame->m_lowres;
    const int32_t* mvs = vectors_of(r, list);
    if ((mvs != nullptr) != r.mcSeen)
        return fail("the compensation slots ran against the vectors' state");
    r.mcSeen = false;
    r.plane = k; r.list = list; r.mvs = mvs;
    r.batchN = 0; r.cur = nullptr;
    if (!r.ctx || r.ctxCsp != r.param->internalCsp)
    {
        // (a context per thread, kept: its arenas and its stream outlive the analysis)
        if (x265hip_wpcost_begin(X265_DEPTH, r.param->internalCsp, &r.ctx))
        {
            r.ctx = nullptr;
            g_wpState.store(-1);
            x265hip_device_failure("weightp", "x265hip_wpcost_begin");
            return fail("a device failure");
        }
        r.ctxCsp = r.param->internalCsp;
    }
    int e;
    if (!k)
    {
        const void* refs[4] = { refLowres.lowresPlane[0], refLowres.lowresPlane[1], refLowres.lowresPlane[2], refLowres.lowresPlane[3] };
        e = x265hip_wpcost_set_luma(r.ctx, fenc.lowresPlane[0], refs, fenc.lumaStride, fenc.width, fenc.lines, fenc.intraCost, mvs);
    }
    else
        e = x265hip_wpcost_set_chroma(r.ctx, k, r.orig[k], refFrame->m_fencPic->m_picOrg[k], r.stride[k], r.width[k], r.height[k], mvs, fenc.width >> 3,
                                      fenc.lines >> 3);
    if (e == X265HIP_EINVAL)
        return fail("a geometry the context refuses");
    if (e || x265hip_wpcost_blocks(r.ctx, k) != r.blocks[k])
    {
        if (e)
        {
            g_wpState.store(-1);
            x265hip_device_failure("weightp", k ? "x265hip_wpcost_set_chroma" : "x265hip_wpcost_set_luma");
        }
        return fail(e ? "a device failure" : "a block count that differs");
    }
    r.opened++;
    if (r.verify)
    {
        const intptr_t st = r.stride[k];
        r.mc.assign((size_t)st * r.height[k], 0);
        const pixel* const low[4] = { refLowres.lowresPlane[0], refLowres.lowresPlane[1], refLowres.lowresPlane[2], refLowres.lowresPlane[3] };
        const pixel* src = k ? refFrame->m_fencPic->m_picOrg[k] : low[0];
        for (int y = 0; y < r.height[k]; y++)
            for (int x = 0; x < r.width[k]; x++)
                r.mc[(size_t)y * st + x] = !mvs ? src[(size_t)y * st + x]
                                         : (pixel)(k ? xw_mc_chroma<pixel>(src, st, r.width[k], r.height[k], mvs, fenc.width >> 3, fenc.lines >> 3, r.hshift, r.vshift,
                                                                           X265_DEPTH, x, y)
                                                     : xw_mc_luma<pixel>(low, st, fenc.width, fenc.lines, mvs, x, y));
    }
    const x265hip_weight_param none = { 0, 0, 0, 0 };
    return evaluate(r, &none, 1, r.unweighted);
}

// ---- the shims ----------------------------------------------------------------------------------------------------------------------------------------
int shim_satd(const pixel* ref, intptr_t, const pixel* fencBlock, intptr_t)
{
    Run& r = t_run;
    if (r.failed)
        return 0;
    int k = -1;
    for (int p = 0; p < r.planes; p++)
        if (r.fenc[p].has(fencBlock))
            k = p;
    if (k < 0 || fencBlock < r.orig[k])
        return fail("a SATD outside the frame's planes");
    const intptr_t off = fencBlock - r.orig[k];
    const int y = (int)(off / r.stride[k]), x = (int)(off % r.stride[k]), bs = r.bs[k];
    if (x >= r.width[k] || y >= r.height[k] || x % bs || y % bs)
        return fail("a SATD off the block grid");
    const int b = (y / bs) * r.blocksX[k] + x / bs;
    if (r.weightTemp.has(ref))
    {
        if (k != r.plane || !r.cur)
            return fail("a candidate that was not evaluated");
        return (int)r.cur[b];
    }
    touch(ref);
    if (!b && !open_plane(r, k))
        return 0;
    if (k != r.plane || r.unweighted.size() != (size_t)r.blocks[k])
        return fail("an unweighted pass that did not start at its first block");
    return (int)r.unweighted[b];
}

void shim_weight_pp(const pixel* src, pixel* dst, intptr_t stride, int, int height, int w0, int round, int shift, int offset)
{
    Run& r = t_run;
    if (r.failed)
        return;
    touch(src);
    const int correction = IF_INTERNAL_PREC - X265_DEPTH, d = shift - correction, o = offset >> (X265_DEPTH - 8);
    if (r.plane < 0 || stride != r.stride[r.plane] || height != r.height[r.plane] || d < 0 || d > 7 || w0 < 0 || w0 > 255 || o < -128 || o > 127 ||
        offset != o << (X265_DEPTH - 8) || round != (d ? 1 << (d - 1) : 0) << correction)
    {
        fail("a weight_pp call that names no candidate of the open plane");
        return;
    }
    r.weightTemp.lo = dst; r.weightTemp.hi = dst + stride * height;
    if (!(r.batchN && r.batchW == w0 && r.batchD == d && o >= r.batchO && o < r.batchO + r.batchN))
    {
        // this offset and the next four of the scale: the body's offset loop (weightPrediction.cpp:440-453) walks them in this order
        x265hip_weight_param cand[5];
        int n = 0;
        for (; n < 5 && o + n <= 127; n++)
        {
            cand[n].inputWeight = w0; cand[n].inputOffset = o + n; cand[n].log2WeightDenom = d; cand[n].wtPresent = 1;
        }
        r.batchN = 0; r.cur = nullptr;
        if (!evaluate(r, cand, n, r.batch))
            return;
        r.batchW = w0; r.batchD = d; r.batchO = o; r.batchN = n;
    }
    r.cur = r.batch.data() + (size_t)(o - r.batchO) * r.blocks[r.plane];
}

void shim_copy(pixel*, intptr_t, const pixel* src, intptr_t) { t_run.mcSeen = true; touch(src); }
void shim_avg(pixel*, intptr_t, const pixel* a, intptr_t, const pixel*, intptr_t, int) { t_run.mcSeen = true; touch(a); }
void shim_hpp(const pixel* src, intptr_t, pixel*, intptr_t, int) { t_run.mcSeen = true; touch(src); }
void shim_hps(const pixel* src, intptr_t, int16_t*, intptr_t, int, int) { t_run.mcSeen = true; touch(src); }
void shim_vsp(const int16_t*, intptr_t, pixel*, intptr_t, int) { t_run.mcSeen = true; }

void make_table()
{
    EncoderPrimitives& t = x265hip_wp_primitives;
    t = primitives;
    t.weight_pp = shim_weight_pp;
    t.pu[LUMA_8x8].satd = shim_satd;
    t.pu[LUMA_16x16].satd = shim_satd;
    t.cu[BLOCK_8x8].copy_pp = shim_copy;
    t.pu[LUMA_8x8].pixelavg_pp[NONALIGNED] = shim_avg;
    t.pu[LUMA_8x8].pixelavg_pp[ALIGNED] = shim_avg;
    for (int csp = 0; csp < X265_CSP_COUNT; csp++)
    {
        t.chroma[csp].pu[LUMA_16x16].copy_pp = shim_copy;
        t.chroma[csp].pu[LUMA_16x16].filter_hpp = shim_hpp;
        t.chroma[csp].pu[LUMA_16x16].filter_vpp = shim_hpp;
        t.chroma[csp].pu[LUMA_16x16].filter_hps = shim_hps;
        t.chroma[csp].pu[LUMA_16x16].filter_vsp = shim_vsp;
    }
}

// what the shims need to know about the analysis; false: a geometry left to the host
bool prepare(Run& r, Slice& slice, Frame& frame, x265_param& param)
{
    x265hip_wpcost* ctx = r.ctx;
    const int ctxCsp = r.ctxCsp;
    r = Run();
    r.ctx = ctx; r.ctxCsp = ctxCsp;
    r.slice = &slice; r.frame = &frame; r.param = &param;
    static const bool verify = getenv("X265HIP_VERIFY") != NULL;
    r.verify = verify;
    const int csp = param.internalCsp;
    PicYuv* pic = frame.m_fencPic;
    Lowres& fenc = frame.m_lowres;
    r.planes = csp != X265_CSP_I400 ? 3 : 1;
    r.lists = slice.isInterP() ? 1 : 2;
    r.hshift = CHROMA_H_SHIFT(csp); r.vshift = CHROMA_V_SHIFT(csp);
    if ((int)pic->m_picCsp != csp || fenc.width < 8 || fenc.lines < 8 || (fenc.width & 7) || (fenc.lines & 7) || !fenc.intraCost || !fenc.lowresPlane[0])
        return false;
    // the lowres planes carry the picture's luma margins (lowres.cpp:59-75)
    const int lmX = pic->m_lumaMarginX, lmY = pic->m_lumaMarginY;
    if (lmX < XW_LUMA_HI || lmY < XW_LUMA_HI)
        return false;
    r.orig[0] = fenc.lowresPlane[0]; r.stride[0] = fenc.lumaStride; r.width[0] = fenc.width; r.height[0] = fenc.lines; r.bs[0] = 8;
    r.fenc[0].lo = fenc.lowresPlane[0] - (intptr_t)lmY * fenc.lumaStride - lmX;
    r.fenc[0].hi = r.fenc[0].lo + fenc.lumaStride * (fenc.lines + 2 * lmY);
    for (int k = 1; k < r.planes; k++)
    {
        r.orig[k] = pic->m_picOrg[k]; r.stride[k] = pic->m_strideC;
        r.width[k] = ((pic->m_picWidth >> 4) << 4) >> r.hshift; r.height[k] = ((pic->m_picHeight >> 4) << 4) >> r.vshift;
        r.bs[k] = csp == X265_CSP_I444 ? 16 : 8;
        const int cmX = pic->m_chromaMarginX, cmY = pic->m_chromaMarginY, ch = pic->m_picHeight >> r.vshift, cw = pic->m_picWidth >> r.hshift;
        // what the compensation may read beyond the clamped extents must lie inside the reference's buffers
        if (r.width[k] < 16 >> r.hshift || r.height[k] < 16 >> r.vshift || cmX < XW_CHROMA_LO || cmY < XW_CHROMA_LO ||
            cmX + (cw - r.width[k]) < XW_CHROMA_HI(16 >> r.hshift) || cmY + (ch - r.height[k]) < XW_CHROMA_HI(16 >> r.vshift))
            return false;
        r.fenc[k].lo = pic->m_picOrg[k] - (intptr_t)cmY * pic->m_strideC - cmX;
        r.fenc[k].hi = r.fenc[k].lo + pic->m_strideC * (ch + 2 * cmY);
    }
    for (int k = 0; k < r.planes; k++)
    {
        r.blocksX[k] = r.width[k] / r.bs[k];
        r.blocks[k] = r.blocksX[k] * (r.height[k] / r.bs[k]);
    }
    for (int l = 0; l < r.lists; l++)
    {
        Frame* rf = slice.m_refFrameList[l][0];
        if (!rf || !rf->m_fencPic || (l && rf == slice.m_refFrameList[0][0]))
            return false;
        Lowres& rl = rf->m_lowres;
        PicYuv* rp = rf->m_fencPic;
        if (rl.lumaStride != fenc.lumaStride || rl.width != fenc.width || rl.lines != fenc.lines || !rl.lowresPlane[0] || !rl.lowresPlane[3] ||
            rp->m_strideC != pic->m_strideC || rp->m_picWidth != pic->m_picWidth || rp->m_picHeight != pic->m_picHeight ||
            rp->m_chromaMarginX != pic->m_chromaMarginX || rp->m_chromaMarginY != pic->m_chromaMarginY)
            return false;
        const intptr_t planeSize = fenc.lumaStride * (fenc.lines + 2 * lmY), pad = (intptr_t)lmY * fenc.lumaStride + lmX;
        for (int i = 1; i < 4; i++)
            if (rl.lowresPlane[i] - rl.lowresPlane[0] != i * planeSize)            // lowres.cpp:132-141: one allocation, four planes
                return false;
        r.ref[l][0].lo = rl.lowresPlane[0] - pad; r.ref[l][0].hi = r.ref[l][0].lo + 4 * planeSize;
        if (r.planes == 3)
        {
            const intptr_t cpad = (intptr_t)rp->m_chromaMarginY * rp->m_strideC + rp->m_chromaMarginX;
            const intptr_t csize = rp->m_strideC * ((rp->m_picHeight >> r.vshift) + 2 * rp->m_chromaMarginY);
            r.ref[l][1].lo = rp->m_picOrg[1] - cpad; r.ref[l][1].hi = r.ref[l][1].lo + csize;
            r.refCr[l].lo = rp->m_picOrg[2] - cpad; r.refCr[l].hi = r.refCr[l].lo + csize;
        }
    }
    return true;
}

} // namespace

void weightAnalyse(Slice& slice, Frame& frame, x265_param& param)
{
    static const bool verbose = getenv("X265HIP_VERBOSE") != NULL;
    static std::once_flag once;
    if (verbose)
        std::call_once(once, [] { atexit(wp_report); });
    const uint64_t t0 = now_ns();
    Run& r = t_run;
    const char* why = NULL;
    if (!wp_on())
        why = g_wpState.load() == -1 ? "switched off, or no device" : "off by default in this build (X265HIP_WEIGHTP=1 opts in)";
    else if (!prepare(r, slice, frame, param))
        why = "a geometry the context refuses";
    else
    {
        std::call_once(g_tableOnce, make_table);
        uint64_t l0 = 0, n0 = 0, l1 = 0, n1 = 0;
        if (r.ctx) x265hip_wpcost_stats(r.ctx, &l0, &n0, NULL);
        r.active = true;
        weightAnalyseWp(slice, frame, param);
        r.active = false;
        if (r.ctx) x265hip_wpcost_stats(r.ctx, &l1, &n1, NULL);
        g_launches.fetch_add(l1 - l0, std::memory_order_relaxed);
        g_deviceNs.fetch_add(n1 - n0, std::memory_order_relaxed);
        g_evals.fetch_add(r.evals, std::memory_order_relaxed);
        if (!r.failed)
        {
            if (r.verify)
            {
                // the reference's untouched object on the same slice: it rewrites the whole table (and finds the chroma borders extended already)
                WeightParam got[2][MAX_NUM_REF][3];
                memcpy(got, slice.m_weightPredTable, sizeof(got));
                weightAnalyseRef(slice, frame, param);
                if (memcmp(got, slice.m_weightPredTable, sizeof(got)))
                {
                    fprintf(stderr, "x265hip: weightp: VERIFY FAILED: poc %d: the weight table differs from the reference's\n", slice.m_poc);
                    abort();
                }
            }
            if (r.opened)
            {
                g_served.fetch_add(1, std::memory_order_relaxed);
                g_servedNs.fetch_add(now_ns() - t0, std::memory_order_relaxed);
            }
            else
                g_early.fetch_add(1, std::memory_order_relaxed);
            return;
        }
        why = r.why;
    }
    const uint64_t t1 = now_ns();
    weightAnalyseRef(slice, frame, param);
    g_host.fetch_add(1, std::memory_order_relaxed);
    g_hostNs.fetch_add(now_ns() - t1, std::memory_order_relaxed);
    left_to_host(why);
}

} // namespace X265_NS
