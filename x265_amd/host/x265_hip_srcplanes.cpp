// x265_hip_srcplanes.cpp — the fourth translation unit of the drop-in: source-picture energy planes and the psy_cost_pp slots they feed
// (include/x265hip.h, x265hip_source_energy).
//
// cu[].psy_cost_pp(source, sstride, recon, rstride) (reference source/common/pixel.cpp:726-757; RDCost::psyCost, encoder/rdcost.h:114) is the
// psycho-visual term of every RD cost at psy-rd > 0 (preset medium: 2.0).  Per 8x8 block it compares |energy(source) - energy(recon)| with
// energy(b) = sa8d_8x8(b, 0) - (sum(b) >> 2).  The source argument is always a block of the encoder's source-CU cache (Search / Analysis
// pass Mode::fencYuv) — a copy of the source picture — and the same block is asked about dozens of times while a CU's modes are compared.
// energy(source) is a function of the source picture and the position only, so the GPU computes it once per picture for every aligned 8x8
// (and 4x4) block of the three planes, and the slot computes only the reconstruction half.
//
// Knowing WHERE a source-cache block lies in the picture takes three pass-through seams (same link technique as the other seams):
//   PicYuv::copyFromPicture (common/picyuv.cpp:209)   a new picture enters a source buffer: its planes are stale from here on
//   Yuv::copyFromPicYuv     (common/yuv.cpp:100)      Analysis::compressCTU fills the CTU's source cache from the picture (analysis.cpp:154):
//                                                     cache buffer -> (picture, x, y); the picture's planes are built here if they are not yet
//   Yuv::copyPartToYuv      (common/yuv.cpp:155)      a sub-CU's cache is cut out of the CTU's (analysis.cpp:600, ...): child buffer -> position
// Exactness does not rest on that bookkeeping: before a plane value is used, the block handed to the slot is compared byte for byte with the
// picture at the claimed position; equal bytes have equal energy.  Anything that does not check out is computed by the C function.
//
// The same worker also runs the edge pass of --aq-mode 4 (x265hip_edge_planes): the edge and angle planes that the reference's
// edgeFilter (encoder/slicetype.cpp:151-215) computes per frame in the pre-lookahead are built when the picture arrives, and the edgeFilter seam at the end
// of this file copies them into the frame, resolves the listed doubtful angles with the reference's own computeEdge, or calls the reference's body.
// And the edge bits of --rskip 2 (x265hip_scene_stats): the 0 / 1 plane that FrameEncoder::compressFrame (frameencoder.cpp:451-461) has
// computeEdge write into Frame::m_edgeBitPic before the frame's first CTU row starts is built when the picture arrives; the computeEdge seam copies it in.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#define protected public
#define private public
#include "common.h"
#include "picyuv.h"
#include "primitives.h"
#include "yuv.h"
#include "frame.h"
#include "slicetype.h"
#undef protected
#undef private

#include "x265hip.h"
#include "x265_hip_debug.h"
#include "../csrc/scenestats.h"

// weak: the CPU emulation of the ABI (tests/support) that this object is also linked against does not define it; there it is NULL and every frame's edge
// planes are computed by the reference's edgeFilter
extern "C" int x265hip_edge_planes(int depth, const void* hostLuma, int64_t stride, int width, int height, const uint16_t specials[X265HIP_EDGE_SPECIALS],
                                   void* edgeOut, void* thetaOut, int64_t outStride, uint32_t* doubts, int doubtCap, int* doubtCount, void* stream) __attribute__((weak));

// weak, for the same reason: there every frame's edge bits are computed by the reference's computeEdge
extern "C" int x265hip_scene_stats(int depth, int numPlanes, const void* const* hostPlanes, const int* widths, const int* heights, const int64_t* strides,
                                   int sampleBytes, int conv, int shift, int mask, int wantHist, void* edgeBits, int64_t edgeStride,
                                   int32_t* edgeHist, int32_t* yuvHist, uint32_t* rangeErrors, void* stream) __attribute__((weak));

namespace X265_NS {

const EncoderPrimitives& x265hip_c_table();          // x265_hip_primitives.cpp

extern void refCopyFromPicture(PicYuv* self, const x265_picture& pic, const x265_param& param, int padx, int pady)
    asm("_ZN4x2659PicYuvRef15copyFromPictureERK12x265_pictureRK10x265_paramii");
extern void refDestroy(PicYuv* self) asm("_ZN4x2659PicYuvRef7destroyEv");
void x265hip_refplanes_retire(const pixel* lo);     // x265_hip_refplanes.cpp
void edgeFilterRef(Frame* curFrame, x265_param* param);   // the reference's body (slicetype_ref.o, compiled with -DedgeFilter=edgeFilterRef)
// likewise (-DcomputeEdge=computeEdgeRef); edgeFilterRef calls this one
bool computeEdgeRef(pixel* edgePic, pixel* refPic, pixel* edgeTheta, intptr_t stride, int height, int width, bool bcalcTheta, pixel whitePixel);
bool x265hip_sadplanes_wanted();                    // x265_hip_sadplanes.cpp: source pictures are kept on the device for the SAD surfaces
extern void refCopyFromPicYuv(Yuv* self, const PicYuv& srcPic, uint32_t cuAddr, uint32_t absPartIdx) asm("_ZN4x2656YuvRef14copyFromPicYuvERKNS_6PicYuvEjj");
extern void refCopyPartToYuv(const Yuv* self, Yuv& dstYuv, uint32_t absPartIdx) asm("_ZNK4x2656YuvRef13copyPartToYuvERS0_j");

namespace {

struct SrcPic                        // one source picture buffer and its energy planes
{
    std::atomic<const PicYuv*> pic;
    std::atomic<uint32_t> version;   // bumped whenever a new picture is copied into the buffer
    std::atomic<uint32_t> built;     // version the planes below belong to (0 = none)
    std::mutex lock;
    int32_t* e8[3];
    int32_t* e4[3];
    int bw[3], bh[3];                // 8x8 blocks per row / column of each plane
    x265hip_srcpic* dev;             // the luma plane on the device (x265_hip_sadplanes.cpp attaches SAD surfaces to it); version `built`
    int devW, devH;
    // --aq-mode 4: the edge and angle planes of the picture (edgeW x edgeH samples, row pitch edgeW) and its doubtful pixels; version `edgeBuilt`
    bool wantEdge;
    std::mutex edgeLock;             // the buffers below: the worker fills them, the edgeFilter seam copies them out
    pixel* edge; pixel* theta; uint32_t* doubts;
    int edgeW, edgeH, doubtCap, doubtCount;
    std::atomic<uint32_t> edgeBuilt;
    // --rskip 2 without --hist-scenecut and without --aq-mode 4: the 0 / 1 edge plane of the picture (bitsW x bitsH samples, row pitch bitsW; the ring is
    // not defined); version `bitsBuilt`.  Under edgeLock too
    bool wantBits;
    pixel* bits;
    int bitsW, bitsH;
    std::atomic<uint32_t> bitsBuilt;
};

const int kMaxPics = 128;
SrcPic g_pics[kMaxPics];
std::atomic<int> g_npics(0);
std::mutex g_lock;
int g_state = 0;
std::atomic<bool> g_noDeviceCopies(false);   // a source picture could not be copied to the device: no further attempts
EncoderPrimitives g_c;
struct alignas(64) Counter { std::atomic<uint64_t> v; };            // one cache line each: the slots run on every pool worker at once
Counter g_hit[64], g_miss[64];
std::atomic<int> g_shardNext(0);
__attribute__((tls_model("initial-exec"))) thread_local int t_shard = -1;
inline int shard() { if (t_shard < 0) t_shard = g_shardNext.fetch_add(1) & 63; return t_shard; }

// per thread: which source-cache buffers hold which part of which picture
struct CacheMap { const pixel* buf[3]; uint32_t size, csize; SrcPic* sp; uint32_t version; int x, y; };
const int kMaps = 8;
__attribute__((tls_model("initial-exec"))) thread_local CacheMap t_map[kMaps];
__attribute__((tls_model("initial-exec"))) thread_local int t_mapNext = 0;

void report()
{
    uint64_t h = 0, m = 0;
    for (int i = 0; i < 64; i++) { h += g_hit[i].v; m += g_miss[i].v; }
    fprintf(stderr, "x265hip: srcplanes: source half of %llu psy-cost calls served from GPU-built energy planes of %d source buffers, %llu computed on the host\n",
            (unsigned long long)h, g_npics.load(), (unsigned long long)m);
}

bool switched_on()
{
    const char* env = getenv("X265HIP_SRCPLANES");
    const char* all = getenv("X265HIP");
    const char* table = getenv("X265HIP_TABLE");
    return !((env && !strcmp(env, "0")) || (all && !strcmp(all, "0")) || (table && !strcmp(table, "percall")));
}

bool enabled()
{
    if (!g_state)
    {
        std::lock_guard<std::mutex> g(g_lock);
        if (!g_state)
        {
            const char* env = getenv("X265HIP_SRCPLANES");
            const char* all = getenv("X265HIP");
            const char* table = getenv("X265HIP_TABLE");
            if ((env && !strcmp(env, "0")) || (all && !strcmp(all, "0")) || (table && !strcmp(table, "percall")) || x265hip_device_count() < 1)
                g_state = -1;
            else
            {
                g_state = 1;
                if (getenv("X265HIP_VERBOSE"))
                    atexit(report);
            }
        }
    }
    return g_state > 0;
}

SrcPic* find_pic(const PicYuv* pic, bool create)
{
    const int n = g_npics.load(std::memory_order_acquire);
    for (int i = 0; i < n; i++)
        if (g_pics[i].pic.load(std::memory_order_relaxed) == pic)
            return &g_pics[i];
    if (!create)
        return NULL;
    std::lock_guard<std::mutex> g(g_lock);
    const int n2 = g_npics.load();
    for (int i = n; i < n2; i++)
        if (g_pics[i].pic.load() == pic)
            return &g_pics[i];
    for (int i = 0; i < n2; i++)
        if (!g_pics[i].pic.load())                     // the entry of a destroyed buffer (retire() below): its planes are reused or resized by build()
        {
            g_pics[i].pic.store(pic);
            return &g_pics[i];
        }
    if (n2 == kMaxPics)
        return NULL;
    SrcPic& s = g_pics[n2];
    s.pic = pic;
    s.version = 1;
    s.built = 0;
    for (int k = 0; k < 3; k++) { s.e8[k] = s.e4[k] = NULL; s.bw[k] = s.bh[k] = 0; }
    s.dev = NULL; s.devW = s.devH = 0;
    s.wantEdge = false; s.edge = s.theta = NULL; s.doubts = NULL; s.edgeW = s.edgeH = s.doubtCap = s.doubtCount = 0; s.edgeBuilt = 0;
    s.wantBits = false; s.bits = NULL; s.bitsW = s.bitsH = 0; s.bitsBuilt = 0;
    g_npics.store(n2 + 1, std::memory_order_release);
    return &s;
}

// ---- the edge pass of --aq-mode 4
std::atomic<int> g_edgeState(0);                     // 0 undecided, 1 on, -1 off (switch, missing symbol, device failure)
std::atomic<uint64_t> g_edgeServed(0), g_edgeKept(0), g_edgeResolved(0);
uint16_t g_specials[X265HIP_EDGE_SPECIALS];
// the seam waits here (briefly) for a pass that is queued or under way; on the heap and never destroyed, like the queue below
struct EdgeSync { std::mutex lock; std::condition_variable cv; };
EdgeSync& edge_sync() { static EdgeSync* s = new EdgeSync; return *s; }
void edge_wake()
{
    EdgeSync& es = edge_sync();
    { std::lock_guard<std::mutex> g(es.lock); }
    es.cv.notify_all();
}

void edge_report()
{
    fprintf(stderr, "x265hip: edgeplanes: %llu frames served, %llu kept on the host, %llu doubtful pixels resolved\n", (unsigned long long)g_edgeServed.load(),
            (unsigned long long)g_edgeKept.load(), (unsigned long long)g_edgeResolved.load());
}

// the angle the reference gives the centre of a 3x3 patch of the Gaussian plane: its own computeEdge with height = width = 3
inline pixel patch_angle(pixel* patch)
{
    pixel e[9], t[9];
    computeEdge(e, patch, t, 3, 3, 3, true);
    return t[4];
}

// X265HIP_EDGEPLANES=1 switches the pass on, =0 off; unset: on in the 8-bit build, off in the Main10 / Main12 builds (the measured default:
// profiles/r13_v1_edgeplanes_ab.txt)
bool edge_on()
{
    int st = g_edgeState.load(std::memory_order_acquire);
    if (!st)
    {
        std::lock_guard<std::mutex> g(g_lock);
        st = g_edgeState.load();
        if (!st)
        {
            const char* env = getenv("X265HIP_EDGEPLANES");
            st = (env ? !strcmp(env, "1") : X265_DEPTH == 8) && x265hip_edge_planes ? 1 : -1;
            // the nine special directions (v == 0, h == 0, |h| == |v|) from the reference itself: gradients (sh * 10, sv * 10)
            for (int sv = -1; sv <= 1 && st > 0; sv++)
                for (int sh = -1; sh <= 1; sh++)
                {
                    pixel patch[9] = { 0, (pixel)(sv < 0), 0, (pixel)(sh < 0), 0, (pixel)(sh > 0), 0, (pixel)(sv > 0), 0 };
                    g_specials[(sv + 1) * 3 + sh + 1] = patch_angle(patch);
                }
            g_edgeState.store(st, std::memory_order_release);
        }
    }
    return st > 0;
}

// worker thread, sp->lock held: the planes of the picture now in the buffer
void build_edge(SrcPic* sp, const PicYuv& pic, uint32_t v)
{
    const int w = pic.m_picWidth, h = pic.m_picHeight;
    if (w > 65535 || h > 65535)
        return;
    std::lock_guard<std::mutex> g(sp->edgeLock);
    if (sp->edgeW != w || sp->edgeH != h)
    {
        free(sp->edge); free(sp->theta); free(sp->doubts);
        sp->doubtCap = w * h / 64 + 256;               // 1.5 % of the picture; noise has 0.2 %, the bench clip 0.3 % (profiles/r13_v1_edgeplanes_ab.txt)
        sp->edge = (pixel*)malloc((size_t)w * h * sizeof(pixel));
        sp->theta = (pixel*)malloc((size_t)w * h * sizeof(pixel));
        sp->doubts = (uint32_t*)malloc((size_t)sp->doubtCap * 4);
        sp->edgeW = w; sp->edgeH = h;
    }
    if (!sp->edge || !sp->theta || !sp->doubts)
    {
        sp->edgeW = sp->edgeH = 0;
        return;
    }
    if (x265hip_edge_planes(X265_DEPTH, pic.m_picOrg[0], pic.m_stride, w, h, g_specials, sp->edge, sp->theta, w, sp->doubts, sp->doubtCap, &sp->doubtCount, NULL))
    {
        g_edgeState.store(-1);                         // the seam computes every later picture on the host
        edge_wake();
        x265hip_device_failure("edgeplanes", "x265hip_edge_planes");
        return;
    }
    sp->edgeBuilt.store(v, std::memory_order_release);
    edge_wake();
}

// ---- the edge bits of --rskip 2
std::atomic<int> g_bitsState(0);                     // 0 undecided, 1 on, -1 off (switch, missing symbol, device failure)
std::atomic<uint64_t> g_bitsServed(0), g_bitsKept(0);

void bits_report()
{
    fprintf(stderr, "x265hip: edgebits: %llu frames served, %llu kept on the host\n", (unsigned long long)g_bitsServed.load(), (unsigned long long)g_bitsKept.load());
}

// X265HIP_SCENESTATS=1 switches the pass on, =0 off (the switch of the --hist-scenecut seam, x265_hip_scenecut.cpp); unset: off in every build — measured
// inside the off leg's span in the 8-bit and Main10 builds, not measured in the Main12 build (profiles/r14_v1_scenestats_ab.txt)
bool bits_on()
{
    int st = g_bitsState.load(std::memory_order_acquire);
    if (!st)
    {
        const char* env = getenv("X265HIP_SCENESTATS");
        st = (env ? !strcmp(env, "1") : false) && x265hip_scene_stats ? 1 : -1;
        g_bitsState.store(st, std::memory_order_release);
    }
    return st > 0;
}

// worker thread, sp->lock held: the bit plane of the picture now in the buffer
void build_bits(SrcPic* sp, const PicYuv& pic, uint32_t v)
{
    const int w = pic.m_picWidth, h = pic.m_picHeight;
    if (w > 65535 || h > 65535 || w < 3 || h < 3)
        return;
    std::lock_guard<std::mutex> g(sp->edgeLock);
    if (sp->bitsW != w || sp->bitsH != h)
    {
        free(sp->bits);
        sp->bits = (pixel*)malloc((size_t)w * h * sizeof(pixel));
        sp->bitsW = w; sp->bitsH = h;
    }
    if (!sp->bits)
    {
        sp->bitsW = sp->bitsH = 0;
        return;
    }
    const void* plane = pic.m_picOrg[0];
    const int64_t stride = pic.m_stride;
    uint32_t outOfRange = 0;
    if (x265hip_scene_stats(X265_DEPTH, 1, &plane, &w, &h, &stride, (int)sizeof(pixel), X265HIP_CONV_NONE, 0, (1 << X265_DEPTH) - 1, 0, sp->bits, w, NULL, NULL,
                            &outOfRange, NULL))
    {
        g_bitsState.store(-1);                         // the seam computes every later picture on the host
        edge_wake();
        x265hip_device_failure("edgebits", "x265hip_scene_stats");
        return;
    }
    sp->bitsBuilt.store(v, std::memory_order_release);
    edge_wake();
}

// worker thread: the edge pass of a queued picture, ahead of everything else that is queued — the pre-lookahead asks for these planes as soon as the
// picture is in the lookahead's input queue, a CTU asks for the energy planes a whole lookahead later
void edge_first(SrcPic* sp, uint32_t v)
{
    std::lock_guard<std::mutex> g(sp->lock);
    const PicYuv* picp = sp->pic.load();
    if (!picp || sp->version.load() != v)
        return;
    if (sp->wantEdge && g_edgeState.load(std::memory_order_acquire) > 0 && sp->edgeBuilt.load() != v)
        build_edge(sp, *picp, v);
    if (sp->wantBits && g_bitsState.load(std::memory_order_acquire) > 0 && sp->bitsBuilt.load() != v)
        build_bits(sp, *picp, v);
}

// the planes of the picture now in the buffer (worker thread: a picture enters the encoder a whole lookahead before its first CTU is analysed)
void build(SrcPic* sp, uint32_t v)
{
    std::lock_guard<std::mutex> g(sp->lock);           // PicYuv::destroy waits here for a build in progress
    const PicYuv* picp = sp->pic.load();
    if (!picp || sp->version.load() != v)
        return;                                        // the buffer is gone, or a newer picture is already on its way into it
    const PicYuv& pic = *picp;
    const int planes = pic.m_picCsp == X265_CSP_I400 ? 1 : 3;
    for (int k = 0; k < planes; k++)
    {
        const int w = k ? (int)(pic.m_picWidth >> pic.m_hChromaShift) : (int)pic.m_picWidth, h = k ? (int)(pic.m_picHeight >> pic.m_vChromaShift) : (int)pic.m_picHeight;
        const int bw = w >> 3, bh = h >> 3;
        if (bw < 1 || bh < 1)
            return;
        if (sp->bw[k] != bw || sp->bh[k] != bh)
        {
            free(sp->e8[k]);
            free(sp->e4[k]);
            sp->e8[k] = (int32_t*)malloc((size_t)bw * bh * 4);
            sp->e4[k] = (int32_t*)malloc((size_t)bw * bh * 16);
            sp->bw[k] = bw; sp->bh[k] = bh;
        }
        if (x265hip_source_energy(X265_DEPTH, pic.m_picOrg[k], k ? pic.m_strideC : pic.m_stride, w, h, sp->e8[k], sp->e4[k]))
        {
            // these planes are never marked built: the psy slots compute the source half themselves; no further attempts
            g_state = -1;
            x265hip_device_failure("srcplanes", "x265hip_source_energy");
            return;
        }
    }
    if (x265hip_sadplanes_wanted() && !g_noDeviceCopies.load(std::memory_order_relaxed))
    {
        if (sp->dev && (sp->devW != (int)pic.m_picWidth || sp->devH != (int)pic.m_picHeight))
        {
            x265hip_srcpic_destroy(sp->dev);
            sp->dev = NULL;
        }
        if (!sp->dev)
        {
            x265hip_debug_mark("create: device copy of a source picture");
            static std::atomic<int> nextPlace(0);
            const int places = x265hip_places_configured();
            sp->dev = places ? x265hip_srcpic_create_at(nextPlace.fetch_add(1) % places, X265_DEPTH, pic.m_picWidth, pic.m_picHeight)
                             : x265hip_srcpic_create(X265_DEPTH, pic.m_picWidth, pic.m_picHeight);
            x265hip_debug_mark("created: device copy of a source picture");
            sp->devW = pic.m_picWidth; sp->devH = pic.m_picHeight;
        }
        if (!sp->dev || x265hip_srcpic_upload(sp->dev, pic.m_picOrg[0], pic.m_stride))
        {
            // no device copy of this source picture (nor of later ones): no SAD surfaces can be attached to it, the searches use the C functions
            if (sp->dev) { x265hip_srcpic_destroy(sp->dev); sp->dev = NULL; }
            g_noDeviceCopies.store(true);
            x265hip_device_failure("srcplanes", "device copy of a source picture");
        }
    }
    if (sp->version.load() == v)                        // otherwise these planes are simply never used
        sp->built.store(v, std::memory_order_release);
}

struct Job { SrcPic* sp; uint32_t version; };
// the queue lives on the heap and is never destroyed: the worker is detached and may be waiting on it while the process runs its static
// destructors at exit (destroying a condition variable somebody waits on hangs)
struct Queue { std::mutex lock; std::condition_variable cv; std::deque<Job> jobs; bool workerUp = false; };
Queue& queue() { static Queue* q = new Queue; return *q; }

void worker()
{
    Queue& q = queue();
    for (;;)
    {
        Job j;
        std::vector<Job> behind;
        {
            std::unique_lock<std::mutex> g(q.lock);
            q.cv.wait(g, [&q] { return !q.jobs.empty(); });
            j = q.jobs.front();
            q.jobs.pop_front();
            if (g_edgeState.load(std::memory_order_acquire) > 0 || g_bitsState.load(std::memory_order_acquire) > 0)
                behind.assign(q.jobs.begin(), q.jobs.end());
        }
        edge_first(j.sp, j.version);
        for (size_t i = 0; i < behind.size(); i++)
            edge_first(behind[i].sp, behind[i].version);
        build(j.sp, j.version);
    }
}

void enqueue(SrcPic* sp, uint32_t version)
{
    Queue& q = queue();
    {
        std::lock_guard<std::mutex> g(q.lock);
        if (!q.workerUp)
        {
            q.workerUp = true;
            std::thread(worker).detach();              // lives as long as the process; idle when no pictures arrive
        }
        q.jobs.push_back(Job{ sp, version });
    }
    q.cv.notify_one();
}

inline void remember(const Yuv* y, SrcPic* sp, uint32_t version, int px, int py)
{
    int slot = -1;
    for (int i = 0; i < kMaps; i++)
        if (t_map[i].buf[0] == y->m_buf[0]) { slot = i; break; }
    if (slot < 0) { slot = t_mapNext; t_mapNext = (t_mapNext + 1) % kMaps; }
    CacheMap& m = t_map[slot];
    m.buf[0] = y->m_buf[0]; m.buf[1] = y->m_buf[1]; m.buf[2] = y->m_buf[2];
    m.size = y->m_size; m.csize = y->m_csize;
    m.sp = sp; m.version = version; m.x = px; m.y = py;
}

// energy of the source block (N x N, N >= 8: sum over its 8x8 blocks is NOT what psyCost needs — it needs each 8x8 energy — so this returns a
// pointer-free accessor): locate `source` in this thread's source caches, verify the bytes against the picture, return the plane and position
struct Located { const int32_t* e8; const int32_t* e4; int bw; int bx8, by8; };

template <int N>
inline bool locate(const pixel* source, intptr_t sstride, Located& out)
{
    for (int i = 0; i < kMaps; i++)
    {
        const CacheMap& m = t_map[i];
        if (!m.buf[0])
            continue;
        for (int k = 0; k < 3; k++)
        {
            const uint32_t sz = k ? m.csize : m.size;
            if (!m.buf[k] || source < m.buf[k] || source >= m.buf[k] + (size_t)sz * sz || (intptr_t)sz != sstride)
                continue;
            SrcPic* sp = m.sp;
            if (sp->built.load(std::memory_order_acquire) != m.version || sp->version.load(std::memory_order_relaxed) != m.version)
                return false;
            const PicYuv* pic = sp->pic.load(std::memory_order_relaxed);
            const ptrdiff_t off = source - m.buf[k];
            const int oy = (int)(off / sz), ox = (int)(off - (ptrdiff_t)oy * sz);
            const int shx = k ? pic->m_hChromaShift : 0, shy = k ? pic->m_vChromaShift : 0;
            const int x = (m.x >> shx) + ox, y = (m.y >> shy) + oy;
            const int G = N >= 8 ? 8 : 4;
            if ((x | y) & (G - 1))
                return false;
            if (x + N > sp->bw[k] * 8 || y + N > sp->bh[k] * 8)
                return false;
            // equal bytes have equal energy: this comparison, not the bookkeeping above, is what makes the lookup exact
            const intptr_t ps = k ? pic->m_strideC : pic->m_stride;
            const pixel* p = pic->m_picOrg[k] + (intptr_t)y * ps + x;
            for (int r = 0; r < N; r++)
                if (memcmp(source + r * sstride, p + r * ps, N * sizeof(pixel)))
                    return false;
            out.e8 = sp->e8[k]; out.e4 = sp->e4[k]; out.bw = sp->bw[k]; out.bx8 = x >> 3; out.by8 = y >> 3;
            if (N < 8) { out.bx8 = x >> 2; out.by8 = y >> 2; }
            return true;
        }
    }
    return false;
}

static pixel s_zero[8];

template <int N, int CU> int psy_lookup(const pixel* source, intptr_t sstride, const pixel* recon, intptr_t rstride)
{
    Located L;
    if (!locate<N>(source, sstride, L))
    {
        g_miss[shard()].v.fetch_add(1, std::memory_order_relaxed);
        return g_c.cu[CU].psy_cost_pp(source, sstride, recon, rstride);
    }
    g_hit[shard()].v.fetch_add(1, std::memory_order_relaxed);
    if (N == 4)
    {
        const int src = L.e4[(size_t)L.by8 * (L.bw * 2) + L.bx8];
        const int rec = g_c.pu[LUMA_4x4].satd(recon, rstride, s_zero, 0) - (g_c.pu[LUMA_4x4].sad(recon, rstride, s_zero, 0) >> 2);     // pixel.cpp:752-753
        return abs(src - rec);
    }
    uint32_t tot = 0;
    for (int i = 0; i < N; i += 8)
        for (int j = 0; j < N; j += 8)
        {
            const int src = L.e8[(size_t)(L.by8 + (i >> 3)) * L.bw + L.bx8 + (j >> 3)];
            const pixel* r = recon + i * rstride + j;
            const int rec = g_c.cu[BLOCK_8x8].sa8d(r, rstride, s_zero, 0) - (g_c.pu[LUMA_8x8].sad(r, rstride, s_zero, 0) >> 2);          // pixel.cpp:743-744
            tot += abs(src - rec);
        }
    return (int)tot;
}

} // namespace

// x265_hip_sadplanes.cpp (MotionEstimate::setSourcePU): which source picture buffer, and where in it, does this thread's source cache `y` hold?
// *pic / *version name the picture (a buffer is reused for later pictures: the version tells them apart), (*x, *y) the luma position of the
// cache's first sample.  false: not a source cache this thread filled through the seams below.
bool x265hip_srcplanes_where(const Yuv& y, const PicYuv** pic, uint32_t* version, int* px, int* py)
{
    if (g_state <= 0)
        return false;
    for (int i = 0; i < kMaps; i++)
    {
        const CacheMap& m = t_map[i];
        if (m.buf[0] && m.buf[0] == y.m_buf[0] && m.size == y.m_size)
        {
            if (m.sp->version.load(std::memory_order_relaxed) != m.version)
                return false;
            *pic = m.sp->pic.load(std::memory_order_relaxed);
            *version = m.version;
            *px = m.x; *py = m.y;
            return *pic != NULL;
        }
    }
    return false;
}

// x265_hip_sadplanes.cpp: the device copy of source picture `pic` in its version `version` (NULL: not built, or the buffer has moved on)
x265hip_srcpic* x265hip_srcplanes_device(const PicYuv* pic, uint32_t version)
{
    SrcPic* sp = find_pic(pic, false);
    if (!sp || sp->built.load(std::memory_order_acquire) != version || sp->version.load(std::memory_order_relaxed) != version)
        return NULL;
    return sp->dev;
}

// is `version` still the picture in `pic`'s buffer?  (x265_hip_sadplanes.cpp retires the surfaces of pictures that have left)
bool x265hip_srcplanes_current(const PicYuv* pic, uint32_t version)
{
    SrcPic* sp = find_pic(pic, false);
    return sp && sp->version.load(std::memory_order_relaxed) == version;
}

// called by setupAssemblyPrimitives in the default table mode, after the C table is complete
void x265hip_install_psy_slots(EncoderPrimitives& p)
{
    // decided by the switches alone: whether a device exists is known a moment later (setupAssemblyPrimitives probes beside the encoder's own set-up),
    // and without one the wrappers find nothing to serve and call the C functions
    if (!switched_on())
        return;
    if (getenv("X265HIP_SRCPLANES_PSY") && !strcmp(getenv("X265HIP_SRCPLANES_PSY"), "0"))
        return;                                        // the seams and the planes stay, the psy slots keep the C functions (a diagnostic)
    // What the slots did before: the reference's C functions, from a table built for the purpose (x265hip_c_table, x265_hip_primitives.cpp), once.
    // Not a copy of `p`: x265_setup_primitives is not serialised between encoders opened at the same time (primitives.cpp:
    // `if (!primitives.pu[0].sad)`), so `p` may be half filled by another thread or already hold these very wrappers — a wrapper that
    // captured itself would call itself for ever (tests/test_encoder_lifetime.py, concurrent sessions).
    {
        static std::mutex once;
        static bool have = false;
        std::lock_guard<std::mutex> g(once);
        if (!have)
        {
            g_c = x265hip_c_table();
            have = true;
        }
    }
    // cu[BLOCK_4x4].sa8d is aliased to satd_4x4 only later (setupAliasPrimitives, primitives.cpp:139); the lookups call the pu[] slots directly
    p.cu[BLOCK_4x4].psy_cost_pp = psy_lookup<4, BLOCK_4x4>;
    p.cu[BLOCK_8x8].psy_cost_pp = psy_lookup<8, BLOCK_8x8>;
    p.cu[BLOCK_16x16].psy_cost_pp = psy_lookup<16, BLOCK_16x16>;
    p.cu[BLOCK_32x32].psy_cost_pp = psy_lookup<32, BLOCK_32x32>;
    p.cu[BLOCK_64x64].psy_cost_pp = psy_lookup<64, BLOCK_64x64>;
}

void PicYuv::copyFromPicture(const x265_picture& pic, const x265_param& param, int padx, int pady)
{
    SrcPic* sp = enabled() ? find_pic(this, true) : NULL;
    uint32_t v = 0;
    if (sp)
    {
        v = sp->version.fetch_add(1) + 1;              // before the pixels change: nobody may trust the old planes from here on
        sp->wantEdge = param.rc.aqMode == X265_AQ_EDGE && edge_on();
        sp->wantBits = param.recursionSkipMode == EDGE_BASED_RSKIP && !param.bHistBasedSceneCut && param.rc.aqMode != X265_AQ_EDGE && bits_on();
    }
    refCopyFromPicture(this, pic, param, padx, pady);
    if (sp)
        enqueue(sp, v);                                 // the picture is complete (padding included): its planes are built in the background
}

// the buffer goes away (encoder close; a process may open another encoder afterwards, with other picture sizes, and malloc may hand the same
// addresses out again): nothing may keep pointing into it — neither the source-picture entry nor a reference-picture mirror
void PicYuv::destroy()
{
    if (g_state > 0)
        if (SrcPic* sp = find_pic(this, false))
        {
            std::lock_guard<std::mutex> g(sp->lock);
            sp->version.fetch_add(1);                   // queued builds and remembered cache positions of this buffer are void
            sp->built.store(0);
            sp->pic.store(nullptr);
        }
    if (m_picBuf[0])
    {
        x265hip_debug_mark("PicYuv::destroy: retire");
        x265hip_refplanes_retire(m_picBuf[0]);
        x265hip_debug_mark("PicYuv::destroy: retired");
    }
    refDestroy(this);
}

// ---- the edgeFilter seam (weakened in slicetype_seam.o; the call from calcAdaptiveQuantFrame goes through the PLT).  Served: the three full-buffer
// memsets of the reference (blocks that hang over the right and bottom edges read those zeros), the width x height region of both planes from the
// worker's buffers, the listed doubtful angles through computeEdge.  Anything else: the reference's body.
void edgeFilter(Frame* curFrame, x265_param* param)
{
    static const bool verbose = getenv("X265HIP_VERBOSE") != NULL, verify = getenv("X265HIP_VERIFY") != NULL;
    static std::once_flag once;
    if (verbose)
        std::call_once(once, [] { atexit(edge_report); });
    PicYuv* pic = curFrame->m_fencPic;
    SrcPic* sp = g_state > 0 && edge_on() ? find_pic(pic, false) : NULL;
    bool served = false;
    if (sp)
    {
        const uint32_t v = sp->version.load();
        const int w = pic->m_picWidth, h = pic->m_picHeight;
        if (sp->wantEdge && sp->edgeBuilt.load(std::memory_order_acquire) != v)
        {
            // the pass is queued or under way (the pre-lookahead reaches a picture right after it has entered the input queue): worth a wait of up to
            // 10 ns per pixel — the reference's body takes 21-29 ns per pixel (43-60 ms for a 1080p plane)
            EdgeSync& es = edge_sync();
            std::unique_lock<std::mutex> lk(es.lock);
            es.cv.wait_for(lk, std::chrono::microseconds(500 + (int64_t)w * h / 100), [&] {
                return sp->edgeBuilt.load(std::memory_order_acquire) == v || g_edgeState.load() <= 0 || sp->version.load() != v; });
        }
        std::lock_guard<std::mutex> g(sp->edgeLock);
        if (sp->pic.load() == pic && sp->edgeBuilt.load(std::memory_order_acquire) == v && sp->edgeW == w && sp->edgeH == h && sp->doubtCount <= sp->doubtCap)
        {
            const intptr_t stride = pic->m_stride;
            const uint32_t numCuInHeight = (h + param->maxCUSize - 1) / param->maxCUSize;
            const size_t bytes = stride * (numCuInHeight * param->maxCUSize + pic->m_lumaMarginY * 2) * sizeof(pixel);
            memset(curFrame->m_edgePic, 0, bytes);
            memset(curFrame->m_gaussianPic, 0, bytes);
            memset(curFrame->m_thetaPic, 0, bytes);
            const intptr_t org = pic->m_lumaMarginY * stride + pic->m_lumaMarginX;
            pixel* edge = curFrame->m_edgePic + org;
            pixel* theta = curFrame->m_thetaPic + org;
            for (int r = 0; r < h; r++)
            {
                memcpy(edge + r * stride, sp->edge + (size_t)r * w, w * sizeof(pixel));
                memcpy(theta + r * stride, sp->theta + (size_t)r * w, w * sizeof(pixel));
            }
            const pixel* src = pic->m_picOrg[0];
            for (int i = 0; i < sp->doubtCount; i++)
            {
                const int x = xe_doubt_x(sp->doubts[i]), y = xe_doubt_y(sp->doubts[i]);
                pixel patch[9];
                for (int j = 0; j < 9; j++)
                    patch[j] = (pixel)xe_gauss_at(src, (int64_t)stride, x - 1 + j % 3, y - 1 + j / 3, w, h);
                theta[y * stride + x] = patch_angle(patch);
            }
            g_edgeResolved.fetch_add(sp->doubtCount, std::memory_order_relaxed);
            served = true;
            if (verify)
            {
                pixel* e = (pixel*)malloc(bytes);
                pixel* t = (pixel*)malloc(bytes);
                memcpy(e, curFrame->m_edgePic, bytes);
                memcpy(t, curFrame->m_thetaPic, bytes);
                edgeFilterRef(curFrame, param);
                if (memcmp(e, curFrame->m_edgePic, bytes) || memcmp(t, curFrame->m_thetaPic, bytes))
                {
                    fprintf(stderr, "x265hip: edgeplanes: VERIFY FAILED: the planes of a %dx%d picture differ from the reference's edgeFilter (%s plane)\n", w, h,
                            memcmp(e, curFrame->m_edgePic, bytes) ? "edge" : "angle");
                    abort();
                }
                free(e);
                free(t);
            }
        }
    }
    if (served)
        g_edgeServed.fetch_add(1, std::memory_order_relaxed);
    else
    {
        g_edgeKept.fetch_add(1, std::memory_order_relaxed);
        edgeFilterRef(curFrame, param);
    }
}

// ---- the computeEdge seam (weakened in slicetype_seam.o; its body stays reachable as computeEdgeRef).  Served: the call of FrameEncoder::compressFrame for
// --rskip 2 — no angles, whitePixel 1, refPic the luma origin of a registered source picture whose bit plane of the current version is built: rows
// 1 .. height - 2, columns 1 .. width - 2 are copied, so the ring of m_edgeBitPic keeps its bytes as the reference leaves it.  Every other call — the 3x3
// patches of the edge pass above, edgeFilter's, the one of an unserved computeHistograms — goes straight to the reference's body.
bool computeEdge(pixel* edgePic, pixel* refPic, pixel* edgeTheta, intptr_t stride, int height, int width, bool bcalcTheta, pixel whitePixel)
{
    SrcPic* sp = NULL;
    if (!bcalcTheta && whitePixel == 1 && edgePic && refPic && g_state > 0)
    {
        const int n = g_npics.load(std::memory_order_acquire);
        for (int i = 0; i < n && !sp; i++)
        {
            const PicYuv* p = g_pics[i].pic.load(std::memory_order_relaxed);
            if (p && p->m_picOrg[0] == refPic && (int)p->m_picWidth == width && (int)p->m_picHeight == height && p->m_stride == stride)
                sp = &g_pics[i];
        }
    }
    if (!sp)
        return computeEdgeRef(edgePic, refPic, edgeTheta, stride, height, width, bcalcTheta, whitePixel);
    static const bool verbose = getenv("X265HIP_VERBOSE") != NULL, verify = getenv("X265HIP_VERIFY") != NULL;
    static std::once_flag once;
    if (verbose)
        std::call_once(once, [] { atexit(bits_report); });
    bool served = false;
    if (bits_on() && sp->wantBits)
    {
        const uint32_t v = sp->version.load();
        if (sp->bitsBuilt.load(std::memory_order_acquire) != v)
        {
            // the picture has been in the encoder for a whole lookahead: a pass that is still queued or under way is rare, and worth a wait of up to 2 ns per
            // pixel — less than the edgeFilter seam allows itself, as the body it replaces is cheaper (no Gaussian, no angle)
            EdgeSync& es = edge_sync();
            std::unique_lock<std::mutex> lk(es.lock);
            es.cv.wait_for(lk, std::chrono::microseconds(200 + (int64_t)width * height / 500), [&] {
                return sp->bitsBuilt.load(std::memory_order_acquire) == v || g_bitsState.load() <= 0 || sp->version.load() != v; });
        }
        std::lock_guard<std::mutex> g(sp->edgeLock);
        if (sp->bitsBuilt.load(std::memory_order_acquire) == v && sp->version.load() == v && sp->bitsW == width && sp->bitsH == height)
        {
            for (int r = 1; r < height - 1; r++)
                memcpy(edgePic + r * stride + 1, sp->bits + (size_t)r * width + 1, (size_t)(width - 2) * sizeof(pixel));
            served = true;
            if (verify)
            {
                pixel* want = (pixel*)malloc((size_t)stride * height * sizeof(pixel));
                bool same = want && computeEdgeRef(want, refPic, NULL, stride, height, width, false, 1);
                for (int r = 1; same && r < height - 1; r++)
                    same = !memcmp(want + r * stride + 1, edgePic + r * stride + 1, (size_t)(width - 2) * sizeof(pixel));
                if (!same)
                {
                    fprintf(stderr, "x265hip: edgebits: VERIFY FAILED: the edge bits of a %dx%d picture differ from the reference's computeEdge\n", width, height);
                    abort();
                }
                free(want);
            }
        }
    }
    if (served)
    {
        g_bitsServed.fetch_add(1, std::memory_order_relaxed);
        return true;
    }
    g_bitsKept.fetch_add(1, std::memory_order_relaxed);
    return computeEdgeRef(edgePic, refPic, edgeTheta, stride, height, width, bcalcTheta, whitePixel);
}

void Yuv::copyFromPicYuv(const PicYuv& srcPic, uint32_t cuAddr, uint32_t absPartIdx)
{
    refCopyFromPicYuv(this, srcPic, cuAddr, absPartIdx);
    if (!enabled())
        return;
    SrcPic* sp = find_pic(&srcPic, false);             // only buffers that went through copyFromPicture are source pictures
    if (!sp)
        return;
    const ptrdiff_t off = srcPic.getLumaAddr(cuAddr, absPartIdx) - srcPic.m_picOrg[0];
    remember(this, sp, sp->version.load(), (int)(off % srcPic.m_stride), (int)(off / srcPic.m_stride));
}

void Yuv::copyPartToYuv(Yuv& dstYuv, uint32_t absPartIdx) const
{
    refCopyPartToYuv(this, dstYuv, absPartIdx);
    if (g_state <= 0)
        return;
    for (int i = 0; i < kMaps; i++)
        if (t_map[i].buf[0] == m_buf[0] && m_buf[0])
        {
            const CacheMap m = t_map[i];
            remember(&dstYuv, m.sp, m.version, m.x + g_zscanToPelX[absPartIdx], m.y + g_zscanToPelY[absPartIdx]);
            return;
        }
    // not a mapped source cache: prediction / reconstruction buffers use this function too.  A stale entry for dstYuv does no harm — the slot
    // verifies the bytes before it uses a plane value
}

} // namespace X265_NS
