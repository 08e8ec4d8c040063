// surfbuild.hip — the host side of the SAD surfaces behind x265hip_srcpic_* / x265hip_sadsurf_* (include/x265hip.h): source pictures, the surface
// object with its pooled table buffers, replicas of a reference picture at other places, and the builder that follows a reference picture's progress.
//
// One surface = one (source picture, reference picture) pair.  Its tables are built as the reference picture's rows arrive — the refpic worker calls
// sadsurf_rows_arrived after each band — by the kernels of sadsurf.hip, reached through the launch interface of sadsurf.h only, and mirrored into
// page-locked host memory, where x265_amd/host/x265_hip_sadplanes.cpp reads them.  The integer rules (which rows a launch takes, how large its grids
// are) are surfplan.h's.
#include "common.h"
#include "refpic.h"
#include "sadsurf.h"
#include "surfplan.h"
#include <cstring>
#include <map>
#include <tuple>
#include <utility>

struct x265hip_srcpic
{
    int depth = 8, w = 0, h = 0, device = 0;
    int place = -1;                     // x265hip_srcpic_create_at; -(device + 1) for x265hip_srcpic_create
    int64_t pitch = 0;                  // bytes between rows of dLuma
    char* dLuma = nullptr;
    char* hStage = nullptr;             // page-locked staging copy (the encoder's buffer is ordinary memory)
    // (no stream: x265hip_srcpic_upload leases one from the pool, runtime.hip stream_lease)
    std::atomic<int> refs{ 1 };         // the creator's + one per SAD surface attached: a surface reads dLuma and files its buffers under `device` until it is freed,
                                        // so x265hip_srcpic_destroy only drops the creator's reference (a resized source buffer used to free under them)
};
static void srcpic_unref(x265hip_srcpic* sp);

struct x265hip_sadsurf
{
    x265hip_srcpic* src = nullptr;
    x265hip_refpic* ref = nullptr;       // null once the reference picture has gone (under g_ssLock)
    int workerPlace = -1;                // the worker that drives this surface (its reference picture's place)
    xh::Replica* rep = nullptr;          // the reference picture's replica at the source's place; null: the mirror itself (same place).  Worker only
    int S = 32, lambda20 = 0, levels = 14;
    xh::SurfLayout lay;
    char* dBuf = nullptr;                // ctuRows * pitch
    char* hBuf = nullptr;                // page-locked mirror, same layout
    size_t bytes = 0;
    int rowsBuilt = 0;                   // worker only
    std::atomic<int> ctuRowsReady{ 0 };
    x265hip_sadsurf_view view;
    std::atomic<bool> released{ false };
};

namespace xh {

static std::mutex g_ssLock;              // the surfaces lists of the mirrors and x265hip_sadsurf::ref
static std::mutex g_poolLock;
struct PoolEntry { char* d; char* h; };
static std::multimap<std::pair<size_t, int>, PoolEntry> g_pool;      // key: (bytes, device of d)      // table buffers of finished surfaces, by size (pinned allocations are expensive: ~ms)
static std::atomic<uint64_t> g_statAttached{ 0 }, g_statRows{ 0 }, g_statLaunches{ 0 };
static std::atomic<uint64_t> g_statReplicas{ 0 }, g_statPeerBands{ 0 }, g_statPeerBytes{ 0 };

static void layout_for(int w, int h, int depth, int levels, SurfLayout& L)
{
    memset(&L, 0, sizeof(L));
    L.ctuCols = (w + 63) / 64; L.ctuRows = (h + 63) / 64;
    int64_t off = 0;
    for (int l = 0; l < 4; l++)
    {
        if (!(levels >> l & 1))
            continue;                             // level not built: no room in the chunks, blocksX = 0
        const int N = 8 << l;
        L.blocksX[l] = w / N; L.blocksY[l] = h / N; L.per[l] = 64 / N;
        L.entryBytes[l] = (uint64_t)N * N * ((1u << depth) - 1) < 65536 ? 2 : 4;
        L.originOff[l] = off; off += (int64_t)L.per[l] * L.blocksX[l] * 4;
        off = (off + 15) & ~(int64_t)15;
        L.tableOff[l] = off; off += (int64_t)L.per[l] * L.blocksX[l] * kWin * kWin * L.entryBytes[l];
        off = (off + 15) & ~(int64_t)15;
        if (l && (levels & 16))
        {
            L.subpelOff[l] = off; off += (int64_t)L.per[l] * L.blocksX[l] * X265HIP_SADSURF_SUBPEL * 4;
            off = (off + 15) & ~(int64_t)15;
        }
    }
    L.pitch = (off + 255) & ~(int64_t)255;
}

// The wide form's surfaces: one buffer per launch in flight, `groups` regions of 16 x (2 maxS)^2 u32 (256 KB at S = 32).  A launch takes a buffer of its device
// that no other launch holds — the workers of two places on one device, or a replica's stream next to its mirror's, may launch at the same time — and gives it
// back once its stream is synchronised; buffers are kept for the next launch and only ever replaced by larger ones (device allocations cost milliseconds).
struct WideBuf { int dev; size_t bytes; char* d; bool busy; };
static std::vector<WideBuf> g_wide;                     // under g_poolLock
static char* wide_take(int dev, size_t bytes)
{
    char* old = nullptr;
    {
        std::lock_guard<std::mutex> g(g_poolLock);
        size_t small = g_wide.size();
        for (size_t i = 0; i < g_wide.size(); i++)
        {
            WideBuf& b = g_wide[i];
            if (b.busy || b.dev != dev) continue;
            if (b.bytes >= bytes) { b.busy = true; return b.d; }
            small = i;
        }
        if (small < g_wide.size()) { old = g_wide[small].d; g_wide[small] = g_wide.back(); g_wide.pop_back(); }
    }
    if (old) (void)device_free(old);                    // too small and idle: replaced (the caller has made `dev` current)
    char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> g(g_poolLock);
    g_wide.push_back(WideBuf{ dev, bytes, d, true });
    return d;
}
static void wide_return(char* d)
{
    if (!d) return;
    std::lock_guard<std::mutex> g(g_poolLock);
    for (WideBuf& b : g_wide)
        if (b.d == d) b.busy = false;
}

static std::vector<x265hip_sadsurf*> surfaces_of(x265hip_refpic* rp)
{
    std::lock_guard<std::mutex> g(g_ssLock);
    return rp->surfaces;
}

static bool still_arriving(const x265hip_refpic* rp) { return !plan::picture_complete(rp->uploaded, rp->marginY, rp->picH); }

// rows of `ss` that the reference's uploaded rows allow now: [ss->rowsBuilt, returned value)
static int rows_possible(x265hip_sadsurf* ss)
{
    x265hip_refpic* rp = ss->ref;
    if (!rp || rp->failed.load() || ss->released)
        return ss->rowsBuilt;
    return plan::rows_possible(ss->rowsBuilt, ss->lay.ctuRows, ss->S, rp->uploaded, rp->marginY, rp->picH);
}

// the replica of rp at `place`, created on first use (worker thread)
static Replica* replica_at(x265hip_refpic* rp, int place)
{
    for (Replica* r : rp->replicas)
        if (r->place == place) return r;
    const int dev = place_device(place);
    if (dev < 0 || hipSetDevice(dev) != hipSuccess)
        return nullptr;
    Replica* r = new Replica;
    r->place = place; r->device = dev;
    const size_t bytes = (size_t)rp->planeElems * rp->B;
    // (the planes: 16 x the picture, plane 0 unused, as in the mirror itself; without them the replica serves integer-pel surfaces only)
    if (hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess || hipMalloc((void**)&r->dPic, bytes) != hipSuccess)
    {
        if (r->st) (void)hipStreamDestroy(r->st);
        delete r;
        (void)hipSetDevice(rp->device);
        return nullptr;
    }
    if (dev != rp->device)
    {
        // direct access between the two GPUs where the fabric offers it (xGMI inside a node); hipMemcpyPeerAsync works either way
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dev, rp->device) == hipSuccess && can && hipDeviceEnablePeerAccess(rp->device, 0) != hipSuccess)
            (void)hipGetLastError();                       // already enabled
    }
    if (hipMalloc((void**)&r->dPlanes, 16 * bytes) != hipSuccess) { (void)hipGetLastError(); r->dPlanes = nullptr; }
    (void)hipSetDevice(rp->device);
    rp->replicas.push_back(r);
    g_statReplicas++;
    return r;
}

// ---- the builder -----------------------------------------------------------------------------------------------------------------------------
// Build what the references' rows allow of every surface attached to the pictures in `rps` (worker thread; the bands' uploads have been synchronised).
// Surfaces that share geometry, table layout and the device they are built on go into ONE launch, whichever reference picture they follow (a job
// carries its own reference pointer): the three surfaces a P frame attaches within microseconds of each other — one per reference picture — are
// 1530 CTUs together, 7 rounds of the 224 CUs the job server leaves free at 0.98 fill, where three launches of 510 CTUs are 3 rounds each at 0.76.
// Surfaces whose source lives at another place are built from the replica there, after the rows it lacks have been pushed device to device.
//
// 148 KB of LDS = one workgroup per CU: a launch takes ceil(CTUs / free CUs) rounds of the same ~54 us whatever the last round holds.  While a
// reference picture is still arriving, its newest rows — the ones no search is waiting for yet — are left out when they would only open a round that
// stays less than 3/4 full; they go with the next band, or with the picture's last band, which takes everything.  X265HIP_SADSURF_ROUNDS=0: every launch
// takes all it can.
//
// progress_multi reads top to bottom: collect, then per group (take_group) plan::trim_to_rounds and per launch of the group next_launch and
// build_launch (push_replica_rows, fill_layout_args, run_launch, publish).  A step that fails has called set_error and returns false; the reference
// pictures of the group are failed and the worker's device restored in ONE place, progress_multi.
struct SurfItem { x265hip_sadsurf* ss; x265hip_refpic* rp; Replica* rep; int dev; int take; bool arriving; };

// one launch of a group: the window kernel's arguments and, per job, the item it came from and the row its surface will have reached
struct Launch
{
    SurfArgs a; size_t in[kMaxJobs]; int upto[kMaxJobs]; int rows, maxS;
    bool quadrantSums;                  // subpel_quadrant_sums (sadsurf.h) of this launch: the window kernel zeroes what the sub-pel kernel adds into
};

static bool xcd_order()
{
    static const bool on = !(getenv("X265HIP_SADSURF_XCD") && !atoi(getenv("X265HIP_SADSURF_XCD")));
    return on;
}

static void fail_refs(const std::vector<SurfItem>& group)
{
    for (const SurfItem& it : group) it.rp->failed = 1;
}

// the surfaces of `rps` that can advance, in the order of `rps` and of each picture's list
static std::vector<SurfItem> collect(const std::vector<x265hip_refpic*>& rps)
{
    std::vector<SurfItem> items;
    for (x265hip_refpic* rp : rps)
    {
        if (rp->failed.load()) continue;
        const bool arriving = still_arriving(rp);
        for (x265hip_sadsurf* ss : surfaces_of(rp))
        {
            if (ss->ref != rp) continue;
            const int take = rows_possible(ss) - ss->rowsBuilt;
            if (take > 0)
                items.push_back(SurfItem{ ss, rp, ss->rep, ss->rep ? ss->rep->device : rp->device, take, arriving });
        }
    }
    return items;
}

// what the surfaces of one launch share: device, geometry, table layout and the kernel form
struct GroupKey
{
    int dev, levels, depth, picW, picH;
    bool wide;                                            // (a launch is of one kernel form)
    int marginX, marginY, bufRows;
    int64_t pitch;
    auto tied() const { return std::tie(dev, levels, depth, picW, picH, wide, marginX, marginY, bufRows, pitch); }
    bool operator==(const GroupKey& o) const { return tied() == o.tied(); }
};
static GroupKey group_key(const SurfItem& x)
{
    return GroupKey{ x.dev, x.ss->levels, x.rp->depth, x.rp->picW, x.rp->picH, surf16_wide(x.rp->depth, x.ss->S), x.rp->marginX, x.rp->marginY, x.rp->bufRows, x.ss->lay.pitch };
}

// the group of items[a0]: every item not yet used that shares its key, in the order of `items` (groups come in the order of their first item, the
// surfaces inside a group in the order of `rps` and of each picture's list; a pass has a handful of items)
static std::vector<SurfItem> take_group(const std::vector<SurfItem>& items, std::vector<bool>& used, size_t a0)
{
    std::vector<SurfItem> group;
    const GroupKey key = group_key(items[a0]);
    for (size_t b0 = a0; b0 < items.size(); b0++)
        if (!used[b0] && group_key(items[b0]) == key) { used[b0] = true; group.push_back(items[b0]); }
    return group;
}

// the next launch of the group: up to kMaxJobs items from `i` on that still take rows; false: none left
static bool next_launch(const std::vector<SurfItem>& items, size_t& i, Launch& L)
{
    memset(&L, 0, sizeof(L));
    SurfArgs& a = L.a;
    a.xcd = xcd_order() ? 1 : 0;
    for (; i < items.size() && a.nJobs < kMaxJobs; i++)
    {
        const SurfItem& it = items[i];
        if (it.take <= 0)
            continue;
        x265hip_sadsurf* ss = it.ss;
        const char* dPic = it.rep ? it.rep->dPic : it.rp->dPic;
        SurfJob& j = a.job[a.nJobs];
        j.ref = (const uint8_t*)dPic + ((size_t)it.rp->marginY * it.rp->stride + it.rp->marginX) * it.rp->B; j.refStride = it.rp->stride;   // stride in samples
        j.src = (const uint8_t*)ss->src->dLuma; j.srcPitch = ss->src->pitch;
        j.out = ss->dBuf; j.S = ss->S; j.lambda20 = ss->lambda20; j.row0 = ss->rowsBuilt; j.rows = it.take;
        j.level0 = (ss->levels & 1) && it.rp->depth == 8;
        L.in[a.nJobs] = i; L.upto[a.nJobs] = ss->rowsBuilt + it.take;
        L.rows += j.rows;
        if (ss->S > L.maxS) L.maxS = ss->S;
        a.nJobs++;
    }
    return a.nJobs > 0;
}

// the reconstructed rows a replica lacks, straight from the owner's device memory (on the replica's stream, waited for: the launch may run on another
// reference's stream), and the replica's own sub-pel planes of the rows whose support has arrived
static bool push_replica_rows(const SurfItem& it)
{
    x265hip_refpic* rp = it.rp;
    Replica* rep = it.rep;
    if (!rep || rep->copied >= rp->uploaded)
        return true;
    const size_t off = (size_t)rep->copied * rp->stride * rp->B, bytes = (size_t)(rp->uploaded - rep->copied) * rp->stride * rp->B;
    if (hipMemcpyPeerAsync(rep->dPic + off, rep->device, rp->dPic + off, rp->device, bytes, rep->st) != hipSuccess || hipStreamSynchronize(rep->st) != hipSuccess)
    {
        set_error(X265HIP_EHIP, "sadsurf: device-to-device push of reference rows failed");
        return false;
    }
    g_statPeerBands++;
    g_statPeerBytes += bytes;
    rep->copied = rp->uploaded;
    // the planes of the rows whose support (y - 3 .. y + 4) has arrived — the same filter launch as the mirror's band (refpic.hip process()), on the
    // replica's device and stream
    const int phaseEnd = rep->copied - 4;
    if (!rep->dPlanes || phaseEnd <= rep->phaseDone)
        return true;
    const char* org = rep->dPic + ((size_t)rp->marginY * rp->stride + rp->marginX) * rp->B;
    char* porg = rep->dPlanes + ((size_t)rp->marginY * rp->stride + rp->marginX) * rp->B;
    DevSpan spanP(X265HIP_CLK_PLANES, rep->st);
    if (build_subpel_rows(rp->depth, org, rp->stride, -rp->marginX + 4, rp->picW + rp->marginX - 4, rep->phaseDone - rp->marginY, phaseEnd - rp->marginY, porg,
                          rp->planeElems, rep->st) || hipStreamSynchronize(rep->st) != hipSuccess)
    {
        set_error(X265HIP_EHIP, "sadsurf: sub-pel planes of a replica failed");
        return false;
    }
    spanP.end();
    spanP.bytes = (uint64_t)(phaseEnd - rep->phaseDone) * (uint64_t)(rp->picW + 2 * rp->marginX - 8) * 16 * rp->B;
    spanP.commit();
    rep->phaseDone = phaseEnd;
    return true;
}

// geometry and table layout of the launch: its first surface's (same picture size and levels: same layout)
static void fill_layout_args(Launch& L, const SurfItem& first)
{
    SurfArgs& a = L.a;
    const x265hip_refpic* rp0 = first.rp;
    const SurfLayout& lay = first.ss->lay;
    a.picW = rp0->picW; a.picH = rp0->picH; a.marginX = rp0->marginX; a.marginY = rp0->marginY; a.bufRows = rp0->bufRows;
    a.pitch = lay.pitch;
    for (int l = 0; l < 4; l++) { a.originOff[l] = lay.originOff[l]; a.tableOff[l] = lay.tableOff[l]; a.blocksX[l] = lay.blocksX[l]; }
    a.blocksY0 = lay.blocksY[0];
    L.quadrantSums = subpel_quadrant_sums(first.ss->levels, rp0->depth);
    a.subpelOff3 = L.quadrantSums ? lay.subpelOff[3] : -1;
}

// the sub-pel SATD tables of job k's rows (same stream as the window kernel: the origins are there); their algorithmic bytes are added to `bytes`
static bool launch_subpel_job(const SurfItem& it, const SurfArgs& a, int k, bool quadrantSums, hipStream_t st, uint64_t& bytes)
{
    if (!(it.ss->levels & 16) || (it.rep && !it.rep->dPlanes))
        return true;
    const x265hip_refpic* rp = it.rp;
    const SurfLayout& lay = it.ss->lay;
    SubpelArgs sa;
    memset(&sa, 0, sizeof(sa));
    // (a surface at another place than its reference's mirror: the replica's rows and the replica's own planes)
    sa.pic = (it.rep ? it.rep->dPic : rp->dPic) + ((size_t)rp->marginY * rp->stride + rp->marginX) * rp->B;
    sa.planes = (it.rep ? it.rep->dPlanes : rp->dPlanes) + ((size_t)rp->marginY * rp->stride + rp->marginX) * rp->B;
    sa.stride = rp->stride; sa.planeElems = rp->planeElems;
    sa.src = a.job[k].src; sa.srcPitch = a.job[k].srcPitch;
    sa.out = a.job[k].out; sa.pitch = lay.pitch;
    sa.row0 = a.job[k].row0; sa.rows = a.job[k].rows;
    for (int l = 1; l < 4; l++)
    {
        sa.originOff[l] = lay.originOff[l]; sa.subpelOff[l] = lay.subpelOff[l];
        sa.blocksX[l] = lay.blocksX[l]; sa.blocksY[l] = lay.blocksY[l]; sa.per[l] = lay.per[l];
        sa.jobs[l] = sa.jobs[l - 1] + sa.rows * lay.per[l] * lay.blocksX[l] * X265HIP_SADSURF_SUBPEL;
    }
    sa.xcd = xcd_order() ? 1 : 0;
    // satd W x H = 2 W H B per call
    bytes += (uint64_t)sa.rows * lay.ctuCols * 3 * 64 * 64 * X265HIP_SADSURF_SUBPEL * 2 * rp->B;
    return launch_subpel(sa, rp->depth, rp->B, quadrantSums, st);
}

// SURVEY.md §8d, "batched exhaustive search of one block over an R x R window counts the unique footprint", applied to what a workgroup stages: ONE
// 64x64 source block and ONE (64 + R - 1)^2 window per CTU (R = 2 S; the 16x16 / 32x32 / 64x64 searches of the CTU all read that one staging, the
// 32 / 64 SADs are sums of the 16x16 ones), plus the bytes the CTU really emits: a 16 x 16 window of entries and an origin per block of the levels built
// (the surfaces themselves never leave LDS; the wide form's region of device memory is working storage, not counted)
static uint64_t window_bytes(const SurfJob& j, const SurfLayout& lay, int B)
{
    const int64_t R = 2 * j.S;
    uint64_t bytes = (uint64_t)j.rows * lay.ctuCols * (64 * 64 + (64 + R - 1) * (64 + R - 1)) * B;
    for (int l = j.level0 ? 0 : 1; l < 4; l++)
    {
        int blockRows = 0;
        for (int r = j.row0; r < j.row0 + j.rows; r++)
            for (int jj = 0; jj < lay.per[l]; jj++)
                blockRows += r * lay.per[l] + jj < lay.blocksY[l];
        bytes += (uint64_t)blockRows * lay.blocksX[l] * (kWin * kWin * lay.entryBytes[l] + 4);
    }
    return bytes;
}

// The launch itself, between events of its own stream (the kernels' device time: x265hip_device_time, x265hip_sadsurf_stats): the window kernel, the
// sub-pel tables of the rows just built, the copy to the host mirrors, the wait.  The wide form borrows a pooled buffer for as long as the stream works.
static bool run_launch(const std::vector<SurfItem>& items, const Launch& L, int dev, hipStream_t st)
{
    const SurfArgs& a = L.a;
    const SurfItem& first = items[L.in[0]];
    const SurfLayout& lay = first.ss->lay;
    const int depth = first.rp->depth;
    // the wide form: as many workgroups as the device holds at once (one per free CU: 16 waves of 128 registers), each with a region of the pooled buffer;
    // X265HIP_SADSURF_WIDE_GROUPS bounds the grid further (read per launch: the tests walk several CTUs per workgroup on small pictures with it)
    char* wideBuf = nullptr;
    int wideGroups = 0;
    if (surf16_wide(depth, L.maxS))
    {
        const int cap = getenv("X265HIP_SADSURF_WIDE_GROUPS") ? atoi(getenv("X265HIP_SADSURF_WIDE_GROUPS")) : 0;
        wideGroups = plan::wide_groups(free_compute_units(dev), cap, lay.ctuCols * L.rows);
        const size_t bytes = (size_t)wideGroups * 16 * (2 * L.maxS) * (2 * L.maxS) * 4;
        if (!(wideBuf = wide_take(dev, bytes)))
        {
            set_error(X265HIP_ENOMEM, "sadsurf: %zu bytes for the surfaces of a launch at range %d", bytes, L.maxS);
            return false;
        }
    }
    DevSpan span(X265HIP_CLK_SADSURF, st);
    bool bad = !launch_windows(a, depth, L.maxS, lay.ctuCols, L.rows, st, wideBuf, wideGroups);
    span.end();
    DevSpan span2(X265HIP_CLK_SUBPEL, st);
    for (int k = 0; k < a.nJobs && !bad; k++)
        bad = !launch_subpel_job(items[L.in[k]], a, k, L.quadrantSums, st, span2.bytes);
    span2.end();
    for (int k = 0; k < a.nJobs; k++)
        span.bytes += window_bytes(a.job[k], lay, first.rp->B);
    for (int k = 0; k < a.nJobs && !bad; k++)
    {
        x265hip_sadsurf* ss = items[L.in[k]].ss;
        const size_t off = (size_t)a.job[k].row0 * lay.pitch, bytes = (size_t)a.job[k].rows * lay.pitch;
        bad = hipMemcpyAsync(ss->hBuf + off, ss->dBuf + off, bytes, hipMemcpyDeviceToHost, st) != hipSuccess;
    }
    const bool synced = hipStreamSynchronize(st) == hipSuccess && !bad;   // (waited for either way: the pooled buffer goes back only when nothing writes it)
    wide_return(wideBuf);                             // (after a failed synchronisation the reference pictures are failed and nothing launches on them again)
    if (!synced)
    {
        set_error(X265HIP_EHIP, "sadsurf: launch, copy or synchronisation failed");
        return false;
    }
    span.commit();
    if (span2.bytes) span2.commit();
    return true;
}

static void publish(const std::vector<SurfItem>& items, const Launch& L)
{
    g_statRows += L.rows;
    g_statLaunches++;
    for (int k = 0; k < L.a.nJobs; k++)
    {
        x265hip_sadsurf* ss = items[L.in[k]].ss;
        ss->rowsBuilt = L.upto[k];
        ss->ctuRowsReady.store(L.upto[k], std::memory_order_release);
    }
}

// one launch from the device switch to the published rows, on the device and stream of its first surface (leaves that device current)
static bool build_launch(const std::vector<SurfItem>& items, Launch& L)
{
    const SurfItem& first = items[L.in[0]];
    if (hipSetDevice(first.dev) != hipSuccess)
        return false;
    for (int k = 0; k < L.a.nJobs; k++)
        if (!push_replica_rows(items[L.in[k]]))
            return false;
    fill_layout_args(L, first);
    if (!raise_lds_limits(first.dev))
    {
        set_error(X265HIP_EHIP, "sadsurf: cannot raise the dynamic LDS limit");
        return false;
    }
    if (!run_launch(items, L, first.dev, first.rep ? first.rep->st : first.rp->st))
        return false;
    publish(items, L);
    return true;
}

static void progress_multi(const std::vector<x265hip_refpic*>& rps)
{
    static const bool rounds = !(getenv("X265HIP_SADSURF_ROUNDS") && !atoi(getenv("X265HIP_SADSURF_ROUNDS")));
    const std::vector<SurfItem> items = collect(rps);
    std::vector<bool> used(items.size(), false);
    for (size_t a0 = 0; a0 < items.size(); a0++)
    {
        if (used[a0]) continue;
        std::vector<SurfItem> group = take_group(items, used, a0);
        // whole rounds: rows of pictures that are still arriving may stay behind
        if (rounds)
            plan::trim_to_rounds(group.data(), (int)group.size(), group[0].ss->lay.ctuCols, free_compute_units(group[0].dev));
        Launch L;
        for (size_t i = 0; next_launch(group, i, L);)
        {
            const bool built = build_launch(group, L);
            (void)hipSetDevice(group[L.in[0]].rp->device);    // the worker's own device again, whatever became of the launch
            if (!built)
            {
                fail_refs(group);
                return;
            }
        }
    }
}

// One workgroup per CTU: a band of one CTU row of one or two surfaces fills a fraction of the chip for the same ~54 us as a full one.  A picture that is
// still arriving therefore lets its rows wait for company — until the pending CTUs reach X265HIP_SADSURF_BATCH (default 224), the picture is complete, or
// X265HIP_SADSURF_DEFER bands (default 8) have gone by: the searches of a frame start at least the reference-lag rows behind the band, so nobody is waiting
// for the newest rows yet; a search that does arrive early measures its candidates on the host, same values (round 4's bench clip: 6 k of 12 million
// lookups at 2 bands, 20-25 k at 8 and at 16).  True: leave this picture's rows for later.
static bool rows_wait(x265hip_refpic* rp)
{
    static const int batch = getenv("X265HIP_SADSURF_BATCH") ? atoi(getenv("X265HIP_SADSURF_BATCH")) : 224;
    static const int maxDefer = getenv("X265HIP_SADSURF_DEFER") ? atoi(getenv("X265HIP_SADSURF_DEFER")) : 8;
    if (batch <= 0)
        return false;
    int pending = 0;
    for (x265hip_sadsurf* ss : surfaces_of(rp))
        if (ss->ref == rp)
            pending += (rows_possible(ss) - ss->rowsBuilt) * ss->lay.ctuCols;
    if (still_arriving(rp) && pending < batch && rp->ssDeferred < maxDefer)
    {
        if (pending) rp->ssDeferred++;
        return true;
    }
    rp->ssDeferred = 0;
    return false;
}

void sadsurf_rows_arrived(x265hip_refpic* rp)
{
    if (!rows_wait(rp))
        progress_multi(std::vector<x265hip_refpic*>{ rp });
}

static void free_surface(x265hip_sadsurf* ss)
{
    x265hip_srcpic* src = ss->src;
    {
        std::lock_guard<std::mutex> g(g_poolLock);
        g_pool.insert({ { ss->bytes, src->device }, PoolEntry{ ss->dBuf, ss->hBuf } });
    }
    delete ss;
    ::srcpic_unref(src);
}

// attach jobs that reached the worker together (refpic.hip RefWorker::run): each surface is set up, then the reference pictures concerned make ONE
// pass of progress_multi — the surfaces of one source picture against its two or three reference pictures share a launch
void sadsurf_attach_batch(const std::vector<RefJob>& jobs)
{
    std::vector<x265hip_refpic*> rps;
    for (const RefJob& j : jobs)
    {
        x265hip_sadsurf* ss = j.ss;
        // the worker has seen every band queued before this job, so `uploaded` is what the surface can start from
        if (!ss->ref || j.epoch != ss->ref->epoch.load() || hipSetDevice(ss->ref->device) != hipSuccess)
            continue;
        if (ss->src->place != ss->ref->place && !(ss->rep = replica_at(ss->ref, ss->src->place)))
        {
            set_error(X265HIP_ENOMEM, "sadsurf: no replica of the reference picture at place %d", ss->src->place);
            ss->ref->failed = 1;
            continue;
        }
        bool seen = false;
        for (x265hip_refpic* rp : rps) seen = seen || rp == ss->ref;
        // together with whatever rows the reference's other surfaces are waiting with (a reference picture that is complete — the usual case —
        // gives the new surface all its rows at once)
        if (!seen && !rows_wait(ss->ref)) rps.push_back(ss->ref);
    }
    if (!rps.empty())
        progress_multi(rps);
}

void sadsurf_job(const RefJob& j)
{
    x265hip_sadsurf* ss = j.ss;
    if (j.kind == 1)
    {
        sadsurf_attach_batch(std::vector<RefJob>{ j });
        return;
    }
    // release
    {
        std::lock_guard<std::mutex> g(g_ssLock);
        if (ss->ref)
        {
            auto& v = ss->ref->surfaces;
            for (size_t i = 0; i < v.size(); i++)
                if (v[i] == ss) { v[i] = v.back(); v.pop_back(); break; }
            ss->ref = nullptr;
        }
    }
    free_surface(ss);
}

void sadsurf_detach_all(x265hip_refpic* rp)
{
    std::lock_guard<std::mutex> g(g_ssLock);
    for (x265hip_sadsurf* ss : rp->surfaces)
        ss->ref = nullptr;
    rp->surfaces.clear();
}

} // namespace xh

using namespace xh;

static void srcpic_unref(x265hip_srcpic* sp)
{
    if (sp->refs.fetch_sub(1) != 1) return;
    int cur = 0;
    const bool had = hipGetDevice(&cur) == hipSuccess;
    (void)hipSetDevice(sp->device);
    if (sp->dLuma) (void)device_free(sp->dLuma);
    if (sp->hStage) (void)pinned_free(sp->hStage);
    if (had && cur != sp->device) (void)hipSetDevice(cur);
    delete sp;
}

static x265hip_srcpic* srcpic_create(int place, int depth, int width, int height)
{
    if (!valid_depth(depth) || width < 16 || height < 16 || width > 16384 || height > 16384)
    {
        set_error(X265HIP_EINVAL, "x265hip_srcpic_create: depth %d %dx%d", depth, width, height);
        return nullptr;
    }
    x265hip_srcpic* sp = new x265hip_srcpic;
    sp->depth = depth; sp->w = width; sp->h = height;
    sp->pitch = ((int64_t)width * (depth == 8 ? 1 : 2) + 255) & ~(int64_t)255;
    (void)hipGetDevice(&sp->device);
    sp->place = place;
    const size_t bytes = (size_t)sp->pitch * height;
    // no stream of its own (3.9 ms each, ~40 source pictures alive in a 1080p encoder): the upload leases one
    if (hipMalloc((void**)&sp->dLuma, bytes + 256) != hipSuccess ||
        pinned_alloc((void**)&sp->hStage, bytes) != hipSuccess)
    {
        set_error(X265HIP_ENOMEM, "x265hip_srcpic_create: %zu bytes", bytes);
        x265hip_srcpic_destroy(sp);
        return nullptr;
    }
    return sp;
}

extern "C" {

x265hip_srcpic* x265hip_srcpic_create(int depth, int width, int height)
{
    if (ensure_device()) return nullptr;
    int dev = 0;
    (void)hipGetDevice(&dev);
    return srcpic_create(place_of_device(dev), depth, width, height);
}

x265hip_srcpic* x265hip_srcpic_create_at(int place, int depth, int width, int height)
{
    const int dev = place >= 0 ? place_device(place) : -1;
    if (dev < 0)
    {
        set_error(X265HIP_EINVAL, "x265hip_srcpic_create_at: no place %d (x265hip_places)", place);
        return nullptr;
    }
    int cur = 0;
    const bool had = hipGetDevice(&cur) == hipSuccess;
    if (hipSetDevice(dev) != hipSuccess) { set_error(X265HIP_EHIP, "x265hip_srcpic_create_at: hipSetDevice(%d)", dev); return nullptr; }
    x265hip_srcpic* sp = srcpic_create(place, depth, width, height);
    if (had) (void)hipSetDevice(cur);
    return sp;
}

int x265hip_srcpic_upload(x265hip_srcpic* sp, const void* hostLuma, int64_t stride)
{
    if (!sp || !hostLuma || stride < sp->w) return set_error(X265HIP_EINVAL, "x265hip_srcpic_upload: bad arguments");
    int cur = 0;
    const bool had = hipGetDevice(&cur) == hipSuccess;
    int e = check_hip(hipSetDevice(sp->device), "hipSetDevice");
    if (e) return e;
    const size_t B = sp->depth == 8 ? 1 : 2;                 // `stride` counts samples, like every stride of the ABI
    for (int y = 0; y < sp->h; y++)
        memcpy(sp->hStage + (size_t)y * sp->pitch, (const char*)hostLuma + (size_t)y * stride * B, sp->w * B);
    hipStream_t st = stream_lease(sp->device);
    if (!st) e = set_error(X265HIP_EHIP, "x265hip_srcpic_upload: no stream");
    else
    {
        if (!(e = check_hip(hipMemcpyAsync(sp->dLuma, sp->hStage, (size_t)sp->pitch * sp->h, hipMemcpyHostToDevice, st), "srcpic h2d")))
            e = check_hip(hipStreamSynchronize(st), "srcpic sync");
        stream_return(sp->device, st);
    }
    if (had && cur != sp->device) (void)hipSetDevice(cur);
    return e;
}

void x265hip_srcpic_destroy(x265hip_srcpic* sp)
{
    if (sp) srcpic_unref(sp);
}

x265hip_sadsurf* x265hip_sadsurf_attach(x265hip_srcpic* src, x265hip_refpic* ref, int searchRange, int lambda20)
{
    return x265hip_sadsurf_attach_levels(src, ref, searchRange, lambda20, 14);
}

x265hip_sadsurf* x265hip_sadsurf_attach_levels(x265hip_srcpic* src, x265hip_refpic* ref, int searchRange, int lambda20, int levels)
{
    if (ensure_device()) return nullptr;
    if (!src || !ref || src->depth != ref->depth || src->w != ref->picW || src->h != ref->picH || searchRange < 8 || searchRange > 32 || (searchRange & 3) ||
        lambda20 < 0 || lambda20 > (1 << 20) || ref->marginX < searchRange + 8 || ref->marginY < searchRange || (levels & ~31) || (levels & 14) != 14 || ((levels & 1) && src->depth != 8))
    {
        set_error(X265HIP_EINVAL, "x265hip_sadsurf_attach: pictures do not match, or range %d (8..32, a multiple of 4) / lambda %d / margins out of bounds", searchRange, lambda20);
        return nullptr;
    }
    x265hip_sadsurf* ss = new x265hip_sadsurf;
    ss->src = src; ss->ref = ref; ss->S = searchRange; ss->lambda20 = lambda20; ss->levels = levels;
    layout_for(src->w, src->h, src->depth, levels, ss->lay);
    ss->bytes = (size_t)ss->lay.pitch * ss->lay.ctuRows;
    {
        std::lock_guard<std::mutex> g(g_poolLock);
        auto it = g_pool.find({ ss->bytes, src->device });
        if (it != g_pool.end()) { ss->dBuf = it->second.d; ss->hBuf = it->second.h; g_pool.erase(it); }
    }
    if (!ss->dBuf)
    {
        // the table is written by the kernel that runs where the SOURCE picture lives
        int cur = 0;
        const bool had = hipGetDevice(&cur) == hipSuccess;
        (void)hipSetDevice(src->device);
        const bool ok = hipMalloc((void**)&ss->dBuf, ss->bytes) == hipSuccess && pinned_alloc((void**)&ss->hBuf, ss->bytes) == hipSuccess;
        if (had && cur != src->device) (void)hipSetDevice(cur);
        if (!ok)
        {
            set_error(X265HIP_ENOMEM, "x265hip_sadsurf_attach: %zu bytes", ss->bytes);
            if (ss->dBuf) (void)device_free(ss->dBuf);
            delete ss;
            return nullptr;
        }
    }
    src->refs.fetch_add(1);
    memset(&ss->view, 0, sizeof(ss->view));
    for (int l = 0; l < 4; l++)
    {
        x265hip_sadsurf_level& v = ss->view.level[l];
        if (!(levels >> l & 1))
            continue;                             // origin == NULL: level not built
        v.blocksX = ss->lay.blocksX[l]; v.blocksY = ss->lay.blocksY[l]; v.entryBytes = ss->lay.entryBytes[l]; v.blocksPerCtuRow = ss->lay.per[l];
        v.origin = (const int16_t*)(ss->hBuf + ss->lay.originOff[l]);
        v.table = ss->hBuf + ss->lay.tableOff[l];
        v.subpel = ss->lay.subpelOff[l] ? (const uint32_t*)(ss->hBuf + ss->lay.subpelOff[l]) : nullptr;
    }
    ss->view.ctuRowPitch = ss->lay.pitch;
    ss->view.ctuRowsReady = reinterpret_cast<const int*>(&ss->ctuRowsReady);
    {
        std::lock_guard<std::mutex> g(g_ssLock);
        ref->surfaces.push_back(ss);
    }
    g_statAttached++;
    ss->workerPlace = ref->place;                 // the release must queue behind the attach: same worker
    RefWorker::worker(ref->place).push(RefJob{ ref, 0, ref->epoch.load(), 1, ss });
    return ss;
}

const x265hip_sadsurf_view* x265hip_sadsurf_get_view(x265hip_sadsurf* ss) { return ss ? &ss->view : nullptr; }

void x265hip_sadsurf_release(x265hip_sadsurf* ss)
{
    if (!ss) return;
    ss->released = true;
    RefWorker::worker(ss->workerPlace).push(RefJob{ nullptr, 0, 0, 2, ss });
}

int x265hip_peer_stats(uint64_t* replicas, uint64_t* bands, uint64_t* bytes)
{
    if (replicas) *replicas = g_statReplicas.load();
    if (bands) *bands = g_statPeerBands.load();
    if (bytes) *bytes = g_statPeerBytes.load();
    return X265HIP_OK;
}

int x265hip_sadsurf_stats(uint64_t* attached, uint64_t* ctuRows, uint64_t* launches, uint64_t* kernelNs)
{
    if (kernelNs) (void)x265hip_device_time(X265HIP_CLK_SADSURF, nullptr, kernelNs, nullptr);
    if (launches) *launches = g_statLaunches.load();
    if (attached) *attached = g_statAttached.load();
    if (ctuRows) *ctuRows = g_statRows.load();
    return X265HIP_OK;
}

} // extern "C"
