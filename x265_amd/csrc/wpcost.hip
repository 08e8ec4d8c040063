// wpcost.hip — the frame encoder's weighted-prediction analysis (x265hip_wpcost_*, include/x265hip.h): what the reference's weightAnalyse
// (source/encoder/weightPrediction.cpp:222-505) measures on a picture whose brightness changed — a motion-compensated copy of the reference plane (mcLuma over
// the four lowres planes, mcChroma over the full-resolution source chroma) and, per candidate (scale, offset), a weight_pp pass plus a whole-plane SATD pass
// (weightCost).  The arithmetic is wpcost.h's; all of it is integer and independent of the order of the parts.
//
// A context holds, per plane, one device arena and one page-locked staging arena.  set_luma / set_chroma pack the source plane and the windows of the
// reference plane(s) the clipped vectors can reach into the staging (whole rows, never tiles), upload them in one copy and launch the compensation kernel once:
// a lane per sample of the compensated plane.  eval is one launch for all candidates: two lanes own one 8x8 block, load its compensated and source
// samples into registers once and loop over the candidates — weight, an 8x4 SATD each, the minimum with the block's intra cost — writing one word per
// (candidate, block); one download, one synchronisation.  The host adds the totals in block order (and the four 8x8 SATDs of a 4:4:4 chroma block).
// A context serves one thread at a time; contexts are independent of each other.
#include "common.h"
#include "wpcost.h"
#include <cstring>

namespace xh {

struct WpCands { xw_cand c[XW_MAX_CANDS]; };

struct WpMcArgs
{
    const void* ref[4];              // sample (0, 0) of the uploaded window(s): luma the four lowres planes, chroma one plane
    int64_t refStride;
    void* mc; int64_t mcPitch;       // the compensated plane, W x H samples
    const int32_t* mvs;              // NULL: a plain copy of ref[0]
    int width, height, W, H;         // the reference's extents (they enter the clip) and the block-covered extents
    int lwcu, lhcu, hshift, vshift, depth, luma;
};

template <typename P>
__global__ __launch_bounds__(256) void wpcost_mc_kernel(WpMcArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H)
        return;
    int v;
    if (!a.mvs)
        v = ((const P*)a.ref[0])[(int64_t)y * a.refStride + x];
    else if (a.luma)
    {
        const P* const planes[4] = { (const P*)a.ref[0], (const P*)a.ref[1], (const P*)a.ref[2], (const P*)a.ref[3] };
        v = xw_mc_luma<P>(planes, a.refStride, a.width, a.height, a.mvs, x, y);
    }
    else
        v = xw_mc_chroma<P>((const P*)a.ref[0], a.refStride, a.width, a.height, a.mvs, a.lwcu, a.lhcu, a.hshift, a.vshift, a.depth, x, y);
    ((P*)a.mc)[(int64_t)y * a.mcPitch + x] = (P)v;
}

// two lanes per 8x8 block, one per 8x4 half (the unit of x265's SATD): 32 compensated and 32 source samples stay in registers over the candidates; the halves
// meet through one cross-lane move and the even lane writes out[c * nb8 + block]
template <typename P>
__global__ __launch_bounds__(64) void wpcost_eval_kernel(const P* __restrict__ fenc, const P* __restrict__ mc, int64_t pitch, int w8, int nb8,
                                                         const int32_t* __restrict__ intra, const xw_cand* __restrict__ cands, int n, int depth,
                                                         uint32_t* __restrict__ out)
{
    const int id = blockIdx.x * 64 + threadIdx.x, half = id & 1;
    const bool valid = (id >> 1) < nb8;
    const int t = valid ? id >> 1 : nb8 - 1;                                     // (both lanes of a pair share t: they stay or idle together)
    const int by = t / w8, bx = t - by * w8;
    const P* r = mc + (int64_t)(by * 8 + half * 4) * pitch + bx * 8;
    const P* f = fenc + (int64_t)(by * 8 + half * 4) * pitch + bx * 8;
    int rv[4][8], fv[4][8];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 8; i++)
        {
            rv[j][i] = r[(int64_t)j * pitch + i];
            fv[j][i] = f[(int64_t)j * pitch + i];
        }
    const int ic = intra ? intra[t] : 0x7fffffff;
#pragma unroll 1
    for (int c = 0; c < n; c++)
    {
        const xw_cand k = cands[c];                                              // (uniform: scalar loads)
        int d[4][8];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                d[j][i] = (k.present ? xw_weight(rv[j][i], k, depth) : rv[j][i]) - fv[j][i];
        const int mine = xw_satd_8x4(d);
        const int satd = mine + __shfl_xor(mine, 1, kWave);
        if (valid && !half)
            out[(size_t)c * nb8 + t] = (uint32_t)(satd < ic ? satd : ic);
    }
}

struct WpPlane
{
    bool set = false;
    char* d = nullptr; char* h = nullptr; size_t cap = 0;        // device arena, page-locked staging of the same layout
    int W = 0, H = 0, bs = 8, w8 = 0, nb8 = 0, blocks = 0;
    int64_t pitch = 0;
    size_t offFenc = 0, offMc = 0, offIntra = 0, offOut = 0, offCand = 0;
    bool luma = false;
};

} // namespace xh

struct x265hip_wpcost
{
    int depth, csp, B, device;
    hipStream_t st;
    bool inflight, mcTimed;
    hipEvent_t ev[4];                // the compensation kernel's pair and the evaluation kernel's: the context's own device-time ledger
    uint64_t launches, deviceNs, uploaded;
    xh::WpPlane p[3];
};

using namespace xh;

namespace {

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int wp_reserve(x265hip_wpcost* c, WpPlane& p, size_t need)
{
    if (p.cap >= need)
        return X265HIP_OK;
    if (p.d) (void)device_free(p.d);
    if (p.h) (void)hipHostFree(p.h);
    p.d = p.h = nullptr; p.cap = 0;
    if (hipMalloc((void**)&p.d, need) != hipSuccess || hipHostMalloc((void**)&p.h, need, hipHostMallocDefault) != hipSuccess)
        return set_error(X265HIP_ENOMEM, "wpcost: %zu bytes", need);
    p.cap = need;
    return X265HIP_OK;
}

// rows [y0, y1) x columns [x0, x1) of a caller's plane into the staging, tightly
void wp_pack(char* dst, const void* plane, int64_t stride, int B, int x0, int x1, int y0, int y1)
{
    const size_t rowBytes = (size_t)(x1 - x0) * B;
    for (int y = y0; y < y1; y++)
        memcpy(dst + (size_t)(y - y0) * rowBytes, (const char*)plane + ((int64_t)y * stride + x0) * B, rowBytes);
}

int wp_quiet(x265hip_wpcost* c)
{
    if (c->inflight && hipStreamSynchronize(c->st) != hipSuccess)
        return set_error(X265HIP_EHIP, "wpcost: synchronise");
    c->inflight = false;
    return X265HIP_OK;
}

// the common part of set_luma / set_chroma: lay the arena out, pack, upload, compensate
int wp_set_plane(x265hip_wpcost* c, int plane, const void* fenc, const void* const* refs, int nref, int64_t stride, int width, int height, int bs, int lo, int hiX, int hiY,
                 const int32_t* intra, const int32_t* mvs, int nmv, int lwcu, int lhcu)
{
    int e = wp_quiet(c);
    if (e) return e;
    WpPlane& p = c->p[plane];
    const int B = c->B;
    p.set = false;
    p.luma = plane == 0;
    p.bs = bs;
    p.W = xw_blocks_x(width, bs) * bs; p.H = xw_blocks_y(height, bs) * bs;
    p.w8 = p.W / 8; p.nb8 = p.w8 * (p.H / 8);
    p.blocks = (p.W / bs) * (p.H / bs);
    p.pitch = (p.W + 15) & ~15;
    const int winW = lo + width + hiX, winH = lo + height + hiY;
    const size_t planeBytes = align256((size_t)p.pitch * p.H * B), winBytes = align256((size_t)winW * winH * B);
    const size_t intraBytes = align256(intra ? sizeof(int32_t) * p.nb8 : 0), mvBytes = align256(mvs ? sizeof(int32_t) * 2 * nmv : 0);
    // uploaded: source plane, windows, intra costs, vectors; device only: compensated plane, block costs
    p.offFenc = 0;
    const size_t offWin = planeBytes, offIntra = offWin + winBytes * nref, offMv = offIntra + intraBytes, upload = offMv + mvBytes;
    p.offIntra = offIntra;
    p.offMc = upload;
    p.offOut = p.offMc + planeBytes;
    p.offCand = p.offOut + align256(sizeof(uint32_t) * XW_MAX_CANDS * p.nb8);
    const size_t need = p.offCand + align256(sizeof(WpCands));
    if ((e = wp_reserve(c, p, need)))
        return e;
    // the source plane, pitch p.pitch (what lies right of W in a row is never read)
    for (int y = 0; y < p.H; y++)
        memcpy(p.h + ((size_t)y * p.pitch) * B, (const char*)fenc + (int64_t)y * stride * B, (size_t)p.W * B);
    for (int k = 0; k < nref; k++)
        wp_pack(p.h + offWin + winBytes * k, refs[k], stride, B, -lo, width + hiX, -lo, height + hiY);
    if (intra) memcpy(p.h + offIntra, intra, sizeof(int32_t) * p.nb8);
    if (mvs) memcpy(p.h + offMv, mvs, sizeof(int32_t) * 2 * nmv);
    if (hipMemcpyAsync(p.d, p.h, upload, hipMemcpyHostToDevice, c->st) != hipSuccess)
        return set_error(X265HIP_EHIP, "wpcost: upload");
    c->inflight = true;
    WpMcArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < nref; k++)
        a.ref[k] = p.d + offWin + winBytes * k + ((size_t)lo * winW + lo) * B;
    a.refStride = winW;
    a.mc = p.d + p.offMc; a.mcPitch = p.pitch;
    a.mvs = mvs ? (const int32_t*)(p.d + offMv) : nullptr;
    a.width = width; a.height = height; a.W = p.W; a.H = p.H;
    a.lwcu = lwcu; a.lhcu = lhcu;
    a.hshift = c->csp == 1 || c->csp == 2; a.vshift = c->csp == 1;
    a.depth = c->depth; a.luma = plane == 0;
    const dim3 grid((p.W + 63) / 64, (p.H + 3) / 4), block(256);
    c->mcTimed = c->ev[0] && hipEventRecord(c->ev[0], c->st) == hipSuccess;
    if (B == 1) hipLaunchKernelGGL((wpcost_mc_kernel<uint8_t>), grid, block, 0, c->st, a);
    else        hipLaunchKernelGGL((wpcost_mc_kernel<uint16_t>), grid, block, 0, c->st, a);
    XH_LAUNCH_CHECK("wpcost_mc_kernel");
    // (no synchronisation here: the kernel's time is read with the next evaluation's)
    c->mcTimed = c->mcTimed && hipEventRecord(c->ev[1], c->st) == hipSuccess;
    c->launches++;
    c->uploaded += upload;
    p.set = true;
    return X265HIP_OK;
}

} // namespace

extern "C" int x265hip_wpcost_begin(int depth, int csp, x265hip_wpcost** ctx)
{
    XH_CHECK_DEV();
    if (!valid_depth(depth) || csp < 0 || csp > 3 || !ctx)
        return set_error(X265HIP_EINVAL, "wpcost_begin: depth %d, csp %d", depth, csp);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return set_error(X265HIP_EHIP, "wpcost_begin: no current device");
    x265hip_wpcost* c = new x265hip_wpcost();
    c->depth = depth; c->csp = csp; c->B = depth == 8 ? 1 : 2; c->device = dev; c->inflight = false;
    c->st = stream_lease(dev);
    if (!c->st)
    {
        delete c;
        return set_error(X265HIP_EHIP, "wpcost_begin: stream");
    }
    c->mcTimed = false;
    c->launches = c->deviceNs = c->uploaded = 0;
    for (int k = 0; k < 4; k++)
        if (hipEventCreate(&c->ev[k]) != hipSuccess) { (void)hipGetLastError(); c->ev[k] = nullptr; }
    if (!c->ev[1]) c->ev[0] = nullptr;
    if (!c->ev[3]) c->ev[2] = nullptr;
    *ctx = c;
    return X265HIP_OK;
}

extern "C" void x265hip_wpcost_stats(const x265hip_wpcost* c, uint64_t* launches, uint64_t* deviceNs, uint64_t* uploadedBytes)
{
    if (launches) *launches = c ? c->launches : 0;
    if (deviceNs) *deviceNs = c ? c->deviceNs : 0;
    if (uploadedBytes) *uploadedBytes = c ? c->uploaded : 0;
}

extern "C" void x265hip_wpcost_end(x265hip_wpcost* c)
{
    if (!c)
        return;
    (void)hipStreamSynchronize(c->st);
    for (int k = 0; k < 3; k++)
    {
        if (c->p[k].d) (void)device_free(c->p[k].d);
        if (c->p[k].h) (void)hipHostFree(c->p[k].h);
    }
    for (int k = 0; k < 4; k++)
        if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
    stream_return(c->device, c->st);
    delete c;
}

extern "C" int x265hip_wpcost_set_luma(x265hip_wpcost* c, const void* fencPlane, const void* const refPlanes[4], int64_t stride, int width, int lines,
                                       const int32_t* intraCost, const int32_t* mvs)
{
    XH_CHECK_DEV();
    // lines % 8 != 0: the reference's weighted pass reads rows of its scratch plane that weight_pp never wrote; width % 8 != 0 does not occur in a Lowres
    if (!c || !fencPlane || !refPlanes || !refPlanes[0] || (mvs && (!refPlanes[1] || !refPlanes[2] || !refPlanes[3])) || !intraCost || width < 8 || lines < 8 ||
        (width & 7) || (lines & 7) || width > 16384 || lines > 16384 || stride < width + XW_LUMA_LO + XW_LUMA_HI)
        return set_error(X265HIP_EINVAL, "wpcost_set_luma: %d x %d, stride %lld", width, lines, (long long)stride);
    return wp_set_plane(c, 0, fencPlane, refPlanes, mvs ? 4 : 1, stride, width, lines, 8, XW_LUMA_LO, XW_LUMA_HI, XW_LUMA_HI, intraCost, mvs, (width >> 3) * (lines >> 3), 0, 0);
}

extern "C" int x265hip_wpcost_set_chroma(x265hip_wpcost* c, int plane, const void* fencPlane, const void* refPlane, int64_t stride, int width, int height,
                                         const int32_t* mvs, int lowresWidthInCU, int lowresHeightInCU)
{
    XH_CHECK_DEV();
    if (!c || c->csp == 0 || (plane != 1 && plane != 2) || !fencPlane || !refPlane)
        return set_error(X265HIP_EINVAL, "wpcost_set_chroma: plane %d", plane);
    const int hshift = c->csp == 1 || c->csp == 2, vshift = c->csp == 1, bs = c->csp == 3 ? 16 : 8;
    if (width < 16 >> hshift || height < 16 >> vshift || width % (16 >> hshift) || height % (16 >> vshift) || width > 16384 || height > 16384 ||
        stride < width + XW_CHROMA_LO + XW_CHROMA_HI(16 >> hshift) || (mvs && (lowresWidthInCU < 1 || lowresHeightInCU < 1)))
        return set_error(X265HIP_EINVAL, "wpcost_set_chroma: %d x %d, stride %lld, %d x %d lowres blocks", width, height, (long long)stride, lowresWidthInCU,
                         lowresHeightInCU);
    return wp_set_plane(c, plane, fencPlane, &refPlane, 1, stride, width, height, bs, XW_CHROMA_LO, XW_CHROMA_HI(16 >> hshift), XW_CHROMA_HI(16 >> vshift), nullptr, mvs, lowresWidthInCU * lowresHeightInCU,
                        lowresWidthInCU, lowresHeightInCU);
}

extern "C" int x265hip_wpcost_blocks(const x265hip_wpcost* c, int plane)
{
    return c && plane >= 0 && plane < 3 && c->p[plane].set ? c->p[plane].blocks : 0;
}

extern "C" int x265hip_wpcost_eval(x265hip_wpcost* c, int plane, const x265hip_weight_param* cand, int n, uint32_t* blockCosts, uint32_t* totals)
{
    XH_CHECK_DEV();
    if (!c || plane < 0 || plane > 2 || !c->p[plane].set || !cand || n < 1 || n > XW_MAX_CANDS || !totals)
        return set_error(X265HIP_EINVAL, "wpcost_eval: plane %d, %d candidates", plane, n);
    for (int i = 0; i < n; i++)
        if (cand[i].wtPresent && (cand[i].log2WeightDenom < 0 || cand[i].log2WeightDenom > 7 || cand[i].inputWeight < 0 || cand[i].inputWeight > 255 ||
                                  cand[i].inputOffset < -128 || cand[i].inputOffset > 127))
            return set_error(X265HIP_EINVAL, "wpcost_eval: weight %d, offset %d, denominator %d", cand[i].inputWeight, cand[i].inputOffset, cand[i].log2WeightDenom);
    WpPlane& p = c->p[plane];
    // the candidates travel through the staging's tail (its own cells: an upload of set_* still in flight reads others), in front of the launch
    WpCands& k = *(WpCands*)(p.h + p.offCand);
    memset(&k, 0, sizeof(k));
    for (int i = 0; i < n; i++)
        k.c[i] = xw_make_cand(c->depth, cand[i].wtPresent, cand[i].inputWeight, cand[i].inputOffset, cand[i].log2WeightDenom);
    const int32_t* intra = p.luma ? (const int32_t*)(p.d + p.offIntra) : nullptr;
    uint32_t* out = (uint32_t*)(p.d + p.offOut);
    const xw_cand* dCands = (const xw_cand*)(p.d + p.offCand);
    if (hipMemcpyAsync(p.d + p.offCand, &k, sizeof(xw_cand) * n, hipMemcpyHostToDevice, c->st) != hipSuccess)
        return set_error(X265HIP_EHIP, "wpcost_eval: candidates");
    const dim3 grid((p.nb8 * 2 + 63) / 64), block(64);
    const bool timed = c->ev[2] && hipEventRecord(c->ev[2], c->st) == hipSuccess;
    if (c->B == 1)
        hipLaunchKernelGGL((wpcost_eval_kernel<uint8_t>), grid, block, 0, c->st, (const uint8_t*)(p.d + p.offFenc), (const uint8_t*)(p.d + p.offMc), p.pitch, p.w8,
                           p.nb8, intra, dCands, n, c->depth, out);
    else
        hipLaunchKernelGGL((wpcost_eval_kernel<uint16_t>), grid, block, 0, c->st, (const uint16_t*)(p.d + p.offFenc), (const uint16_t*)(p.d + p.offMc), p.pitch, p.w8,
                           p.nb8, intra, dCands, n, c->depth, out);
    XH_LAUNCH_CHECK("wpcost_eval_kernel");
    const bool timed1 = timed && hipEventRecord(c->ev[3], c->st) == hipSuccess;
    c->launches++;
    // the staging's tail (behind everything uploaded) receives the block costs
    uint32_t* hOut = (uint32_t*)(p.h + p.offOut);
    c->inflight = true;
    if (hipMemcpyAsync(hOut, out, sizeof(uint32_t) * (size_t)n * p.nb8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)
        return set_error(X265HIP_EHIP, "wpcost_eval: download");
    c->inflight = false;
    float ms = 0;
    if (timed1 && hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess)
        c->deviceNs += (uint64_t)((double)ms * 1e6);
    if (c->mcTimed && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess)
        c->deviceNs += (uint64_t)((double)ms * 1e6);
    c->mcTimed = false;
    (void)hipGetLastError();
    const int wb = p.W / p.bs;
    for (int i = 0; i < n; i++)
    {
        const uint32_t* src = hOut + (size_t)i * p.nb8;
        uint32_t total = 0;
        for (int b = 0; b < p.blocks; b++)
        {
            uint32_t v;
            if (p.bs == 8)
                v = src[b];
            else
            {
                // satd 16x16 = its four 8x8 SATDs
                const int by = b / wb, bx = b - by * wb, at = by * 2 * p.w8 + bx * 2;
                v = src[at] + src[at + 1] + src[at + p.w8] + src[at + p.w8 + 1];
            }
            total += v;
            if (blockCosts)
                blockCosts[(size_t)i * p.blocks + b] = v;
        }
        totals[i] = total;
    }
    return X265HIP_OK;
}
