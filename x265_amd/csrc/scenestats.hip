// scenestats.hip — the per-picture statistics of --hist-scenecut and the edge bits of --rskip 2 (x265hip_scene_stats, include/x265hip.h): what the
// reference's Encoder::computeHistograms (source/encoder/encoder.cpp:1361-1487) and the computeEdge call of FrameEncoder::compressFrame
// (frameencoder.cpp:451-461) compute on the host, as one launch group.  The arithmetic is scenestats.h's (and through it edgepass.h's); all of it is integer.
//
// One kernel, two kinds of workgroup (256 threads each):
//   luma     workgroups 0 .. lumaBlocks-1 walk the 64 x 16 tiles of the luma plane (grid-stride).  The device copy is padded to whole tiles plus a halo
//            (sample (0, 0) at row 1, column kPadX), so no load or store needs a bounds check.  Tile + halo are CONVERTED into LDS as uint16 (18 rows x 72
//            samples, rows 36 dwords apart as in edgepass.hip); a thread takes 4 horizontally adjacent pixels: Sobel pair, h^2 + v^2 >= T^2, one 4-sample
//            vector store of the bits when they are wanted, popcount -> wave sum -> one add per workgroup for the edge count, and the 4 samples into the
//            histogram
//   chroma   the following workgroups read the U / V planes (packed, a linear array) with 16-byte loads, histogram only
// Histograms are integer counts: exact whatever the arrival order.  A workgroup keeps one private histogram per wave and replica in LDS (8 replicas of
// 256 bins or 2 of 1024 per wave, the replica chosen by the lane); a thread merges equal adjacent samples into one add, and a wave all of whose samples are equal (a flat picture: every sample of the
// chip goes to one bin) makes ONE add.  At the end the copies are summed per bin and every non-zero bin leaves by one global integer atomic (measured
// against per-workgroup slabs with a sum pass, which took five times as long: profiles/r14_v1_scenestats_kernel.txt).
#include "common.h"
#include "scenestats.h"
#include <cstring>

namespace xh {

constexpr int kSsTileW = 64, kSsTileH = 16, kSsPadX = 4;
constexpr int kSsStageW = kSsTileW + 2 * kSsPadX, kSsStageH = kSsTileH + 2;       // 72 x 18
constexpr int kSsHistWords = 2048;                                                // per wave: replicas x bins (8 x 256 or 2 x 1024)
constexpr int kSsMaxBins = 1024;
constexpr int kSsLumaBlocksMax = 512, kSsChromaBlocksMax = 128;

struct SceneArgs
{
    const void* src[3];              // device copies: luma padded (pitch lumaPitch, sample (0, 0) at row 1, column kSsPadX), chroma packed
    int width[3], height[3];
    int lumaPitch, tilesX, tilesY, lumaBlocks, chromaBlocks, planes;
    int conv, shift, mask, pixelBytes, bins, wantHist, threshold;
    void* bits; int bitsPitch;       // NULL: not wanted
    int32_t* hist;                   // planes x bins
    unsigned* counters;              // [0] edge count, [1] range errors
};

// one add of `n` to bin `v` of the wave's replica; samples outside the bins are range errors
__device__ __forceinline__ void ss_add(int* H, int bins, int v, int n, int& rangeErr)
{
    if (v < bins) atomicAdd(&H[v], n);
    else rangeErr += n;
}

// the thread's `count` samples v[0..count-1] (count <= N; all N when full) into the histogram: equal adjacent samples are one add; a wave whose every
// sample is the same value makes one add
template <int N>
__device__ __forceinline__ void ss_hist_add(int* Hwave, int* Hrep, int bins, const int v[N], int count, int& rangeErr)
{
    bool same = count == N;
#pragma unroll
    for (int k = 1; k < N; k++)
        same = same && v[k] == v[0];
    const int first = __shfl(v[0], 0, kWave);
    if (__all(same && v[0] == first))
    {
        if ((threadIdx.x & (kWave - 1)) == 0)
            ss_add(Hwave, bins, first, N * kWave, rangeErr);
        return;
    }
    int cur = 0, run = 0;
#pragma unroll
    for (int k = 0; k < N; k++)
        if (k < count)
        {
            if (run && v[k] == cur)
                run++;
            else
            {
                if (run) ss_add(Hrep, bins, cur, run, rangeErr);
                cur = v[k]; run = 1;
            }
        }
    if (run) ss_add(Hrep, bins, cur, run, rangeErr);
}

template <typename S> struct SsVec;                       // a 16-byte load of samples
template <> struct SsVec<uint8_t>  { static constexpr int N = 16; };
template <> struct SsVec<uint16_t> { static constexpr int N = 8; };

template <typename S, typename P>
__global__ __launch_bounds__(256) void scene_stats_kernel(SceneArgs a)
{
    __shared__ __align__(16) uint16_t T[kSsStageH][kSsStageW];
    __shared__ int H[4][kSsHistWords];
    __shared__ unsigned blockEdges, blockErrs;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int bins = a.bins, replicas = kSsHistWords / bins;
    int* Hwave = &H[wave][0];
    int* Hrep = &H[wave][(lane & (replicas - 1)) * bins];
    if (a.wantHist)
        for (int i = tid; i < 4 * kSsHistWords; i += 256)
            (&H[0][0])[i] = 0;
    if (tid == 0) { blockEdges = 0; blockErrs = 0; }
    __syncthreads();
    int rangeErr = 0, edges = 0, plane = 0;
    if ((int)blockIdx.x < a.lumaBlocks)
    {
        const S* src = (const S*)a.src[0];
        const int width = a.width[0], height = a.height[0];
        const int ty = tid >> 4, tx = (tid & 15) * 4;
        for (int tile = blockIdx.x; tile < a.tilesX * a.tilesY; tile += a.lumaBlocks)
        {
            const int tileY = tile / a.tilesX, x0 = (tile - tileY * a.tilesX) * kSsTileW, y0 = tileY * kSsTileH;
            // T[r][c] = converted picture sample (x0 - kSsPadX + c, y0 - 1 + r) = src[(y0 + r) * lumaPitch + x0 + c]
            for (int i = tid; i < kSsStageH * (kSsStageW / 4); i += 256)
            {
                const int r = i / (kSsStageW / 4), c = (i - r * (kSsStageW / 4)) * 4;
                int v[4];
                load4(src + (int64_t)(y0 + r) * a.lumaPitch + x0 + c, v);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    v[k] = xs_convert(v[k], a.conv, a.shift, a.mask, a.pixelBytes);
                uint2 pk;
                pk.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
                pk.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
                *reinterpret_cast<uint2*>(&T[r][c]) = pk;
            }
            __syncthreads();
            const int y = y0 + ty;
            int e[4], s[4];
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const uint16_t* g = &T[ty + 1][tx + k + kSsPadX];
                s[k] = g[0];
                int h, v;
                xe_sobel(g, (int64_t)kSsStageW, &h, &v);
                e[k] = xe_sobel_applies(y, x0 + tx + k, width, height) && xe_is_edge(h, v, a.threshold);
                bits |= (uint32_t)e[k] << k;
            }
            if (a.bits)
                store4((P*)a.bits + (int64_t)y * a.bitsPitch + x0 + tx, e);
            edges += __popc(bits);
            if (a.wantHist)
            {
                const int left = y < height ? width - (x0 + tx) : 0;         // samples of this thread inside the picture
                ss_hist_add<4>(Hwave, Hrep, bins, s, left < 0 ? 0 : (left > 4 ? 4 : left), rangeErr);
            }
            __syncthreads();
        }
        edges = wave_sum(edges);
        if (lane == 0 && edges)
            atomicAdd(&blockEdges, (unsigned)edges);
    }
    else
    {
        constexpr int N = SsVec<S>::N;
        const int cb = blockIdx.x - a.lumaBlocks;
        plane = 1 + cb / a.chromaBlocks;
        const int b = cb - (plane - 1) * a.chromaBlocks;
        const S* src = (const S*)a.src[plane];
        const int64_t n = (int64_t)a.width[plane] * a.height[plane], vecs = (n + N - 1) / N;
        // (the trip count is the workgroup's, not the lane's: ss_hist_add speaks to the whole wave)
        for (int64_t base = (int64_t)b * 256; base < vecs; base += (int64_t)a.chromaBlocks * 256)
        {
            const int64_t i = base + tid;
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (i < vecs)
                raw = *reinterpret_cast<const uint4*>(src + i * N);
            const uint32_t w[4] = { raw.x, raw.y, raw.z, raw.w };
            int v[N];
#pragma unroll
            for (int k = 0; k < N; k++)
            {
                const int sample = sizeof(S) == 1 ? (w[k >> 2] >> ((k & 3) * 8)) & 0xff : (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;
                v[k] = xs_convert(sample, a.conv, a.shift, a.mask, a.pixelBytes);
            }
            const int64_t left = n - i * N;
            ss_hist_add<N>(Hwave, Hrep, bins, v, left > N ? N : (left < 0 ? 0 : (int)left), rangeErr);
        }
    }
    rangeErr = wave_sum(rangeErr);
    if (lane == 0 && rangeErr)
        atomicAdd(&blockErrs, (unsigned)rangeErr);
    __syncthreads();
    if (tid == 0)
    {
        if (blockEdges) atomicAdd(&a.counters[0], blockEdges);
        if (blockErrs) atomicAdd(&a.counters[1], blockErrs);
    }
    if (!a.wantHist)
        return;
    for (int bin = tid; bin < bins; bin += 256)
    {
        int sum = 0;
        for (int w = 0; w < 4; w++)
            for (int r = 0; r < replicas; r++)
                sum += H[w][r * bins + bin];
        if (sum)
            atomicAdd(&a.hist[plane * bins + bin], sum);
    }
}

// per calling thread: a stream, device buffers and page-locked staging, kept between calls (a picture arrives per frame)
struct SceneScratch
{
    hipStream_t st = nullptr;
    char* d = nullptr; char* h = nullptr;
    size_t cap = 0;
    int device = -1;
};
static thread_local SceneScratch t_scene;

inline size_t ss_align(size_t n) { return (n + 255) & ~(size_t)255; }

} // namespace xh

using namespace xh;

extern "C" int x265hip_scene_stats(int depth, int numPlanes, const void* const* hostPlanes, const int* widths, const int* heights, const int64_t* strides,
                                   int sampleBytes, int conv, int shift, int mask, int wantHist, void* edgeBits, int64_t edgeStride,
                                   int32_t* edgeHist, int32_t* yuvHist, uint32_t* rangeErrors, void* stream)
{
    XH_CHECK_DEV();
    const int B = depth == 8 ? 1 : 2;                                  // sizeof(pixel) of the build
    bool ok = valid_depth(depth) && (numPlanes == 1 || numPlanes == 3) && hostPlanes && widths && heights && strides && rangeErrors &&
              (sampleBytes == 1 || sampleBytes == 2) && conv >= XS_CONV_NONE && conv <= XS_CONV_SHL_MASK && shift >= 0 && shift <= 8 &&
              (conv != XS_CONV_NONE || sampleBytes == B) && (wantHist || edgeBits) && (!wantHist || (yuvHist && depth <= 10)) && (wantHist || numPlanes == 1);
    for (int k = 0; ok && k < numPlanes; k++)
        ok = hostPlanes[k] && widths[k] >= 1 && heights[k] >= 1 && widths[k] <= 65535 && heights[k] <= 65535 && strides[k] >= widths[k] &&
             (int64_t)widths[k] * heights[k] < ((int64_t)1 << 31);
    if (ok && edgeBits)
        ok = edgeStride >= widths[0];
    if (!ok)
        return set_error(X265HIP_EINVAL, "scene_stats: depth %d, %d planes, %d-byte samples, conversion %d shift %d, histograms %d, edge bits %p stride %lld", depth,
                         numPlanes, sampleBytes, conv, shift, wantHist, edgeBits, (long long)edgeStride);
    const int width = widths[0], height = heights[0], bins = xs_bins(depth);
    SceneArgs a;
    memset(&a, 0, sizeof(a));
    a.tilesX = (width + kSsTileW - 1) / kSsTileW; a.tilesY = (height + kSsTileH - 1) / kSsTileH;
    a.lumaPitch = a.tilesX * kSsTileW + 2 * kSsPadX;
    a.bitsPitch = a.tilesX * kSsTileW;
    const int lumaRows = a.tilesY * kSsTileH + 2, bitsRows = a.tilesY * kSsTileH;
    a.planes = numPlanes;
    a.lumaBlocks = a.tilesX * a.tilesY < kSsLumaBlocksMax ? a.tilesX * a.tilesY : kSsLumaBlocksMax;
    if (numPlanes == 3)
    {
        // a chroma workgroup takes at least four 16-byte vectors per thread while there is that much
        const int64_t n = (int64_t)(widths[1] > widths[2] ? widths[1] : widths[2]) * (heights[1] > heights[2] ? heights[1] : heights[2]);
        const int64_t want = (n * sampleBytes + 256 * 64 - 1) / (256 * 64);
        a.chromaBlocks = (int)(want < 1 ? 1 : (want > kSsChromaBlocksMax ? kSsChromaBlocksMax : want));
    }
    const int blocks = a.lumaBlocks + (numPlanes - 1) * a.chromaBlocks;
    // input region: the padded luma plane, then the chroma planes as linear arrays (whole 16-byte vectors); output region: the histograms, the two counters,
    // the bit plane
    size_t srcOff[3], srcBytes = 0;
    for (int k = 0; k < numPlanes; k++)
    {
        srcOff[k] = srcBytes;
        srcBytes += ss_align(k ? (size_t)widths[k] * heights[k] * sampleBytes + 16 : (size_t)a.lumaPitch * lumaRows * sampleBytes);
    }
    const size_t histBytes = ss_align((size_t)3 * kSsMaxBins * 4 + 8);
    const size_t bitsBytes = edgeBits ? ss_align((size_t)a.bitsPitch * bitsRows * B) : 0;
    const size_t need = srcBytes + histBytes + bitsBytes;
    SceneScratch& ss = t_scene;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (ss.device != dev || ss.cap < need)
    {
        if (ss.d) (void)device_free(ss.d);
        if (ss.h) (void)hipHostFree(ss.h);
        if (ss.st && ss.device != dev) { (void)hipStreamDestroy(ss.st); ss.st = nullptr; }
        ss.d = ss.h = nullptr; ss.cap = 0; ss.device = dev;
        if (!ss.st && hipStreamCreateWithFlags(&ss.st, hipStreamNonBlocking) != hipSuccess)
            return set_error(X265HIP_EHIP, "scene_stats: stream");
        if (hipMalloc((void**)&ss.d, need) != hipSuccess || hipHostMalloc((void**)&ss.h, need, hipHostMallocDefault) != hipSuccess)
            return set_error(X265HIP_ENOMEM, "scene_stats: %zu bytes", need);
        ss.cap = need;
        memset(ss.h, 0, need);                         // the halo and the tile padding are read (never used): let them be defined
    }
    hipStream_t st = stream ? as_stream(stream) : ss.st;
    for (int r = 0; r < height; r++)
        memcpy(ss.h + srcOff[0] + ((size_t)(r + 1) * a.lumaPitch + kSsPadX) * sampleBytes, (const char*)hostPlanes[0] + (size_t)r * strides[0] * sampleBytes,
               (size_t)width * sampleBytes);
    for (int k = 1; k < numPlanes; k++)
        for (int r = 0; r < heights[k]; r++)
            memcpy(ss.h + srcOff[k] + (size_t)r * widths[k] * sampleBytes, (const char*)hostPlanes[k] + (size_t)r * strides[k] * sampleBytes,
                   (size_t)widths[k] * sampleBytes);
    char* dHist = ss.d + srcBytes;
    char* dBits = dHist + histBytes;
    if (hipMemcpyAsync(ss.d, ss.h, srcBytes, hipMemcpyHostToDevice, st) != hipSuccess || hipMemsetAsync(dHist, 0, histBytes, st) != hipSuccess)
        return set_error(X265HIP_EHIP, "scene_stats: upload");
    for (int k = 0; k < numPlanes; k++)
    {
        a.src[k] = ss.d + srcOff[k];
        a.width[k] = widths[k]; a.height[k] = heights[k];
    }
    a.conv = conv; a.shift = shift; a.mask = mask; a.pixelBytes = B; a.bins = bins; a.wantHist = wantHist != 0; a.threshold = xe_threshold(depth);
    a.bits = edgeBits ? dBits : nullptr;
    a.hist = (int32_t*)dHist;
    a.counters = (unsigned*)(dHist + (size_t)3 * kSsMaxBins * 4);
    const dim3 grid(blocks), block(256);
    DevSpan span(X265HIP_CLK_SCENE, st);
    if (sampleBytes == 1 && B == 1)
        hipLaunchKernelGGL((scene_stats_kernel<uint8_t, uint8_t>), grid, block, 0, st, a);
    else if (sampleBytes == 1)
        hipLaunchKernelGGL((scene_stats_kernel<uint8_t, uint16_t>), grid, block, 0, st, a);
    else if (B == 1)
        hipLaunchKernelGGL((scene_stats_kernel<uint16_t, uint8_t>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((scene_stats_kernel<uint16_t, uint16_t>), grid, block, 0, st, a);
    XH_LAUNCH_CHECK("scene_stats_kernel");
    span.end();
    for (int k = 0; k < numPlanes; k++)
        span.bytes += (uint64_t)widths[k] * heights[k] * sampleBytes;
    // one download: the histograms and counters, and behind them the bit plane when it is wanted
    if (hipMemcpyAsync(ss.h + srcBytes, dHist, histBytes + bitsBytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return set_error(X265HIP_EHIP, "scene_stats: download");
    span.commit();
    const int32_t* hHist = (const int32_t*)(ss.h + srcBytes);
    const unsigned* hCounters = (const unsigned*)(ss.h + srcBytes + (size_t)3 * kSsMaxBins * 4);
    *rangeErrors = hCounters[1];
    if (edgeHist)
    {
        edgeHist[0] = (int32_t)((int64_t)width * height - hCounters[0]);
        edgeHist[1] = (int32_t)hCounters[0];
    }
    if (wantHist)
        memcpy(yuvHist, hHist, (size_t)numPlanes * bins * 4);
    if (edgeBits)
    {
        // the interior only: the ring is "not written by computeEdge", and what lies there is the caller's
        const char* hBits = ss.h + srcBytes + histBytes;
        for (int r = 1; r < height - 1; r++)
            if (width > 2)
                memcpy((char*)edgeBits + ((size_t)r * edgeStride + 1) * B, hBits + ((size_t)r * a.bitsPitch + 1) * B, (size_t)(width - 2) * B);
    }
    return X265HIP_OK;
}
