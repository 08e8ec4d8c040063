// edgepass.hip — the edge and angle planes of a source picture (x265hip_edge_planes, include/x265hip.h): what the reference's edgeFilter
// (source/encoder/slicetype.cpp:151-215) computes for --aq-mode 4, as one pixel-parallel launch.  The arithmetic is edgepass.h's.
//
// A workgroup of 256 owns a 64 x 16 tile.  The device copy of the picture is laid out so that no load or store needs a bounds check: the picture's
// sample (0, 0) sits at row kPadY, column kPadX of a buffer that is a whole number of tiles plus the halo wide and high, and the output planes are a whole
// number of tiles wide and high (the host copies the width x height region out).
//   stage     tile + 3 rows above / below and 4 columns left / right (3 are needed — 2 for the Gaussian, 1 for the Sobel; 4 keeps every row a whole
//             number of aligned 4-sample vectors), as uint16 whatever the pixel width: 22 rows x 72 samples
//   Gaussian  tile + 1 sample per side out of the staged samples into a second LDS array: 18 rows x 66 samples
//   Sobel     each thread takes 4 horizontally adjacent pixels out of the Gaussian array: magnitude test, angle class, one 4-sample vector store per
//             plane (4 B at 8 bit, 8 B above; a wave covers 4 rows of 64 contiguous samples)
//   doubts    appended with one atomicAdd per wave: per-lane counts, a wave prefix sum, lane 0 reserves the wave's entries
// LDS rows are 72 uint16 = 36 dwords apart, so the 16 lanes of a tile row read consecutive dwords and the next row's lanes start 36 banks further on: of
// the two 32-lane halves the LDS serves per cycle only the 4 banks where rows wrap are touched twice.  No Gaussian plane leaves the device.
#include "common.h"
#include "edgepass.h"
#include <cstring>

namespace xh {

constexpr int kTileW = 64, kTileH = 16, kPadX = 4, kPadY = 3;
constexpr int kStageW = kTileW + 2 * kPadX, kStageH = kTileH + 2 * kPadY;      // 72 x 22
constexpr int kGaussW = kTileW + 2, kGaussH = kTileH + 2;                      // 66 x 18

struct EdgeSpecials { uint16_t v[XE_SPECIALS]; };

template <typename P>
__global__ __launch_bounds__(256) void edge_planes_kernel(const P* __restrict__ src, int srcPitch, int width, int height, EdgeSpecials specials, int threshold,
                                                          P* __restrict__ edge, P* __restrict__ theta, int outPitch,
                                                          uint32_t* __restrict__ doubts, int doubtCap, unsigned* __restrict__ doubtCount)
{
    __shared__ __align__(16) uint16_t S[kStageH][kStageW];      // rows of 144 bytes: every 4-sample group is 8-byte aligned
    __shared__ __align__(16) uint16_t G[kGaussH][kStageW];
    __shared__ uint16_t spc[XE_SPECIALS];
    const int tid = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    if (tid < XE_SPECIALS)
        spc[tid] = specials.v[tid];
    // S[r][c] = picture sample (x0 - kPadX + c, y0 - kPadY + r) = src[(y0 + r) * srcPitch + x0 + c]
    for (int i = tid; i < kStageH * (kStageW / 4); i += 256)
    {
        const int r = i / (kStageW / 4), c = (i - r * (kStageW / 4)) * 4;
        int v[4];
        load4(src + (int64_t)(y0 + r) * srcPitch + x0 + c, v);
        uint2 pk;
        pk.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
        pk.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
        *reinterpret_cast<uint2*>(&S[r][c]) = pk;
    }
    __syncthreads();
    // G[gr][gc] = Gaussian plane at picture (x0 - 1 + gc, y0 - 1 + gr), centred on S[gr + 2][gc + 3]
    for (int i = tid; i < kGaussH * kGaussW; i += 256)
    {
        const int gr = i / kGaussW, gc = i - gr * kGaussW;
        const uint16_t* p = &S[gr + kPadY - 1][gc + kPadX - 1];
        G[gr][gc] = (uint16_t)(xe_gauss_applies(y0 - 1 + gr, x0 - 1 + gc, width, height) ? xe_gauss25(p, (int64_t)kStageW) : (int)p[0]);
    }
    __syncthreads();
    const int ty = tid >> 4, tx = (tid & 15) * 4, y = y0 + ty;
    int e[4], a[4], nDoubt = 0;
    uint32_t doubtBits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const int x = x0 + tx + k;
        e[k] = S[ty + kPadY][tx + k + kPadX];          // outside the Sobel range the edge plane keeps the source sample, the angle is 0
        a[k] = 0;
        if (xe_sobel_applies(y, x, width, height))
        {
            int h, v, val;
            xe_sobel(&G[ty + 1][tx + k + 1], (int64_t)kStageW, &h, &v);
            e[k] = xe_is_edge(h, v, threshold) ? threshold : 0;
            if (xe_angle(h, v, spc, &val) == XE_DOUBTFUL)
            {
                doubtBits |= 1u << k;
                nDoubt++;
            }
            a[k] = val;
        }
    }
    store4(edge + (int64_t)y * outPitch + x0 + tx, e);
    store4(theta + (int64_t)y * outPitch + x0 + tx, a);
    // the wave's doubtful pixels: inclusive prefix sum of the per-lane counts, one reservation
    const int lane = tid & (kWave - 1);
    int incl = nDoubt;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1)
    {
        const int n = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += n;
    }
    const int total = __shfl(incl, kWave - 1, kWave);
    if (total)
    {
        unsigned base = 0;
        if (lane == 0)
            base = atomicAdd(doubtCount, (unsigned)total);
        base = __shfl(base, 0, kWave);
        unsigned pos = base + incl - nDoubt;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (doubtBits & (1u << k))
            {
                if (pos < (unsigned)doubtCap)
                    doubts[pos] = xe_doubt_pack(x0 + tx + k, y);
                pos++;
            }
    }
}

// per calling thread: a stream, device buffers and page-locked staging, kept between calls (a picture arrives per frame)
struct EdgeScratch
{
    hipStream_t st = nullptr;
    char* d = nullptr; char* h = nullptr;
    size_t cap = 0;
    int device = -1;
};
static thread_local EdgeScratch t_edge;

} // namespace xh

using namespace xh;

extern "C" int x265hip_edge_planes(int depth, const void* hostLuma, int64_t stride, int width, int height, const uint16_t specials[X265HIP_EDGE_SPECIALS],
                                   void* edgeOut, void* thetaOut, int64_t outStride, uint32_t* doubts, int doubtCap, int* doubtCount, void* stream)
{
    XH_CHECK_DEV();
    if (!valid_depth(depth) || !hostLuma || !specials || !edgeOut || !thetaOut || !doubtCount || (doubtCap > 0 && !doubts) || doubtCap < 0 ||
        width < 1 || height < 1 || width > 65535 || height > 65535 || stride < width + 2 || outStride < width)
        return set_error(X265HIP_EINVAL, "edge_planes: depth %d %dx%d stride %lld out stride %lld doubt capacity %d", depth, width, height, (long long)stride,
                         (long long)outStride, doubtCap);
    const int B = depth == 8 ? 1 : 2;
    const int tilesX = (width + kTileW - 1) / kTileW, tilesY = (height + kTileH - 1) / kTileH;
    const int outPitch = tilesX * kTileW, outRows = tilesY * kTileH, srcPitch = outPitch + 2 * kPadX, srcRows = outRows + 2 * kPadY;
    const size_t srcBytes = ((size_t)srcPitch * srcRows * B + 255) & ~(size_t)255, planeBytes = (size_t)outPitch * outRows * B;
    const size_t listBytes = ((size_t)doubtCap * 4 + 4 + 255) & ~(size_t)255;                // the count, then the entries
    const size_t need = srcBytes + 2 * planeBytes + listBytes;
    EdgeScratch& es = t_edge;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (es.device != dev || es.cap < need)
    {
        if (es.d) (void)device_free(es.d);
        if (es.h) (void)hipHostFree(es.h);
        if (es.st && es.device != dev) { (void)hipStreamDestroy(es.st); es.st = nullptr; }
        es.d = es.h = nullptr; es.cap = 0; es.device = dev;
        if (!es.st && hipStreamCreateWithFlags(&es.st, hipStreamNonBlocking) != hipSuccess)
            return set_error(X265HIP_EHIP, "edge_planes: stream");
        if (hipMalloc((void**)&es.d, need) != hipSuccess || hipHostMalloc((void**)&es.h, need, hipHostMallocDefault) != hipSuccess)
            return set_error(X265HIP_ENOMEM, "edge_planes: %zu bytes", need);
        es.cap = need;
        memset(es.h, 0, need);                         // the halo outside the picture is read (never used): let it be defined
    }
    hipStream_t st = stream ? as_stream(stream) : es.st;
    // the picture with the two rows and columns past it that the Gaussian of row height-1 / column width-1 reads, as the host buffer holds them
    for (int r = 0; r < height + 2; r++)
        memcpy(es.h + ((size_t)(r + kPadY) * srcPitch + kPadX) * B, (const char*)hostLuma + (size_t)r * stride * B, (size_t)(width + 2) * B);
    char* dEdge = es.d + srcBytes;
    char* dTheta = dEdge + planeBytes;
    unsigned* dCount = (unsigned*)(dTheta + planeBytes);
    uint32_t* dList = (uint32_t*)(dCount + 1);
    if (hipMemcpyAsync(es.d, es.h, srcBytes, hipMemcpyHostToDevice, st) != hipSuccess || hipMemsetAsync(dCount, 0, 4, st) != hipSuccess)
        return set_error(X265HIP_EHIP, "edge_planes: upload");
    EdgeSpecials sp;
    memcpy(sp.v, specials, sizeof(sp.v));
    const dim3 grid(tilesX, tilesY), block(256);
    DevSpan span(X265HIP_CLK_EDGE, st);
    if (depth == 8)
        hipLaunchKernelGGL((edge_planes_kernel<uint8_t>), grid, block, 0, st, (const uint8_t*)es.d, srcPitch, width, height, sp, xe_threshold(depth),
                           (uint8_t*)dEdge, (uint8_t*)dTheta, outPitch, dList, doubtCap, dCount);
    else
        hipLaunchKernelGGL((edge_planes_kernel<uint16_t>), grid, block, 0, st, (const uint16_t*)es.d, srcPitch, width, height, sp, xe_threshold(depth),
                           (uint16_t*)dEdge, (uint16_t*)dTheta, outPitch, dList, doubtCap, dCount);
    XH_LAUNCH_CHECK("edge_planes_kernel");
    span.end();
    span.bytes = (uint64_t)width * height * B * 3;
    if (hipMemcpyAsync(es.h + srcBytes, dEdge, 2 * planeBytes + listBytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return set_error(X265HIP_EHIP, "edge_planes: download");
    span.commit();
    const char* hEdge = es.h + srcBytes;
    const char* hTheta = hEdge + planeBytes;
    for (int r = 0; r < height; r++)
    {
        memcpy((char*)edgeOut + (size_t)r * outStride * B, hEdge + (size_t)r * outPitch * B, (size_t)width * B);
        memcpy((char*)thetaOut + (size_t)r * outStride * B, hTheta + (size_t)r * outPitch * B, (size_t)width * B);
    }
    const unsigned n = *(const unsigned*)(hTheta + planeBytes);
    *doubtCount = (int)n;
    if (doubtCap > 0)
        memcpy(doubts, hTheta + planeBytes + 4, (size_t)(n < (unsigned)doubtCap ? n : (unsigned)doubtCap) * 4);
    return X265HIP_OK;
}
