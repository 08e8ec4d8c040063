// pichash.hip — the decoded-picture hashes of --hash 2 (CRC) and --hash 3 (checksum) (x265hip_picture_hash, include/x265hip.h): what the reference's
// updateCRC / updateChecksum (source/common/picyuv.cpp:507-571) compute for a band of rows of up to three planes of a reconstructed picture, as one launch.
// The arithmetic is pichash.h's; all of it is integer and independent of the order of the parts.
//
// The call packs every plane band into page-locked staging (rows one after the other, the stride padding skipped): a band is then ONE byte stream — the
// bytes of a 16-bit sample lie low byte first, which is the order updateCRC takes them in.  The stream is placed so that it ENDS on a segment boundary: the
// zero bytes in front of it change no CRC entered with state 0 and are skipped by the checksum, so every load is a whole aligned 16-byte chunk, every tree
// constant is fixed, and the short chunk of a band (any width >= 1, chunks that straddle row ends) is its first.
//
// One kernel, one workgroup (256 threads) per segment of XP_SEGMENT_BYTES, the segments of all planes of the call in one grid:
//   CRC        a lane folds its chunk byte by byte from state 0 with T (256 entries) in LDS; the wave combines its lanes by a log-tree
//              v = v_left * x^(8 len_right) + v_right (six steps, the constants x^(128 << step) precomputed by the host); thread 0 combines the four waves,
//              multiplies by x^(8 * bytes behind the segment) (square-and-multiply, not reduced by any period of x) and leaves the result by one atomic XOR
//   checksum   a lane sums the terms of its samples at their picture positions; wave reduction, then one atomic add per workgroup
// The host enters the caller's running value: state * x^(8 bytes) + result for the CRC, state + result for the checksum.
#include "common.h"
#include "pichash.h"
#include <cstring>

namespace xh {

constexpr int kPhTreeSteps = 6;

struct HashArgs
{
    const uint8_t* src[3];           // device copies: the padded byte stream of each plane band (a whole number of segments)
    uint32_t bytes[3], pad[3];       // the band's bytes, and the zero bytes in front of them
    int firstSeg[4];                 // plane k owns workgroups firstSeg[k] .. firstSeg[k + 1] - 1
    int width[3], y0[3];             // in samples / picture rows (checksum positions)
    int depth, planes;
    uint32_t tree[kPhTreeSteps];     // x^(8 * XP_CHUNK_BYTES << step) mod P
    uint32_t waveShift;              // x^(8 * XP_WAVE_BYTES) mod P
    uint32_t* result;                // one word per plane, zero before the launch
};

// S = the sample type (the CRC form reads bytes whatever S is: a packed plane is its own byte stream), METHOD = XP_METHOD_*
template <typename S, int METHOD>
__global__ __launch_bounds__(256) void picture_hash_kernel(HashArgs a)
{
    __shared__ uint16_t T[256];
    __shared__ uint32_t waveVal[4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    int plane = 0;
    while (plane + 1 < a.planes && (int)blockIdx.x >= a.firstSeg[plane + 1])
        plane++;
    const uint32_t seg = blockIdx.x - a.firstSeg[plane];
    const uint32_t total = a.pad[plane] + a.bytes[plane];                    // a multiple of XP_SEGMENT_BYTES
    const uint32_t at = seg * XP_SEGMENT_BYTES + tid * XP_CHUNK_BYTES;       // < total: the grid has total / XP_SEGMENT_BYTES workgroups for the plane
    const uint4 raw = *reinterpret_cast<const uint4*>(a.src[plane] + at);
    const uint32_t w[4] = { raw.x, raw.y, raw.z, raw.w };
    if (METHOD == XP_METHOD_CRC)
    {
        T[tid] = (uint16_t)xp_table_entry(tid);
        __syncthreads();
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < XP_CHUNK_BYTES; k++)
            v = xp_crc_byte(v, T, (w[k >> 2] >> ((k & 3) * 8)) & 0xff);
#pragma unroll
        for (int s = 0; s < kPhTreeSteps; s++)
        {
            const uint32_t other = (uint32_t)__shfl_xor((int)v, 1 << s, kWave);
            const bool left = !(lane & (1 << s));
            v = xp_mul(left ? v : other, a.tree[s]) ^ (left ? other : v);
        }
        if (lane == 0)
            waveVal[wave] = v;
        __syncthreads();
        if (tid == 0)
        {
            uint32_t r = waveVal[0];
            for (int k = 1; k < 4; k++)
                r = xp_mul(r, a.waveShift) ^ waveVal[k];
            const uint64_t behind = (uint64_t)total - (uint64_t)(seg + 1) * XP_SEGMENT_BYTES;
            r = xp_mul(r, xp_xpow(8 * behind));
            if (r)
                atomicXor(&a.result[plane], r);
        }
    }
    else
    {
        constexpr int N = XP_CHUNK_BYTES / (int)sizeof(S);
        const uint32_t pad = a.pad[plane], width = (uint32_t)a.width[plane];
        uint32_t sum = 0;
        if (at + XP_CHUNK_BYTES > pad)
        {
            // the chunk's first sample inside the band, its position, then along the row
            const uint32_t first = at > pad ? 0 : (pad - at) / (uint32_t)sizeof(S);
            const uint32_t idx = (at + first * (uint32_t)sizeof(S) - pad) / (uint32_t)sizeof(S);
            uint32_t y = idx / width, x = idx - y * width;
            y += (uint32_t)a.y0[plane];
#pragma unroll
            for (int k = 0; k < N; k++)
                if (k >= (int)first)
                {
                    const uint32_t p = sizeof(S) == 1 ? (w[k >> 2] >> ((k & 3) * 8)) & 0xff : (w[k >> 1] >> ((k & 1) * 16)) & 0xffff;
                    sum += xp_checksum_term(p, x, y, a.depth);
                    if (++x == width) { x = 0; y++; }
                }
        }
        sum = (uint32_t)wave_sum((int)sum);
        if (lane == 0)
            waveVal[wave] = sum;
        __syncthreads();
        if (tid == 0)
        {
            const uint32_t r = waveVal[0] + waveVal[1] + waveVal[2] + waveVal[3];
            if (r)
                atomicAdd(&a.result[plane], r);
        }
    }
}

// per calling thread (several frame encoders finish rows at the same time): a stream, device buffers and page-locked staging, kept between calls
struct HashScratch
{
    hipStream_t st = nullptr;
    char* d = nullptr; char* h = nullptr;
    size_t cap = 0;
    int device = -1;
};
static thread_local HashScratch t_hash;

constexpr size_t kPhResultBytes = 256;               // the three result words, in front of the streams

} // namespace xh

using namespace xh;

extern "C" int x265hip_picture_hash(int depth, int method, const x265hip_hash_plane* planes, int numPlanes, uint32_t* state, void* stream)
{
    XH_CHECK_DEV();
    const int B = depth == 8 ? 1 : 2;
    bool ok = valid_depth(depth) && (method == XP_METHOD_CRC || method == XP_METHOD_CHECKSUM) && planes && state && numPlanes >= 1 && numPlanes <= 3;
    uint64_t segs = 0;
    for (int k = 0; ok && k < numPlanes; k++)
    {
        const x265hip_hash_plane& p = planes[k];
        ok = p.plane && p.width >= 1 && p.height >= 1 && p.width <= 65535 && p.height <= 65535 && p.y0 >= 0 && p.stride >= p.width &&
             (uint64_t)p.width * p.height * B < ((uint64_t)1 << 31);
        if (ok)
            segs += ((uint64_t)p.width * p.height * B + XP_SEGMENT_BYTES - 1) / XP_SEGMENT_BYTES;
    }
    if (!ok || segs >= ((uint64_t)1 << 30))
        return set_error(X265HIP_EINVAL, "picture_hash: depth %d, method %d, %d planes%s", depth, method, numPlanes, ok ? ": too large" : "");
    HashArgs a;
    memset(&a, 0, sizeof(a));
    size_t off[3], need = kPhResultBytes;
    for (int k = 0; k < numPlanes; k++)
    {
        const uint32_t bytes = (uint32_t)planes[k].width * planes[k].height * B;
        const uint32_t nseg = (bytes + XP_SEGMENT_BYTES - 1) / XP_SEGMENT_BYTES;
        a.bytes[k] = bytes;
        a.pad[k] = nseg * XP_SEGMENT_BYTES - bytes;
        a.firstSeg[k + 1] = a.firstSeg[k] + (int)nseg;
        a.width[k] = planes[k].width; a.y0[k] = planes[k].y0;
        off[k] = need;
        need += (size_t)nseg * XP_SEGMENT_BYTES;
    }
    for (int k = numPlanes; k < 3; k++)
        a.firstSeg[k + 1] = a.firstSeg[numPlanes];
    a.depth = depth; a.planes = numPlanes;
    for (int s = 0; s < kPhTreeSteps; s++)
        a.tree[s] = xp_xpow((uint64_t)8 * XP_CHUNK_BYTES << s);
    a.waveShift = xp_xpow((uint64_t)8 * XP_WAVE_BYTES);
    HashScratch& hs = t_hash;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hs.device != dev || hs.cap < need)
    {
        if (hs.d) (void)device_free(hs.d);
        if (hs.h) (void)hipHostFree(hs.h);
        if (hs.st && hs.device != dev) { (void)hipStreamDestroy(hs.st); hs.st = nullptr; }
        hs.d = hs.h = nullptr; hs.cap = 0; hs.device = dev;
        if (!hs.st && hipStreamCreateWithFlags(&hs.st, hipStreamNonBlocking) != hipSuccess)
            return set_error(X265HIP_EHIP, "picture_hash: stream");
        // room to spare: the bands of a picture differ in height (the last CTU row is partial), and the next call should not allocate again
        const size_t cap = need + need / 4;
        if (hipMalloc((void**)&hs.d, cap) != hipSuccess || hipHostMalloc((void**)&hs.h, cap, hipHostMallocDefault) != hipSuccess)
            return set_error(X265HIP_ENOMEM, "picture_hash: %zu bytes", cap);
        hs.cap = cap;
    }
    hipStream_t st = stream ? as_stream(stream) : hs.st;
    memset(hs.h, 0, kPhResultBytes);
    for (int k = 0; k < numPlanes; k++)
    {
        const x265hip_hash_plane& p = planes[k];
        char* dst = hs.h + off[k];
        memset(dst, 0, a.pad[k]);
        dst += a.pad[k];
        const size_t rowBytes = (size_t)p.width * B;
        for (int r = 0; r < p.height; r++)
            memcpy(dst + (size_t)r * rowBytes, (const char*)p.plane + (size_t)r * p.stride * B, rowBytes);
        a.src[k] = (const uint8_t*)hs.d + off[k];
    }
    a.result = (uint32_t*)hs.d;
    // one upload: the zeroed result words and the streams behind them
    if (hipMemcpyAsync(hs.d, hs.h, need, hipMemcpyHostToDevice, st) != hipSuccess)
        return set_error(X265HIP_EHIP, "picture_hash: upload");
    const dim3 grid(a.firstSeg[numPlanes]), block(256);
    DevSpan span(X265HIP_CLK_PICHASH, st);
    if (method == XP_METHOD_CRC)
    {
        if (B == 1) hipLaunchKernelGGL((picture_hash_kernel<uint8_t, XP_METHOD_CRC>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((picture_hash_kernel<uint16_t, XP_METHOD_CRC>), grid, block, 0, st, a);
    }
    else
    {
        if (B == 1) hipLaunchKernelGGL((picture_hash_kernel<uint8_t, XP_METHOD_CHECKSUM>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((picture_hash_kernel<uint16_t, XP_METHOD_CHECKSUM>), grid, block, 0, st, a);
    }
    XH_LAUNCH_CHECK("picture_hash_kernel");
    span.end();
    for (int k = 0; k < numPlanes; k++)
        span.bytes += a.bytes[k];
    if (hipMemcpyAsync(hs.h, hs.d, kPhResultBytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return set_error(X265HIP_EHIP, "picture_hash: download");
    span.commit();
    const uint32_t* res = (const uint32_t*)hs.h;
    for (int k = 0; k < numPlanes; k++)
        state[k] = method == XP_METHOD_CRC ? xp_crc_enter(state[k], res[k], a.bytes[k]) : state[k] + res[k];
    return X265HIP_OK;
}
