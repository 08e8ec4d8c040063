// x265_hip_scenecut.cpp — the translation unit of the drop-in that serves --hist-scenecut: Encoder::computeHistograms
// (reference source/encoder/encoder.cpp:1361-1487) runs for every input picture on the thread that calls x265_encoder_encode, before the picture is handed
// to the lookahead — a memset, a Sobel pass with a sqrtf per luma pixel, a count of the edge plane, three histogram loops and, when the input depth is not
// the build's, three plane conversions.  Here it is one synchronous x265hip_scene_stats call (x265_amd/csrc/scenestats.hip; the arithmetic once, in
// scenestats.h); m_curEdgeHist, m_curYUVHist and — only when --rskip 2 will read it (encoder.cpp:1771) — m_edgePic are left exactly as the reference leaves
// them.  The method is weakened in encoder_seam.o and its body stays reachable as Encoder::computeHistogramsRef from a second compile of encoder.cpp
// (integration/Makefile).  Only the product's encoders link this unit: the emulated encoders of the tests keep the reference's encoder.o.
//
// Served when: the build is 8 or 10 bit (the Main12 build's 4096 sample values do not fit its own 1024 bins: it stays on the host), the library has
// x265hip_scene_stats, the switch is on, the picture's colour space is the encoder's, every plane's stride is its width in bytes (the reference converts with
// pic->stride and then reads the planes as packed arrays: the only layout for which its own indexing is sane), and the sizes are the ones the encoder's
// buffers were made for.  A picture with converted samples outside the bins (the reference indexes past its arrays there) and everything else: the
// reference's body.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#define protected public
#define private public
#include "common.h"
#include "primitives.h"
#include "encoder.h"
#undef protected
#undef private

#include "x265hip.h"
#include "x265_hip_debug.h"
#include "../csrc/scenestats.h"

// weak: a library without the entry point leaves every picture to the reference's body
extern "C" int x265hip_scene_stats(int depth, int numPlanes, const void* const* hostPlanes, const int* widths, const int* heights, const int64_t* strides,
                                   int sampleBytes, int conv, int shift, int mask, int wantHist, void* edgeBits, int64_t edgeStride,
                                   int32_t* edgeHist, int32_t* yuvHist, uint32_t* rangeErrors, void* stream) __attribute__((weak));

namespace X265_NS {

// the reference's body (encoder_ref.o, compiled with -DcomputeHistograms=computeHistogramsRef)
extern bool refComputeHistograms(Encoder* self, x265_picture* pic) asm("_ZN4x2657Encoder20computeHistogramsRefEP12x265_picture");

namespace {

std::atomic<int> g_sceneState(0);                    // 0 undecided, 1 on, -1 off (switch, missing symbol, no device, device failure)
std::atomic<uint64_t> g_served(0), g_kept(0), g_outOfRange(0), g_servedNs(0), g_keptNs(0);
std::mutex g_sceneLock;

void scene_report()
{
    const uint64_t s = g_served.load(), k = g_kept.load();
    fprintf(stderr, "x265hip: scenestats: %llu pictures served, %llu kept on the host, %llu with samples out of range (per picture: %.3f ms served, %.3f ms on the host)\n",
            (unsigned long long)s, (unsigned long long)k, (unsigned long long)g_outOfRange.load(), s ? g_servedNs.load() * 1e-6 / s : 0.0,
            k ? g_keptNs.load() * 1e-6 / k : 0.0);
}

// X265HIP_SCENESTATS=1 switches the pass on, =0 off; unset: on in the 8-bit and Main10 builds, both measured (profiles/r14_v1_scenestats_ab.txt);
// the Main12 build never serves (file comment)
bool scene_on()
{
    int st = g_sceneState.load(std::memory_order_acquire);
    if (!st)
    {
        std::lock_guard<std::mutex> g(g_sceneLock);
        st = g_sceneState.load();
        if (!st)
        {
            const char* env = getenv("X265HIP_SCENESTATS");
            const char* all = getenv("X265HIP");
            st = (env ? !strcmp(env, "1") : true) && !(all && !strcmp(all, "0")) && x265hip_scene_stats && X265_DEPTH <= 10 && x265hip_device_count() > 0 ? 1 : -1;
            g_sceneState.store(st, std::memory_order_release);
        }
    }
    return st > 0;
}

inline uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

bool Encoder::computeHistograms(x265_picture* pic)
{
    static const bool verbose = getenv("X265HIP_VERBOSE") != NULL, verify = getenv("X265HIP_VERIFY") != NULL;
    static std::once_flag once;
    if (verbose)
        std::call_once(once, [] { atexit(scene_report); });
    const uint64_t t0 = now_ns();
    const int csp = pic->colorSpace, planes = csp == X265_CSP_I400 ? 1 : 3;
    int widths[3], heights[3], conv, shift, mask, sampleBytes;
    int64_t strides[3];
    const void* ptrs[3];
    xs_conversion_of(pic->bitDepth, X265_DEPTH, &conv, &shift, &mask, &sampleBytes);
    bool serve = scene_on() && csp == m_param->internalCsp && pic->bitDepth >= 8 && pic->bitDepth <= 16 && pic->width > 2 && pic->height > 2 &&
                 pic->width <= 65535 && pic->height <= 65535 && (int64_t)pic->width * pic->height < ((int64_t)1 << 31) && m_edgePic &&
                 (pic->bitDepth == X265_DEPTH || m_inputPic[0]);
    for (int k = 0; serve && k < planes; k++)
    {
        widths[k] = k ? pic->width >> CHROMA_H_SHIFT(csp) : pic->width;
        heights[k] = k ? pic->height >> CHROMA_V_SHIFT(csp) : pic->height;
        strides[k] = widths[k];
        ptrs[k] = pic->planes[k];
        serve = pic->planes[k] && pic->stride[k] == widths[k] * sampleBytes && m_planeSizes[k] == (uint32_t)(widths[k] * heights[k]);
    }
    if (serve)
    {
        const bool wantBits = m_param->recursionSkipMode == EDGE_BASED_RSKIP;        // Encoder::encode (encoder.cpp:1771) is m_edgePic's only reader
        int32_t edgeHist[2], yuvHist[3][HISTOGRAM_BINS];
        uint32_t outOfRange = 0;
        if (wantBits)
            memset(m_edgePic, 0, sizeof(pixel) * m_planeSizes[0]);                   // the call writes the interior: the ring is the memset's, as in the reference
        if (x265hip_scene_stats(X265_DEPTH, planes, ptrs, widths, heights, strides, sampleBytes, conv, shift, mask, 1, wantBits ? m_edgePic : NULL, pic->width,
                                edgeHist, &yuvHist[0][0], &outOfRange, NULL))
        {
            g_sceneState.store(-1);
            x265hip_device_failure("scenestats", "x265hip_scene_stats");
            serve = false;
        }
        else if (outOfRange)
        {
            g_outOfRange.fetch_add(1, std::memory_order_relaxed);
            serve = false;
        }
        else
        {
            m_curEdgeHist[0] = edgeHist[0];
            m_curEdgeHist[1] = edgeHist[1];
            for (int k = 0; k < planes; k++)
                memcpy(m_curYUVHist[k], yuvHist[k], sizeof(m_curYUVHist[k]));
            g_served.fetch_add(1, std::memory_order_relaxed);
            g_servedNs.fetch_add(now_ns() - t0, std::memory_order_relaxed);
            if (verify)
            {
                const size_t planeBytes = sizeof(pixel) * m_planeSizes[0];
                pixel* bits = wantBits ? (pixel*)malloc(planeBytes) : NULL;
                if (bits)
                    memcpy(bits, m_edgePic, planeBytes);
                const bool ok = refComputeHistograms(this, pic);
                const char* what = !ok ? "the reference's body failed" : memcmp(edgeHist, m_curEdgeHist, sizeof(edgeHist)) ? "edge bins" : NULL;
                for (int k = 0; k < planes && !what; k++)
                    if (memcmp(yuvHist[k], m_curYUVHist[k], sizeof(m_curYUVHist[k])))
                        what = k == 0 ? "Y histogram" : (k == 1 ? "U histogram" : "V histogram");
                if (!what && bits && memcmp(bits, m_edgePic, planeBytes))
                    what = "edge plane";
                if (what)
                {
                    fprintf(stderr, "x265hip: scenestats: VERIFY FAILED: %s of a %dx%d picture (input depth %d) differ from the reference's computeHistograms\n", what,
                            pic->width, pic->height, pic->bitDepth);
                    abort();
                }
                free(bits);
            }
            return true;
        }
    }
    const uint64_t t1 = now_ns();
    const bool r = refComputeHistograms(this, pic);
    g_kept.fetch_add(1, std::memory_order_relaxed);
    g_keptNs.fetch_add(now_ns() - t1, std::memory_order_relaxed);
    return r;
}

} // namespace X265_NS
