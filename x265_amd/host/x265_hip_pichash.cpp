// x265_hip_pichash.cpp — the translation unit of the drop-in that serves the decoded-picture hashes of --hash 2 (CRC) and --hash 3 (checksum)
// (INTEGRATION.md §6p): FrameEncoder::initDecodedPictureHashSEI (reference source/encoder/frameencoder.cpp:1167-1237) runs for every finished CTU row
// (FrameFilter::processPostRow, framefilter.cpp:713-717) or, with --slices > 1, once per picture from compressFrame (frameencoder.cpp:924-929): updateCRC
// walks every sample a bit at a time, updateChecksum sums masked bytes (picyuv.cpp:507-571).  Here it is one synchronous x265hip_picture_hash call per row
// covering all planes (x265_amd/csrc/pichash.hip; the arithmetic once, in pichash.h), with the reference's own widths, heights, strides and addresses;
// m_seiReconPictureDigest.m_crc / m_checksum are left exactly as the reference leaves them.  The method is weakened in frameencoder_seam.o and its body stays
// reachable as FrameEncoder::initDecodedPictureHashSEIRef from a second compile of frameencoder.cpp (integration/Makefile).  Only the product's encoders link
// this unit: the emulated encoders of the tests keep the reference's frameencoder.o.
//
// The reference's quirks, kept to the letter:
//   * the per-row CRC path sets m_crc[1] = m_crc[2] = 0xffff on EVERY row (frameencoder.cpp:1211): with one slice the chroma CRCs of the bitstream cover the
//     last CTU row only; with --slices > 1 the one call covers the picture and they cover everything
//   * the checksum's bands are addressed from m_picOrg[] with row * cuHeight, the CRC's through getLumaAddr / getCbAddr / getCrAddr(cuAddr)
//   * 4:0:0 has one plane
// MD5 (--hash 1, one serial chain per plane), a library without the entry point, a refused call, a device failure and the switched-off case: the
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
#include "frame.h"
#include "picyuv.h"
#include "frameencoder.h"
#undef protected
#undef private

#include "x265hip.h"
#include "x265_hip_debug.h"
#include "../csrc/pichash.h"

// weak: a library without the entry point leaves every row to the reference's body
extern "C" int x265hip_picture_hash(int depth, int method, const x265hip_hash_plane* planes, int numPlanes, uint32_t* state, void* stream) __attribute__((weak));

// x265_hip_refplanes.cpp reports the rows of an encoder linked WITHOUT this unit; with it, the report is this unit's
extern "C" void x265hip_pichash_linked() {}

namespace X265_NS {

// the reference's body (frameencoder_ref.o, compiled with -DinitDecodedPictureHashSEI=initDecodedPictureHashSEIRef)
extern void refInitDecodedPictureHashSEI(FrameEncoder* self, int row, int cuAddr, int height) asm("_ZN4x26512FrameEncoder28initDecodedPictureHashSEIRefEiii");

namespace {

std::atomic<int> g_hashState(0);                     // 0 undecided, 1 asked for (X265HIP_PICHASH=1), 2 usable and left to the default, -1 off (switch, missing symbol,
                                                     // no device, device failure)
std::atomic<uint64_t> g_served(0), g_kept(0), g_servedNs(0), g_keptNs(0);
std::mutex g_hashLock;

void hash_report()
{
    const uint64_t s = g_served.load(), k = g_kept.load();
    fprintf(stderr, "x265hip: pichash: %llu rows served, %llu kept on the host (per row: %.3f ms served, %.3f ms on the host)\n", (unsigned long long)s,
            (unsigned long long)k, s ? g_servedNs.load() * 1e-6 / s : 0.0, k ? g_keptNs.load() * 1e-6 / k : 0.0);
}

// X265HIP_PICHASH=1 switches the seam on, =0 off; unset: on for the CRC in the Main10 build, off for everything else — each method and build by its own
// measurement (profiles/r15_v1_pichash_ab.txt); the Main12 build was not measured
bool hash_on(int method)
{
    int st = g_hashState.load(std::memory_order_acquire);
    if (!st)
    {
        std::lock_guard<std::mutex> g(g_hashLock);
        st = g_hashState.load();
        if (!st)
        {
            const char* env = getenv("X265HIP_PICHASH");
            const char* all = getenv("X265HIP");
            const bool usable = !(env && strcmp(env, "1")) && !(all && !strcmp(all, "0")) && x265hip_picture_hash && x265hip_device_count() > 0;
            st = !usable ? -1 : (env ? 1 : 2);
            g_hashState.store(st, std::memory_order_release);
        }
    }
    return st == 1 || (st == 2 && method == XP_METHOD_CRC && X265_DEPTH == 10);
}

inline uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

void FrameEncoder::initDecodedPictureHashSEI(int row, int cuAddr, int height)
{
    static const bool verbose = getenv("X265HIP_VERBOSE") != NULL, verify = getenv("X265HIP_VERIFY") != NULL;
    static std::once_flag once;
    const int method = m_param->decodedPictureHashSEI;
    static const bool asked = getenv("X265HIP_PICHASH") != NULL;
    if (!method || (method != XP_METHOD_CRC && method != XP_METHOD_CHECKSUM && !asked))
    {
        // no hash: the body does nothing; MD5 with the switch unset: an encode that prints what it always printed
        refInitDecodedPictureHashSEI(this, row, cuAddr, height);
        return;
    }
    if (verbose)
        std::call_once(once, [] { atexit(hash_report); });
    const uint64_t t0 = now_ns();
    if ((method == XP_METHOD_CRC || method == XP_METHOD_CHECKSUM) && hash_on(method) && height > 0)
    {
        PicYuv* reconPic = m_frame->m_reconPic;
        const int planes = m_param->internalCsp != X265_CSP_I400 ? 3 : 1;
        const uint32_t hShift = CHROMA_H_SHIFT(m_param->internalCsp), vShift = CHROMA_V_SHIFT(m_param->internalCsp);
        const uint32_t width = reconPic->m_picWidth, maxCUHeight = m_param->maxCUSize;
        uint32_t* running = method == XP_METHOD_CRC ? m_seiReconPictureDigest.m_crc : m_seiReconPictureDigest.m_checksum;
        x265hip_hash_plane p[3];
        uint32_t state[3];
        bool serve = true;                                                       // (a band the library would refuse is the reference's, not a failure)
        for (int k = 0; k < planes; k++)
        {
            p[k].width = (int32_t)(k ? width >> hShift : width);
            p[k].height = (int32_t)(k ? (uint32_t)height >> vShift : (uint32_t)height);
            p[k].stride = k ? reconPic->m_strideC : reconPic->m_stride;
            p[k].y0 = (int32_t)(row * (k ? maxCUHeight >> vShift : maxCUHeight));
            if (method == XP_METHOD_CRC)
            {
                p[k].plane = k == 0 ? reconPic->getLumaAddr(cuAddr) : (k == 1 ? reconPic->getCbAddr(cuAddr) : reconPic->getCrAddr(cuAddr));
                state[k] = k == 0 && row ? running[0] : 0xffff;                  // chroma: 0xffff on every row (frameencoder.cpp:1211)
            }
            else
            {
                p[k].plane = reconPic->m_picOrg[k] + (intptr_t)p[k].y0 * p[k].stride;
                state[k] = row ? running[k] : 0;
            }
            serve = serve && p[k].width >= 1 && p[k].height >= 1 && p[k].width <= 65535 && p[k].height <= 65535;
        }
        const uint32_t before[3] = { state[0], state[1], state[2] };
        if (!serve)
            ;
        else if (x265hip_picture_hash(X265_DEPTH, method, p, planes, state, NULL))
        {
            g_hashState.store(-1);
            x265hip_device_failure("pichash", "x265hip_picture_hash");
        }
        else
        {
            if (verify)
                for (int k = 0; k < planes; k++)
                {
                    uint32_t want = before[k];
                    if (method == XP_METHOD_CRC)
                        updateCRC((const pixel*)p[k].plane, want, p[k].height, p[k].width, p[k].stride);
                    else
                        updateChecksum(reconPic->m_picOrg[k], want, p[k].height, p[k].width, p[k].stride, row, k ? maxCUHeight >> vShift : maxCUHeight);
                    if (want != state[k])
                    {
                        fprintf(stderr, "x265hip: pichash: VERIFY FAILED: plane %d of row %d (%d x %d, method %d): %08x, the reference's %08x\n", k, row, p[k].width,
                                p[k].height, method, state[k], want);
                        abort();
                    }
                }
            for (int k = 0; k < planes; k++)
                running[k] = state[k];
            g_served.fetch_add(1, std::memory_order_relaxed);
            g_servedNs.fetch_add(now_ns() - t0, std::memory_order_relaxed);
            return;
        }
    }
    const uint64_t t1 = now_ns();
    refInitDecodedPictureHashSEI(this, row, cuAddr, height);
    g_kept.fetch_add(1, std::memory_order_relaxed);
    g_keptNs.fetch_add(now_ns() - t1, std::memory_order_relaxed);
}

} // namespace X265_NS
