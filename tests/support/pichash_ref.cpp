// pichash_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_pichash.py, tests/golden/make_pichash_golden.py): the reference's own
// FrameEncoder::initDecodedPictureHashSEI (source/encoder/frameencoder.cpp:1167-1237) on a Frame whose reconstructed picture is the test's planes, with the
// host path of x265_amd/csrc/pichash.h beside it.  Built by the test against oracle/_ref/libx265ref{8,10,12}.so and the reference's headers.
//   pichash_ref MANIFEST IN OUT
//       MANIFEST = one line per case: NAME W H CSP CTU PAD OFFSET — CSP = 0 (4:0:0), 1 (4:2:0), 2 (4:2:2), 3 (4:4:4); CTU = param->maxCUSize; every plane of
//             the case lies in IN from byte OFFSET on, one after the other, rows of (plane width + PAD) samples of the build's pixel type (the padding holds
//             the test's poison)
//       OUT = JSON, per case and method (crc = --hash 2, sum = --hash 3):
//             rows        the running values m_crc[3] / m_checksum[3] after each per-row call (row, row * CTUs per row, the row's height), as
//                         FrameFilter::processPostRow makes them with one slice; planes the function does not write keep the sentinel 0x5a5a5a5a
//             digest      what crcFinish / checksumFinish make of the last of them, as hexadecimal strings
//             whole, whole_digest   the same after the single call (0, 0, picture height) of the multi-slice path
//             host_rows, host_whole pichash.h's host path, fed the same bands with the same running values
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define private public
#define protected public
#include "common.h"
#include "frame.h"
#include "picyuv.h"
#include "frameencoder.h"
#undef private
#undef protected

#include "../../x265_amd/csrc/pichash.h"

using namespace X265_NS;

static const uint32_t kSentinel = 0x5a5a5a5au;

struct Case
{
    std::string name;
    int w, h, csp, ctu, pad;
    size_t offset;
};

static void put3(FILE* f, const uint32_t v[3])
{
    fprintf(f, "[%u, %u, %u]", v[0], v[1], v[2]);
}

static void put_digest(FILE* f, int method, const uint32_t v[3], int planes)
{
    fprintf(f, "[");
    for (int k = 0; k < planes; k++)
    {
        uint8_t d[16] = { 0 };
        uint32_t s = v[k];
        if (method == 2)
            crcFinish(s, d);
        else
            checksumFinish(s, d);
        fprintf(f, "%s\"", k ? ", " : "");
        for (int i = 0; i < (method == 2 ? 2 : 4); i++)
            fprintf(f, "%02x", d[i]);
        fprintf(f, "\"");
    }
    fprintf(f, "]");
}

// pichash.h's restatement of one call of the function: the bands, the running values and the resets as the seam makes them
static void host_call(int method, PicYuv* pic, const x265_param* param, int row, int cuAddr, int height, uint32_t state[3])
{
    const int planes = param->internalCsp == X265_CSP_I400 ? 1 : 3;
    const int hs = CHROMA_H_SHIFT(param->internalCsp), vs = CHROMA_V_SHIFT(param->internalCsp);
    for (int k = 0; k < planes; k++)
    {
        const int w = k ? (int)(pic->m_picWidth >> hs) : (int)pic->m_picWidth, h = k ? height >> vs : height;
        const int64_t stride = k ? pic->m_strideC : pic->m_stride;
        const int y0 = row * (int)(k ? param->maxCUSize >> vs : param->maxCUSize);
        const pixel* p;
        if (method == XP_METHOD_CRC)
        {
            p = k == 0 ? pic->getLumaAddr(cuAddr) : (k == 1 ? pic->getCbAddr(cuAddr) : pic->getCrAddr(cuAddr));
            if (k || !row)
                state[k] = 0xffff;
        }
        else
        {
            p = pic->m_picOrg[k] + (intptr_t)y0 * stride;
            if (!row)
                state[k] = 0;
        }
        state[k] = xp_hash_plane(method, p, stride, w, h, y0, X265_DEPTH, state[k]);
    }
}

int main(int argc, char** argv)
{
    if (argc != 4)
    {
        fprintf(stderr, "usage: %s MANIFEST IN OUT\n", argv[0]);
        return 2;
    }
    std::vector<Case> cases;
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char name[256];
    Case c;
    while (fscanf(f, "%255s %d %d %d %d %d %zu", name, &c.w, &c.h, &c.csp, &c.ctu, &c.pad, &c.offset) == 7)
    {
        c.name = name;
        cases.push_back(c);
    }
    fclose(f);
    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    std::vector<char> in((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(in.data(), 1, in.size(), f) != in.size()) { fprintf(stderr, "%s: short read\n", argv[2]); return 2; }
    fclose(f);
    FILE* out = fopen(argv[3], "w");
    if (!out) { perror(argv[3]); return 2; }
    fprintf(out, "{\n");
    for (size_t ci = 0; ci < cases.size(); ci++)
    {
        const Case& cs = cases[ci];
        x265_param* param = x265_param_alloc();
        x265_param_default(param);
        param->internalCsp = cs.csp;
        param->sourceWidth = cs.w; param->sourceHeight = cs.h;
        param->internalBitDepth = X265_DEPTH;
        param->maxCUSize = cs.ctu;
        const int planes = cs.csp == X265_CSP_I400 ? 1 : 3;
        const int hs = CHROMA_H_SHIFT(cs.csp), vs = CHROMA_V_SHIFT(cs.csp);
        const int cw = (cs.w + cs.ctu - 1) / cs.ctu, rows = (cs.h + cs.ctu - 1) / cs.ctu;

        PicYuv* pic = new PicYuv;
        pic->m_param = param;
        pic->m_picWidth = cs.w; pic->m_picHeight = cs.h;
        pic->m_picCsp = cs.csp;
        pic->m_hChromaShift = hs; pic->m_vChromaShift = vs;
        pic->m_stride = cs.w + cs.pad;
        pic->m_strideC = planes == 3 ? (cs.w >> hs) + cs.pad : 0;
        size_t at = cs.offset;
        for (int k = 0; k < planes; k++)
        {
            const size_t bytes = (size_t)(k ? pic->m_strideC : pic->m_stride) * (k ? cs.h >> vs : cs.h) * sizeof(pixel);
            if (at + bytes > in.size()) { fprintf(stderr, "%s: case %s lies outside the input\n", argv[2], cs.name.c_str()); return 2; }
            pic->m_picOrg[k] = (pixel*)(in.data() + at);
            at += bytes;
        }
        std::vector<intptr_t> offY((size_t)cw * rows), offC((size_t)cw * rows);
        for (int r = 0; r < rows; r++)
            for (int col = 0; col < cw; col++)
            {
                // PicYuv::createOffsets (picyuv.cpp:164-165)
                offY[r * cw + col] = pic->m_stride * r * cs.ctu + col * cs.ctu;
                offC[r * cw + col] = pic->m_strideC * r * (cs.ctu >> vs) + col * (cs.ctu >> hs);
            }
        pic->m_cuOffsetY = offY.data();
        pic->m_cuOffsetC = offC.data();
        Frame* frame = new Frame;
        frame->m_reconPic = pic;
        FrameEncoder* fe = new FrameEncoder;
        fe->m_param = param;
        fe->m_frame = frame;

        fprintf(out, "%s\"%s\": {", ci ? ",\n" : "", cs.name.c_str());
        for (int method = 2; method <= 3; method++)
        {
            param->decodedPictureHashSEI = method;
            uint32_t* running = method == 2 ? fe->m_seiReconPictureDigest.m_crc : fe->m_seiReconPictureDigest.m_checksum;
            const char* tag = method == 2 ? "crc" : "sum";
            std::string hostRows;
            uint32_t host[3] = { kSentinel, kSentinel, kSentinel };
            running[0] = running[1] = running[2] = kSentinel;
            fprintf(out, "%s\"%s\": {\"rows\": [", method == 2 ? "" : ", ", tag);
            for (int r = 0; r < rows; r++)
            {
                const int height = cs.h - r * cs.ctu < cs.ctu ? cs.h - r * cs.ctu : cs.ctu;
                fe->initDecodedPictureHashSEI(r, r * cw, height);
                host_call(method, pic, param, r, r * cw, height, host);
                fprintf(out, "%s", r ? ", " : "");
                put3(out, running);
                char buf[96];
                snprintf(buf, sizeof(buf), "%s[%u, %u, %u]", r ? ", " : "", host[0], host[1], host[2]);
                hostRows += buf;
            }
            fprintf(out, "], \"host_rows\": [%s], \"digest\": ", hostRows.c_str());
            put_digest(out, method, running, planes);
            running[0] = running[1] = running[2] = kSentinel;
            host[0] = host[1] = host[2] = kSentinel;
            fe->initDecodedPictureHashSEI(0, 0, cs.h);
            host_call(method, pic, param, 0, 0, cs.h, host);
            fprintf(out, ", \"whole\": ");
            put3(out, running);
            fprintf(out, ", \"host_whole\": ");
            put3(out, host);
            fprintf(out, ", \"whole_digest\": ");
            put_digest(out, method, running, planes);
            fprintf(out, "}");
        }
        fprintf(out, "}");
        // (the objects point into this function's buffers: they are left to the process's end)
    }
    fprintf(out, "\n}\n");
    fclose(out);
    return 0;
}
