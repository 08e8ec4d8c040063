// hist_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_scenestats.py, tests/golden/make_scenestats_golden.py): the reference's own Encoder::computeHistograms
// on an x265_picture around the test's planes and its computeEdge on a strided plane, with the host path of x265_amd/csrc/scenestats.h beside them.  Built by
// the test against oracle/_ref/libx265ref{8,10,12}.so and the reference's headers.
//   hist_ref hist W H CSP PICDEPTH RSKIP REF IN OUT
//       IN  = the picture's planes one after the other, packed (row pitch = width), 1-byte samples when PICDEPTH is 8, else 2-byte; CSP = 0 (4:0:0),
//             1 (4:2:0), 2 (4:2:2), 3 (4:4:4); RSKIP = param->recursionSkipMode; REF = 0: do not call the reference (a picture with samples out of range
//             makes it index past its arrays)
//       OUT = int32 values: the range-error count of scenestats.h, then the reference's m_curEdgeHist[2], scenestats.h's two edge bins, the reference's
//             m_curYUVHist[3][bins] (planes the function does not write keep the sentinel -7), scenestats.h's, the reference's m_edgePic (W x H) and
//             scenestats.h's edge plane with the ring zeroed
//   hist_ref bits W H STRIDE IN OUT
//       IN  = H rows of STRIDE samples of the build's pixel type; OUT = int32 values: the plane computeEdge(plane, IN, NULL, STRIDE, H, W, false, 1) leaves
//             when every sample held 0x5A before, and scenestats.h's (interior only, written over the same sentinel)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define private public
#define protected public
#include "common.h"
#include "primitives.h"
#include "encoder.h"
#include "slicetype.h"
#undef private
#undef protected

#include "../../x265_amd/csrc/scenestats.h"

using namespace X265_NS;

static void put(FILE* f, const std::vector<int32_t>& v) { fwrite(v.data(), 4, v.size(), f); }

static int bits_mode(char** argv)
{
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    const intptr_t stride = atoi(argv[4]);
    const size_t n = (size_t)stride * h;
    std::vector<pixel> src(n), ref(n, (pixel)0x5A);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(src.data(), sizeof(pixel), n, f) != n) { fprintf(stderr, "%s: not %zu samples\n", argv[5], n); return 2; }
    fclose(f);
    if (!computeEdge(ref.data(), src.data(), NULL, stride, h, w, false, 1))
        return 3;
    std::vector<int32_t> a(n), b(n, 0x5A);
    for (size_t i = 0; i < n; i++)
        a[i] = ref[i];
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            const int e = xs_edge_bit(&src[y * stride + x], (int64_t)stride, y, x, w, h, X265_DEPTH);
            if (e >= 0)
                b[y * stride + x] = e;
        }
    f = fopen(argv[6], "wb");
    if (!f) { perror(argv[6]); return 2; }
    put(f, a);
    put(f, b);
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "bits"))
        return bits_mode(argv);
    if (argc != 10 || strcmp(argv[1], "hist"))
    {
        fprintf(stderr, "usage: %s hist W H CSP PICDEPTH RSKIP REF IN OUT | bits W H STRIDE IN OUT\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[2]), h = atoi(argv[3]), csp = atoi(argv[4]), picDepth = atoi(argv[5]), rskip = atoi(argv[6]), callRef = atoi(argv[7]);
    const int planes = csp == X265_CSP_I400 ? 1 : 3, bins = xs_bins(X265_DEPTH), sb = picDepth == 8 ? 1 : 2;
    int pw[3], ph[3];
    size_t off[3], total = 0;
    for (int k = 0; k < 3; k++)
    {
        pw[k] = k ? w >> CHROMA_H_SHIFT(csp) : w;
        ph[k] = k ? h >> CHROMA_V_SHIFT(csp) : h;
        off[k] = total;
        if (k < planes)
            total += (size_t)pw[k] * ph[k] * sb;
    }
    std::vector<char> in(total);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(in.data(), 1, total, f) != total) { fprintf(stderr, "%s: not %zu bytes\n", argv[8], total); return 2; }
    fclose(f);

    std::vector<int32_t> refEdge(2, -7), refHist((size_t)3 * bins, -7), refPlane((size_t)w * h, 0);
    if (callRef)
    {
        x265_param* param = x265_param_alloc();
        x265_param_default(param);
        param->internalCsp = csp;
        param->sourceWidth = w; param->sourceHeight = h;
        param->internalBitDepth = X265_DEPTH; param->sourceBitDepth = picDepth;
        param->bHistBasedSceneCut = 1;
        param->recursionSkipMode = rskip;
        x265_setup_primitives(param);
        Encoder* enc = new Encoder;
        enc->m_param = param;
        std::vector<pixel> edgePic((size_t)w * h, (pixel)0x5A);
        std::vector<pixel> conv[3];
        enc->m_edgePic = edgePic.data();
        for (int k = 0; k < 3; k++)
        {
            enc->m_planeSizes[k] = k < planes ? pw[k] * ph[k] : 0;
            conv[k].assign((size_t)pw[k] * ph[k] + 64, (pixel)0x33);
            enc->m_inputPic[k] = conv[k].data();
            for (int b = 0; b < bins; b++)
                enc->m_curYUVHist[k][b] = -7;
        }
        enc->m_curEdgeHist[0] = enc->m_curEdgeHist[1] = -7;
        x265_picture pic;
        x265_picture_init(param, &pic);
        pic.bitDepth = picDepth;
        pic.colorSpace = csp;
        pic.width = w; pic.height = h;
        for (int k = 0; k < planes; k++)
        {
            pic.planes[k] = in.data() + off[k];
            pic.stride[k] = pw[k] * sb;
        }
        if (!enc->computeHistograms(&pic))
            return 3;
        refEdge[0] = enc->m_curEdgeHist[0]; refEdge[1] = enc->m_curEdgeHist[1];
        for (int k = 0; k < 3; k++)
            for (int b = 0; b < bins; b++)
                refHist[(size_t)k * bins + b] = enc->m_curYUVHist[k][b];
        for (size_t i = 0; i < (size_t)w * h; i++)
            refPlane[i] = edgePic[i];
    }

    // ---- scenestats.h on the host
    int conv, shift, mask, sampleBytes;
    xs_conversion_of(picDepth, X265_DEPTH, &conv, &shift, &mask, &sampleBytes);
    if (sampleBytes != sb)
        return 4;
    std::vector<int32_t> errs(1, 0), edge(2, 0), hist((size_t)3 * bins, -7), plane((size_t)w * h, 0);
    std::vector<int> luma((size_t)w * h);
    for (int k = 0; k < planes; k++)
    {
        for (int b = 0; b < bins; b++)
            hist[(size_t)k * bins + b] = 0;
        for (size_t i = 0; i < (size_t)pw[k] * ph[k]; i++)
        {
            const int s = sb == 1 ? ((const uint8_t*)(in.data() + off[k]))[i] : ((const uint16_t*)(in.data() + off[k]))[i];
            const int v = xs_convert(s, conv, shift, mask, (int)sizeof(pixel));
            if (!k)
                luma[i] = v;
            if (v >= bins)
                errs[0]++;
            else
                hist[(size_t)k * bins + v]++;
        }
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            const int e = xs_edge_bit(&luma[(size_t)y * w + x], (int64_t)w, y, x, w, h, X265_DEPTH);
            plane[(size_t)y * w + x] = e > 0;
            edge[1] += e > 0;
        }
    edge[0] = w * h - edge[1];
    f = fopen(argv[9], "wb");
    if (!f) { perror(argv[9]); return 2; }
    put(f, errs);
    put(f, refEdge);
    put(f, edge);
    put(f, refHist);
    put(f, hist);
    put(f, refPlane);
    put(f, plane);
    fclose(f);
    return 0;
}
