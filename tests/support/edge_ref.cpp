// edge_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_edgeplanes.py, tests/golden/make_edgeplanes_golden.py): the reference's own edgeFilter on a Frame
// built around the test's planes, and the host path of x265_amd/csrc/edgepass.h beside it.  Built by the test against oracle/_ref/libx265ref{8,10,12}.so
// and the reference's headers.
//   edge_ref planes W H MARGINX MARGINY CTU IN OUT
//       IN  = the source buffer, (ceil(H / CTU) * CTU + 2 * MARGINY) rows of W + 2 * MARGINX samples (the picture's sample (0, 0) at row MARGINY, column
//             MARGINX), samples of the build's pixel type
//       OUT = five buffers of the same shape — the reference's m_edgePic and m_thetaPic after edgeFilter, the edge plane, the angle plane with provisional
//             values and the angle plane with the doubt list resolved as edgepass.h + the binding's rule give them (memsets included) — then uint32 n and the
//             n entries of the doubt list
//       stdout: the nine specials (made like the binding makes them)
//   edge_ref specials
//       for each of the nine special directions: every gradient magnitude that 3x3 patches of this pixel range can produce, through computeEdge;
//       one line per direction: index, smallest angle seen, largest angle seen, magnitudes tried
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define private public
#define protected public
#include "common.h"
#include "frame.h"
#include "picyuv.h"
#include "slicetype.h"
#undef private
#undef protected

#include "../../x265_amd/csrc/edgepass.h"

namespace X265_NS {
void edgeFilter(Frame* curFrame, x265_param* param);         // slicetype.cpp:151 (not declared in slicetype.h)
}
using namespace X265_NS;

static pixel patch_angle(pixel* patch)
{
    pixel e[9], t[9];
    computeEdge(e, patch, t, 3, 3, 3, true);
    return t[4];
}

// patch index: 0 tl, 1 tm, 2 tr, 3 ml, 4 centre, 5 mr, 6 bl, 7 bm, 8 br
static void make_specials(uint16_t* sp)
{
    for (int sv = -1; sv <= 1; sv++)
        for (int sh = -1; sh <= 1; sh++)
        {
            pixel patch[9] = { 0, (pixel)(sv < 0), 0, (pixel)(sh < 0), 0, (pixel)(sh > 0), 0, (pixel)(sv > 0), 0 };
            sp[(sv + 1) * 3 + sh + 1] = patch_angle(patch);
        }
}

static int specials_mode()
{
    const int pmax = (1 << X265_DEPTH) - 1;
    for (int sv = -1; sv <= 1; sv++)
        for (int sh = -1; sh <= 1; sh++)
        {
            int lo = 1 << 30, hi = -1, tried = 0;
            if (!sv && !sh)
            {
                const int flat[3] = { 0, 1, pmax };
                for (int i = 0; i < 3; i++)
                {
                    pixel patch[9];
                    for (int j = 0; j < 9; j++) patch[j] = (pixel)flat[i];
                    const int a = patch_angle(patch);
                    lo = a < lo ? a : lo; hi = a > hi ? a : hi; tried++;
                }
            }
            else
            {
                // |gradient| = m: m = 6 a + 10 b on an axis (two corners a, one edge sample b), m = 3 a + 10 b on a diagonal (one corner, two edge samples)
                const int ca = sv && sh ? 3 : 6;
                for (int m = 1; m <= 16 * pmax; m++)
                {
                    int a = -1, b = m / 10 < pmax ? m / 10 : pmax;
                    for (; b >= 0; b--)
                        if ((m - 10 * b) % ca == 0 && (m - 10 * b) / ca <= pmax) { a = (m - 10 * b) / ca; break; }
                    if (a < 0)
                        continue;
                    pixel patch[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
                    if (sv && sh)
                    {
                        patch[(sv > 0 ? 6 : 0) + (sh > 0 ? 2 : 0)] = (pixel)a;
                        patch[sh > 0 ? 5 : 3] = (pixel)b;
                        patch[sv > 0 ? 7 : 1] = (pixel)b;
                    }
                    else if (sh)
                    {
                        patch[sh > 0 ? 2 : 0] = patch[sh > 0 ? 8 : 6] = (pixel)a;
                        patch[sh > 0 ? 5 : 3] = (pixel)b;
                    }
                    else
                    {
                        patch[sv > 0 ? 6 : 0] = patch[sv > 0 ? 8 : 2] = (pixel)a;
                        patch[sv > 0 ? 7 : 1] = (pixel)b;
                    }
                    int h, v;
                    const int g[9] = { patch[0], patch[1], patch[2], patch[3], patch[4], patch[5], patch[6], patch[7], patch[8] };
                    xe_sobel(g + 4, (int64_t)3, &h, &v);
                    if (h != sh * m || v != sv * m || xe_special_index(h, v) != (sv + 1) * 3 + sh + 1)
                    {
                        fprintf(stderr, "patch for (%d, %d) x %d gives (%d, %d)\n", sh, sv, m, h, v);
                        return 3;
                    }
                    const int ang = patch_angle(patch);
                    lo = ang < lo ? ang : lo; hi = ang > hi ? ang : hi; tried++;
                }
            }
            printf("%d %d %d %d\n", (sv + 1) * 3 + sh + 1, lo, hi, tried);
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "specials"))
        return specials_mode();
    if (argc != 9 || strcmp(argv[1], "planes")) { fprintf(stderr, "usage: %s planes W H MARGINX MARGINY CTU IN OUT | specials\n", argv[0]); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), mx = atoi(argv[4]), my = atoi(argv[5]), ctu = atoi(argv[6]);
    const intptr_t stride = w + 2 * mx;
    const int rows = (h + ctu - 1) / ctu * ctu + 2 * my;
    const size_t n = (size_t)stride * rows;
    std::vector<pixel> src(n), refEdge(n, 0x55), refGauss(n, 0x55), refTheta(n, 0x55), edge(n, 0), theta(n, 0), resolved(n, 0);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(src.data(), sizeof(pixel), n, f) != n) { fprintf(stderr, "%s: not %zu samples\n", argv[7], n); return 2; }
    fclose(f);
    const intptr_t org = (intptr_t)my * stride + mx;

    // ---- the reference
    PicYuv* pic = new PicYuv;
    pic->m_picWidth = w; pic->m_picHeight = h; pic->m_stride = stride; pic->m_lumaMarginX = mx; pic->m_lumaMarginY = my;
    pic->m_picOrg[0] = src.data() + org;
    Frame* frame = new Frame;
    frame->m_fencPic = pic;
    frame->m_edgePic = refEdge.data(); frame->m_gaussianPic = refGauss.data(); frame->m_thetaPic = refTheta.data();
    x265_param param;
    memset(&param, 0, sizeof(param));
    param.maxCUSize = ctu;
    edgeFilter(frame, &param);

    // ---- edgepass.h on the host
    uint16_t specials[XE_SPECIALS];
    make_specials(specials);
    for (int i = 0; i < XE_SPECIALS; i++)
        printf(i ? " %d" : "%d", specials[i]);
    printf("\n");
    const pixel* s = src.data() + org;
    const int T = xe_threshold(X265_DEPTH);
    std::vector<int> G((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            G[(size_t)y * w + x] = xe_gauss_at(s, (int64_t)stride, x, y, w, h);
    std::vector<uint32_t> doubts;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
        {
            int e = s[y * stride + x], a = 0;
            if (xe_sobel_applies(y, x, w, h))
            {
                int gh, gv;
                xe_sobel(&G[(size_t)y * w + x], (int64_t)w, &gh, &gv);
                e = xe_is_edge(gh, gv, T) ? T : 0;
                if (xe_angle(gh, gv, specials, &a) == XE_DOUBTFUL)
                    doubts.push_back(xe_doubt_pack(x, y));
            }
            edge[org + y * stride + x] = (pixel)e;
            theta[org + y * stride + x] = (pixel)a;
        }
    resolved = theta;
    for (size_t i = 0; i < doubts.size(); i++)
    {
        const int x = xe_doubt_x(doubts[i]), y = xe_doubt_y(doubts[i]);
        pixel patch[9];
        for (int j = 0; j < 9; j++)
            patch[j] = (pixel)xe_gauss_at(s, (int64_t)stride, x - 1 + j % 3, y - 1 + j / 3, w, h);
        resolved[org + y * stride + x] = patch_angle(patch);
    }
    f = fopen(argv[8], "wb");
    if (!f) { perror(argv[8]); return 2; }
    const uint32_t nd = (uint32_t)doubts.size();
    fwrite(refEdge.data(), sizeof(pixel), n, f);
    fwrite(refTheta.data(), sizeof(pixel), n, f);
    fwrite(edge.data(), sizeof(pixel), n, f);
    fwrite(theta.data(), sizeof(pixel), n, f);
    fwrite(resolved.data(), sizeof(pixel), n, f);
    fwrite(&nd, 4, 1, f);
    fwrite(doubts.data(), 4, nd, f);
    fclose(f);
    return 0;
}
