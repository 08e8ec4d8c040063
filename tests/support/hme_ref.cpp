// hme_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_lookahead_hme.py, tests/golden/make_hme_golden.py): the reference's own two-level lookahead estimate
// under --hme.  Lowres objects created and initialised with bEnableHME around the test's pictures, LookaheadTLD::lowresIntraEstimate and weightsAnalyse of the
// reference, and a CostEstimateGroup subclass calling estimateCUCost(…, hme) in the loop order of estimateFrameCost (serial) or processTasks (cooperative
// slices, run one after the other in slice order).  Built by the test against oracle/_ref/libx265ref{8,10,12}.so and the reference's headers.
//   hme_ref OUT CASE...
//       CASE = a file of int64 words followed by samples of the build's pixel type (tests/test_lookahead_hme.py: case_blob):
//             words   picW, picH, margin, frames (2 or 3), lookaheadSlices, method0, method1, range0, range1, weightp, then per frame wp_ssd[0], wp_sum[0]
//             data    per frame the padded picture: (picH + 2 margin) rows of (picW + 2 margin + 8) samples
//             two frames: the P estimate (p0, p1, b) = (0, 1, 1); three: the B estimate (0, 2, 1)
//       OUT = JSON per case (named after its file): "geom" (lumaStride, width, lines, planesize, padoffset, the two grids, rows per slice of both levels, slices),
//             "planes" / "lower" (position-weighted sums of the frames' lowres and lower-res buffers), "intraCost", per searched list "l0" / "l1": level-0 and level-1 vectors and
//             costs, per level-1 block numc, whether the fifth predictor was taken, whether it won the MVP choice; "lowresCosts",
//             "rowSatds", "costEst" (before the B scaling of estimateFrameCost), "costEstAq", "intraMbs", "weighted"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define private public
#define protected public
#include "common.h"
#include "primitives.h"
#include "picyuv.h"
#include "lowres.h"
#include "mv.h"
#include "slicetype.h"
#undef private
#undef protected

using namespace X265_NS;

namespace {

struct HmeGroup : public CostEstimateGroup
{
    HmeGroup(Lookahead& l, Lowres** f) : CostEstimateGroup(l, f) {}
    void cu(LookaheadTLD& tld, int x, int y, int p0, int p1, int b, bool doSearch[2], bool lastRow, int slice, bool hme)
    { estimateCUCost(tld, x, y, p0, p1, b, doSearch, lastRow, slice, hme); }
};

struct Block { int numc, fifth, won; };

// position-weighted sum of the samples modulo 2^64 (tests/test_lookahead_hme.py: plane_hash)
uint64_t plane_hash(const pixel* p, size_t n)
{
    uint64_t h = 0;
    for (size_t i = 0; i < n; i++) h += (uint64_t)(p[i] + 1) * ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull);
    return h;
}

template <typename T> void put(FILE* f, const char* name, const T* v, int n, const char* tail = ",")
{
    fprintf(f, "\"%s\": [", name);
    for (int i = 0; i < n; i++) fprintf(f, "%s%lld", i ? "," : "", (long long)v[i]);
    fprintf(f, "]%s\n", tail);
}

// what the level-1 call of estimateCUCost is about to see for list i of block (cuX, cuY): the candidates of slicetype.cpp:3270-3285 read from the frame's own
// arrays, and which of them the SATD comparison of :3297-3302 picks.  A witness beside the reference's run, not a part of it.
Block witness(Lookahead& la, Lowres* fenc, ReferencePlanes* fref, int i, int dist, int cuX, int cuY, bool lastRow)
{
    const int W = la.m_8x8Width;
    const int cuXY = cuX + cuY * W, k = (cuX / 2) + (cuY / 2) * W / 2;
    MV* mv = &fenc->lowresMvs[i][dist][cuXY];
    MV mvc[5];
    Block b = { 0, 0, 0 };
    if (cuX < W - 1) mvc[b.numc++] = mv[1];
    if (!lastRow)
    {
        mvc[b.numc++] = mv[W];
        if (cuX > 0) mvc[b.numc++] = mv[W - 1];
        if (cuX < W - 1) mvc[b.numc++] = mv[W + 1];
    }
    if (fenc->lowerResMvCosts[i][dist][k] > 0)
    {
        mvc[b.numc++] = fenc->lowerResMvs[i][dist][k] * 2;
        b.fifth = 1;
    }
    const intptr_t pelOffset = 8 * cuX + 8 * cuY * fenc->lumaStride;
    int best = 1 << 28, at = -1;
    for (int c = 0; c < b.numc; c++)
    {
        ALIGN_VAR_32(pixel, buf[64]);
        intptr_t stride = 8;
        pixel* src = fref->lowresMC(pelOffset, mvc[c], buf, stride, 0);
        int cost = primitives.pu[LUMA_8x8].satd(fenc->lowresPlane[0] + pelOffset, fenc->lumaStride, src, stride);
        if (cost < best) { best = cost; at = c; }
    }
    b.won = b.fifth && at == b.numc - 1;
    return b;
}

int run_case(const char* path, FILE* out, bool first)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "hme_ref: cannot read %s\n", path); return 2; }
    int64_t w[10];
    if (fread(w, 8, 10, f) != 10) return 2;
    const int picW = (int)w[0], picH = (int)w[1], margin = (int)w[2], frames = (int)w[3], slices = (int)w[4];
    int64_t wp[3][2];
    if (frames < 2 || frames > 3 || fread(wp, 16, frames, f) != (size_t)frames) return 2;
    const intptr_t stride = picW + 2 * margin + 8;
    const size_t elems = (size_t)stride * (picH + 2 * margin);
    std::vector<std::vector<pixel> > data(frames, std::vector<pixel>(elems));
    for (int i = 0; i < frames; i++)
        if (fread(data[i].data(), sizeof(pixel), elems, f) != elems) return 2;
    fclose(f);

    x265_param* param = x265_param_alloc();
    x265_param_default(param);
    param->sourceWidth = picW;
    param->sourceHeight = picH;
    param->rc.aqMode = 0;
    param->rc.hevcAq = 0;
    param->bAQMotion = 0;
    param->bEnableHME = 1;
    param->hmeSearchMethod[0] = (int)w[5];
    param->hmeSearchMethod[1] = (int)w[6];
    param->hmeRange[0] = (int)w[7];
    param->hmeRange[1] = (int)w[8];
    param->bEnableWeightedPred = (int)w[9];
    param->bEnableWeightedBiPred = 0;
    param->lookaheadSlices = 0;
    param->bframes = 3;
    PicYuv pics[3];
    Lowres lr[3];
    bool ok = true;
    for (int i = 0; i < frames; i++)
    {
        pics[i].m_picWidth = picW;
        pics[i].m_picHeight = picH;
        pics[i].m_lumaMarginX = margin;
        pics[i].m_lumaMarginY = margin;
        pics[i].m_stride = stride;
        pics[i].m_picOrg[0] = data[i].data() + (size_t)margin * stride + margin;
        pics[i].m_param = param;
        memset((void*)&lr[i], 0, sizeof(Lowres));
        ok = ok && lr[i].create(param, &pics[i], param->rc.qgSize);
    }
    if (!ok) { fprintf(stderr, "hme_ref: Lowres::create failed\n"); return 3; }
    for (int i = 0; i < frames; i++)
    {
        lr[i].init(&pics[i], i);
        lr[i].wp_ssd[0] = wp[i][0];
        lr[i].wp_sum[0] = wp[i][1];
    }
    Lookahead la(param, NULL);
    la.create();
    LookaheadTLD& tld = la.m_tld[0];
    const int p0 = 0, b = 1, p1 = frames == 3 ? 2 : 1;
    const bool bidir = p1 > b;
    tld.lowresIntraEstimate(lr[b], param->rc.qgSize);
    Lowres* fr[3] = { &lr[0], &lr[1], &lr[2] };
    HmeGroup g(la, fr);
    Lowres* fenc = fr[b];
    const int W8 = la.m_8x8Width, H8 = la.m_8x8Height, W4 = la.m_4x4Width, H4 = la.m_4x4Height;
    // the slice geometry of the Lookahead constructor (slicetype.cpp:1028-1040), which refuses slices without a pool and below 720 lines
    int rows8 = H8, nSlices = 1;
    if (slices > 1)
    {
        rows8 = H8 / slices;
        rows8 = rows8 > 10 ? rows8 : 10;
        rows8 = rows8 < H8 ? rows8 : H8;
        nSlices = H8 / rows8;
    }
    la.m_numRowsPerSlice = rows8;
    la.m_numCoopSlices = nSlices;
    param->lookaheadSlices = nSlices > 1 ? nSlices : 0;
    int rows4 = H4;
    if (nSlices > 1)
    {
        rows4 = H4 / nSlices;
        rows4 = rows4 > 5 ? rows4 : 5;
        rows4 = rows4 < H4 ? rows4 : H4;
    }

    // estimateFrameCost's preamble (:3125-3141)
    bool doSearch[2] = { true, bidir };
    fenc->weightedRef[b - p0].isWeighted = false;
    if (param->bEnableWeightedPred)
        tld.weightsAnalyse(*fr[b], *fr[p0]);
    fenc->costEst[b - p0][p1 - b] = 0;
    fenc->costEstAq[b - p0][p1 - b] = 0;
    memset(g.m_slice, 0, sizeof(g.m_slice));
    std::vector<Block> blocks[2];
    blocks[0].resize(W8 * H8);
    blocks[1].resize(W8 * H8);
    ReferencePlanes* wfref0 = fenc->weightedRef[b - p0].isWeighted ? &fenc->weightedRef[b - p0] : (ReferencePlanes*)fr[p0];
    for (int sl = 0; sl < nSlices; sl++)
    {
        const int slice = nSlices > 1 ? sl : -1;
        int firstY = rows4 * sl, lastY = sl == nSlices - 1 ? H4 - 1 : rows4 * (sl + 1) - 1;
        bool lastRow = true;
        for (int cuY = lastY; cuY >= firstY; cuY--)
        {
            for (int cuX = W4 - 1; cuX >= 0; cuX--)
                g.cu(tld, cuX, cuY, p0, p1, b, doSearch, lastRow, slice, true);
            lastRow = false;
        }
        firstY = rows8 * sl;
        lastY = sl == nSlices - 1 ? H8 - 1 : rows8 * (sl + 1) - 1;
        lastRow = true;
        for (int cuY = lastY; cuY >= firstY; cuY--)
        {
            fenc->rowSatds[b - p0][p1 - b][cuY] = 0;
            for (int cuX = W8 - 1; cuX >= 0; cuX--)
            {
                blocks[0][cuX + cuY * W8] = witness(la, fenc, wfref0, 0, b - p0, cuX, cuY, lastRow);
                if (bidir)
                {
                    // list 1's candidates do not depend on list 0's search of the same block, so both witnesses may precede the call
                    blocks[1][cuX + cuY * W8] = witness(la, fenc, fr[p1], 1, p1 - b, cuX, cuY, lastRow);
                }
                g.cu(tld, cuX, cuY, p0, p1, b, doSearch, lastRow, slice, false);
            }
            lastRow = false;
        }
    }
    int64_t costEst = fenc->costEst[b - p0][p1 - b], costEstAq = fenc->costEstAq[b - p0][p1 - b];
    int intraMbs = fenc->intraMbs[b - p0];
    for (int sl = 0; nSlices > 1 && sl < nSlices; sl++)
    {
        costEst += g.m_slice[sl].costEst;
        costEstAq += g.m_slice[sl].costEstAq;
        if (!bidir) intraMbs += g.m_slice[sl].intraMbs;
    }

    std::string name(path);
    name = name.substr(name.find_last_of('/') + 1);
    fprintf(out, "%s\"%s\": {\n", first ? "" : ",", name.c_str());
    const size_t planesize = (size_t)fenc->lumaStride * (fenc->lines + 2 * margin);
    const long long geom[12] = { (long long)fenc->lumaStride, fenc->width, fenc->lines, (long long)planesize, (long long)(fenc->lumaStride * margin + margin),
                                 W8, H8, W4, H4, rows8, rows4, nSlices };
    put(out, "geom", geom, 12);
    fprintf(out, "\"planes\": [");
    for (int i = 0; i < frames; i++) fprintf(out, "%s\"%016llx\"", i ? "," : "", (unsigned long long)plane_hash(lr[i].buffer[0], 4 * planesize));
    fprintf(out, "],\n\"lower\": [");
    for (int i = 0; i < frames; i++) fprintf(out, "%s\"%016llx\"", i ? "," : "", (unsigned long long)plane_hash(lr[i].lowerResBuffer[0], 4 * (planesize / 2)));
    fprintf(out, "],\n");
    put(out, "intraCost", fenc->intraCost, W8 * H8);
    for (int i = 0; i < 1 + bidir; i++)
    {
        const int dist = i ? p1 - b : b - p0;
        std::vector<int> v;
        fprintf(out, "\"l%d\": {\n", i);
        for (int k = 0; k < W4 * H4; k++) { v.push_back(fenc->lowerResMvs[i][dist][k].x); v.push_back(fenc->lowerResMvs[i][dist][k].y); }
        put(out, "mvs0", v.data(), (int)v.size());
        put(out, "costs0", fenc->lowerResMvCosts[i][dist], W4 * H4);
        v.clear();
        for (int k = 0; k < W8 * H8; k++) { v.push_back(fenc->lowresMvs[i][dist][k].x); v.push_back(fenc->lowresMvs[i][dist][k].y); }
        put(out, "mvs1", v.data(), (int)v.size());
        put(out, "costs1", fenc->lowresMvCosts[i][dist], W8 * H8);
        std::vector<int> numc, fifth, won;
        for (const Block& bl : blocks[i]) { numc.push_back(bl.numc); fifth.push_back(bl.fifth); won.push_back(bl.won); }
        put(out, "numc", numc.data(), W8 * H8);
        put(out, "fifth", fifth.data(), W8 * H8);
        put(out, "won", won.data(), W8 * H8, "");
        fprintf(out, "},\n");
    }
    put(out, "lowresCosts", fenc->lowresCosts[b - p0][p1 - b], W8 * H8);
    put(out, "rowSatds", fenc->rowSatds[b - p0][p1 - b], H8);
    fprintf(out, "\"costEst\": %lld, \"costEstAq\": %lld, \"intraMbs\": %d, \"weighted\": %d\n}\n", (long long)costEst, (long long)costEstAq, intraMbs,
            fenc->weightedRef[b - p0].isWeighted ? 1 : 0);

    la.destroy();
    for (int i = 0; i < frames; i++)
    {
        lr[i].destroy();
        pics[i].m_picOrg[0] = NULL;
        pics[i].m_param = NULL;
    }
    x265_param_free(param);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: hme_ref OUT CASE...\n"); return 1; }
    x265_param* p = x265_param_alloc();
    x265_param_default(p);
    x265_setup_primitives(p);
    x265_param_free(p);
    FILE* out = fopen(argv[1], "w");
    if (!out) return 1;
    fprintf(out, "{\n");
    for (int i = 2; i < argc; i++)
    {
        int e = run_case(argv[i], out, i == 2);
        if (e) return e;
    }
    fprintf(out, "}\n");
    fclose(out);
    return 0;
}
