// wpcost_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_wpcost.py, tests/golden/make_wpcost_golden.py): the reference's own weightAnalyse
// (source/encoder/weightPrediction.cpp:222-505) on a Frame / Slice / Lowres around the test's planes, with the table slots the function calls wrapped so that
// every evaluation it makes is logged, and the host path of x265_amd/csrc/wpcost.h beside it.  Built by the test against oracle/_ref/libx265ref{8,10,12}.so
// and the reference's headers.
//   wpcost_ref OUT CASE...
//       CASE = a file of int64 words followed by samples of the build's pixel type (tests/test_wpcost.py: case_blob):
//             words   csp, picW, picH, marginX, marginY, sliceIsB, bframes, poc, lists, then fenc wp_sum[3], wp_ssd[3], then per list: refPoc, hasMvs,
//                     wp_sum[3], wp_ssd[3]
//             data    the frame: lowres plane 0, cb, cr (padded buffers), intraCost (int32 per lowres block); per list: the reference's four lowres planes, cb,
//                     cr (padded buffers), vectors (two int32 per lowres block)
//             lowres buffers are (lines + 2 marginY) rows of (width + 2 marginX) samples, width and lines = picW / 2 and picH / 2 rounded up to whole 8x8
//             blocks (Lowres::create); chroma buffers likewise from the chroma extents and twice the margins
//             shifted by the chroma shifts.  The chroma borders of the references arrive NOT extended: the function extends them.
//       OUT = JSON, per case (named after its file): "evals": every evaluation in the order the function made it — plane, list, present, w, o, d, total, blocks,
//             and host_total / host_blocks from wpcost.h over the same planes, clip0 / clipmax (weighted samples that met the clip); "table": the slice's
//             weights of reference 0 per list; "calls": how often each compensation slot ran; "luma" / "chroma": the branches and clipped sides wpcost.h
//             finds in the vectors; "extended": whether the function extended the references' chroma borders
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define private public
#define protected public
#include "common.h"
#include "primitives.h"
#include "frame.h"
#include "picyuv.h"
#include "lowres.h"
#include "slice.h"
#include "mv.h"
#undef private
#undef protected

#include "../../x265_amd/csrc/wpcost.h"

namespace X265_NS { void weightAnalyse(Slice& slice, Frame& frame, x265_param& param); }
using namespace X265_NS;

namespace {

struct Eval
{
    int plane, list, present, w, o, d;
    std::vector<uint32_t> blocks;
};

struct Range { const pixel* lo; const pixel* hi; bool has(const void* p) const { return (const pixel*)p >= lo && (const pixel*)p < hi; } };

// what the wrappers know about the run
struct Run
{
    Range fenc[3] = {};              // the frame's lowres plane 0, cb, cr buffers
    const pixel* orig[3] = {};       // their sample (0, 0)
    Range ref[2][2] = {};            // per list: the lowres buffers, the chroma buffers
    int curList = 0;
    bool pending = false;            // a weight_pp call not yet followed by its first SATD
    int pw = 0, po = 0, pd = 0;
    std::vector<Eval> evals;
    long calls[8] = {};              // copy 8x8, pixelavg, chroma copy, hpp, vpp, hps, vsp, weight_pp
} g;

EncoderPrimitives g_orig;

void touch(const void* p)
{
    for (int l = 0; l < 2; l++)
        if (g.ref[l][0].has(p) || g.ref[l][1].has(p))
            g.curList = l;
}

void w_copy8(pixel* dst, intptr_t ds, const pixel* src, intptr_t ss) { g.calls[0]++; touch(src); g_orig.cu[BLOCK_8x8].copy_pp(dst, ds, src, ss); }
void w_avg0(pixel* dst, intptr_t ds, const pixel* a, intptr_t as, const pixel* b, intptr_t bs, int w)
{ g.calls[1]++; touch(a); g_orig.pu[LUMA_8x8].pixelavg_pp[0](dst, ds, a, as, b, bs, w); }
void w_avg1(pixel* dst, intptr_t ds, const pixel* a, intptr_t as, const pixel* b, intptr_t bs, int w)
{ g.calls[1]++; touch(a); g_orig.pu[LUMA_8x8].pixelavg_pp[1](dst, ds, a, as, b, bs, w); }
int g_csp;
void w_ccopy(pixel* dst, intptr_t ds, const pixel* src, intptr_t ss) { g.calls[2]++; touch(src); g_orig.chroma[g_csp].pu[LUMA_16x16].copy_pp(dst, ds, src, ss); }
void w_hpp(const pixel* src, intptr_t ss, pixel* dst, intptr_t ds, int c) { g.calls[3]++; touch(src); g_orig.chroma[g_csp].pu[LUMA_16x16].filter_hpp(src, ss, dst, ds, c); }
void w_vpp(const pixel* src, intptr_t ss, pixel* dst, intptr_t ds, int c) { g.calls[4]++; touch(src); g_orig.chroma[g_csp].pu[LUMA_16x16].filter_vpp(src, ss, dst, ds, c); }
void w_hps(const pixel* src, intptr_t ss, int16_t* dst, intptr_t ds, int c, int ext)
{ g.calls[5]++; touch(src); g_orig.chroma[g_csp].pu[LUMA_16x16].filter_hps(src, ss, dst, ds, c, ext); }
void w_vsp(const int16_t* src, intptr_t ss, pixel* dst, intptr_t ds, int c) { g.calls[6]++; g_orig.chroma[g_csp].pu[LUMA_16x16].filter_vsp(src, ss, dst, ds, c); }
void w_weight(const pixel* src, pixel* dst, intptr_t stride, int width, int height, int w0, int round, int shift, int offset)
{
    g.calls[7]++;
    touch(src);
    g.pending = true;
    g.pw = w0; g.pd = shift - (14 - X265_DEPTH); g.po = offset >> (X265_DEPTH - 8);
    g_orig.weight_pp(src, dst, stride, width, height, w0, round, shift, offset);
}
int log_satd(int v, const pixel* r, const pixel* f)
{
    touch(r);
    int plane = -1;
    for (int k = 0; k < 3; k++)
        if (g.fenc[k].has(f))
            plane = k;
    if (plane < 0) { fprintf(stderr, "wpcost_ref: a SATD outside the frame's planes\n"); exit(3); }
    if (f == g.orig[plane])
    {
        Eval e;
        e.plane = plane; e.list = g.curList; e.present = g.pending;
        e.w = g.pending ? g.pw : 0; e.o = g.pending ? g.po : 0; e.d = g.pending ? g.pd : 0;
        g.pending = false;
        g.evals.push_back(e);
    }
    if (g.evals.empty()) { fprintf(stderr, "wpcost_ref: a SATD before the first block of a plane\n"); exit(3); }
    g.evals.back().blocks.push_back((uint32_t)v);
    return v;
}
int w_satd8(const pixel* r, intptr_t rs, const pixel* f, intptr_t fs) { return log_satd(g_orig.pu[LUMA_8x8].satd(r, rs, f, fs), r, f); }
int w_satd16(const pixel* r, intptr_t rs, const pixel* f, intptr_t fs) { return log_satd(g_orig.pu[LUMA_16x16].satd(r, rs, f, fs), r, f); }

struct Reader
{
    std::vector<char> buf; size_t at = 0;
    int64_t word() { int64_t v; memcpy(&v, buf.data() + at, 8); at += 8; return v; }
    void* take(size_t bytes)
    {
        if (at + bytes > buf.size()) { fprintf(stderr, "wpcost_ref: a case file is short\n"); exit(2); }
        void* p = buf.data() + at; at += bytes; return p;
    }
};

struct Planes { pixel* low[4]; pixel* c[2]; };

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s OUT CASE...\n", argv[0]); return 2; }
    x265_param* param = x265_param_alloc();
    x265_param_default(param);
    x265_setup_primitives(param);
    g_orig = primitives;
    FILE* out = fopen(argv[1], "w");
    if (!out) { perror(argv[1]); return 2; }
    fprintf(out, "{\n");
    for (int ci = 2; ci < argc; ci++)
    {
        Reader rd;
        FILE* f = fopen(argv[ci], "rb");
        if (!f) { perror(argv[ci]); return 2; }
        fseek(f, 0, SEEK_END);
        rd.buf.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(rd.buf.data(), 1, rd.buf.size(), f) != rd.buf.size()) { fprintf(stderr, "%s: short read\n", argv[ci]); return 2; }
        fclose(f);
        const int csp = (int)rd.word(), picW = (int)rd.word(), picH = (int)rd.word(), mX = (int)rd.word(), mY = (int)rd.word(), isB = (int)rd.word(),
                  bframes = (int)rd.word(), poc = (int)rd.word(), lists = (int)rd.word();
        const int hs = CHROMA_H_SHIFT(csp), vs = CHROMA_V_SHIFT(csp), planes = csp == X265_CSP_I400 ? 1 : 3;
        const int lw = ((picW / 2 + 7) >> 3) << 3, ll = ((picH / 2 + 7) >> 3) << 3, lstride = lw + 2 * mX, cu = (lw >> 3) * (ll >> 3);
        const int cw = picW >> hs, ch = picH >> vs, cmX = (2 * mX) >> hs, cmY = (2 * mY) >> vs, cstride = cw + 2 * cmX;
        const size_t lowBytes = (size_t)lstride * (ll + 2 * mY) * sizeof(pixel), cBytes = planes == 3 ? (size_t)cstride * (ch + 2 * cmY) * sizeof(pixel) : 0;
        const size_t lowOrg = (size_t)lstride * mY + mX, cOrg = (size_t)cstride * cmY + cmX;
        uint64_t sums[3][2][3];                                                  // [frame, list 0, list 1][sum, ssd][plane]
        int refPoc[2] = { 0, 0 }, hasMvs[2] = { 0, 0 };
        for (int q = 0; q < 2; q++) for (int k = 0; k < 3; k++) sums[0][q][k] = (uint64_t)rd.word();
        for (int l = 0; l < lists; l++)
        {
            refPoc[l] = (int)rd.word(); hasMvs[l] = (int)rd.word();
            for (int q = 0; q < 2; q++) for (int k = 0; k < 3; k++) sums[1 + l][q][k] = (uint64_t)rd.word();
        }
        param->internalCsp = csp; param->bframes = bframes; param->logLevel = X265_LOG_NONE;
        param->sourceWidth = picW; param->sourceHeight = picH;

        auto make_pic = [&](pixel* cb, pixel* cr) {
            PicYuv* pic = new PicYuv;
            pic->m_param = param;
            pic->m_picWidth = picW; pic->m_picHeight = picH; pic->m_picCsp = csp;
            pic->m_hChromaShift = hs; pic->m_vChromaShift = vs;
            pic->m_stride = picW + 2 * mX * 2; pic->m_strideC = cstride;
            pic->m_lumaMarginX = mX * 2; pic->m_lumaMarginY = mY * 2; pic->m_chromaMarginX = cmX; pic->m_chromaMarginY = cmY;
            pic->m_picOrg[0] = NULL; pic->m_picOrg[1] = cb ? cb + cOrg : NULL; pic->m_picOrg[2] = cr ? cr + cOrg : NULL;
            return pic;
        };
        g = Run();
        g_csp = csp;

        // the frame
        Frame* frame = new Frame;
        pixel* fl = (pixel*)rd.take(lowBytes);
        pixel* fcb = planes == 3 ? (pixel*)rd.take(cBytes) : NULL;
        pixel* fcr = planes == 3 ? (pixel*)rd.take(cBytes) : NULL;
        int32_t* intra = (int32_t*)rd.take(sizeof(int32_t) * cu);
        frame->m_fencPic = make_pic(fcb, fcr);
        frame->m_poc = poc;
        Lowres& fenc = frame->m_lowres;
        memset(&fenc, 0, sizeof(fenc));
        fenc.width = lw; fenc.lines = ll; fenc.lumaStride = lstride;
        fenc.lowresPlane[0] = fl + lowOrg;
        fenc.intraCost = intra;
        for (int k = 0; k < 3; k++) { fenc.wp_sum[k] = sums[0][0][k]; fenc.wp_ssd[k] = sums[0][1][k]; }
        g.fenc[0].lo = fl; g.fenc[0].hi = fl + lowBytes / sizeof(pixel);
        g.orig[0] = fenc.lowresPlane[0];
        if (planes == 3)
        {
            g.fenc[1].lo = fcb; g.fenc[1].hi = fcb + cBytes / sizeof(pixel); g.orig[1] = fcb + cOrg;
            g.fenc[2].lo = fcr; g.fenc[2].hi = fcr + cBytes / sizeof(pixel); g.orig[2] = fcr + cOrg;
        }
        Slice* slice = new Slice;
        slice->m_poc = poc;
        slice->m_sliceType = isB ? B_SLICE : P_SLICE;
        memset(slice->m_weightPredTable, 0x5a, sizeof(slice->m_weightPredTable));
        Planes rp[2];
        const int32_t* mvs[2] = { NULL, NULL };
        Frame* refs[2] = { NULL, NULL };
        for (int l = 0; l < lists; l++)
        {
            Frame* rf = new Frame;
            refs[l] = rf;
            pixel* base = (pixel*)rd.take(lowBytes * 4);
            for (int i = 0; i < 4; i++) rp[l].low[i] = base + i * (lowBytes / sizeof(pixel)) + lowOrg;
            pixel* cb = planes == 3 ? (pixel*)rd.take(cBytes) : NULL;
            pixel* cr = planes == 3 ? (pixel*)rd.take(cBytes) : NULL;
            rp[l].c[0] = cb ? cb + cOrg : NULL; rp[l].c[1] = cr ? cr + cOrg : NULL;
            mvs[l] = (const int32_t*)rd.take(sizeof(int32_t) * 2 * cu);
            rf->m_fencPic = make_pic(cb, cr);
            rf->m_poc = refPoc[l];
            rf->m_bChromaExtended = false;
            Lowres& rl = rf->m_lowres;
            memset(&rl, 0, sizeof(rl));
            rl.width = lw; rl.lines = ll; rl.lumaStride = lstride;
            for (int i = 0; i < 4; i++) rl.lowresPlane[i] = rp[l].low[i];
            for (int k = 0; k < 3; k++) { rl.wp_sum[k] = sums[1 + l][0][k]; rl.wp_ssd[k] = sums[1 + l][1][k]; }
            g.ref[l][0].lo = base; g.ref[l][0].hi = base + 4 * (lowBytes / sizeof(pixel));
            if (planes == 3) { g.ref[l][1].lo = cb; g.ref[l][1].hi = cr + cBytes / sizeof(pixel); }          // (cb and cr lie one after the other)
            slice->m_refFrameList[l][0] = rf;
            slice->m_numRefIdx[l] = 1;
            // the vectors of this distance; every other distance reads as "not searched"
            const int diff = abs(poc - refPoc[l]);
            static MV none; none.x = 0x7FFF; none.y = 0;
            for (int i = 0; i < X265_BFRAME_MAX + 2; i++) fenc.lowresMvs[l][i] = &none;
            if (diff < X265_BFRAME_MAX + 2 && hasMvs[l]) fenc.lowresMvs[l][diff] = (MV*)mvs[l];
        }

        primitives.weight_pp = w_weight;
        primitives.pu[LUMA_8x8].satd = w_satd8;
        primitives.pu[LUMA_16x16].satd = w_satd16;
        primitives.cu[BLOCK_8x8].copy_pp = w_copy8;
        primitives.pu[LUMA_8x8].pixelavg_pp[0] = w_avg0;
        primitives.pu[LUMA_8x8].pixelavg_pp[1] = w_avg1;
        primitives.chroma[csp].pu[LUMA_16x16].copy_pp = w_ccopy;
        primitives.chroma[csp].pu[LUMA_16x16].filter_hpp = w_hpp;
        primitives.chroma[csp].pu[LUMA_16x16].filter_vpp = w_vpp;
        primitives.chroma[csp].pu[LUMA_16x16].filter_hps = w_hps;
        primitives.chroma[csp].pu[LUMA_16x16].filter_vsp = w_vsp;
        weightAnalyse(*slice, *frame, *param);
        primitives = g_orig;

        // wpcost.h beside it: per list the compensated planes (the chroma borders are extended by now, or were never needed), then every logged candidate
        const char* name = strrchr(argv[ci], '/') ? strrchr(argv[ci], '/') + 1 : argv[ci];
        fprintf(out, "%s\"%s\": {\"evals\": [", ci > 2 ? ",\n" : "", name);
        const int cwC = ((picW >> 4) << 4) >> hs, chC = ((picH >> 4) << 4) >> vs;
        std::vector<pixel> mc[2][3];
        long lumaBr[2] = { 0, 0 }, lumaClip[4] = { 0, 0, 0, 0 }, chromaBr[5] = { 0, 0, 0, 0, 0 }, chromaClip[4] = { 0, 0, 0, 0 };
        for (int l = 0; l < lists; l++)
        {
            const int diff = abs(poc - refPoc[l]);
            const bool comp = hasMvs[l] && diff <= bframes + 1;
            mc[l][0].resize((size_t)lstride * ll);
            for (int y = 0; y < ll; y++)
                for (int x = 0; x < lw; x++)
                    mc[l][0][(size_t)y * lstride + x] = comp ? (pixel)xw_mc_luma<pixel>(rp[l].low, lstride, lw, ll, mvs[l], x, y) : rp[l].low[0][(size_t)y * lstride + x];
            for (int k = 1; k < planes; k++)
            {
                mc[l][k].resize((size_t)cstride * chC);
                for (int y = 0; y < chC; y++)
                    for (int x = 0; x < cwC; x++)
                        mc[l][k][(size_t)y * cstride + x] = comp ? (pixel)xw_mc_chroma<pixel>(rp[l].c[k - 1], cstride, cwC, chC, mvs[l], lw >> 3, ll >> 3, hs, vs, X265_DEPTH, x, y)
                                                                 : rp[l].c[k - 1][(size_t)y * cstride + x];
            }
            bool lumaRan = false, chromaRan = false;
            for (size_t i = 0; i < g.evals.size(); i++)
            {
                lumaRan = lumaRan || (g.evals[i].list == l && g.evals[i].plane == 0);
                chromaRan = chromaRan || (g.evals[i].list == l && g.evals[i].plane == 1);
            }
            if (comp && lumaRan)
                for (int y = 0; y < ll; y += 8)
                    for (int x = 0; x < lw; x += 8)
                    {
                        int cl;
                        lumaBr[xw_mc_luma_branch(lw, ll, mvs[l], x, y, &cl)]++;
                        for (int b = 0; b < 4; b++) lumaClip[b] += (cl >> b) & 1;
                    }
            if (comp && chromaRan)
                for (int y = 0; y < chC; y += 16 >> vs)
                    for (int x = 0; x < cwC; x += 16 >> hs)
                    {
                        int mx, my, cl;
                        const int in = xw_mc_chroma_mv(cwC, chC, mvs[l], lw >> 3, ll >> 3, hs, vs, x, y, &mx, &my, &cl);
                        chromaBr[xw_mc_chroma_branch(in, mx, my)]++;
                        for (int b = 0; b < 4; b++) chromaClip[b] += (cl >> b) & 1;
                    }
        }
        for (size_t i = 0; i < g.evals.size(); i++)
        {
            const Eval& e = g.evals[i];
            const int k = e.plane, bs = k && csp == X265_CSP_I444 ? 16 : 8;
            const int w = k ? cwC : lw, h = k ? chC : ll;
            const intptr_t st = k ? cstride : lstride;
            const pixel* fo = g.orig[k];
            const pixel* ro = mc[e.list][k].data();
            const xw_cand c = xw_make_cand(X265_DEPTH, e.present, e.w, e.o, e.d);
            uint32_t total = 0, htotal = 0;
            long clip0 = 0, clipmax = 0;
            std::string hb;
            int b = 0;
            for (int y = 0; y < h; y += bs)
                for (int x = 0; x < w; x += bs, b++)
                {
                    const uint32_t v = xw_block_cost<pixel>(ro + (size_t)y * st + x, st, fo + (size_t)y * st + x, st, bs, k ? NULL : intra + b, c, X265_DEPTH);
                    htotal += v;
                    char t[24];
                    snprintf(t, sizeof(t), "%s%u", b ? "," : "", v);
                    hb += t;
                    if (e.present)
                        for (int j = 0; j < bs; j++)
                            for (int q = 0; q < bs; q++)
                            {
                                const int16_t val = (int16_t)(ro[(size_t)(y + j) * st + x + q] << (14 - X265_DEPTH));
                                const int u = ((c.w0 * val + c.round) >> c.shift) + c.offset;
                                clip0 += u < 0; clipmax += u > (1 << X265_DEPTH) - 1;
                            }
                }
            fprintf(out, "%s\n {\"plane\": %d, \"list\": %d, \"present\": %d, \"w\": %d, \"o\": %d, \"d\": %d, \"blocks\": [", i ? "," : "", e.plane, e.list, e.present, e.w,
                    e.o, e.d);
            for (size_t q = 0; q < e.blocks.size(); q++)
            {
                // the function takes the minimum with the intra cost itself (weightPrediction.cpp:204): the logged luma value is the block's share of the total
                const uint32_t v = k ? e.blocks[q] : (uint32_t)X265_MIN((int)e.blocks[q], intra[q]);
                total += v;
                fprintf(out, "%s%u", q ? "," : "", v);
            }
            fprintf(out, "], \"total\": %u, \"host_blocks\": [%s], \"host_total\": %u, \"clip0\": %ld, \"clipmax\": %ld}", total, hb.c_str(), htotal, clip0, clipmax);
        }
        fprintf(out, "],\n \"table\": [");
        for (int l = 0; l < lists; l++)
        {
            fprintf(out, "%s[", l ? ", " : "");
            for (int k = 0; k < 3; k++)
            {
                const WeightParam& w = slice->m_weightPredTable[l][0][k];
                fprintf(out, "%s[%d, %d, %d, %d]", k ? ", " : "", w.inputWeight, w.inputOffset, (int)w.log2WeightDenom, w.wtPresent);
            }
            fprintf(out, "]");
        }
        fprintf(out, "],\n \"calls\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld], \"luma\": {\"branch\": [%ld, %ld], \"clipped\": [%ld, %ld, %ld, %ld]}, "
                "\"chroma\": {\"branch\": [%ld, %ld, %ld, %ld, %ld], \"clipped\": [%ld, %ld, %ld, %ld]}, \"extended\": [%d, %d]}",
                g.calls[0], g.calls[1], g.calls[2], g.calls[3], g.calls[4], g.calls[5], g.calls[6], g.calls[7], lumaBr[0], lumaBr[1], lumaClip[0], lumaClip[1],
                lumaClip[2], lumaClip[3], chromaBr[0], chromaBr[1], chromaBr[2], chromaBr[3], chromaBr[4], chromaClip[0], chromaClip[1], chromaClip[2], chromaClip[3],
                refs[0] ? (int)refs[0]->m_bChromaExtended : 0, refs[1] ? (int)refs[1]->m_bChromaExtended : 0);
        // (the objects point into this iteration's buffers: they are left to the process's end, the buffers with them)
        new std::vector<char>(std::move(rd.buf));
    }
    fprintf(out, "\n}\n");
    fclose(out);
    return 0;
}
