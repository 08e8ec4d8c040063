"""CU jobs at the pixel rails and at both ends of the QP range (x265_amd/csrc/cuserve.hip; inputs: tests/rails_cases.py).

The other job tests draw QPs from [bd + 10, bd + 46) and pixels from noise.  Here the residual is +-pmax (flat, alternating, the sign pattern of one DCT
basis function, a lone spike), source == prediction, or a prediction on a rail under a source just inside it; the QPs are 0, 1, 5, 6, 11, 12, 17, 18, bd + 4,
bd + 46, bd + 48, bd + 51 (bd = 6 * (depth - 8)), luma and chroma chosen independently.  What that reaches:
  - block sums at their limit: a thread's four squared differences 4 * 4095^2 < 2^26, a 16-lane row 1.07e9 < 2^31, a 32x32 unit's zeroDist 1024 * 4095^2
    = 1.7e10 > 2^32 (the 64-bit path from the LDS partials to x265hip_cujob_unit::zeroDist);
  - the largest coefficient there is, the rail residual's DC pmax * 2^(15 - depth) = 32640 / 32736 / 32760, whose level quant_c clips to +-32767 at low QPs of
    10 / 12 bit (never at 8 bit), the line `if (v == 32767 || v == -32768) finalChange = -1` of sign hiding behind that clip, the lone-DC inverse;
  - dequant_normal's clip to int16 (the rail's level at bd + 46 dequantises to 32768), both branches of dequant_scaling with a table set;
  - the inverse half alone for levels made elsewhere, up to the largest whose dequantisation the reference defines;
  - the 8-bit SAO column word (count in the high half, signed sum in the low one) at 64 samples of difference +-255.

Which chain serves a unit (rails_cases.chain_of; the team form is on by default, X265HIP_CUSERVE_TEAM unset): 32x32 luma the four-wave team chain; the lone
16x16 chroma unit of a 32x32 CU at 4:2:0 the solo chain; 4:4:4 chroma of 32x32 tile_chain<32>; 16x16 luma and chroma planes of several units tile_chain<16>;
8x8 chroma tile_chain<8>.  Shape (5, 5, 4) at 4:2:0 holds team + solo + tile16 + tile8, at 4:4:4 team + tile32 + tile16: every kind runs on both at 12 bit.

CPU tier: the restatement against the reference's Quant class on these inputs; the emulated ABI on the GPU tier's jobs; independent NumPy statements of the
rail's zeroDist, DC and clip rule; the witnesses (counted from the restatement, never from the device).
GPU tier: every job through test_cuserve_formats.run_on (one in flight, 20 s deadline), every unit compared as test_cuserve._compare does, both hand-off modes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rails_cases as rc   # noqa: E402

vp, u32 = C.c_void_p, C.c_uint32
QUANT_SCALES = [26214, 23302, 20560, 18396, 16384, 14564]
INV_QUANT_SCALES = [40, 45, 51, 57, 64, 72]
DENOISE, LOWPASS = 16, 32

# rail+dither seeds (rails_cases.dither) at which sign hiding moves a level that quant_c clipped to 32767, found with the restatement among seeds 0..1999 of
# every (depth, size) at QP 0: (depth, n) -> (seed, sliceI).  Levels clip at 10 bit for 32x32 only and at 12 bit for all three sizes (the clip rule below), so
# these four are all there is; the search found every one of them within the first four seeds.
HIDE_ON_CLIP = {(10, 32): (2, 1), (12, 8): (0, 0), (12, 16): (1, 0), (12, 32): (3, 0)}


def _mods():
    import test_cuserve as tc
    import test_cuserve_formats as tcf
    from x265_amd import hipprim as hp
    return hp, tc, tcf


# ---- jobs and what is expected of them ---------------------------------------------------------------------------------------------------------------

def _tiles(j, pick):
    """the unit size per plane that a pattern repeats in: the job's largest transform size (pick 0) or its smallest (pick 1)"""
    hp, tc, tcf = _mods()
    hi, lo = min(5, j.log2TrMax, j.log2CUSize), max(4, j.log2TrMin)
    s = lo if pick else hi
    return [1 << s] + ([1 << (s - tcf.HS[j.chroma])] * 2 if j.chroma else [])


def _pixels(j, kind, pick=0, seed=1):
    hp, tc, tcf = _mods()
    return rc.job_pixels(kind, tcf.plane_dims(j.log2CUSize, j.chroma), _tiles(j, pick), j.bitDepth, seed)


def _expected(j, pix, table=None, seen=None):
    """({unitIndex: (numSig, zeroDist, codedDist, codedEnergy)}, levels, resi): the restatement's job (orc_cujob_run_*) for 4:0:0 / 4:2:0, the composition
    pinned to it (test_cuserve_formats.statement) for 4:2:2 / 4:4:4, test_cuserve_scaling.statement with a table set"""
    hp, tc, tcf = _mods()
    import test_cuserve_scaling as tcs
    O = tcs._orc()
    if table is not None:
        return tcs.statement(hp, O, j, pix, table[0], table[1], seen)
    if j.chroma > 1:
        return tcf.statement(hp, O, j, pix)
    done, wu, wl, wr = tc._oracle_job(hp, O, j, pix)
    lay = tcf.layout(j)
    assert done == len(lay)
    return {k[4]: (wu[k[4]].numSig, wu[k[4]].zeroDist, wu[k[4]].codedDist if wu[k[4]].numSig else None, wu[k[4]].codedEnergy if wu[k[4]].numSig else None) for k in lay}, wl, wr


def _header(shape, depth, qps, sliceI, signHide, **kw):
    hp, tc, tcf = _mods()
    return tc._job_header(hp, shape[0], shape[1], shape[2], shape[3], depth, qps, sliceI, signHide, **kw)


def _unhidden(j, pix):
    plain = type(j).from_buffer_copy(j)
    plain.signHide = 0
    return _expected(plain, pix)[1]


def _witness(j, pix, want, w, dq_of=None):
    """adds the job's witnesses to w, all counted from the expected values: units with a level at +-32767 / -32768 ("clip<depth>"), lone-DC units ("dc"), a
    job without a level ("empty job"; every unit's zeroDist is checked against the int64 sum of squared differences in NumPy on the way), units whose levels sign hiding changed ("hidden") and changed at a clipped level ("hidden on clip", per chain and
    depth), zeroDist > 2^32 ("zero64"), reconstructed samples clipped at 0 / pmax ("rec<0", "rec>max"), dequantised coefficients clipped ("dq clip")"""
    hp, tc, tcf = _mods()
    wu, wl, wr = want
    depth, pmax = j.bitDepth, (1 << j.bitDepth) - 1
    lay = tcf.layout(j)
    dims = tcf.plane_dims(j.log2CUSize, j.chroma)
    half = sum(h * w_ for h, w_ in dims)
    starts = np.cumsum([0] + [h * w_ for h, w_ in dims])
    plain = _unhidden(j, pix) if j.signHide and dq_of is None else None
    per_plane = {}
    for k in lay:
        per_plane[(k[0], k[1])] = per_plane.get((k[0], k[1]), 0) + 1
    for (s, plane, tx, ty, ui, eo, n) in lay:
        chain = rc.chain_of(plane, n, per_plane[(s, plane)])
        w["units"] = w.get("units", 0) + 1
        w[chain] = w.get(chain, 0) + 1
        lv = wl[eo:eo + n * n].astype(np.int64)
        clipped = (lv == 32767) | (lv == -32768)
        if clipped.any():
            w["clip%d" % depth] = w.get("clip%d" % depth, 0) + 1
        h, pw = dims[plane]
        at = starts[plane] + ty * n * pw + tx * n
        diff = np.stack([pix[at + y * pw:at + y * pw + n].astype(np.int64) - pix[half + at + y * pw:half + at + y * pw + n] for y in range(n)])
        assert wu[ui][1] == int((diff * diff).sum()), ("zeroDist is not the int64 sum of squared differences", s, plane, tx, ty, wu[ui][1])
        if wu[ui][1] > 1 << 32:
            w["zero64"] = w.get("zero64", 0) + 1
            assert depth == 12 and n == 32
        if plain is not None:
            pl = plain[eo:eo + n * n].astype(np.int64)
            if not np.array_equal(pl, lv):
                w["hidden"] = w.get("hidden", 0) + 1
            if ((pl != lv) & ((pl == 32767) | (pl == -32768))).any():
                w[("hidden on clip", depth, chain)] = w.get(("hidden on clip", depth, chain), 0) + 1
        if not wu[ui][0]:
            continue
        w["coded"] = w.get("coded", 0) + 1
        if wu[ui][0] == 1 and lv[0]:
            w["dc"] = w.get("dc", 0) + 1
        # dequant_normal / dequant_scaling of the levels in int64: what int16 cannot hold was clipped
        tshift = 15 - depth - (n.bit_length() - 1)
        if dq_of is None:
            raw = (lv * (j.dequantScale[plane] << j.qpPer[plane]) + (1 << (6 - tshift - 1))) >> (6 - tshift)
        else:
            raw = dq_of(lv, plane, n, 10 - tshift)
        w["dq clip"] = w.get("dq clip", 0) + int(((raw > 32767) | (raw < -32768)).sum())
        h, pw = dims[plane]
        prd = pix[half + starts[plane]:half + starts[plane] + h * pw].reshape(h, pw)[ty * n:(ty + 1) * n, tx * n:(tx + 1) * n].astype(np.int64)
        rec = prd + wr[eo:eo + n * n].reshape(n, n)
        w["rec<0"] = w.get("rec<0", 0) + int((rec < 0).sum())
        w["rec>max"] = w.get("rec>max", 0) + int((rec > pmax).sum())
    if not any(wu[k[4]][0] for k in lay):
        w["empty job"] = w.get("empty job", 0) + 1


def _format_shapes():
    """test_cuserve.JOB_SHAPES as they are, and with 4:2:2 and 4:4:4 in place of the chroma flag (what test_cuserve_formats adds)"""
    hp, tc, tcf = _mods()
    return [s for s in tc.JOB_SHAPES] + [(s[0], s[1], s[2], fmt) for fmt in (2, 3) for s in tc.JOB_SHAPES]


@functools.lru_cache(maxsize=None)
def _ordinary_jobs(depth):
    """[(label, header, pixels, expected)] of the ordinary jobs of one depth, their witnesses and the pairs they cover; built once, shared by the CPU tests
    and both device modes.
      deal: every kind on the next of the 27 (shape, format) pairs, QPs round-robin with different strides for Y, Cb, Cr;
      forms: at 12 bit every kind on (5, 5, 4) at 4:2:0 and 4:4:4, which together hold all five chains;
      ends: rail+, rail-, rail+dither at QP 0, bd + 46 (I-slice offset: the level dequantises to 32768) and bd + 51;
      hide: the jobs whose dither seeds put sign hiding on a clipped level, in every chain that has such levels at this depth"""
    shapes = _format_shapes()
    jobs, w = [], {}
    pairs = set()
    di = (8, 10, 12).index(depth)

    def add(group, shape, kind, qps, sliceI, signHide, pick=0, seed=1):
        j = _header(shape, depth, qps, sliceI, signHide)
        pix = _pixels(j, kind, pick, seed)
        want = _expected(j, pix)
        _witness(j, pix, want, w)
        jobs.append(((group, depth, shape, kind, qps, sliceI, signHide, pick), j, pix, want))
        pairs.add(("kind", kind, depth))
        for q in qps[:3 if shape[3] else 1]:
            pairs.add(("qp", q, depth))
        if depth == 12:
            lay = _mods()[2].layout(j)
            for (s, plane) in {(k[0], k[1]) for k in lay}:
                n = next(k[6] for k in lay if (k[0], k[1]) == (s, plane))
                pairs.add(("chain", kind, rc.chain_of(plane, n, sum(1 for k in lay if (k[0], k[1]) == (s, plane)))))

    Q = rc.qps(depth)
    bd = 6 * (depth - 8)
    for i, kind in enumerate(rc.KINDS):
        qps = (Q[(i + di) % 12], Q[(5 * i + 3 + di) % 12], Q[(7 * i + 6 + di) % 12])
        add("deal", shapes[(i + 8 * di) % len(shapes)], kind, qps, i % 2, int(i % 4 != 3), pick=(i // 2) % 2)
        if depth == 12:
            qps = (Q[(5 * i + 1) % 12], Q[(i + 4) % 12], Q[(7 * i) % 12])
            add("forms", (5, 5, 4, 1), kind, qps, (i + 1) % 2, int(i % 4 != 1), pick=i % 2)
            add("forms", (5, 5, 4, 3), kind, qps[::-1], i % 2, int(i % 4 != 2), pick=(i + 1) % 2)
    for i, kind in enumerate(("rail+", "rail-", "rail+dither")):
        for k, (q, sliceI) in enumerate(((0, 0), (bd + 46, 1), (bd + 51, 0))):
            add("ends", ((5, 5, 4, 1), (5, 5, 4, 3), (6, 5, 5, 2))[(i + k) % 3], kind, (q, q, q), sliceI, 1, pick=k % 2)
    if depth == 12:
        s32, s16, s8 = HIDE_ON_CLIP[(12, 32)][0], HIDE_ON_CLIP[(12, 16)][0], HIDE_ON_CLIP[(12, 8)][0]
        add("hide", (5, 5, 4, 1), "rail+dither", (0, 0, 0), 0, 1, pick=0, seed=(s32, s16, s16))      # team + solo
        add("hide", (5, 5, 4, 1), "rail+dither", (0, 0, 0), 0, 1, pick=1, seed=(s16, s8, s8))        # tile16 + tile8
        add("hide", (5, 5, 5, 3), "rail+dither", (0, 0, 0), 0, 1, pick=0, seed=(s32, s32, s32))      # team + tile32
    elif depth == 10:
        add("hide", (5, 5, 5, 3), "rail+dither", (0, 0, 0), HIDE_ON_CLIP[(10, 32)][1], 1, pick=0, seed=(HIDE_ON_CLIP[(10, 32)][0],) * 3)
    return jobs, w, pairs


def _all_ordinary_jobs():
    jobs, w, pairs = [], {}, set()
    for depth in (8, 10, 12):
        j_, w_, p_ = _ordinary_jobs(depth)
        jobs += j_
        pairs |= p_
        for k, v in w_.items():
            w[k] = w.get(k, 0) + v
    return jobs, w, pairs


def _show(name, jobs, w):
    print("%s: %d jobs, %d units, %d coded; witnesses %r" % (name, jobs, w.get("units", 0), w.get("coded", 0),
                                                             {str(k): v for k, v in sorted(w.items(), key=lambda kv: str(kv[0])) if k not in ("units", "coded")}))


# ---- CPU tier: the restatement against the reference's Quant class ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 10, 12])
def test_transform_restatement_matches_the_reference_quant_class_at_the_rails(depth):
    """orc_transform_nxn / orc_invtransform_nxn == Quant::transformNxN / ::invtransformNxN on the bare kinds (rails, dither, checker and stripes, basis signs,
    spikes), N = 8 / 16 / 32, text types 0-2, the twelve QPs, both slice offsets, sign hiding on and off.  Levels clip at 10 / 12 bit and never at 8."""
    hp, tc, tcf = _mods()
    O, R = tc._orc(), tc._ref(depth)
    n_cases = clipped = hidden = hidden_on_clip = lone_dc = 0
    for log2n in (3, 4, 5):
        n = 1 << log2n
        resis = [rc.residual(kind, n, depth, seed) for kind in rc.BARE_KINDS for seed in ((1, HIDE_ON_CLIP.get((depth, n), (2, 0))[0]) if kind == "rail+dither" else (1,))]
        for ttype in (0, 1, 2):
            for qp in rc.qps(depth):
                qparam = (C.c_int32 * 4)()
                R.ref_qp_param(qp, qparam)
                rem, per, qs, dqs = qparam[0], qparam[1], qparam[2], qparam[3]
                assert (rem, per, qs, dqs) == (qp % 6, qp // 6, QUANT_SCALES[qp % 6], INV_QUANT_SCALES[qp % 6])
                for sliceI in (0, 1):
                    for ri, resi in enumerate(resis):
                        plain = None
                        for signHide in (0, 1):
                            c_o, c_r = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16)
                            d_o, d_r = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16)
                            ns_r = R.ref_transform_nxn(resi.ctypes.data, n, c_r.ctypes.data, d_r.ctypes.data, log2n, ttype, qp, sliceI, signHide)
                            ns_o = O.orc_transform_nxn(resi.ctypes.data, n, c_o.ctypes.data, d_o.ctypes.data, log2n, depth, rem, per, qs, 171 if sliceI else 85, signHide)
                            label = (log2n, ttype, qp, sliceI, signHide, ri)
                            assert ns_o == ns_r and np.array_equal(c_o, c_r) and np.array_equal(d_o, d_r), label
                            assert ns_o == int(np.count_nonzero(c_o)), label
                            if ns_r:
                                b_o, b_r = np.full((n, n), 77, np.int16), np.full((n, n), 77, np.int16)
                                R.ref_invtransform_nxn(b_r.ctypes.data, n, c_r.ctypes.data, log2n, ttype, qp, ns_r)
                                O.orc_invtransform_nxn(b_o.ctypes.data, n, c_o.ctypes.data, log2n, depth, per, dqs, ns_o)
                                assert np.array_equal(b_o, b_r), label
                            if signHide:
                                hidden += int(not np.array_equal(plain, c_o))
                                hidden_on_clip += int(((plain != c_o) & ((plain == 32767) | (plain == -32768))).any())
                            else:
                                plain = c_o
                                clipped += int(((c_o == 32767) | (c_o == -32768)).any())
                                lone_dc += int(ns_o == 1 and c_o[0] != 0)
                            n_cases += 1
    print("depth %d: %d cases, %d with a clipped level, %d lone-DC, %d changed by sign hiding, %d of them at a clipped level" % (depth, n_cases, clipped, lone_dc, hidden, hidden_on_clip))
    assert n_cases == 3 * 3 * 12 * 2 * 2 * (len(rc.BARE_KINDS) + 1)
    assert lone_dc > 0 and hidden > 0
    assert (clipped == 0 and hidden_on_clip == 0) if depth == 8 else (clipped > 0 and hidden_on_clip > 0)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_inverse_restatement_matches_the_reference_for_levels_made_elsewhere(depth):
    """orc_invtransform_nxn == Quant::invtransformNxN for levels the forward half never makes (what Quant::rdoQuant may hand over): full-range random, all at the
    top, all at the bottom, a lone top / bottom level at DC (the lone-DC path) and at the last scan position, 1 % dense; N = 8 / 16 / 32, text types 0-2, the
    twelve QPs.  Bound: dequant_normal computes level * scale + add in int, scale = invQuantScales[rem] << per, add = 1 << (shift - 1); beyond 2^31 the
    reference itself is undefined, so every |level| <= (2^31 - 1 - add) // scale (rails_cases.level_limit) — 32767 up to per 10 (all of 8 and 10 bit), 9 196 at 12 bit's last QP."""
    hp, tc, tcf = _mods()
    O, R = tc._orc(), tc._ref(depth)
    n_cases = dq_clipped = lone_dc = limited = 0
    for log2n in (3, 4, 5):
        n = 1 << log2n
        shift = 6 - (15 - depth - log2n)
        for qp in rc.qps(depth):
            rem, per = qp % 6, qp // 6
            scale = INV_QUANT_SCALES[rem] << per
            limit = rc.level_limit(scale, shift)
            limited += int(limit < 32767)
            for name in rc.LEVEL_SETS:
                lv = rc.levels(name, n, limit, seed=qp)
                assert np.abs(lv.astype(np.int64) * scale).max() + (1 << (shift - 1)) < 1 << 31
                ns = int(np.count_nonzero(lv))
                raw = (lv.astype(np.int64) * scale + (1 << (shift - 1))) >> shift
                dq_clipped += int(((raw > 32767) | (raw < -32768)).sum())
                lone_dc += int(ns == 1 and lv[0] != 0)
                for ttype in (0, 1, 2):
                    b_o, b_r = np.full((n, n), 77, np.int16), np.full((n, n), 77, np.int16)
                    R.ref_invtransform_nxn(b_r.ctypes.data, n, lv.ctypes.data, log2n, ttype, qp, ns)
                    O.orc_invtransform_nxn(b_o.ctypes.data, n, lv.ctypes.data, log2n, depth, per, INV_QUANT_SCALES[rem], ns)
                    assert np.array_equal(b_o, b_r), (log2n, qp, name, ttype)
                    n_cases += 1
    print("depth %d: %d cases, %d dequantised coefficients clipped, %d lone-DC, %d (size, QP) with a level limit below 32767" % (depth, n_cases, dq_clipped, lone_dc, limited))
    assert n_cases == 3 * 12 * len(rc.LEVEL_SETS) * 3 and dq_clipped > 0 and lone_dc > 0
    assert (limited > 0) == (depth == 12)


def test_rail_statements_in_numpy():
    """independent of any C code: zeroDist of a rail unit is n^2 * pmax^2 (in int64: above 2^32 for 32x32 at 12 bit alone); the rail's DC coefficient is
    pmax * 2^(15 - depth); the level of that DC is clipped exactly where (DC * quantScale[rem] + add) >> qBits exceeds 32767.  The restatement agrees on all
    three.  The clip needs qBits <= 14, i.e. per <= depth + log2n - 15: all of 10 bit 32x32 QP 0-5 and 12 bit 32 / 16 / 8 up to QP 17 / 11 / 5 — except that AT
    qBits == 14 the two smallest quantiser scales (rem 4, 5: 16384, 14564) leave DC * scale >> 14 at 32736 / 29099 and below: no clip.  Never at 8 bit."""
    hp, tc, tcf = _mods()
    O = tc._orc()
    clipped, rule = set(), set()
    for depth in (8, 10, 12):
        pmax = (1 << depth) - 1
        for log2n in (3, 4, 5):
            n = 1 << log2n
            for sign, kind in ((1, "rail+"), (-1, "rail-")):
                resi = rc.residual(kind, n, depth)
                zero = int((resi.astype(np.int64) ** 2).sum())
                assert zero == n * n * pmax * pmax
                assert (zero > 1 << 32) == (depth == 12 and n == 32)
                for qp in range(0, 6 * (depth - 8) + 52):
                    rem, per = qp % 6, qp // 6
                    lv, dct = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16)
                    ns = O.orc_transform_nxn(resi.ctypes.data, n, lv.ctypes.data, dct.ctypes.data, log2n, depth, rem, per, QUANT_SCALES[rem], 85, 0)
                    assert dct[0] == sign * (pmax << (15 - depth)) and not dct[1:].any(), (depth, n, qp)
                    qbits = 14 + per + 15 - depth - log2n
                    level = ((pmax << (15 - depth)) * QUANT_SCALES[rem] + (85 << (qbits - 9))) >> qbits
                    assert int(lv[0]) == max(-32768, min(32767, sign * level)), (depth, n, qp, int(lv[0]), level)
                    assert ns == int(level != 0) and not lv[1:].any()
                    if sign > 0:
                        if lv[0] == 32767:
                            clipped.add((depth, n, qp))
                            assert level > 32767
                        if qbits <= 14:
                            rule.add((depth, n, qp))
    assert clipped <= rule
    assert rule - clipped == {(d, n, qp) for (d, n, qp) in rule if 14 + qp // 6 + 15 - d - n.bit_length() + 1 == 14 and qp % 6 >= 4}
    assert rule == {(10, 32, q) for q in range(6)} | {(12, 32, q) for q in range(18)} | {(12, 16, q) for q in range(12)} | {(12, 8, q) for q in range(6)}
    assert not any(d == 8 for d, n, q in rule)
    print("rail DC clipped at %d of the %d (depth, size, QP) with qBits <= 14" % (len(clipped), len(rule)))


def test_sign_hiding_lands_on_a_clipped_level_at_the_recorded_seeds():
    """HIDE_ON_CLIP still hits: with hiding on and off the level differs at a position whose unhidden value is 32767, and hiding took it DOWN (the line
    `if (coeff[minPos] == 32767 || coeff[minPos] == -32768) finalChange = -1` of signBitHidingHDQ: up is not representable)"""
    hp, tc, tcf = _mods()
    O = tc._orc()
    for (depth, n), (seed, sliceI) in sorted(HIDE_ON_CLIP.items()):
        s, p = rc.dither(n, depth, seed)
        assert s.min() >= (1 << depth) - 4 and p.max() <= 3
        resi = np.ascontiguousarray((s - p).astype(np.int16))
        a, b, d = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16), np.zeros(n * n, np.int16)
        O.orc_transform_nxn(resi.ctypes.data, n, a.ctypes.data, d.ctypes.data, n.bit_length() - 1, depth, 0, 0, QUANT_SCALES[0], 171 if sliceI else 85, 0)
        O.orc_transform_nxn(resi.ctypes.data, n, b.ctypes.data, d.ctypes.data, n.bit_length() - 1, depth, 0, 0, QUANT_SCALES[0], 171 if sliceI else 85, 1)
        at = np.nonzero((a != b) & (a == 32767))[0]
        assert at.size >= 1 and (b[at] == 32766).all(), (depth, n, seed, at, b[at])


def test_ordinary_rail_jobs_cover_what_they_claim():
    """the deal of the ordinary jobs: every (kind, depth) and every (QP, depth) pair occurs, every (kind, chain) pair at 12 bit; and the witnesses, counted
    from the restatement: clipped levels at 10 and 12 bit and none at 8, lone-DC units, jobs whose every unit is empty, units whose levels sign hiding changed,
    sign hiding on a clipped level in all five chains at 12 bit and in the two 32x32 chains at 10 bit, zeroDist > 2^32, reconstructions clipped at 0 and at
    pmax, dequantised coefficients clipped to int16"""
    jobs, w, pairs = _all_ordinary_jobs()
    _show("ordinary rail jobs", len(jobs), w)
    assert len(jobs) == 151
    for depth in (8, 10, 12):
        assert all(("kind", kind, depth) in pairs for kind in rc.KINDS), depth
        assert all(("qp", q, depth) in pairs for q in rc.qps(depth)), depth
    missing = [(kind, chain) for kind in rc.KINDS for chain in rc.CHAINS if ("chain", kind, chain) not in pairs]
    assert not missing, missing
    assert all(w.get(c, 0) > 0 for c in rc.CHAINS)
    assert w.get("clip8", 0) == 0 and w.get("clip10", 0) > 0 and w.get("clip12", 0) > 0, w
    for k in ("dc", "empty job", "hidden", "zero64", "rec<0", "rec>max", "dq clip"):
        assert w.get(k, 0) > 0, (k, w)
    for chain in rc.CHAINS:
        assert w.get(("hidden on clip", 12, chain), 0) > 0, (chain, w)
    assert w.get(("hidden on clip", 10, "team32"), 0) > 0 and w.get(("hidden on clip", 10, "tile32"), 0) > 0, w
    assert not any(k[1] == 8 for k in w if isinstance(k, tuple))


class _Emul:
    """hp-like holder for run_on over the emulated library"""
    def __init__(self, hp):
        self.CuJobUnit, self.CUJOB_MAX_ELEMS, self.CUJOB_MAX_UNITS, self.CUJOB_PIXEL_BYTES = hp.CuJobUnit, hp.CUJOB_MAX_ELEMS, hp.CUJOB_MAX_UNITS, hp.CUJOB_PIXEL_BYTES

    @staticmethod
    def check(rc_):
        assert rc_ == 0, rc_


def test_emulated_rail_jobs_are_the_restatement():
    """tests/support/libx265hip_emul.so (what the CPU-tier encodes run on) on the GPU tier's 4:0:0 / 4:2:0 jobs — ordinary, coefficient mode and inverse —
    through the same submit / poll protocol: it accepts every QP from 0 to bd + 51, as x265hip_cuserve_submit does, and answers what orc_cujob_run_* answers"""
    hp, tc, tcf = _mods()
    if not os.path.exists(tc.EMUL):
        pytest.skip("tests/support/libx265hip_emul.so not built (make -C oracle emul)")
    em = C.CDLL(tc.EMUL)
    for name, (res, args) in hp.PROTOTYPES.items():
        if name.startswith("x265hip_cuserve_"):
            fn = getattr(em, name)
            fn.restype, fn.argtypes = res, args
    cs = vp()
    assert em.x265hip_cuserve_open(2, 0, C.byref(cs)) == 0
    try:
        total = units = 0
        for group in (_all_ordinary_jobs()[0], _coefficient_jobs()[0], _inverse_jobs()[0]):
            for label, j, pix, want in group:
                if j.chroma > 1:
                    continue
                got = tcf.run_on(_Emul(hp), em, cs, total % 2, j, pix)
                n, c = _compare_inverse(got, want, label) if j.coefMode == 8 else tcf.compare(j, got, want, label)
                total += 1; units += n
        print("emulated ABI: %d jobs, %d units" % (total, units))
        assert total > 100
    finally:
        assert em.x265hip_cuserve_close(cs) == 0


# ---- the other job lists -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _coefficient_jobs():
    """coefficient mode with and without sourceDct on rail+ (the source block's transform is the largest DC there is), checker and the three basis kinds"""
    jobs, w = [], {"source transforms": 0}
    shapes = ((5, 5, 4, 1), (5, 5, 4, 3), (6, 5, 5, 1), (4, 4, 4, 1), (6, 5, 4, 2), (5, 5, 5, 0))
    total = 0
    for depth in (8, 10, 12):
        Q = rc.qps(depth)
        for kind in ("rail+", "checker", "basis:1,1", "basis:N-1,N-1", "basis:1,0"):
            for sdct in (1, 0):
                shape = shapes[total % len(shapes)]
                j = _header(shape, depth, (Q[total % 12], Q[(total + 5) % 12], Q[(total + 7) % 12]), total % 2, 1, coef=1, source_dct=sdct)
                pix = _pixels(j, kind, (total // 2) % 2)
                want = _expected(j, pix)
                lay = _mods()[2].layout(j)
                w["units"] = w.get("units", 0) + len(lay)
                if sdct:
                    w["source transforms"] += sum(1 for k in lay if k[1] == 0)
                    if kind == "rail+":
                        # the largest DC: a flat source block at pmax
                        assert all(want[2][k[5]] == ((1 << depth) - 1) << (15 - depth) for k in lay if k[1] == 0)
                        w["largest source DC"] = w.get("largest source DC", 0) + 1
                jobs.append((("coef", depth, shape, kind, sdct), j, pix, want))
                total += 1
    return jobs, w


@functools.lru_cache(maxsize=None)
def _inverse_jobs():
    """X265HIP_CUJOB_INVERSE jobs (one 32x32 luma unit) for the level sets of rails_cases.LEVEL_SETS under the bound of the CPU test, every set at three of the
    twelve QPs per depth (every QP twice), composed as test_device_inverse_jobs_match_the_restatement composes them: the two pixel blocks, then the levels"""
    hp, tc, tcf = _mods()
    O = tc._orc()
    jobs, w = [], {}
    for depth in (8, 10, 12):
        Q = rc.qps(depth)
        rng = np.random.default_rng(3100 + depth)
        shift = 6 - (15 - depth - 5)
        for si, name in enumerate(rc.LEVEL_SETS):
            for k in range(3):
                qp = Q[(si + 4 * k) % 12]
                scale = INV_QUANT_SCALES[qp % 6] << (qp // 6)
                lv = rc.levels(name, 32, rc.level_limit(scale, shift), seed=qp)
                j = _header((5, 5, 5, 0), depth, (qp, qp, qp), 0, 0, coef=8)
                pix = tc._job_pixels(rng, 5, 0, depth, (si + k) % 3) if (si + k) % 4 else _pixels(j, ("rail+", "rail-")[k % 2])
                blob = np.frombuffer(pix.tobytes() + lv.tobytes(), np.uint8).copy()
                done, wu, wl, wr = tc._oracle_job(hp, O, j, blob)
                assert done == 1 and wu[0].numSig == int(np.count_nonzero(lv)) > 0
                raw = (lv.astype(np.int64) * scale + (1 << (shift - 1))) >> shift
                w["dq clip"] = w.get("dq clip", 0) + int(((raw > 32767) | (raw < -32768)).sum())
                w["dc"] = w.get("dc", 0) + int(wu[0].numSig == 1 and lv[0] != 0)
                w["units"] = w.get("units", 0) + 1
                w["coded"] = w.get("coded", 0) + 1
                pmax = (1 << depth) - 1
                rec = pix[1024:2048].astype(np.int64) + wr[:1024]
                w["rec<0"] = w.get("rec<0", 0) + int((rec < 0).sum())
                w["rec>max"] = w.get("rec>max", 0) + int((rec > pmax).sum())
                # (an inverse job writes no levels: the block it is compared on is empty in both)
                want = ({0: (wu[0].numSig, wu[0].zeroDist, wu[0].codedDist, wu[0].codedEnergy)}, np.zeros(hp.CUJOB_MAX_ELEMS, np.int16), wr)
                jobs.append((("inverse", depth, name, qp), j, blob, want))
    return jobs, w


def _compare_inverse(got, want, label):
    (gu, gl, gr), (wu, wl, wr) = got, want
    assert gu[0] == wu[0], (label, gu[0], wu[0])
    assert np.array_equal(gr[:1024], wr[:1024]), (label, "resi")
    return 1, 1


def test_coefficient_and_inverse_rail_jobs_cover_what_they_claim():
    jobs, w = _coefficient_jobs()
    _show("coefficient-mode rail jobs", len(jobs), w)
    assert len(jobs) == 30 and w["source transforms"] > 0 and w.get("largest source DC", 0) >= 3
    jobs, w = _inverse_jobs()
    _show("inverse jobs", len(jobs), w)
    assert len(jobs) == 3 * 3 * len(rc.LEVEL_SETS)
    for k in ("dq clip", "dc", "rec<0", "rec>max"):
        assert w.get(k, 0) > 0, (k, w)


def _sets():
    """the default set; an all-8 set (the largest quantiser entries the service accepts: (quantScales[rem] << 4) / 8); an all-255 set"""
    import test_cuserve_scaling as tcs
    return [tcs.default_set(), tcs.derive_tables(np.full((3, 3, 64), 8), np.full((3, 3), 8)), tcs.derive_tables(np.full((3, 3, 64), 255), np.full((3, 3), 255))]


@functools.lru_cache(maxsize=None)
def _table_set_jobs():
    """jobs with a table set: rail+, rail-, rail+dither, checker at QPs 0, 5, bd + 4, bd + 42, bd + 48, bd + 51 per depth, the three sets round-robin so that
    every (set, QP) pair occurs at every depth; against test_cuserve_scaling.statement"""
    hp, tc, tcf = _mods()
    import test_cuserve_scaling as tcs
    sets = _sets()
    jobs, w, seen = [], {}, {}
    total = 0
    for di, depth in enumerate((8, 10, 12)):
        bd = 6 * (depth - 8)
        for qi, q in enumerate((0, 5, bd + 4, bd + 42, bd + 48, bd + 51)):
            for ki, kind in enumerate(("rail+", "rail-", "rail+dither", "checker")):
                sid = 1 + (qi + ki + di) % 3
                shape = ((5, 5, 4), (5, 5, 5), (6, 5, 4), (4, 4, 4))[total % 4]
                fmt = (1, 3, 1, 2, 0, 1)[total % 6]
                j = tcs.job_header(hp, tc, shape, fmt, depth, (q, max(0, q - 1), max(0, q - 3)) if qi % 2 else (q, q, q), total % 2, int(total % 3 != 0), sid)
                pix = _pixels(j, kind, total % 2, HIDE_ON_CLIP.get((depth, 32), (1, 0))[0])
                q_, dq_ = sets[sid - 1]
                want = tcs.statement(hp, tcs._orc(), j, pix, q_, dq_, seen)

                def dq_of(lv, plane, n, shift, j=j, dq_=dq_):
                    tab = tcs.table_offset(n.bit_length() - 1, plane, j.qpRem[plane])
                    prod, per = lv * dq_[tab:tab + n * n].astype(np.int64), j.qpPer[plane]
                    if shift > per:
                        return (prod + (1 << (shift - per - 1))) >> (shift - per)
                    return np.where(np.abs(prod) > 32767, prod, np.clip(prod, -32768, 32767) << (per - shift))
                _witness(j, pix, want, w, dq_of)
                jobs.append((("table set", depth, shape, fmt, kind, q, sid), j, pix, want))
                total += 1
    for k, v in seen.items():
        w[k] = v
    return jobs, w


def test_table_set_rail_jobs_cover_what_they_claim():
    """both branches of dequant_scaling ("b1", "b2" of test_cuserve_scaling.statement), lone-DC units, hidden signs, clipped levels and clipped dequantised
    coefficients, counted from the statement"""
    jobs, w = _table_set_jobs()
    _show("table-set rail jobs", len(jobs), w)
    assert len(jobs) == 72
    for k in ("b1", "b2", "dc", "hidden", "dq clip", "clip10", "clip12", "zero64"):
        assert w.get(k, 0) > 0, (k, w)
    assert w.get("clip8", 0) == 0


# ---- SAO planes at the rails -----------------------------------------------------------------------------------------------------------------------------

SAO_GEOMETRIES = ([(64, 64, 0), (32, 32, 2), (32, 32, 2)], [(32, 64, 2)], [(64, 64, 2)], [(64, 64, 0), (32, 64, 2)], [(64, 64, 0), (64, 64, 2)])


def _sao_rail_jobs():
    """full 8-bit planes (w, h, chroma offset) of 4:2:0 and of the 4:2:2 / 4:4:4 chroma geometries, rectangles covering the whole plane (right and bottom set,
    left and above clear); contents: reconstruction 0 under source 255, the reverse, and column stripes 0 / 255 under the inverse stripes — every sample of a
    column is then a valley (or a peak) of the horizontal edge class with difference +255 (-255): 64 samples of one bin in one column word, +-16 320"""
    import test_saostats_formats as sf
    hp, tc, tcf = _mods()
    rng = np.random.default_rng(5)
    jobs = []
    for planes in SAO_GEOMETRIES:
        for kind in ("max+", "max-", "stripes"):
            j, pix = sf.make_job(hp, rng, 8, planes, eo23=1, kind=kind if kind != "stripes" else "max+", edges=(1, 1, 0, 0))
            if kind == "stripes":
                blocks = []
                for (w, h, po) in planes:
                    rec = np.tile(np.where(np.arange(w + 1) % 2 == 1, 0, 255), (h + 1, 1))
                    blocks += [rec.astype(np.uint8).ravel(), (255 - rec[1:, 1:]).astype(np.uint8).ravel()]
                pix = np.ascontiguousarray(np.concatenate(blocks))
            jobs.append(((tuple(planes), kind), j, pix))
    return jobs


def test_sao_rail_jobs_fill_the_column_word():
    """the restatement (orc_saojob_run_8), the numpy statement (test_saostats_formats.restate) and a per-sample count as in
    test_sao_job_restatement_counts_what_the_reference_counts agree on the rail planes; a 64-row plane puts 64 samples of +255 (and of -255) into one column of
    one bin: a sum of 16 320 per column in sixteen signed bits, 1 044 480 for the bin"""
    import test_saostats_formats as sf
    hp, tc, tcf = _mods()
    O = tc._orc()
    full = 0
    for label, j, pix in _sao_rail_jobs():
        want = tc._oracle_sao(hp, O, j, pix)
        assert np.array_equal(want, sf.restate(j, pix)), label
        for b, w, h, rec, src, rects in sf._planes_of(j, pix):
            rec, src = rec.astype(np.int64), src.astype(np.int64)
            for c in (0, 1):
                x0, y0, x1, y1 = rects[c]
                sums, cnts = np.zeros(32, np.int64), np.zeros(32, np.int64)
                for y in range(y0, y1):
                    for x in range(x0, x1):
                        v = rec[y + 1, x + 1]
                        k = v >> 3 if c == 0 else sf.EO[int(np.sign(v - rec[y + 1, x + 2])) + int(np.sign(v - rec[y + 1, x])) + 2]
                        sums[k] += src[y, x] - v
                        cnts[k] += 1
                assert np.array_equal(want[b * 160 + c * 32:b * 160 + c * 32 + 32], sums) and np.array_equal(want[480 + b * 160 + c * 32:480 + b * 160 + c * 32 + 32], cnts), (label, b, c)
                if c == 0 and h == 64:
                    # the band class takes whole columns: a bin all of whose samples differ by +-255, 64 to a column
                    full += int(any(abs(int(s)) == 255 * n and n % 64 == 0 for s, n in zip(sums, cnts) if n))
    assert full == 3 * sum(1 for planes in SAO_GEOMETRIES for (w, h, po) in planes if h == 64)


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------------------------

def _open(mode, slots=2):
    hp, tc, tcf = _mods()
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    cs = vp()
    hp.check(L.x265hip_cuserve_open(slots, mode, C.byref(cs)))
    return hp, L, cs


def _run_group(name, mode, jobs, compare=None, prepare=None):
    """every job of the list on one service, one in flight at a time; the service is closed whatever happens"""
    hp, tc, tcf = _mods()
    hp, L, cs = _open(mode)
    try:
        if prepare:
            prepare(hp, L, cs)
        units = coded = 0
        for k, (label, j, pix, want) in enumerate(jobs):
            got = tcf.run_on(hp, L, cs, k % 2, j, pix)
            n, c = (compare or (lambda g, w_, lb: tcf.compare(j, g, w_, lb)))(got, want, (mode,) + tuple(label))
            units += n; coded += c
        print("%s, mode %d: %d jobs, %d units, %d coded units / source transforms" % (name, mode, len(jobs), units, coded))
        return units
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("mode", [1, 0])
def test_device_ordinary_rail_jobs_match_the_restatement(mode, depth):
    """the default kernels (cu_job_kernel / cu_server_kernel) on every kind, formats 0-3, all five chains (module docstring), the twelve QPs: numSig,
    zeroDist, levels, and for coded units codedDist, codedEnergy and the reconstructed residual.  One case per depth: 33 / 34 / 84 jobs"""
    jobs, w, pairs = _ordinary_jobs(depth)
    _show("ordinary rail jobs, %d bit" % depth, len(jobs), w)
    assert _run_group("ordinary rail jobs, %d bit" % depth, mode, jobs) == w["units"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_coefficient_rail_jobs_match_the_restatement(mode):
    """coefficient mode with and without sourceDct on rail+, checker and basis blocks: the residual's transform, and for luma units the source block's"""
    jobs, w = _coefficient_jobs()
    _show("coefficient-mode rail jobs", len(jobs), w)
    assert _run_group("coefficient-mode rail jobs", mode, jobs) == w["units"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_inverse_jobs_of_levels_made_elsewhere_match_the_restatement(mode):
    """inverse-only jobs: the team's dequantiser and inverse passes clip where the reference's do, for levels up to the largest it defines"""
    jobs, w = _inverse_jobs()
    _show("inverse jobs", len(jobs), w)
    assert _run_group("inverse jobs", mode, jobs, compare=_compare_inverse) == len(jobs)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_table_set_rail_jobs_match_the_statement(mode):
    """the *_sets kernels with the default, all-8 and all-255 sets at both ends of the QP range: dequant_scaling's shift-and-clip branch at the last QPs"""
    import test_cuserve_scaling as tcs
    jobs, w = _table_set_jobs()
    _show("table-set rail jobs", len(jobs), w)

    def prepare(hp, L, cs):
        assert [tcs._add(hp, L, cs, t) for t in _sets()] == [1, 2, 3]
    assert _run_group("table-set rail jobs", mode, jobs, prepare=prepare) == w["units"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_denoise_and_lowpass_jobs_at_the_qp_ends(mode):
    """the QP ends of the denoise and low-pass jobs (their own tests have the rails, at QP steps 22 / 30 / 37): one rail+ and one rail+dither job per depth at
    QP 0 and at bd + 51 each, against test_cuserve_denoise.statement / test_cuserve_lowpass.statement"""
    hp, tc, tcf = _mods()
    import test_cuserve_denoise as tcd
    import test_cuserve_lowpass as tcl
    import test_cuserve_scaling as tcs
    O = tcs._orc()
    flat = tcs.flat16_set()
    hp, L, cs = _open(mode)
    try:
        hp.check(L.x265hip_cujob_lowpass(cs))
        rng = np.random.default_rng(3300)
        total = units = 0
        seen = {}
        for depth in (8, 10, 12):
            for q in (0, 6 * (depth - 8) + 51):
                for kind in ("rail+", "rail+dither"):
                    for flag in (DENOISE, LOWPASS):
                        shape, fmt = (((5, 5, 4), 1), ((5, 5, 5), 3))[total % 2]
                        j = tcd.header(hp, tc, shape, fmt, depth, (q, q, q), total % 2, 1, 0, flag, 0)
                        pix = _pixels(j, kind, 0, HIDE_ON_CLIP.get((depth, 32), (1, 0))[0])
                        if flag == DENOISE:
                            tables = tcd.make_tables(rng, j, "plausible")
                            want = tcd.statement(hp, O, j, pix, flat[0], flat[1], tables, seen)
                            n, c = tcd.compare(hp, j, tcd.run_on(hp, L, cs, total % 2, j, pix, tcd.pack_block(j, tables)), want, (mode, depth, q, kind, "denoise"))
                        else:
                            want = tcl.statement(hp, O, j, pix, flat[0], flat[1], None, seen)
                            n, c = tcl.compare(hp, j, tcl.run_on(hp, L, cs, total % 2, j, pix), want, (mode, depth, q, kind, "lowpass"))
                        total += 1; units += n
        print("denoise and low-pass jobs at the QP ends, mode %d: %d jobs, %d units; %r" % (mode, total, units, seen))
        assert total == 24 and seen.get("coded", 0) > 0
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_8bit_sao_jobs_fill_the_column_word(mode):
    """SaoColumn<uint8_t> full: 64 samples of one bin at difference +-255 in one column, for 4:2:0 and the 4:2:2 / 4:4:4 chroma geometries, against
    orc_saojob_run_8 and the numpy statement"""
    import test_saostats_formats as sf
    hp, tc, tcf = _mods()
    O = tc._orc()
    hp, L, cs = _open(mode)
    try:
        measured = 0
        jobs = _sao_rail_jobs()
        for k, (label, j, pix) in enumerate(jobs):
            want = tc._oracle_sao(hp, O, j, pix)
            assert np.array_equal(want, sf.restate(j, pix)), label
            measured += tc._same_sao(j, tc._run_sao_on(hp, L, cs, k % 2, j, pix), want, (mode,) + label)
        print("8-bit SAO rail jobs, mode %d: %d jobs, %d samples classified" % (mode, len(jobs), measured))
        assert len(jobs) == 15 and measured > 100000
    finally:
        hp.check(L.x265hip_cuserve_close(cs))
