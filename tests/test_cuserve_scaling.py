"""CU residual quad-tree jobs of encodes with scaling lists (include/x265hip.h: x265hip_cujob::scaling, x265hip_cujob_scaling_add, x265hip_cujob_features).

Statement: a unit composed from pinned oracle pieces only — orc_dct -> orc_quant with the matrix m_quantCoef[size][3 + plane][rem] -> orc_sign_hide_hdq when
numSig >= 2 and the job hides signs -> orc_dequant_scaling with m_dequantCoef[size][3 + plane][rem] -> the lone-DC shortcut or orc_idct (reference
quant.cpp:460-476, :559-603; dct.cpp:636-662), sse_pp / psy_cost_pp as in test_cuserve_formats.statement, laid out by that file's layout().  The tables are
derived the way scalinglist.cpp:342-415 derives them: quantCoef = (quantScales[rem] << 4) / entry, dequantCoef = invQuantScales[rem] * entry, 16x16 and 32x32
from the 8x8 entry at (y / ratio, x / ratio) with their own DC.

CPU tier: with an all-16 list the statement is the flat restatement unit for unit (both dequantiser branches, lone-DC units); the library's feature bit and the
ABI's constants; the emulated-ABI encoder with --scaling-list default (no table sets there: no CU job, the reference's bytes).
GPU tier: device jobs of two registered sets against the statement in both server modes, inverse jobs with a set, the limits, and the bound encoders against
the unmodified reference under X265HIP_VERIFY."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
vp, i32, u32 = C.c_void_p, C.c_int, C.c_uint32

QUANT_SCALES = [26214, 23302, 20560, 18396, 16384, 14564]       # scalinglist.cpp:129-130 (checked against the reference by test_cuserve.py)
INV_QUANT_SCALES = [40, 45, 51, 57, 64, 72]
ENTRIES = (64 + 256 + 1024) * 3 * 6
SETS = 8
SCALING_RE = r"cuserve: scaling lists: (\d+) sets registered, (\d+) jobs carried one, (\d+) CUs kept on the host because of their list"
# the 32-only, 32 + 16 and 16-only shapes of test_cuserve.JOB_SHAPES at log2CU 5 and 6 (log2CU, trMax, trMin; the format takes the chroma flag's place)
SHAPES = [(5, 5, 5), (6, 5, 5), (5, 5, 4), (6, 5, 4), (6, 4, 4)]
QP_STEPS = (22, 37, 43, 49, 51)                                  # + 6 * (depth - 8): from 37 / 43 / 49 on 8x8 / 16x16 / 32x32 units take dequant_scaling's second branch


def _orc():
    import test_cuserve as tc
    O = tc._orc()
    O.orc_sign_hide_hdq.restype, O.orc_sign_hide_hdq.argtypes = u32, [vp, vp, vp, u32, i32, i32]
    return O


# ---- table sets --------------------------------------------------------------------------------------------------------------------------------------

def table_offset(log2n, plane, rem):
    """where matrix (size, plane, rem) starts in a packed array: [size 8, 16, 32][plane Y, Cb, Cr][rem][n * n]"""
    return {3: 0, 4: 64 * 18, 5: (64 + 256) * 18}[log2n] + ((plane * 6 + rem) << (2 * log2n))


def derive_tables(mats, dcs):
    """mats[si][plane]: the 64 entries of the 8x8 base matrix of size 8 << si; dcs[si][plane]: the DC of sizes 16 and 32 (si 1, 2).  Returns the packed
    quantCoef / dequantCoef arrays of a table set"""
    q, dq = np.zeros(ENTRIES, np.int32), np.zeros(ENTRIES, np.int32)
    for si, n in enumerate((8, 16, 32)):
        ratio = n // 8
        idx = np.arange(n) // ratio
        for plane in range(3):
            ent = np.asarray(mats[si][plane], np.int64).reshape(8, 8)[idx][:, idx].copy()
            if ratio > 1:
                ent[0, 0] = dcs[si][plane]
            for rem in range(6):
                at = table_offset(3 + si, plane, rem)
                q[at:at + n * n] = ((QUANT_SCALES[rem] << 4) // ent).ravel()
                dq[at:at + n * n] = (INV_QUANT_SCALES[rem] * ent).ravel()
    assert table_offset(5, 2, 5) + 1024 == ENTRIES
    return q, dq


def default_set():
    """set A: the default inter 8x8 matrix of the standard (tests/golden/hevc_default_scaling_lists.json) for every size and plane, DC 16"""
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "hevc_default_scaling_lists.json")))
    inter = d["inter8x8"]
    assert len(inter) == 64 and min(inter) == 16 and max(inter) == 91
    return derive_tables([[inter] * 3] * 3, [[16] * 3] * 3)


def random_set(seed):
    """set B: entries 8..255 drawn per size and plane, random DCs"""
    rng = np.random.default_rng(seed)
    return derive_tables(rng.integers(8, 256, (3, 3, 64)), rng.integers(8, 256, (3, 3)))


def flat16_set():
    return derive_tables(np.full((3, 3, 64), 16), np.full((3, 3), 16))


# ---- the statement -------------------------------------------------------------------------------------------------------------------------------------

def job_header(hp, tc, shape, fmt, depth, qps, sliceI, signHide, scaling, coef=0, source_dct=0):
    j = tc._job_header(hp, shape[0], shape[1], shape[2], fmt, depth, qps, sliceI, signHide, coef=coef, source_dct=source_dct)
    j.scaling = scaling
    if scaling:
        for p in range(3):                                       # ignored with a set: anything read from them would show
            j.quantScale[p] = j.dequantScale[p] = 0
    return j


def dc_pixels(rng, log2cu, fmt, depth):
    """source + prediction whose difference is nearly constant: units whose only level is the DC"""
    import test_cuserve_formats as tcf
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    src, prd = [], []
    for (h, w) in tcf.plane_dims(log2cu, fmt):
        base = np.clip(np.rint(rng.normal(pmax / 2, pmax / 8, (h, w))), pmax // 8, pmax - pmax // 8)
        step = int(rng.integers(6, 40)) * (1 << (depth - 8)) * (1 if rng.integers(0, 2) else -1)
        p = np.clip(base + step + rng.integers(-1, 2, (h, w)), 0, pmax)
        src.append(base.astype(dt).ravel())
        prd.append(p.astype(dt).ravel())
    return np.ascontiguousarray(np.concatenate(src + prd))


def pixels(rng, log2cu, fmt, depth, kind):
    import test_cuserve_formats as tcf
    return dc_pixels(rng, log2cu, fmt, depth) if kind == 3 else tcf.job_pixels(rng, log2cu, fmt, depth, kind)


def statement(hp, O, j, pix, q, dq, seen=None):
    """the job with the table set (q, dq), composed from pinned pieces: ({unitIndex: (numSig, zeroDist, codedDist, codedEnergy)}, levels, resi).  seen: a dict
    that counts the inverse units of each dequantiser branch ("b1", "b2"), lone-DC units ("dc") and units whose levels sign hiding changed ("hidden")"""
    import test_cuserve_formats as tcf
    from backends import Orc
    if j.coefMode:
        return tcf.statement(hp, O, j, pix)                      # the host quantises: the set is carried and unused
    depth, fmt = j.bitDepth, j.chroma
    be = Orc(depth)
    pmax = (1 << depth) - 1
    dims = tcf.plane_dims(j.log2CUSize, fmt)
    half = sum(h * w for h, w in dims)
    src, prd, at = [], [], 0
    for (h, w) in dims:
        src.append(pix[at:at + h * w].reshape(h, w))
        prd.append(pix[half + at:half + at + h * w].reshape(h, w))
        at += h * w
    levels, resi = np.zeros(hp.CUJOB_MAX_ELEMS, np.int16), np.zeros(hp.CUJOB_MAX_ELEMS, np.int16)
    units = {}
    seen = seen if seen is not None else {}
    for (s, plane, tx, ty, ui, eo, n) in tcf.layout(j):
        log2n = n.bit_length() - 1
        f = np.ascontiguousarray(src[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        p = np.ascontiguousarray(prd[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        r = np.ascontiguousarray((f.astype(np.int32) - p.astype(np.int32)).astype(np.int16))
        rem, per = j.qpRem[plane], j.qpPer[plane]
        tab = table_offset(log2n, plane, rem)
        qc, dqc = np.ascontiguousarray(q[tab:tab + n * n]), np.ascontiguousarray(dq[tab:tab + n * n])
        # quant.cpp:408, :461, :466
        transform_shift = 15 - depth - log2n
        qbits = 14 + per + transform_shift
        coef = be.dct(n, r, (0, 0))
        lv, du, ns = be.quant(coef, qc, qbits, j.quantOffset << (qbits - 9))
        if ns >= 2 and j.signHide:
            plain = lv.copy()
            ns = O.orc_sign_hide_hdq(lv.ctypes.data, du.ctypes.data, coef.ctypes.data, ns, log2n, 0)
            seen["hidden"] = seen.get("hidden", 0) + int(not np.array_equal(plain, lv))
        assert ns == int(np.count_nonzero(lv))
        zero = be.sse_pp(n, f, (0, 0), p, (0, 0))
        levels[eo:eo + n * n] = lv
        if not ns:
            units[ui] = (0, zero, None, None)
            continue
        # quant.cpp:556-564: dequant_scaling adds 4 to the shift and takes `per` apart from the matrix
        shift = 20 - 14 - transform_shift
        seen["b1" if shift + 4 > per else "b2"] = seen.get("b1" if shift + 4 > per else "b2", 0) + 1
        back_c = be.dequant_scaling(lv, dqc, per, shift)
        if ns == 1 and lv[0] != 0:
            # quant.cpp:588-597
            dc = ((((int(back_c[0]) * (64 >> 6) + 1) >> 1) * (64 >> 3)) + (1 << (12 - (depth - 8) - 3 - 1))) >> (12 - (depth - 8) - 3)
            back = np.full((n, n), np.int16(dc), np.int16)
            seen["dc"] = seen.get("dc", 0) + 1
        else:
            back = be.idct(n, back_c)
        rec = np.ascontiguousarray(np.clip(p.astype(np.int32) + back, 0, pmax).astype(f.dtype))
        units[ui] = (ns, zero, be.sse_pp(n, f, (0, 0), rec, (0, 0)), be.psy_cost_pp(n, f, (0, 0), rec, (0, 0)))
        resi[eo:eo + n * n] = back.ravel()
    return units, levels, resi


def qps_of(depth, step):
    q = 6 * (depth - 8) + step
    return (q, q - 1, q - 3)


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def test_all_16_list_is_the_flat_quantiser():
    """tables of an all-16 list (quantCoef = quantScales[rem], dequantCoef = 16 * invQuantScales[rem]): the statement equals the flat restatement —
    test_cuserve_formats.statement (orc_transform_nxn / orc_invtransform_nxn) in every format, and orc_cujob_run_8 / _16 for chroma 0 / 1 — unit for unit:
    sizes 8 / 16 / 32, 8 / 10 / 12 bit, QPs on both sides of dequant_scaling's branch for every size, lone-DC units among them"""
    import test_cuserve as tc
    import test_cuserve_formats as tcf
    from x265_amd import hipprim as hp
    O = _orc()
    q, dq = flat16_set()
    for rem in range(6):
        for log2n in (3, 4, 5):
            at = table_offset(log2n, 1, rem)
            assert (q[at:at + (1 << (2 * log2n))] == QUANT_SCALES[rem]).all() and (dq[at:at + (1 << (2 * log2n))] == 16 * INV_QUANT_SCALES[rem]).all()
    rng = np.random.default_rng(1607)
    seen, total, units, coded, sizes = {}, 0, 0, 0, set()
    for depth in (8, 10, 12):
        for shape in SHAPES:
            for step in QP_STEPS:
                fmt = total % 4
                qps = qps_of(depth, step)
                j = job_header(hp, tc, shape, fmt, depth, qps, (total // 2) % 2, int(total % 3 != 0), 1)
                flat = tc._job_header(hp, shape[0], shape[1], shape[2], fmt, depth, qps, (total // 2) % 2, int(total % 3 != 0))
                pix = pixels(rng, shape[0], fmt, depth, (total // 4) % 4 if step != 51 else 3)
                got = statement(hp, O, j, pix, q, dq, seen)
                n, c = tcf.compare(flat, got, tcf.statement(hp, O, flat, pix), (depth, shape, fmt, qps))
                if fmt < 2:
                    done, wu, wl, wr = tc._oracle_job(hp, O, flat, pix)
                    want = ({ui: (wu[ui].numSig, wu[ui].zeroDist, wu[ui].codedDist, wu[ui].codedEnergy) for ui in got[0]}, wl, wr)
                    assert tcf.compare(flat, got, want, ("restatement", depth, shape, fmt, qps))[0] == done
                sizes |= {k[6] for k in tcf.layout(j)}
                total += 1; units += n; coded += c
    print("all-16 list: %d jobs, %d units, %d coded; %r" % (total, units, coded, seen))
    assert total == 3 * len(SHAPES) * len(QP_STEPS) and sizes == {8, 16, 32} and units > 0
    # both branches of dequant_scaling, lone-DC units and units whose levels sign hiding changed were among them
    assert min(seen.get(k, 0) for k in ("b1", "b2", "dc", "hidden")) > 0, seen
    assert seen["b1"] + seen["b2"] == coded


def test_library_takes_table_sets_and_the_abi_agrees():
    """x265hip_cujob_features() bit 0 (needs no device); the header's constants, the struct's new trailing field and the ctypes mirror agree"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    assert L.x265hip_cujob_features() & 1
    hdr = open(os.path.join(ROOT, "include", "x265hip.h")).read()
    m = re.search(r"#define X265HIP_CUJOB_SCALING_ENTRIES\s+\(\(64 \+ 256 \+ 1024\) \* 3 \* 6\)", hdr)
    assert m and ENTRIES == 24192
    assert int(re.search(r"#define X265HIP_CUJOB_SCALING_SETS\s+(\d+)", hdr).group(1)) == SETS
    body = re.search(r"typedef struct x265hip_cujob\s*\{(.*?)\}\s*x265hip_cujob;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "uint32_t scaling" and hp.CuJob._fields_[-1][0] == "scaling"
    assert C.sizeof(hp.CuJob) == 92 <= 128 and hp.CuJob.scaling.offset == 88
    assert hp.CuJob().scaling == 0                               # every existing constructor leaves the field 0: a flat job
    res, args = hp.PROTOTYPES["x265hip_cujob_scaling_add"]
    assert len(args) == 4 and hp.PROTOTYPES["x265hip_cujob_features"][1] == []


def _list_file(path, seed, low=None):
    """a scaling list file as ScalingList::parseScalingList reads it (scalinglist.cpp:246-339): every matrix by name, entries 8..255; low: one entry of the
    inter 8x8 luma matrix takes this value"""
    rng = np.random.default_rng(seed)
    lines = []
    for size, count in ((4, 16), (8, 64), (16, 64), (32, 64)):
        for kind in ("INTRA", "INTER"):
            for comp in (("LUMA",) if size == 32 else ("LUMA", "CHROMAU", "CHROMAV")):
                name = "%s%dX%d_%s" % (kind, size, size, comp)
                vals = rng.integers(8, 256, count)
                if low is not None and name == "INTER8X8_LUMA":
                    vals[27] = low
                lines.append(name)
                lines.append(",".join(str(int(v)) for v in vals) + ",")
                if size >= 16:
                    lines.append(name + "_DC")
                    lines.append("%d," % int(rng.integers(8, 256)))
    # (the parser walks sizes, then lists 0..5: intra Y, U, V, inter Y, U, V — the order written here)
    open(path, "w").write("\n".join(lines) + "\n")


def test_emulated_encoder_keeps_scaling_list_cus_on_the_host(tmp_path):
    """the emulated ABI has neither x265hip_cujob_features nor x265hip_cujob_scaling_add: with --scaling-list default the binding hands it no CU
    job (under require a rejected job would end the encode), says nothing about a failure, and the bytes are the reference's"""
    import test_cuserve_formats as tcf
    import test_saostats_formats as sf
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    sf._need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=93)
    args = ["--input", yuv, "--input-res", "328x200", "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2",
            "--scaling-list", "default"]
    err = sf._encode_pair(tmp_path, ref, emul, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1"))
    assert "OFF" not in err and "did not come back" not in err and "VERIFY FAILED" not in err, err[-1200:]
    m = re.search(tcf.JOBS_RE, err)
    assert m is None or int(m.group(1)) == 0, err[-1200:]
    s = re.search(SCALING_RE, err)
    assert s is None or (int(s.group(1)) == 0 and int(s.group(2)) == 0), err[-1200:]


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def _device(mode, slots=4):
    import test_cuserve as tc
    import test_cuserve_formats as tcf
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    cs = vp()
    hp.check(L.x265hip_cuserve_open(slots, mode, C.byref(cs)))
    return hp, L, tc, tcf, cs


def _add(hp, L, cs, tables):
    q, dq = tables
    sid = u32()
    hp.check(L.x265hip_cujob_scaling_add(cs, q.ctypes.data, dq.ctypes.data, C.byref(sid)))
    return sid.value


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_jobs_with_table_sets_match_the_statement(mode):
    """two sets on one service — A from the standard's default inter matrix, B random entries 8..255 with random DCs — named alternately by the jobs: 8 / 10 / 12
    bit, formats 1 and 3 on every shape and QP, 0 and 2 on every shape, QPs 6 * (depth - 8) + {22, 37, 43, 49, 51} with chroma a little below, sign hiding on
    and off, P and I offsets, coefficient mode with and without sourceDct; a flat 4:2:0 job on the same slot after every fourth against orc_cujob_run_*.  The
    first job of mode 0 starts the resident server BEFORE the sets are registered."""
    hp, L, tc, tcf, cs = _device(mode)
    O = _orc()
    try:
        rng = np.random.default_rng(1700 + mode)
        j0 = tc._job_header(hp, 5, 5, 5, 1, 8, (30, 29, 29), 0, 1)
        p0 = tc._job_pixels(rng, 5, 1, 8, 1)
        done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
        assert tc._compare(hp, j0, tc._run_on(hp, L, cs, 0, j0, p0), wu, wl, wr, "flat job before any set")[0] == done
        sets = {}
        for tables in (default_set(), random_set(77)):
            sets[_add(hp, L, cs, tables)] = tables
        assert sorted(sets) == [1, 2]
        seen, total, units, coded, sources, between = {}, 0, 0, 0, 0, 0
        per_set = {1: 0, 2: 0}
        for depth in (8, 10, 12):
            for fmt in (1, 3, 0, 2):
                for shape in SHAPES:
                    for step in (QP_STEPS if fmt in (1, 3) else (QP_STEPS[(total // 3) % 5],)):
                        sid = 1 + total % 2
                        coef, source_dct = (1, 1) if total % 7 == 2 else (1, 0) if total % 7 == 5 else (0, 0)
                        qps = qps_of(depth, step)
                        j = job_header(hp, tc, shape, fmt, depth, qps, (total // 2) % 2, int(total % 3 != 0), sid, coef=coef, source_dct=source_dct)
                        pix = pixels(rng, shape[0], fmt, depth, (total // 3) % 4)
                        q, dq = sets[sid]
                        n, c = tcf.compare(j, tcf.run_on(hp, L, cs, total % 4, j, pix), statement(hp, O, j, pix, q, dq, seen), (mode, depth, fmt, shape, qps, sid, coef))
                        total += 1; units += n
                        if coef:
                            sources += c
                        else:
                            coded += c
                            per_set[sid] += c
                        if total % 4 == 0:
                            j0 = tc._job_header(hp, 6, 5, 4, 1, depth, qps, 0, 1)
                            p0 = tc._job_pixels(rng, 6, 1, depth, 1)
                            done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
                            assert tc._compare(hp, j0, tc._run_on(hp, L, cs, (total - 1) % 4, j0, p0), wu, wl, wr, ("flat job between", mode, depth, total))[0] == done
                            between += 1
        print("mode %d: %d jobs, %d units, %d coded (%r per set), %d source transforms, %d flat jobs between; %r" % (mode, total, units, coded, per_set, sources, between, seen))
        assert total == 3 * (2 * len(SHAPES) * len(QP_STEPS) + 2 * len(SHAPES)) and between == total // 4
        # units per shape: 4:2:0 and 4:4:4 3 + 12 + 15 + 60 + 48, luma alone 1 + 4 + 5 + 20 + 16, 4:2:2 five per luma unit
        assert units == 3 * (2 * 5 * 138 + 46 + 5 * 46) and min(per_set.values()) > 0 and sources > 0
        # both branches of dequant_scaling, lone-DC units and units whose levels sign hiding changed all occurred
        assert min(seen.get(k, 0) for k in ("b1", "b2", "dc", "hidden")) > 0, seen
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_inverse_jobs_with_a_table_set_are_exact():
    """X265HIP_CUJOB_INVERSE with an id: dequant_scaling with the set's [32][Y][rem] matrix -> idct -> the measurements, for the levels of the statement's
    forward half: 32x32, 8 bit, QP 30 (first branch) and 49 (second)"""
    hp, L, tc, tcf, cs = _device(0)
    O = _orc()
    try:
        sets = {}
        for tables in (default_set(), random_set(78)):
            sets[_add(hp, L, cs, tables)] = tables
        rng = np.random.default_rng(1750)
        seen, served = {}, 0
        for qp in (30, 49):
            for sid in (1, 2):
                for kind in (0, 1, 3):
                    q, dq = sets[sid]
                    j = job_header(hp, tc, (5, 5, 5), 0, 8, (qp, qp, qp), 0, 1, sid)
                    pix = pixels(rng, 5, 0, 8, kind)
                    wu, wl, wr = statement(hp, O, j, pix, q, dq, seen)
                    if not wu[0][0]:
                        continue
                    ji = job_header(hp, tc, (5, 5, 5), 0, 8, (qp, qp, qp), 0, 0, sid, coef=8)
                    blob = np.frombuffer(pix.tobytes() + wl[:1024].tobytes(), np.uint8).copy()
                    gu, _, gr = tcf.run_on(hp, L, cs, served % 4, ji, blob)
                    assert gu[0] == wu[0], (qp, sid, kind, gu[0], wu[0])
                    assert np.array_equal(gr[:1024], wr[:1024]), (qp, sid, kind, "resi")
                    served += 1
        assert served >= 8 and seen.get("b1", 0) > 0 and seen.get("b2", 0) > 0, (served, seen)
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_table_set_limits():
    """a job that names a set nobody registered, and id 9, are X265HIP_EINVAL; the ninth x265hip_cujob_scaling_add fails and the service goes on serving: a
    job with set 1 and a flat job afterwards still match"""
    hp, L, tc, tcf, cs = _device(0)
    O = _orc()
    try:
        rng = np.random.default_rng(1760)
        job = vp()
        hp.check(L.x265hip_cuserve_slot(cs, 1, C.byref(job), None, None, None, None))
        seq = u32()

        def refused(sid):
            bad = job_header(hp, tc, (5, 5, 4), 1, 8, (30, 29, 29), 0, 1, sid)
            C.memmove(job, C.byref(bad), C.sizeof(bad))
            return L.x265hip_cuserve_submit(cs, 1, C.byref(seq)) == -1      # X265HIP_EINVAL

        def flat_matches(label):
            j0 = tc._job_header(hp, 5, 5, 4, 1, 8, (30, 29, 29), 0, 1)
            p0 = tc._job_pixels(rng, 5, 1, 8, 1)
            done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
            assert tc._compare(hp, j0, tc._run_on(hp, L, cs, 1, j0, p0), wu, wl, wr, label)[0] == done

        assert refused(1) and refused(9)
        flat_matches("flat job after the refused ones")
        first = default_set()
        assert _add(hp, L, cs, first) == 1
        assert refused(2) and refused(9) and refused(0xffffffff)
        for k in range(2, SETS + 1):
            assert _add(hp, L, cs, random_set(100 + k)) == k
        sid = u32(77)
        q9, dq9 = random_set(109)
        assert L.x265hip_cujob_scaling_add(cs, q9.ctypes.data, dq9.ctypes.data, C.byref(sid)) != 0
        assert refused(9)
        j = job_header(hp, tc, (5, 5, 4), 1, 8, (30, 29, 27), 0, 1, 1)
        pix = pixels(rng, 5, 1, 8, 0)                            # (uniform noise: every unit is coded)
        n, c = tcf.compare(j, tcf.run_on(hp, L, cs, 1, j, pix), statement(hp, O, j, pix, *first), "set 1 after the ninth was refused")
        assert n == 15 and c > 0
        flat_matches("flat job after the ninth set was refused")
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


BOUND = {   # depth, csp, preset, extra arguments, list ("default", "file": entries 8..255, "low": one entry 4)
    "8bit": (8, "i420", "medium", [], "default"), "main10": (10, "i420", "medium", [], "default"), "main12": (12, "i420", "medium", [], "default"),
    "8bit-444": (8, "i444", "medium", [], "default"), "main10-422": (10, "i422", "medium", [], "default"),
    "8bit-ctu32": (8, "i420", "medium", ["--ctu", "32"], "default"),
    "8bit-rdoq": (8, "i420", "slow", [], "default"),
    "8bit-qp49": (8, "i420", "medium", ["--qp", "49"], "default"),
    "8bit-list-file": (8, "i420", "medium", [], "file"),
    "8bit-entry-4": (8, "i420", "medium", [], "low"),
}


def _hip_run(hip, args, out, env):
    import subprocess
    r = subprocess.run([hip] + args + ["-o", out], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-1200:]
    return r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND))
def test_bound_encoders_serve_scaling_list_cus_byte_identical(tmp_path, name):
    """the product's encoders (oracle/_ref/integration) with scaling lists against the unmodified reference, 328x200 with partial CTUs, X265HIP_VERIFY
    recomputing every served unit with the reference's own Quant and tables: the same bytes; every CU job carried a set (J == the jobs of the cuserve line,
    J > 0), no CU was kept on the host because of its list, more forward units than jobs.  A list with an entry 4 stays on the host (J == 0, D > 0).  With
    X265HIP_CUSERVE_SCALING=0: the same bytes and no CU job."""
    import test_cuserve_formats as tcf
    import test_saostats_formats as sf
    depth, csp, preset, extra, lst = BOUND[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % depth), os.path.join(REF, "integration", "x265_hip_%dbit" % depth)
    sf._need(ref, hip)
    yuv = str(tmp_path / "clip.yuv")
    sf._clip(yuv, 328, 200, 6, depth, csp, 95 + depth)
    if lst != "default":
        _list_file(str(tmp_path / "lists.txt"), 31, low=4 if lst == "low" else None)
        lst = str(tmp_path / "lists.txt")
    args = ["--input", yuv, "--input-res", "328x200", "--input-depth", str(depth), "--input-csp", csp, "--fps", "30", "--frames", "6", "--preset", preset,
            "--hash", "1", "--pools", "4", "-F", "2", "--scaling-list", lst] + extra
    env = dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1")
    err = sf._encode_pair(tmp_path, ref, hip, args, env)
    m, s = re.search(tcf.JOBS_RE, err), re.search(SCALING_RE, err)
    assert s, err[-1500:]
    sets, carried, kept = (int(g) for g in s.groups())
    jobs, fwd, inv = (int(g) for g in m.groups()) if m else (0, 0, 0)
    print("%s: %d sets, %d jobs carried one, %d CUs kept; %d jobs, %d forward units, %d inverse units" % (name, sets, carried, kept, jobs, fwd, inv))
    if name == "8bit-entry-4":
        assert carried == 0 and kept > 0 and jobs == 0, (sets, carried, kept, jobs)
        return
    assert carried > 0, (sets, carried, kept)
    if name != "8bit-qp49":
        assert sets == 1 and carried == jobs and kept == 0 and fwd > jobs, (sets, carried, kept, jobs, fwd)
    if name == "8bit-rdoq":
        assert inv > 0, (jobs, fwd, inv)
    off = _hip_run(hip, args, str(tmp_path / "off.hevc"), dict(env, X265HIP_CUSERVE_SCALING="0"))
    m = re.search(tcf.JOBS_RE, off)
    assert m is None or int(m.group(1)) == 0, off[-1200:]
    assert open(str(tmp_path / "off.hevc"), "rb").read() == open(str(tmp_path / "ref.hevc"), "rb").read(), "X265HIP_CUSERVE_SCALING=0: bitstreams differ"
