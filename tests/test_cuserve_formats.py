"""CU residual quad-tree jobs (include/x265hip.h x265hip_cujob) of 4:2:2 and 4:4:4 pictures: x265hip_cujob::chroma = 2 / 3.

CPU tier: a Python composition of one job in any chroma format — per unit orc_transform_nxn / orc_invtransform_nxn (pinned to the reference's Quant class by
test_cuserve.py), sse_pp and psy_cost_pp of tests/backends.py, laid out by a Python mirror of the header's layout rules — itself pinned: for chroma 0 and 1 it
is orc_cujob_run_8 / _16 unit for unit, and its layout is test_cuserve._layout; the library's format mask; the emulated-ABI encoders, whose library takes no
such jobs, on 4:2:2 / 4:4:4 clips.
GPU tier: device jobs of both formats against the composition (both server modes, 8 / 10 / 12 bit, every shape, ordinary and coefficient mode, 4:2:0 jobs
between them on the same slots), the limits, and the bound encoders against the unmodified reference under X265HIP_VERIFY."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
vp, u32 = C.c_void_p, C.c_uint32

HS, VS = {0: 0, 1: 1, 2: 1, 3: 0}, {0: 0, 1: 1, 2: 0, 3: 0}          # chroma shifts of x265hip_cujob::chroma (X265_CSP_I400..I444)
CSP = {"i420": 1, "i422": 2, "i444": 3}
JOBS_RE = r"cuserve: (\d+) CU residual quad-trees .*?: (\d+) forward transform\+quant units and (\d+) inverse units served"


# ---- the layout rules and the statement of a job -------------------------------------------------------------------------------------------------

def plane_dims(log2cu, fmt):
    """[(height, width)] of the planes of a job's pixel block"""
    N = 1 << log2cu
    return [(N, N)] + ([(N >> VS[fmt], N >> HS[fmt])] * 2 if fmt else [])


def layout(j):
    """[(s, plane, tx, ty, unitIndex, elemOffset, n)]: levels from the largest luma transform size down; in a level Y, Cb, Cr; in a plane raster order of its
    units — (N >> s)^2 luma units of size s, (N >> hs >> (s - hs)) x (N >> vs >> (s - hs)) chroma units of size s - hs; a unit's block of levels / residual
    holds n * n entries, the blocks in the same order"""
    fmt = j.chroma
    hi, lo = min(5, j.log2TrMax, j.log2CUSize), max(4, j.log2TrMin)
    out, unit, elem = [], 0, 0
    for s in range(hi, lo - 1, -1):
        for plane, (h, w) in enumerate(plane_dims(j.log2CUSize, fmt)):
            n = 1 << (s - HS[fmt] if plane else s)
            for ty in range(h // n):
                for tx in range(w // n):
                    out.append((s, plane, tx, ty, unit, elem, n))
                    unit += 1
                    elem += n * n
    return out


def job_pixels(rng, log2cu, fmt, depth, kind):
    """source + prediction, Y then Cb, Cr, as the job's pixel block (the three kinds of test_cuserve._job_pixels)"""
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    src, prd = [], []
    for (h, w) in plane_dims(log2cu, fmt):
        base = rng.integers(0, pmax + 1, (h, w)) if kind == 0 else np.clip(np.rint(rng.normal(pmax / 2, pmax / 6, (h, w))), 0, pmax)
        if kind == 0:
            p = rng.integers(0, pmax + 1, (h, w))
        else:
            p = np.clip(base + np.rint(rng.normal(0, (2 + 3 * kind) * (1 << (depth - 8)), (h, w))), 0, pmax)
        src.append(base.astype(dt).ravel())
        prd.append(p.astype(dt).ravel())
    return np.ascontiguousarray(np.concatenate(src + prd))


def statement(hp, O, j, pix):
    """the job composed from pinned pieces: {unitIndex: (numSig, zeroDist, codedDist, codedEnergy)}, levels, resi"""
    from backends import Orc
    depth, fmt = j.bitDepth, j.chroma
    be = Orc(depth)
    pmax = (1 << depth) - 1
    dims = plane_dims(j.log2CUSize, fmt)
    half = sum(h * w for h, w in dims)
    src, prd, at = [], [], 0
    for (h, w) in dims:
        src.append(pix[at:at + h * w].reshape(h, w))
        prd.append(pix[half + at:half + at + h * w].reshape(h, w))
        at += h * w
    levels, resi = np.zeros(hp.CUJOB_MAX_ELEMS, np.int16), np.zeros(hp.CUJOB_MAX_ELEMS, np.int16)
    units = {}
    for (s, plane, tx, ty, ui, eo, n) in layout(j):
        log2n = n.bit_length() - 1
        f = np.ascontiguousarray(src[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        p = np.ascontiguousarray(prd[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        r = np.ascontiguousarray((f.astype(np.int32) - p.astype(np.int32)).astype(np.int16))
        coeff, dct = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16)
        ns = O.orc_transform_nxn(r.ctypes.data, n, coeff.ctypes.data, dct.ctypes.data, log2n, depth, j.qpRem[plane], j.qpPer[plane], j.quantScale[plane],
                                 j.quantOffset, j.signHide)
        zero = be.sse_pp(n, f, (0, 0), p, (0, 0))
        if j.coefMode:
            levels[eo:eo + n * n] = dct
            if j.sourceDct and plane == 0:
                f16 = np.ascontiguousarray(f.astype(np.int16))
                sdct = np.zeros(n * n, np.int16)
                O.orc_transform_nxn(f16.ctypes.data, n, coeff.ctypes.data, sdct.ctypes.data, log2n, depth, j.qpRem[plane], j.qpPer[plane], j.quantScale[plane],
                                    j.quantOffset, 0)
                resi[eo:eo + n * n] = sdct
            units[ui] = (0, zero, None, None)
            continue
        levels[eo:eo + n * n] = coeff
        if ns:
            back = np.zeros((n, n), np.int16)
            O.orc_invtransform_nxn(back.ctypes.data, n, coeff.ctypes.data, log2n, depth, j.qpPer[plane], j.dequantScale[plane], ns)
            rec = np.ascontiguousarray(np.clip(p.astype(np.int32) + back, 0, pmax).astype(f.dtype))
            units[ui] = (ns, zero, be.sse_pp(n, f, (0, 0), rec, (0, 0)), be.psy_cost_pp(n, f, (0, 0), rec, (0, 0)))
            resi[eo:eo + n * n] = back.ravel()
        else:
            units[ui] = (0, zero, None, None)
    return units, levels, resi


def run_on(hp, L, cs, slot, j, pix, timeout=20.0):
    """the job through submit / poll on library L: ({unitIndex: (numSig, zeroDist, codedDist, codedEnergy)}, levels, resi)"""
    job, pixels, units, levels, resi = vp(), vp(), vp(), vp(), vp()
    hp.check(L.x265hip_cuserve_slot(cs, slot, C.byref(job), C.byref(pixels), C.byref(units), C.byref(levels), C.byref(resi)))
    assert pix.nbytes <= hp.CUJOB_PIXEL_BYTES
    C.memmove(job, C.byref(j), C.sizeof(j))
    C.memmove(pixels, pix.ctypes.data, pix.nbytes)
    seq = u32()
    hp.check(L.x265hip_cuserve_submit(cs, slot, C.byref(seq)))
    lay = layout(j)
    assert len(lay) <= hp.CUJOB_MAX_UNITS and lay[-1][5] + lay[-1][6] ** 2 <= hp.CUJOB_MAX_ELEMS
    un = C.cast(units, C.POINTER(hp.CuJobUnit))
    t0 = time.time()
    while any(un[k[4]].ready != seq.value or un[k[4]].readyInv != seq.value for k in lay):
        pk = L.x265hip_cuserve_poke(cs, slot)
        if pk < 0:
            hp.check(pk)
        assert time.time() - t0 < timeout, "job not finished after %.0f s" % timeout
    lv = np.ctypeslib.as_array(C.cast(levels, C.POINTER(C.c_int16)), (hp.CUJOB_MAX_ELEMS,)).copy()
    rs = np.ctypeslib.as_array(C.cast(resi, C.POINTER(C.c_int16)), (hp.CUJOB_MAX_ELEMS,)).copy()
    return {k[4]: (un[k[4]].numSig, un[k[4]].zeroDist, un[k[4]].codedDist, un[k[4]].codedEnergy) for k in lay}, lv, rs


def compare(j, got, want, label):
    """every unit's numSig, zeroDist, levels, and for coded units codedDist, codedEnergy and resi: exact.  Returns (units, coded units + source transforms)"""
    (gu, gl, gr), (wu, wl, wr) = got, want
    n_units = coded = 0
    for (s, plane, tx, ty, ui, eo, n) in layout(j):
        where = (label, s, plane, tx, ty)
        assert gu[ui][0] == wu[ui][0], (where, "numSig", gu[ui][0], wu[ui][0])
        assert gu[ui][1] == wu[ui][1], (where, "zeroDist", gu[ui][1], wu[ui][1])
        assert np.array_equal(gl[eo:eo + n * n], wl[eo:eo + n * n]), (where, "levels")
        if j.coefMode:
            if j.sourceDct and plane == 0:
                assert np.array_equal(gr[eo:eo + n * n], wr[eo:eo + n * n]), (where, "source transform")
                coded += 1
        elif wu[ui][0]:
            assert gu[ui][2] == wu[ui][2], (where, "codedDist", gu[ui][2], wu[ui][2])
            assert gu[ui][3] == wu[ui][3], (where, "codedEnergy", gu[ui][3], wu[ui][3])
            assert np.array_equal(gr[eo:eo + n * n], wr[eo:eo + n * n]), (where, "resi")
            coded += 1
        n_units += 1
    return n_units, coded


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------------------

def test_layout_rules_of_the_formats():
    """the mirror of the layout rules: for chroma 0 and 1 it is test_cuserve._layout entry for entry; for 4:2:2 and 4:4:4 the counts the header's constants are
    derived from (units, entries and pixel bytes of the largest job of each kind)"""
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    for shape in tc.JOB_SHAPES:
        for fmt in (0, 1):
            j = tc._job_header(hp, shape[0], shape[1], shape[2], fmt, 8, (30, 30, 30), 0, 1)
            assert layout(j) == tc._layout(hp, j), (shape, fmt)
    most_units = most_elems = 0
    for fmt in (0, 1, 2, 3):
        for log2cu in (4, 5, 6):
            for tr_max, tr_min in ((5, 5), (5, 4), (4, 4), (5, 2)):
                lay = layout(tc._job_header(hp, log2cu, tr_max, tr_min, fmt, 8, (30, 30, 30), 0, 1))
                if not lay:
                    continue
                assert [k[4] for k in lay] == list(range(len(lay)))
                most_units, most_elems = max(most_units, len(lay)), max(most_elems, lay[-1][5] + lay[-1][6] ** 2)
    assert (most_units, most_elems) == (hp.CUJOB_MAX_UNITS, hp.CUJOB_MAX_ELEMS) == (100, 2 * 12288)
    assert hp.CUJOB_PIXEL_BYTES == 2 * 2 * sum(h * w for h, w in plane_dims(6, 3)) == 49152
    # 4:2:2, 64x64, sizes 32 + 16: a chroma plane is 32 x 64 — 2 x 4 units of 16, then 4 x 8 units of 8; the two sub-TUs of transform unit (tuX, tuY) are rows
    # 2 * tuY and 2 * tuY + 1 of the plane's raster
    lay = layout(tc._job_header(hp, 6, 5, 4, 2, 8, (30, 30, 30), 0, 1))
    cb = [k for k in lay if k[0] == 5 and k[1] == 1]
    assert [(k[2], k[3]) for k in cb] == [(x, y) for y in range(4) for x in range(2)] and cb[0][4] == 4 and cb[0][5] == 4096 and cb[0][6] == 16
    cr8 = [k for k in lay if k[0] == 4 and k[1] == 2]
    assert len(cr8) == 32 and cr8[0][4] == 20 + 16 + 32 and cr8[-1][4] == 99 and cr8[-1][6] == 8 and cr8[-1][5] + 64 == 2 * 8192
    # 4:4:4: chroma units of the luma size
    lay = layout(tc._job_header(hp, 6, 5, 5, 3, 8, (30, 30, 30), 0, 1))
    assert [k[6] for k in lay] == [32] * 12 and [k[5] for k in lay] == [1024 * i for i in range(12)]


@pytest.mark.parametrize("depth", [8, 10])
def test_statement_is_the_restatement_for_420_and_400(depth):
    """statement() == orc_cujob_run_8 / _16 unit for unit on every shape of test_cuserve.JOB_SHAPES, ordinary and coefficient mode"""
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    O = tc._orc()
    total = units = coded = 0
    for shape, kind, qps, sliceI, signHide, rng in tc._cases(depth, 300 + depth):
        variant = total % 3                                   # 0: ordinary, 1: coefficients + source transform, 2: coefficients only
        j = tc._job_header(hp, *shape, depth, qps, sliceI, signHide, coef=int(variant != 0), source_dct=int(variant == 1))
        pix = tc._job_pixels(rng, shape[0], shape[3], depth, kind)
        assert pix.size == 2 * sum(h * w for h, w in plane_dims(shape[0], shape[3]))
        done, wu, wl, wr = tc._oracle_job(hp, O, j, pix)
        su, sl, sr = statement(hp, O, j, pix)
        assert len(su) == done
        want = ({ui: (wu[ui].numSig, wu[ui].zeroDist, wu[ui].codedDist, wu[ui].codedEnergy) for ui in su}, wl, wr)
        n, c = compare(j, (su, sl, sr), want, (depth, shape, kind, qps, variant))
        total += 1; units += n; coded += c
    assert total == len(tc.JOB_SHAPES) * 6 and units > 700 and coded > 100


def test_library_reports_its_cu_job_formats():
    """x265hip_cujob_formats: 4:0:0, 4:2:0, 4:2:2 and 4:4:4; needs no device"""
    from x265_amd import hipprim as hp
    assert hp.lib().x265hip_cujob_formats() == 0xF


@pytest.mark.parametrize("csp", ["i422", "i444"])
def test_emulated_encoder_keeps_422_and_444_cus_on_the_host(tmp_path, csp):
    """the emulated ABI has no x265hip_cujob_formats and its CU jobs are 4:2:0 / 4:0:0 ones: the binding hands it no job of another format (under require a
    rejected job would end the encode), says nothing about a failure, and the bytes are the reference's"""
    import test_saostats_formats as sf
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    sf._need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=91, csp=csp)
    args = ["--input", yuv, "--input-res", "328x200", "--input-csp", csp, "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2"]
    err = sf._encode_pair(tmp_path, ref, emul, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1"))
    assert "OFF" not in err and "did not come back" not in err, err[-1200:]
    m = re.search(JOBS_RE, err)
    assert m is None or int(m.group(1)) == 0, err[-1200:]


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------------------

def _device(mode, slots=4):
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    cs = vp()
    hp.check(L.x265hip_cuserve_open(slots, mode, C.byref(cs)))
    return hp, L, tc, cs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_jobs_of_422_and_444_match_the_statement(mode):
    """chroma = 2 and 3 on the MI355X against statement(): 8 / 10 / 12 bit, every shape of JOB_SHAPES with the format in place of its chroma flag (the largest
    jobs — 64x64, two levels, 16-bit samples — fill the slot's units, levels and pixel block to the last entry), three pixel kinds, sign hiding on and off,
    coefficient mode with and without sourceDct; a 4:2:0 job on the same slot after every fourth (the format is chosen per job)"""
    hp, L, tc, cs = _device(mode)
    O = tc._orc()
    try:
        total = units = coded = sources = between = 0
        seen = set()
        for depth in (8, 10, 12):
            for fmt in (2, 3):
                for shape, kind, qps, sliceI, signHide, rng in tc._cases(depth, 500 + 10 * fmt + depth):
                    variant = total % 3                       # 0: ordinary, 1: coefficients + source transform, 2: coefficients only
                    signHide = (total // 3) % 2
                    j = tc._job_header(hp, shape[0], shape[1], shape[2], fmt, depth, qps, sliceI, signHide, coef=int(variant != 0), source_dct=int(variant == 1))
                    pix = job_pixels(rng, shape[0], fmt, depth, kind)
                    n, c = compare(j, run_on(hp, L, cs, total % 4, j, pix), statement(hp, O, j, pix), (mode, depth, fmt, shape, kind, qps, variant, signHide))
                    seen.add((fmt, variant, signHide))
                    total += 1; units += n
                    if variant == 0:
                        coded += c
                    elif variant == 1:
                        sources += c
                    if total % 4 == 0:
                        j0 = tc._job_header(hp, 6, 5, 4, 1, depth, qps, sliceI, 1)
                        p0 = tc._job_pixels(rng, 6, 1, depth, kind)
                        done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
                        assert tc._compare(hp, j0, tc._run_on(hp, L, cs, (total - 1) % 4, j0, p0), wu, wl, wr, ("4:2:0 job between", mode, depth, total))[0] == done
                        between += 1
        assert len(seen) == 2 * 3 * 2
        assert total == 3 * 2 * len(tc.JOB_SHAPES) * 6 and units > 8000 and coded > 1000 and sources > 300 and between == total // 4
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_device_job_format_limits():
    """chroma == 4 and an inverse job with chroma are X265HIP_EINVAL; a 4:2:0 job submitted afterwards on the same slot still matches"""
    hp, L, tc, cs = _device(0)
    O = tc._orc()
    try:
        assert L.x265hip_cujob_formats() == 0xF
        rng = np.random.default_rng(12)
        job, pixels = vp(), vp()
        hp.check(L.x265hip_cuserve_slot(cs, 1, C.byref(job), C.byref(pixels), None, None, None))
        seq = u32()
        for bad in (tc._job_header(hp, 5, 5, 5, 4, 8, (30, 30, 30), 0, 1), tc._job_header(hp, 6, 5, 4, 7, 10, (40, 40, 40), 0, 1),
                    tc._job_header(hp, 5, 5, 5, 1, 8, (26, 26, 26), 0, 0, coef=8), tc._job_header(hp, 5, 5, 5, 2, 8, (26, 26, 26), 0, 0, coef=8),
                    tc._job_header(hp, 5, 5, 5, 3, 8, (26, 26, 26), 0, 0, coef=8)):
            C.memmove(job, C.byref(bad), C.sizeof(bad))
            assert L.x265hip_cuserve_submit(cs, 1, C.byref(seq)) == -1, (bad.chroma, bad.coefMode)      # X265HIP_EINVAL
        for fmt in (1, 2, 3, 1):
            j = tc._job_header(hp, 5, 5, 4, fmt, 8, (30, 29, 29), 0, 1)
            pix = job_pixels(rng, 5, fmt, 8, 1)
            if fmt == 1:
                done, wu, wl, wr = tc._oracle_job(hp, O, j, pix)
                assert tc._compare(hp, j, tc._run_on(hp, L, cs, 1, j, pix), wu, wl, wr, "4:2:0 after the refused jobs")[0] == done
            else:
                compare(j, run_on(hp, L, cs, 1, j, pix), statement(hp, O, j, pix), ("after the refused jobs", fmt))
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


BOUND = {
    "8bit-422": (8, "i422", "medium", []), "8bit-444": (8, "i444", "medium", []),
    "main10-422": (10, "i422", "medium", []), "main10-444": (10, "i444", "medium", []),
    "main12-422": (12, "i422", "medium", []), "main12-444": (12, "i444", "medium", []),
    "8bit-422-rdoq": (8, "i422", "slow", []), "main10-444-rdoq": (10, "i444", "slow", []),
    "main10-422-ctu32": (10, "i422", "medium", ["--ctu", "32"]),
}


def _hip_counts(hip, args, out, env):
    import subprocess
    r = subprocess.run([hip] + args + ["-o", out], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-1200:]
    m = re.search(JOBS_RE, r.stderr)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND))
def test_bound_encoders_serve_cu_jobs_of_422_and_444_byte_identical(tmp_path, name):
    """the product's encoders (oracle/_ref/integration) on 4:2:2 / 4:4:4 clips against the unmodified reference, 328x200 with partial CTUs: the same bytes with
    X265HIP_VERIFY recomputing every served unit, and the CU jobs ran — at least half as many as the same encoder hands over for the 4:2:0 rendition of the same
    clip (a count the 4:2:0 path produces; one half allows for the other format's mode decisions), with more forward units than jobs.  With
    X265HIP_CUSERVE_FORMATS=0: the same bytes and no CU job."""
    import test_saostats_formats as sf
    depth, csp, preset, extra = BOUND[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % depth), os.path.join(REF, "integration", "x265_hip_%dbit" % depth)
    sf._need(ref, hip)
    yuv, yuv420 = str(tmp_path / "clip.yuv"), str(tmp_path / "clip420.yuv")
    sf._clip(yuv, 328, 200, 6, depth, csp, 90 + depth)
    sf._clip(yuv420, 328, 200, 6, depth, "i420", 90 + depth)
    tail = ["--fps", "30", "--frames", "6", "--preset", preset, "--hash", "1", "--pools", "4", "-F", "2"] + extra
    args = ["--input", yuv, "--input-res", "328x200", "--input-depth", str(depth), "--input-csp", csp] + tail
    env = dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1")
    err = sf._encode_pair(tmp_path, ref, hip, args, env)
    m = re.search(JOBS_RE, err)
    assert m, err[-1500:]
    jobs, fwd = int(m.group(1)), int(m.group(2))
    jobs420, _ = _hip_counts(hip, ["--input", yuv420, "--input-res", "328x200", "--input-depth", str(depth)] + tail, str(tmp_path / "420.hevc"), env)
    print("%s: %d jobs, %d forward units; 4:2:0 rendition: %d jobs" % (name, jobs, fwd, jobs420))
    assert jobs420 > 0 and 2 * jobs >= jobs420 and fwd > jobs, (jobs, fwd, jobs420)
    off, _ = _hip_counts(hip, args, str(tmp_path / "off.hevc"), dict(env, X265HIP_CUSERVE_FORMATS="0"))
    assert off == 0
    assert open(str(tmp_path / "off.hevc"), "rb").read() == open(str(tmp_path / "ref.hevc"), "rb").read(), "X265HIP_CUSERVE_FORMATS=0: bitstreams differ"


@pytest.mark.gpu
def test_1080p_main10_422_encode_serves_cu_jobs_byte_identical():
    """the size users run: 1920x1080 Main 4:2:2 10, preset medium, 30 frames, against the unmodified reference; the job count against the 4:2:0 rendition's"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import encode_fps
    counts = {}
    for csp in ("i422", "i420"):
        r = encode_fps.measure(frames=30, width=1920, height=1080, bits=10, preset="medium", extra=(), seed=36, input_depth=10, csp=csp)
        if "error" in r and "not built" in r["error"]:
            pytest.skip(r["error"])
        assert "error" not in r, r
        assert r["byte_identical"], r
        m = re.search(JOBS_RE, "\n".join(r["gpu"]["served"]))
        assert m, r["gpu"]["served"]
        counts[csp] = (int(m.group(1)), int(m.group(2)))
    print("1080p Main10: 4:2:2 %d jobs, %d forward units; 4:2:0 %d jobs" % (counts["i422"] + counts["i420"][:1]))
    assert counts["i420"][0] > 0 and 2 * counts["i422"][0] >= counts["i420"][0] and counts["i422"][1] > counts["i422"][0], counts
