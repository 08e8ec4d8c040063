"""SAO statistics jobs (include/x265hip.h x265hip_saojob) at 10 and 12 bit, and the chroma planes of 4:2:2 / 4:4:4 pictures.

CPU tier: a direct numpy statement of one job at any depth, pinned against the saoCuStats* primitives (the oracle's restatements and, where built, the
reference's own Main10 / Main12 C); the emulated-ABI encoders: 8-bit 4:2:2 / 4:4:4 with every chroma plane served, and Main10, where the emulation takes no
16-bit jobs, on the host without a device-failure message (the binding reads x265hip_saojob_depths through a weak reference).
GPU tier: the ABI's depth mask and limits, device jobs at 10 / 12 bit against the statement (both server modes, 1x1 .. 64x64 planes, column packing at
its extremes), 8-bit jobs of 4:2:2 / 4:4:4 chroma geometry, and the bound Main10 / Main12 encoders against the reference under X265HIP_VERIFY."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
vp, u32 = C.c_void_p, C.c_uint32

EO = np.array([1, 2, 0, 3, 4])                                   # SAO::s_eoTable: sign + sign + 2 -> edge category
NB = {1: ((0, 1), (0, -1)), 2: ((1, 0), (-1, 0)), 3: ((1, 1), (-1, -1)), 4: ((1, -1), (-1, 1))}
SAO_RE = r"saostats: SAO statistics of (\d+) CTU planes .*? in (\d+) jobs, (\d+) planes on the host"


# ---- jobs and their statement --------------------------------------------------------------------------------------------------------------------

def _rects(w, h, po, right, bottom, left, above):
    """the five rectangles as SAO::calcSaoStatsCTU's start / end expressions produce them (po: the chroma offset 2)"""
    rects = [(0, 0, w if right else w - 5 + po, h if bottom else h - 4 + po),
             (left, 0, w - 1 if right else w - 5 + po, h - 4 + po),
             (0, above, w if right else w - 5 + po, h - 1 if bottom else h - 4 + po),
             (left, above, w - 1 if right else w - 5 + po, h - 1 if bottom else h - 4 + po),
             (left, above, w - 1 if right else w - 5 + po, h - 1 if bottom else h - 4 + po)]
    return [(0, 0, 0, 0) if x1 <= x0 or y1 <= y0 else (x0, y0, x1, y1) for x0, y0, x1, y1 in rects]


def make_job(hp, rng, depth, planes, eo23=1, kind=None, edges=None):
    """a job of `planes` = [(w, h, po), ...] at `depth`: rectangles as the reference draws them, samples of one of three kinds (uniform, normal around mid-grey,
    flat steps), source = reconstruction + noise; kind "max+" / "max-": flat reconstruction at 0 / the top with the source at the other end (every column word
    of a class holds as many samples of difference +-(2^depth - 1) as it can)"""
    j = hp.SaoCtuJob()
    j.bitDepth, j.planes, j.eo23 = depth, len(planes), eo23
    pmax, dt = (1 << depth) - 1, np.uint8 if depth == 8 else np.uint16
    blocks = []
    for b, (w, h, po) in enumerate(planes):
        e = edges if edges is not None else tuple(int(rng.integers(0, 3) == 0) for _ in range(4))
        j.plane[b].w, j.plane[b].h = w, h
        for c, (x0, y0, x1, y1) in enumerate(_rects(w, h, po, *e)):
            j.plane[b].x0[c], j.plane[b].y0[c], j.plane[b].x1[c], j.plane[b].y1[c] = x0, y0, x1, y1
        k = kind if kind is not None else int(rng.integers(0, 3))
        if k == "max+":
            rec, src = np.zeros((h + 1, w + 1), np.int64), np.full((h, w), pmax, np.int64)
        elif k == "max-":
            rec, src = np.full((h + 1, w + 1), pmax, np.int64), np.zeros((h, w), np.int64)
        else:
            rec = rng.integers(0, pmax + 1, (h + 1, w + 1)) if k == 0 else np.clip(np.rint(rng.normal(pmax / 2, pmax / 8, (h + 1, w + 1))), 0, pmax).astype(np.int64)
            if k == 2:
                rec = (rec >> (depth - 4)) << (depth - 4)                             # flat steps: many equal neighbours (the zero-sign category)
            src = np.clip(rec[1:, 1:] + np.rint(rng.normal(0, 4 << (depth - 8), (h, w))).astype(np.int64), 0, pmax)
        blocks += [rec.astype(dt).ravel(), src.astype(dt).ravel()]
    return j, np.ascontiguousarray(np.concatenate(blocks))


def _planes_of(j, pix):
    at = 0
    for b in range(j.planes):
        w, h = j.plane[b].w, j.plane[b].h
        rec = pix[at:at + (w + 1) * (h + 1)].reshape(h + 1, w + 1); at += (w + 1) * (h + 1)
        src = pix[at:at + w * h].reshape(h, w); at += w * h
        yield b, w, h, rec, src, [(j.plane[b].x0[c], j.plane[b].y0[c], j.plane[b].x1[c], j.plane[b].y1[c]) for c in range(5)]


def restate(j, pix):
    """the job in numpy: per plane and class every sample of the rectangle, band = rec >> (depth - 5), edge category = s_eoTable[sign + sign + 2] of the
    class's two neighbours; sums of (source - reconstruction) and counts in the slot's layout"""
    out = np.zeros(2 * 480, np.int64)
    for b, w, h, rec, src, rects in _planes_of(j, pix):
        rec, src = rec.astype(np.int64), src.astype(np.int64)
        for c, (x0, y0, x1, y1) in enumerate(rects):
            if (c >= 3 and not j.eo23) or x1 <= x0 or y1 <= y0:
                continue
            v = rec[1 + y0:1 + y1, 1 + x0:1 + x1]
            if c == 0:
                k = v >> (j.bitDepth - 5)
            else:
                (ay, ax), (by, bx) = NB[c]
                k = EO[np.sign(v - rec[1 + y0 + ay:1 + y1 + ay, 1 + x0 + ax:1 + x1 + ax]) + np.sign(v - rec[1 + y0 + by:1 + y1 + by, 1 + x0 + bx:1 + x1 + bx]) + 2]
            d = src[y0:y1, x0:x1] - v
            out[b * 160 + c * 32:b * 160 + c * 32 + 32] = np.bincount(k.ravel(), weights=d.ravel(), minlength=32).astype(np.int64)
            out[480 + b * 160 + c * 32:480 + b * 160 + c * 32 + 32] = np.bincount(k.ravel(), minlength=32)
    assert np.abs(out).max() < 2 ** 31
    return out.astype(np.int32)


def compose(j, pix, be):
    """the job as SAO::calcSaoStatsCTU walks it (oracle/x265_oracle_rqt.c orc_saojob_run_8's calls at any depth): diff = source - reconstruction at
    pitch 64, then saoCuStatsBO / E0..E3 of backend `be` (tests/backends.py Orc / Ref) with the sign buffers the reference primes"""
    out = np.zeros(2 * 480, np.int32)
    sign = lambda a, b: np.sign(a.astype(np.int32) - b.astype(np.int32)).astype(np.int8)      # noqa: E731  (saoSign / signOf)
    pad = np.zeros(96, np.int8)
    for b, w, h, rec, src, R in _planes_of(j, pix):
        diff = np.zeros(64 * 64 + 64, np.int16)
        diff[:64 * 64].reshape(64, 64)[:h, :w] = src.astype(np.int32) - rec[1:, 1:].astype(np.int32)
        rec = np.ascontiguousarray(rec)
        st, ct = out[b * 160:b * 160 + 160], out[480 + b * 160:480 + b * 160 + 160]

        def run(c, kind, off, pos, endX, endY, up1=pad, upt=pad):
            # (the class's 32 entries start at zero: the primitives add into them; an edge class fills entries 0..4)
            if endX > 0 and endY > 0:
                s, n, _, _ = be.sao_stats(kind, diff[off:], rec, pos, endX, endY, np.zeros(32, np.int32), np.zeros(32, np.int32), up1, upt)
                st[c * 32:c * 32 + 32] += s
                ct[c * 32:c * 32 + 32] += n

        run(0, 0, 0, (1, 1), R[0][2], R[0][3])
        run(1, 1, R[1][0], (1, 1 + R[1][0]), R[1][2] - R[1][0], R[1][3])
        x0, y0, x1, y1 = R[2]
        run(2, 2, y0 * 64, (1 + y0, 1), x1, y1 - y0, np.r_[np.int8(0), sign(rec[1 + y0, 1:], rec[y0, 1:]), pad])
        if j.eo23:
            x0, y0, x1, y1 = R[3]
            if x1 > x0 and y1 > y0:
                run(3, 3, y0 * 64 + x0, (1 + y0, 1 + x0), x1 - x0, y1 - y0, np.r_[np.int8(0), sign(rec[1 + y0, 1 + x0:1 + x1], rec[y0, x0:x1]), pad], np.zeros(96, np.int8))
            x0, y0, x1, y1 = R[4]
            if x1 > x0 and y1 > y0:
                # (E3's buffer starts one sample left of the rectangle: the function's upBuff1[-1])
                run(4, 4, y0 * 64 + x0, (1 + y0, 1 + x0), x1 - x0, y1 - y0, np.r_[sign(rec[1 + y0, x0:1 + x1], rec[y0, 1 + x0:2 + x1]), pad])
    return out


LUMA_CHROMA = [(64, 64, 0), (32, 32, 2), (32, 64, 2), (64, 64, 2)]


def _random_planes(rng, full):
    w, h, po = LUMA_CHROMA[int(rng.integers(0, 4))]
    if not full:
        w, h = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
    return [(w, h, po)]


@pytest.mark.parametrize("depth", [10, 12])
def test_sao_job_statement_matches_the_reference_primitives(depth):
    """restate() against the saoCuStats* primitives composed as the reference calls them: the oracle's restatements at this depth, and the reference's own
    C of the Main10 / Main12 build where it was built; random jobs of every plane geometry, and the extreme jobs of the device test"""
    from backends import Orc, Ref
    from oracle import pyoracle as po
    from x265_amd import hipprim as hp
    bes = [Orc(depth)] + ([Ref(depth)] if po.ref_available(depth) else [])
    rng = np.random.default_rng(40 + depth)
    jobs = [make_job(hp, rng, depth, _random_planes(rng, it % 4 == 0), eo23=int(it % 5 != 0)) for it in range(48)]
    jobs += [make_job(hp, rng, depth, [p], kind=k, edges=(1, 1, 0, 0)) for p in LUMA_CHROMA for k in ("max+", "max-")]
    checked = 0
    for it, (j, pix) in enumerate(jobs):
        want = restate(j, pix)
        for be in bes:
            got = compose(j, pix, be)
            assert np.array_equal(got, want), (be.name, it, np.nonzero(got != want)[0][:8])
        checked += int(want[480:].sum())
    assert checked > 100000
    # the statement's band is the reference's: a 10 / 12-bit sample falls into band sample >> (depth - 5)
    j, pix = make_job(hp, rng, depth, [(64, 64, 0)], kind="max-", edges=(1, 1, 0, 0))
    assert restate(j, pix)[480 + 31] == 64 * 64 and restate(j, pix)[31] == -64 * 64 * ((1 << depth) - 1)


# ---- the binding on the emulated ABI (CPU tier) ------------------------------------------------------------------------------------------------

def _encode_pair(tmp_path, ref, other, args, env, clip_bytes=None):
    want, got = str(tmp_path / "ref.hevc"), str(tmp_path / "other.hevc")
    r0 = subprocess.run([ref] + args + ["-o", want], capture_output=True, text=True, timeout=900)
    assert r0.returncode == 0, r0.stderr[-800:]
    r = subprocess.run([other] + args + ["-o", got], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-1200:]
    assert open(got, "rb").read() == open(want, "rb").read(), "bitstreams differ"
    return r.stderr


def _need(*paths):
    for p in paths:
        if not os.path.exists(p):
            pytest.skip("%s not built (make -C oracle ref emul; make -C integration hip)" % os.path.relpath(p, ROOT))


@pytest.mark.parametrize("csp", ["i422", "i444"])
def test_emulated_encoder_serves_chroma_sao_planes_of_422_and_444(tmp_path, csp):
    """8-bit 4:2:2 / 4:4:4, 328x200 (partial CTUs): every plane's statistics are jobs (the emulated ABI takes 8-bit planes up to 64x64), byte-identical,
    X265HIP_VERIFY beside every served plane"""
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    _need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=78, csp=csp)
    args = ["--input", yuv, "--input-res", "328x200", "--input-csp", csp, "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2"]
    err = _encode_pair(tmp_path, ref, emul, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1"))
    m = re.search(SAO_RE, err)
    assert m and int(m.group(1)) > 100 and int(m.group(3)) == 0, err[-1200:]


def test_emulated_main10_encoder_keeps_sao_statistics_on_the_host(tmp_path):
    """the emulated ABI takes no 16-bit SAO jobs and does not define x265hip_saojob_depths: the Main10 seam stays off without asking it (under require a
    rejected job would end the encode), and says nothing about a failure"""
    ref, emul = os.path.join(REF, "x265_10bit"), os.path.join(REF, "x265_emul_10bit")
    _need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=79, depth=10)
    args = ["--input", yuv, "--input-res", "328x200", "--input-depth", "10", "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2"]
    err = _encode_pair(tmp_path, ref, emul, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_SAOSTATS="1"))
    # (the seam never switched on: no report line, no planes, no failure)
    assert "saostats" not in err and "GPU path is OFF" not in err, err[-1200:]
    assert re.search(r"x265hip: cuserve: \d+ CU residual quad-trees", err), err[-1200:]     # (the bound modules did report: the run was the emulated one)


def test_library_reports_its_sao_job_depths():
    from x265_amd import hipprim as hp
    L = hp.lib()
    assert L.x265hip_saojob_depths() == (1 << 8) | (1 << 10) | (1 << 12)
    j = hp.SaoCtuJob()
    j.planes, j.plane[0].w, j.plane[0].h = 1, 64, 64
    for d, n in ((8, 65 * 65 + 64 * 64), (10, 2 * (65 * 65 + 64 * 64)), (12, 2 * (65 * 65 + 64 * 64))):
        j.bitDepth = d
        assert 128 + n <= 128 + 24576 and (128 + n + 511) // 512 <= 63, d       # one 64x64 plane fits the slot and the ticket's size field at every depth


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------------------

def _device(mode):
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    cs = vp()
    hp.check(L.x265hip_cuserve_open(4, mode, C.byref(cs)))
    return hp, L, tc, cs


def _submit(L, cs, slot, j, pix):
    job, pixels, units, levels, resi = vp(), vp(), vp(), vp(), vp()
    assert L.x265hip_cuserve_slot(cs, slot, C.byref(job), C.byref(pixels), C.byref(units), C.byref(levels), C.byref(resi)) == 0
    C.memmove(pixels, pix.ctypes.data, min(pix.nbytes, 24576))
    seq = u32()
    return L.x265hip_cuserve_submit_sao(cs, slot, C.byref(j), C.byref(seq))


@pytest.mark.gpu
def test_sao_job_depths_and_limits():
    """x265hip_saojob_depths reports 8, 10 and 12; a 10-bit job is accepted and measured; depths 9 and 16, planes over 64 and blocks over the slot are not"""
    hp, L, tc, cs = _device(0)
    try:
        assert L.x265hip_saojob_depths() == (1 << 8) | (1 << 10) | (1 << 12)
        rng = np.random.default_rng(3)
        j, pix = make_job(hp, rng, 10, [(64, 64, 0)])
        assert tc._same_sao(j, tc._run_sao_on(hp, L, cs, 0, j, pix), restate(j, pix), "10-bit job") == int(restate(j, pix)[480:].sum())
        einval = -1
        for depth in (9, 16, 0, 7, 11, 32, 1 << 31):
            jb, pb = make_job(hp, rng, 10, [(16, 16, 0)])
            jb.bitDepth = depth
            assert _submit(L, cs, 1, jb, pb) == einval, depth
        jb, pb = make_job(hp, rng, 12, [(64, 64, 0)])
        jb.plane[0].w = 65
        assert _submit(L, cs, 1, jb, pb) == einval
        jb.plane[0].w, jb.plane[0].x1[0] = 64, 65
        assert _submit(L, cs, 1, jb, pb) == einval
        jb, pb = make_job(hp, rng, 10, [(64, 64, 0), (64, 64, 2)])                # 33 284 bytes: more than a slot holds
        assert _submit(L, cs, 1, jb, pb) == einval
        jb, pb = make_job(hp, rng, 10, [(64, 64, 0), (32, 32, 2)])                # 20 868 bytes: fits
        want = restate(jb, pb)
        assert tc._same_sao(jb, tc._run_sao_on(hp, L, cs, 2, jb, pb), want, "two planes at 10 bit") > 0
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_sao_jobs_at_10_and_12_bit_match_the_statement(mode):
    """10 / 12-bit jobs on the MI355X against restate(): one plane of 1x1 .. 64x64 (luma) and of 32x32 / 32x64 / 64x64 (4:2:0 / 4:2:2 / 4:4:4 chroma),
    every availability pattern, eo23 on and off, a whole column of one bin at difference +-(2^depth - 1); CU and 8-bit SAO jobs on the same slots"""
    hp, L, tc, cs = _device(mode)
    O = tc._orc()
    try:
        rng = np.random.default_rng(900 + mode)
        measured = 0
        jobs = []
        for depth in (10, 12):
            jobs += [make_job(hp, rng, depth, [(w, h, 0)]) for w, h in ((1, 1), (1, 64), (64, 1), (2, 3), (7, 9), (33, 17), (63, 64), (64, 63))]
            jobs += [make_job(hp, rng, depth, [p], kind=k, edges=(1, 1, 0, 0)) for p in LUMA_CHROMA for k in ("max+", "max-")]
            jobs += [make_job(hp, rng, depth, [p], edges=e) for p in LUMA_CHROMA for e in ((0, 0, 0, 0), (1, 1, 1, 1))]
            jobs += [make_job(hp, rng, depth, _random_planes(rng, it % 3 == 0), eo23=int(it % 4 != 3)) for it in range(60)]
        for it, (j, pix) in enumerate(jobs):
            if it % 7 == 6:
                # an 8-bit job of the existing kind between them (the 8-bit form is selected per job)
                j8, p8 = tc._sao_job(hp, rng, 3, False)
                tc._same_sao(j8, tc._run_sao_on(hp, L, cs, it % 4, j8, p8), tc._oracle_sao(hp, O, j8, p8), ("8-bit job between", it))
            measured += tc._same_sao(j, tc._run_sao_on(hp, L, cs, it % 4, j, pix), restate(j, pix), (mode, it, j.bitDepth, j.plane[0].w, j.plane[0].h))
        assert measured > 300000
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_device_8bit_sao_jobs_of_422_and_444_chroma_geometry():
    """8-bit chroma planes of 4:2:2 (32x64) and 4:4:4 (64x64) with the chroma offset 2, partial ones too, against the restatement the emulated ABI runs"""
    hp, L, tc, cs = _device(0)
    O = tc._orc()
    try:
        rng = np.random.default_rng(422)
        measured = 0
        for it in range(40):
            p = [(32, 64, 2), (64, 64, 2)][it % 2]
            if it % 3 == 2:
                p = (int(rng.integers(1, p[0] + 1)), int(rng.integers(1, p[1] + 1)), 2)
            planes = [p] if it % 4 < 2 else [(64, 64, 0), p]
            j, pix = make_job(hp, rng, 8, planes, eo23=int(it % 5 != 4))
            want = tc._oracle_sao(hp, O, j, pix)
            assert np.array_equal(want, restate(j, pix)), it
            measured += tc._same_sao(j, tc._run_sao_on(hp, L, cs, it % 4, j, pix), want, ("8-bit chroma", it))
        assert measured > 100000
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


def _clip(path, w, h, frames, depth, csp, seed):
    from x265_amd.synth import make_clip
    make_clip(path, w, h, frames, seed=seed, csp=csp, depth=10 if depth > 8 else 8)
    if depth == 12:
        # 12 significant bits: the 10-bit clip times four plus two more bits from this test's seed
        a = np.fromfile(path, "<u2").astype(np.uint32)
        rng = np.random.default_rng(seed)
        ((a << 2) | rng.integers(0, 4, a.shape, dtype=np.uint32)).astype("<u2").tofile(path)


BOUND = {
    "main10-420": (10, "i420", []), "main10-422": (10, "i422", []), "main10-444": (10, "i444", []),
    "main10-420-limit-sao": (10, "i420", ["--limit-sao"]), "main10-420-sao-non-deblock": (10, "i420", ["--sao-non-deblock"]),
    "main10-420-ctu32": (10, "i420", ["--ctu", "32"]), "main10-420-slices2": (10, "i420", ["--slices", "2"]),
    "main12-420": (12, "i420", []), "main12-422": (12, "i422", []), "main12-444": (12, "i444", []),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND))
def test_bound_main10_main12_encoders_serve_sao_statistics_byte_identical(tmp_path, name):
    """the product's Main10 / Main12 encoders (oracle/_ref/integration) against the unmodified reference, 328x200 with partial CTUs: the same bytes, every
    plane's statistics measured by the device (X265HIP_VERIFY runs the reference's own body beside each and aborts on a difference)"""
    depth, csp, extra = BOUND[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % depth), os.path.join(REF, "integration", "x265_hip_%dbit" % depth)
    _need(ref, hip)
    yuv = str(tmp_path / "clip.yuv")
    _clip(yuv, 328, 200, 6, depth, csp, 80 + depth)
    args = ["--input", yuv, "--input-res", "328x200", "--input-depth", str(depth), "--input-csp", csp, "--fps", "30", "--frames", "6", "--preset", "medium",
            "--hash", "1", "--pools", "4", "-F", "2"] + extra
    err = _encode_pair(tmp_path, ref, hip, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_SAOSTATS="1"))
    m = re.search(SAO_RE, err)
    assert m and int(m.group(1)) > 100 and int(m.group(3)) == 0, err[-1200:]


@pytest.mark.gpu
def test_1080p_main10_encode_serves_sao_statistics_byte_identical(monkeypatch):
    """the size users run: 1920x1080 Main10 preset medium, 30 frames of 10-bit material, against the unmodified reference"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import encode_fps
    monkeypatch.setenv("X265HIP_SAOSTATS", "1")
    r = encode_fps.measure(frames=30, width=1920, height=1080, bits=10, preset="medium", extra=(), seed=35, input_depth=10)
    if "error" in r and "not built" in r["error"]:
        pytest.skip(r["error"])
    assert "error" not in r, r
    assert r["byte_identical"], r
    m = re.search(SAO_RE, "\n".join(r["gpu"]["served"]))
    assert m and int(m.group(1)) > 1000 and int(m.group(1)) > 10 * int(m.group(3)), r["gpu"]["served"]
