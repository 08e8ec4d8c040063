"""The 35-mode intra scan of Search::checkIntra -> estIntraPredQT (every CU of an I slice, the intra try of RD levels 5-6) as jobs of the CU-job service, and
the scan split over the slot's pair of workgroups (include/x265hip.h X265HIP_INTRAJOB_SPLIT, x265_amd/csrc/cuserve.hip run_intra, x265_amd/host/
x265_hip_intrascan.cpp).

CPU tier (emulated ABI, X265HIP_INTRASCAN_CHECKINTRA=1, X265HIP_INTRASCAN_SYNC_MIN=4): the bound encoder against the unmodified one byte for byte, with
X265HIP_VERIFY comparing every served cost with the sa8d the reference measures; the seam's own counters; the off switch; a lost job; the ABI.
The share of adopted jobs at RD 5-6 is taken over the scans of P and B slices: the first picture of every encode is an I slice, whose scans are served too
(SYNC_MIN=4) and can never be adopted from a job ahead (a CU's neighbours are final only when the CU before it is coded) — the seam's line counts them apart.
GPU tier: split jobs on the MI355X against the restatement (orc_intrajob_run), both ready words, job orders on one slot that a stale units[1] word would
break, the refusal of a split 8x8 scan, and the bound encoder on the device."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
vp, u32 = C.c_void_p, C.c_uint32

LINE = re.compile(r"x265hip: intrascan: Search::checkIntra \((on|off)\): (\d+) scans served by the GPU in (\d+) jobs \((\d+) of the scans in I slices[^)]*\), (\d+) scans on the host; "
                  r"(\d+) jobs left ahead when predInterSearch was entered, (\d+) of them adopted, (\d+) never asked for; (\d+) waits of \d+ cycles on average; (\d+) split jobs")
ENV = {"X265HIP": "require", "X265HIP_VERBOSE": "1", "X265HIP_INTRASCAN_CHECKINTRA": "1", "X265HIP_INTRASCAN_SYNC_MIN": "4", "X265HIP_INTRASCAN_SPLIT": "1"}


def _need(name):
    p = os.path.join(REF, "integration", name) if "_hip" in name else os.path.join(REF, name)
    if not os.path.exists(p):
        pytest.skip("%s not built (needs the reference sources at build time: make -C oracle ref emul; make -C integration hip)" % name)
    return p


def _counts(stderr):
    m = LINE.search(stderr)
    assert m, stderr[-1200:]
    keys = ("served", "jobs", "served_i", "host", "ahead", "adopted", "dropped", "waits", "split")
    d = dict(zip(keys, (int(v) for v in m.groups()[1:])))
    d["on"] = m.group(1) == "on"
    return d


_clips = {}


def _clip_and_reference(tmp_path_factory, bits, frames, seed, extra):
    """the clip and the unmodified encoder's stream, made once per (depth, option set)"""
    key = (bits, frames, seed, tuple(extra))
    if key not in _clips:
        from x265_amd.synth import make_clip
        ref = _need("x265_%dbit" % bits)
        d = tmp_path_factory.mktemp("checkintra")
        yuv = str(d / "clip.yuv")
        make_clip(yuv, 416, 240, frames, seed=seed)
        args = ["--input", yuv, "--input-res", "416x240", "--fps", "30", "--frames", str(frames), "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2"] + list(extra)
        want = str(d / "ref.hevc")
        r = subprocess.run([ref] + args + ["-o", want], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-600:]
        _clips[key] = (args, open(want, "rb").read(), d)
    return _clips[key]


def _bound(binary, args, d, env, tag):
    out = str(d / (tag + ".hevc"))
    r = subprocess.run([binary] + args + ["-o", out], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    return r, (open(out, "rb").read() if os.path.exists(out) else b"")


# (name, options, frames, an RD 5-6 run: jobs leave ahead from predInterSearch)
RUNS = [("keyint1", ["--keyint", "1"], 8, False), ("keyint1-ctu32", ["--keyint", "1", "--ctu", "32"], 8, False),
        ("keyint1-constrained-intra", ["--keyint", "1", "--constrained-intra"], 8, False),
        ("keyint1-no-strong-intra-smoothing", ["--keyint", "1", "--no-strong-intra-smoothing"], 8, False),
        ("rd5", ["--rd", "5"], 10, True), ("slower", ["--preset", "slower"], 6, True), ("rd6-b-intra", ["--rd", "6", "--b-intra"], 8, True),
        ("keyint1-tskip", ["--keyint", "1", "--tskip"], 8, False)]
SEED = 80      # tests/test_cuserve.py's intra scan clip; its P and B slices try intra often enough at RD 5-6 for the adopted share to mean something (asserted below)


@pytest.mark.parametrize("name,extra,frames,rd56", RUNS, ids=[r[0] for r in RUNS])
def test_bound_encoder_check_intra_scans_stay_byte_identical(tmp_path_factory, name, extra, frames, rd56):
    """Search::checkIntra's scan served by jobs, X265HIP_VERIFY=1: the same bytes as the unmodified encoder, more than 20 scans served; at RD 5-6 jobs left
    ahead and at least 90 % of the scans served in P / B slices were adopted from them"""
    emul = _need("x265_emul_8bit")
    args, want, d = _clip_and_reference(tmp_path_factory, 8, frames, SEED, extra)
    r, got = _bound(emul, args, d, dict(ENV, X265HIP_VERIFY="1"), "verify")
    assert r.returncode == 0, r.stderr[-1200:]
    assert got == want
    c = _counts(r.stderr)
    print(name, c)
    assert c["on"] and c["served"] > 20 and c["jobs"] >= c["served"], c
    assert c["split"] == 0, c            # (the emulated ABI reports no feature bit 2: the binding never sets the flag there)
    if rd56:
        inter = c["served"] - c["served_i"]
        assert c["ahead"] > 0 and inter > 20, c
        assert c["adopted"] >= 0.9 * inter, c
    else:
        assert c["ahead"] == 0 and c["served_i"] == c["served"], c


def test_bound_encoder_check_intra_scans_without_verify_and_off(tmp_path_factory):
    """--keyint 1 once more with the slots answering alone (no VERIFY), and switched off: no scan served, the same stream"""
    emul = _need("x265_emul_8bit")
    args, want, d = _clip_and_reference(tmp_path_factory, 8, 8, SEED, ["--keyint", "1"])
    r, got = _bound(emul, args, d, ENV, "plain")
    assert r.returncode == 0 and got == want, r.stderr[-1200:]
    c = _counts(r.stderr)
    assert c["on"] and c["served"] > 20, c
    r, got = _bound(emul, args, d, dict(ENV, X265HIP_INTRASCAN_CHECKINTRA="0", X265HIP_VERIFY="1"), "off")
    assert r.returncode == 0 and got == want, r.stderr[-1200:]
    c = _counts(r.stderr)
    assert not c["on"] and c["served"] == 0 and c["jobs"] == 0 and c["ahead"] == 0, c


def test_bound_encoder_check_intra_scans_main10(tmp_path_factory):
    emul = _need("x265_emul_10bit")
    args, want, d = _clip_and_reference(tmp_path_factory, 10, 8, SEED, ["--keyint", "1"])
    r, got = _bound(emul, args, d, dict(ENV, X265HIP_VERIFY="1"), "verify10")
    assert r.returncode == 0 and got == want, r.stderr[-1200:]
    assert _counts(r.stderr)["served"] > 20


def test_a_lost_check_intra_scan_job_falls_back(tmp_path_factory):
    """the third scan job never comes back: the seam says so once, the rest of the encode runs the reference's code, the bytes are the reference's"""
    emul = _need("x265_emul_8bit")
    args, want, d = _clip_and_reference(tmp_path_factory, 8, 8, SEED, ["--keyint", "1"])
    env = dict(ENV, X265HIP_EMUL_FAIL="intrascan_job:3")
    del env["X265HIP"]
    r, got = _bound(emul, args, d, env, "lost")
    assert r.returncode == 0, r.stderr[-1200:]
    assert got == want
    said = [l for l in r.stderr.splitlines() if "OFF from here on" in l and "x265hip: intrascan:" in l]
    assert len(said) == 1, r.stderr[-1200:]
    c = _counts(r.stderr)
    assert c["served"] == 2 and c["jobs"] == 3, c


def test_library_takes_split_intra_jobs_and_the_abi_agrees():
    """x265hip_cujob_features() bit 2 (needs no device), the flag's value, a job header that has not grown, the ctypes mirror"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    assert L.x265hip_cujob_features() & 4
    hdr = open(os.path.join(ROOT, "include", "x265hip.h")).read()
    assert int(re.search(r"#define X265HIP_INTRAJOB_SPLIT\s+(\d+)u", hdr).group(1)) == 1 == hp.INTRAJOB_SPLIT
    body = re.search(r"typedef struct x265hip_intrajob\s*\{(.*?)\}\s*x265hip_intrajob;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls == ["uint32_t bitDepth", "uint32_t mark", "uint32_t log2Size", "uint32_t flags"]
    assert [f[0] for f in hp.IntraScanJob._fields_] == ["bitDepth", "mark", "log2Size", "flags"] and C.sizeof(hp.IntraScanJob) == 16
    assert hp.IntraScanJob.flags.offset == 12


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def _submit_intra(hp, L, cs, slot, j, pix):
    job, pixels, units, levels, resi = vp(), vp(), vp(), vp(), vp()
    hp.check(L.x265hip_cuserve_slot(cs, slot, C.byref(job), C.byref(pixels), C.byref(units), C.byref(levels), C.byref(resi)))
    C.memmove(pixels, pix.ctypes.data, pix.nbytes)
    seq = u32()
    hp.check(L.x265hip_cuserve_submit_intra(cs, slot, C.byref(j), C.byref(seq)))
    return seq.value, C.cast(units, C.POINTER(hp.CuJobUnit)), levels


def _collect_intra(hp, L, cs, slot, split, seq, un, levels, timeout=20.0):
    """waits (bounded) for the job's ready words — both of a split job — and returns the 35 costs and the device's ticks of each share"""
    t0 = time.time()
    words = (0, 1) if split else (0,)
    while any(un[k].ready != seq or un[k].readyInv != seq for k in words):
        pk = L.x265hip_cuserve_poke(cs, slot)
        if pk < 0:
            hp.check(pk)
        assert time.time() - t0 < timeout, "intra scan job not finished after %.0f s: ready words %s, ticket %#x" % (timeout, [hex(un[k].ready) for k in (0, 1)], seq)
    return np.ctypeslib.as_array(C.cast(levels, C.POINTER(C.c_int32)), (35,)).copy(), [int(un[k].fwdTicks) for k in words]


def _run_intra(hp, L, cs, slot, j, pix):
    seq, un, levels = _submit_intra(hp, L, cs, slot, j, pix)
    return _collect_intra(hp, L, cs, slot, bool(j.flags & hp.INTRAJOB_SPLIT), seq, un, levels)


@pytest.fixture(scope="module")
def split_cases():
    """(job, pixel block, the restatement's 35 costs): log2Size 4 and 5, 8 / 10 / 12 bit, textured and unrelated neighbours; computed once"""
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    O = tc._orc()
    rng = np.random.default_rng(1007)
    cases = []
    for depth in (8, 10, 12):
        for log2n in (4, 5):
            for wild in (False, True):
                j, blob = tc._intra_job(hp, rng, log2n, depth, wild)
                want = tc._oracle_intra(hp, O, j, blob)          # (the restatement ignores the flag: one statement of the 35 costs)
                j.flags = hp.INTRAJOB_SPLIT
                cases.append((j, blob, want))
    return cases


def _open(hp, L, slots, mode):
    hp.check(L.x265hip_init(0))
    cs = vp()
    hp.check(L.x265hip_cuserve_open(slots, mode, C.byref(cs)))
    return cs


def _unsplit(hp, j):
    k = hp.IntraScanJob()
    k.bitDepth, k.mark, k.log2Size, k.flags = j.bitDepth, j.mark, j.log2Size, 0
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_split_intra_jobs_match_the_restatement(mode, split_cases):
    """all 35 costs of a split job equal the restatement's, units[0].ready == units[1].ready == the ticket; the device's own time per size, split and unsplit"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    cs = _open(hp, L, 4, mode)
    ticks = {}
    try:
        for rep in range(4):
            for i, (j, blob, want) in enumerate(split_cases):
                got, tk = _run_intra(hp, L, cs, (i + rep) % 4, j, blob)
                assert np.array_equal(got, want), (mode, i, j.log2Size, j.bitDepth, np.nonzero(got != want)[0][:8], got[:4], want[:4])
                ticks.setdefault((j.log2Size, "split"), []).append(max(tk))
                got, tk = _run_intra(hp, L, cs, (i + rep) % 4, _unsplit(hp, j), blob)
                assert np.array_equal(got, want), (mode, i, "unsplit")
                ticks.setdefault((j.log2Size, "unsplit"), []).append(tk[0])
        print("intra scan jobs, device time (doorbell seen -> costs out; split: the later share), mode %d: " % mode +
              ", ".join("%dx%d %s median %.1f us" % (1 << k[0], 1 << k[0], k[1], sorted(v)[len(v) // 2] / 100.0) for k, v in sorted(ticks.items())))
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_split_intra_jobs_in_orders_that_expose_a_stale_second_word(mode, split_cases):
    """on ONE slot: a split job after a 4:2:0 CU job with chroma (whose units[1] belongs to the CU job), two split jobs back to back, split / unsplit / split;
    then a split job on each of four slots in flight at once"""
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    L = hp.lib()
    O = tc._orc()
    cs = _open(hp, L, 4, mode)
    try:
        rng = np.random.default_rng(77)
        a, b, c = split_cases[2], split_cases[5], split_cases[8]
        for shape in ((5, 5, 4, 1), (4, 4, 4, 1), (6, 5, 5, 1)):
            cj = tc._job_header(hp, *shape, 8, (30, 29, 29), 0, 1)
            cpix = tc._job_pixels(rng, shape[0], 1, 8, 1)
            done, wu, wl, wr = tc._oracle_job(hp, O, cj, cpix)
            tc._compare(hp, cj, tc._run_on(hp, L, cs, 1, cj, cpix), wu, wl, wr, ("cu job before a split scan", shape))
            got, _ = _run_intra(hp, L, cs, 1, a[0], a[1])
            assert np.array_equal(got, a[2]), ("split after a CU job with chroma", shape)
        for (j, blob, want) in (a, b, b, c):                 # back to back
            got, _ = _run_intra(hp, L, cs, 1, j, blob)
            assert np.array_equal(got, want), "back to back"
        for (j, blob, want), split in ((a, True), (b, False), (c, True), (a, False), (b, True)):
            got, _ = _run_intra(hp, L, cs, 1, j if split else _unsplit(hp, j), blob)
            assert np.array_equal(got, want), ("split, unsplit, split", split)
        for rep in range(3):
            flight = [(s, split_cases[(4 * rep + s) % len(split_cases)]) for s in range(4)]
            out = [(s, case, _submit_intra(hp, L, cs, s, case[0], case[1])) for s, case in flight]
            for s, case, (seq, un, levels) in out:
                got, _ = _collect_intra(hp, L, cs, s, True, seq, un, levels)
                assert np.array_equal(got, case[2]), ("four slots in flight", rep, s)
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_device_refuses_a_split_8x8_scan():
    import test_cuserve as tc
    from x265_amd import hipprim as hp
    L = hp.lib()
    cs = _open(hp, L, 2, 0)
    try:
        j, blob = tc._intra_job(hp, np.random.default_rng(3), 3, 8, False)
        j.flags = hp.INTRAJOB_SPLIT
        seq = u32()
        assert L.x265hip_cuserve_submit_intra(cs, 0, C.byref(j), C.byref(seq)) == -1          # X265HIP_EINVAL
        # the service goes on serving
        j.flags = 0
        got, _ = _run_intra(hp, L, cs, 0, j, blob)
        assert np.array_equal(got, tc._oracle_intra(hp, tc._orc(), j, blob))
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,frames", [("keyint1", ["--keyint", "1"], 6), ("rd5", ["--rd", "5"], 8)])
def test_bound_encoder_check_intra_scans_on_the_device(tmp_path_factory, name, extra, frames):
    """oracle/_ref/integration/x265_hip_8bit with X265HIP_VERIFY=1: the unmodified encoder's bytes, scans served, split jobs sent"""
    hip = _need("x265_hip_8bit")
    args, want, d = _clip_and_reference(tmp_path_factory, 8, frames, SEED, extra)
    r, got = _bound(hip, args, d, dict(ENV, X265HIP_VERIFY="1"), "device")
    assert r.returncode == 0, r.stderr[-1200:]
    assert got == want
    c = _counts(r.stderr)
    print(name, c)
    assert c["served"] > 0 and c["split"] > 0, c
