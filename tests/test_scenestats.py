"""The histograms of --hist-scenecut and the edge bits of --rskip 2 (include/x265hip.h: x265hip_scene_stats; x265_amd/csrc/scenestats.h, scenestats.hip; the
Encoder::computeHistograms seam of x265_amd/host/x265_hip_scenecut.cpp and the computeEdge seam of x265_hip_srcplanes.cpp).

What is compared is the reference's own Encoder::computeHistograms (source/encoder/encoder.cpp:1361-1487) on an x265_picture around the test's planes, and its
computeEdge (slicetype.cpp:90-149) into a sentinel-filled plane (tests/support/hist_ref.cpp, built here against oracle/_ref/libx265ref<depth>.so).  Everything
is integer: both edge bins, every histogram bin and every byte of the edge plane are compared for equality, nothing has a tolerance.

The threshold picture.  A pixel's gradients are h = 3 (tr - tl + br - bl) + 10 (mr - ml) and v = 3 (bl - tl + br - tr) + 10 (bm - tm), so
h + v = 6 (br - tl) + 10 (...) is always even and h^2 + v^2 is always even, while T^2 (255^2, 1023^2) is odd: no picture has a pixel with h^2 + v^2 == T^2
exactly, (h, v) = (T, 0) included.  The picture therefore holds the two values closest to the threshold that 3x3 neighbourhoods CAN produce, found by search:
the smallest reachable h^2 + v^2 above T^2 and the largest reachable one below it.  The CPU tier asserts that pixels of both kinds exist (with the sums
computed here in numpy) and that the reference puts them on their sides.

CPU tier: scenestats.h's host path against the reference (builds 8 / 10; 12 for the edge-bit form), the recorded golden file (tests/golden/scenestats.json,
written by tests/golden/make_scenestats_golden.py from the same driver) against the driver, the sums of the histograms, the conditions of the encoder cases
(the options change the reference's bitstream), the emulated-ABI encoder.
GPU tier: the library against the golden file (no reference needed), the bound encoders against the unmodified reference.  Unset, the switch serves
--hist-scenecut in the 8-bit and Main10 builds and leaves the --rskip 2 bits on the host: the tests say X265HIP_SCENESTATS=1 / 0."""
import base64
import ctypes as C
import hashlib
import json
import math
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scenestats.json")

SIZES = ((16, 16), (24, 20), (66, 34), (328, 200))
FULL = SIZES[:2]                                   # the golden file holds these sizes' outputs in full, the others as digests
KINDS = ("noise", "flat", "rails", "ramp", "smooth", "threshold")
CSPS = {"i400": 0, "i420": 1, "i422": 2, "i444": 3}
SHIFTS = {"i400": (0, 0), "i420": (1, 1), "i422": (1, 0), "i444": (0, 0)}          # (horizontal, vertical) chroma shifts
SENTINEL = 0x5A
BITS_PAD = 37                                      # the strided plane of the edge-bit form is this much wider than the picture
SCENE_RE = r"scenestats: (\d+) pictures served, (\d+) kept on the host, (\d+) with samples out of range"
BITS_RE = r"edgebits: (\d+) frames served, (\d+) kept on the host"


def bins_of(build):
    return 256 if build == 8 else 1024


def hist_cases():
    """(build depth, picture depth, csp, width, height, kind) of the computeHistograms form"""
    out = []
    for build in (8, 10):
        for (w, h) in SIZES:
            for kind in KINDS:
                out.append((build, build, "i420", w, h, kind))
        for csp in ("i422", "i444", "i400"):
            for kind in ("noise", "ramp"):
                out.append((build, build, csp, 66, 34, kind))
    for (w, h) in SIZES[2:]:
        out.append((10, 10, "i420", w, h, "dirty"))
        for (build, pic) in ((10, 8), (8, 10), (8, 12), (10, 12)):
            for kind in ("noise", "ramp"):
                out.append((build, pic, "i420", w, h, kind))
    return out


def bits_cases():
    """(build depth, width, height, kind) of the --rskip 2 form"""
    return [(build, w, h, kind) for build in (8, 10, 12) for (w, h) in SIZES for kind in KINDS]


def hist_key(case):
    return "hist/%d/%d/%s/%dx%d/%s" % case


def bits_key(case):
    return "bits/%d/%dx%d/%s" % case


def seed_of(key):
    return int(hashlib.sha256(key.encode()).hexdigest()[:8], 16)


# ---- the threshold picture ---------------------------------------------------------------------------------------------------------------------------

def _patch_for(h, v, pmax):
    """a 3x3 patch (tl tm tr / ml c mr / bl bm br) whose centre has the gradients (h, v), or None"""
    for n in range(h // 10, h // 10 - 8, -1):
        if (h - 10 * n) % 3 or abs(n) > pmax:
            continue
        c = (h - 10 * n) // 3
        for m in range(v // 10, v // 10 - 8, -1):
            if (v - 10 * m) % 3 or abs(m) > pmax:
                continue
            d = (v - 10 * m) // 3
            if (c + d) % 2:
                continue
            p, q = (c + d) // 2, (c - d) // 2                    # br - tl, tr - bl
            if abs(p) > pmax or abs(q) > pmax:
                continue
            tl, br = (0, p) if p >= 0 else (-p, 0)
            bl, tr = (0, q) if q >= 0 else (-q, 0)
            ml, mr = (0, n) if n >= 0 else (-n, 0)
            tm, bm = (0, m) if m >= 0 else (-m, 0)
            return np.array([[tl, tm, tr], [ml, 0, mr], [bl, bm, br]])
    return None


_threshold_memo = {}


def threshold_patches(build):
    """((sum, patch) just above T^2, (sum, patch) just below): the reachable h^2 + v^2 closest to the threshold from both sides"""
    if build in _threshold_memo:
        return _threshold_memo[build]
    pmax, T = (1 << build) - 1, 255 if build == 8 else 1023

    def first(sums):
        for s in sums:
            for h in range(math.isqrt(s), math.isqrt(s // 2) - 1, -1):
                v = math.isqrt(s - h * h)
                if v * v == s - h * h and (h + v) % 2 == 0:
                    patch = _patch_for(h, v, pmax)
                    if patch is not None:
                        return s, patch
        raise AssertionError("no reachable gradient pair near the threshold")

    _threshold_memo[build] = (first(range(T * T, T * T + 4096)), first(range(T * T - 1, T * T - 4096, -1)))
    return _threshold_memo[build]


def sobel_sums(luma):
    """h^2 + v^2 of every interior pixel (int64), restated in numpy"""
    p = luma.astype(np.int64)
    tl, tm, tr = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    ml, mr = p[1:-1, :-2], p[1:-1, 2:]
    bl, bm, br = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    h = 3 * (tr - tl + br - bl) + 10 * (mr - ml)
    v = 3 * (bl - tl + br - tr) + 10 * (bm - tm)
    return h * h + v * v


# ---- pictures ----------------------------------------------------------------------------------------------------------------------------------------

def luma_of(kind, depth, w, h, rng):
    pmax = (1 << depth) - 1
    y, x = np.mgrid[0:h, 0:w]
    if kind in ("noise", "dirty"):
        return rng.integers(0, pmax + 1, (h, w))
    if kind == "flat":
        return np.full((h, w), pmax // 3)
    if kind == "rails":
        return (((x // 4) + (y // 4)) & 1) * pmax                # 0 / pmax: bins 0 and bins - 1, gradients up to 16 * pmax
    if kind == "ramp":
        return (x + y * w) % (pmax + 1)                          # every bin, where the plane has that many samples
    if kind == "smooth":
        return np.clip(pmax * (0.5 + 0.22 * np.sin(x / 9.0) + 0.22 * np.cos(y / 7.0)) + rng.integers(-4, 5, (h, w)), 0, pmax).astype(np.int64)
    assert kind == "threshold"
    (_, above), (_, below) = threshold_patches(depth)
    p = np.zeros((h, w), np.int64)
    for j in range(0, h - 2, 4):
        for i in range(0, w - 2, 4):
            p[j:j + 3, i:i + 3] = above if ((i + j) // 4) & 1 else below
    return p


def planes_of(case):
    """the planes of a computeHistograms case in the picture's sample format, and the number of samples out of range it holds"""
    build, pic, csp, w, h, kind = case
    rng = np.random.default_rng(seed_of(hist_key(case)))
    dt = np.uint8 if pic == 8 else np.uint16
    pmax = (1 << pic) - 1
    out = [luma_of(kind, pic, w, h, rng)]
    if csp != "i400":
        cw, ch = w >> SHIFTS[csp][0], h >> SHIFTS[csp][1]
        for k in (1, 2):
            if kind in ("flat", "threshold"):
                c = np.full((ch, cw), pmax // (k + 1))
            elif kind == "rails":
                y, x = np.mgrid[0:ch, 0:cw]
                c = ((x + y + k) & 1) * pmax
            elif kind == "ramp":
                y, x = np.mgrid[0:ch, 0:cw]
                c = (k * 100 + x + y * cw) % (pmax + 1)
            else:
                c = rng.integers(0, pmax + 1, (ch, cw))
            out.append(c)
    bad = 0
    if kind == "dirty":
        for k, p in enumerate(out):
            for i, v in enumerate((1024, 4095, 65535, 1024 + k)):
                yy, xx = (3 + 5 * i + k) % p.shape[0], (7 + 11 * i) % p.shape[1]
                bad += int(p[yy, xx] < 1024)
                p[yy, xx] = v
    return [np.ascontiguousarray(p.astype(dt)) for p in out], bad


def strided_plane(case):
    """the source plane of an edge-bit case: height rows of width + BITS_PAD samples of the build's pixel type (what lies beside the picture is noise)"""
    build, w, h, kind = case
    rng = np.random.default_rng(seed_of(bits_key(case)))
    buf = rng.integers(0, 1 << build, (h, w + BITS_PAD))
    buf[:, :w] = luma_of(kind, build, w, h, rng)
    return np.ascontiguousarray(buf.astype(np.uint8 if build == 8 else np.uint16))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).astype("<i4").tobytes()).hexdigest()


def pack(a):
    """base64 of the deflated little-endian int32 values (the arrays are small numbers and runs of them: a sixteenth of the raw size)"""
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a).astype("<i4").tobytes(), 9)).decode()


def unpack(s, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), "<i4").reshape(shape)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------

def reference_source():
    mk = open(os.path.join(ROOT, "oracle", "reference.mk")).read()
    return os.path.join(os.environ.get("X265_REFERENCE") or re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1), "source")


_drivers = {}


def build_driver(tmp_dir, depth):
    """tests/support/hist_ref.cpp against oracle/_ref/libx265ref<depth>.so; skips where the reference is not there"""
    if depth in _drivers:
        return _drivers[depth]
    lib, src = os.path.join(REF, "libx265ref%d.so" % depth), reference_source()
    if not (os.path.exists(lib) and os.path.exists(os.path.join(src, "encoder", "encoder.h")) and os.path.exists(os.path.join(REF, "x265_config.h"))):
        pytest.skip("the reference (its sources, oracle/_ref/libx265ref%d.so) is not here" % depth)
    exe = os.path.join(str(tmp_dir), "hist_ref%d" % depth)
    defs = ["-DEXPORT_C_API=1", "-DX265_ARCH_X86=1", "-DX86_64=1", "-DHAVE_INT_TYPES_H=1", "-DHAVE_STRTOK_R=1", "-DENABLE_LIBNUMA=0", "-D__STDC_LIMIT_MACROS=1",
            "-DX265_DEPTH=%d" % depth, "-DHIGH_BIT_DEPTH=%d" % int(depth > 8), "-DX265_NS=x265"]
    subprocess.check_call(["g++", "-O2", "-std=gnu++11", "-w"] + defs + ["-I" + REF, "-I" + src, "-I" + os.path.join(src, "common"), "-I" + os.path.join(src, "encoder"),
                           os.path.join(ROOT, "tests", "support", "hist_ref.cpp"), "-o", exe, lib, "-Wl,-rpath," + REF, "-lpthread", "-ldl"])
    _drivers[depth] = exe
    return exe


def drive_hist(exe, tmp_dir, case, rskip=0):
    build, pic, csp, w, h, kind = case
    planes, bad = planes_of(case)
    fin, fout = os.path.join(str(tmp_dir), "in.raw"), os.path.join(str(tmp_dir), "out.raw")
    with open(fin, "wb") as f:
        for p in planes:
            f.write(p.tobytes())
    r = subprocess.run([exe, "hist", str(w), str(h), str(CSPS[csp]), str(pic), str(rskip), str(int(kind != "dirty")), fin, fout], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    a = np.fromfile(fout, "<i4")
    b = bins_of(build)
    cuts = np.cumsum([1, 2, 2, 3 * b, 3 * b, w * h, w * h])
    assert a.size == cuts[-1]
    errs, ref_edge, edge, ref_hist, hist, ref_plane, plane = np.split(a, cuts[:-1])
    return dict(errs=int(errs[0]), bad=bad, ref_edge=ref_edge, edge=edge, ref_hist=ref_hist.reshape(3, b), hist=hist.reshape(3, b),
                ref_plane=ref_plane.reshape(h, w), plane=plane.reshape(h, w), planes=planes)


def drive_bits(exe, tmp_dir, case):
    build, w, h, kind = case
    src = strided_plane(case)
    fin, fout = os.path.join(str(tmp_dir), "in.raw"), os.path.join(str(tmp_dir), "out.raw")
    src.tofile(fin)
    r = subprocess.run([exe, "bits", str(w), str(h), str(w + BITS_PAD), fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    a = np.fromfile(fout, "<i4").reshape(2, h, w + BITS_PAD)
    return dict(ref=a[0], mine=a[1], src=src)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("scenestats")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


_hist_memo = {}


def hist_results(work, build):
    """the driver's results for every computeHistograms case of a build: computed once, shared by the tests, not modified"""
    if build not in _hist_memo:
        exe = build_driver(work, build)
        _hist_memo[build] = dict((hist_key(c), drive_hist(exe, work, c, rskip=2)) for c in hist_cases() if c[0] == build)
    return _hist_memo[build]


_bits_memo = {}


def bits_results(work, build):
    if build not in _bits_memo:
        exe = build_driver(work, build)
        _bits_memo[build] = dict((bits_key(c), drive_bits(exe, work, c)) for c in bits_cases() if c[0] == build)
    return _bits_memo[build]


def golden_hist_entry(case, got):
    build, pic, csp, w, h, kind = case
    if kind == "dirty":
        return {"range_errors": got["errs"]}
    e = {"range_errors": 0, "edge_hist": [int(v) for v in got["ref_edge"]], "hist_sha": sha(got["ref_hist"]), "plane_sha": sha(got["ref_plane"])}
    if (w, h) in FULL:
        e["hist"], e["plane"] = pack(got["ref_hist"]), pack(got["ref_plane"])
    return e


def golden_bits_entry(case, got):
    e = {"plane_sha": sha(got["ref"])}
    if case[1:3] in FULL:
        e["plane"] = pack(got["ref"])
    return e


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def test_abi_announces_the_optional_entry():
    """the header, the ctypes table and the library agree; the bindings look the symbol up weakly; the emulated library does not have it"""
    from x265_amd import hipprim as hp
    assert len(hp.PROTOTYPES["x265hip_scene_stats"][1]) == 17
    assert hasattr(hp.lib(), "x265hip_scene_stats")
    for tu in ("x265_hip_scenecut.cpp", "x265_hip_srcplanes.cpp"):
        host = open(os.path.join(ROOT, "x265_amd", "host", tu)).read()
        assert re.search(r"x265hip_scene_stats\([^;]*\)\s*__attribute__\(\(weak\)\);", host, flags=re.S), tu
    emul = os.path.join(ROOT, "tests", "support", "libx265hip_emul.so")
    if os.path.exists(emul):
        assert not hasattr(C.CDLL(emul), "x265hip_scene_stats")


@pytest.mark.parametrize("build", (8, 10))
def test_threshold_picture_has_pixels_on_both_sides(work, build):
    """no pixel can sit on T^2 itself (module docstring); the two reachable sums closest to it exist in the picture and the reference's computeHistograms
    puts them on their sides"""
    T = 255 if build == 8 else 1023
    (s_above, _), (s_below, _) = threshold_patches(build)
    print("build %d: T^2 = %d, closest reachable sums %d and %d" % (build, T * T, s_below, s_above))
    assert s_below < T * T < s_above and s_above - T * T <= 64 and T * T - s_below <= 64
    for (w, h) in SIZES:
        got = hist_results(work, build)[hist_key((build, build, "i420", w, h, "threshold"))]
        sums = sobel_sums(got["planes"][0])
        inner = got["ref_plane"][1:-1, 1:-1]
        assert (sums == s_above).any() and (sums == s_below).any()
        assert np.all(inner[sums == s_above] == 1) and np.all(inner[sums == s_below] == 0)
        assert np.array_equal(inner, (sums >= T * T).astype(np.int32))


@pytest.mark.parametrize("build", (8, 10))
def test_host_path_is_the_reference_compute_histograms(work, build):
    res = hist_results(work, build)
    for case in hist_cases():
        if case[0] != build:
            continue
        what, got = hist_key(case), res[hist_key(case)]
        _, pic, csp, w, h, kind = case
        if kind == "dirty":
            assert got["errs"] == got["bad"] > 0, what
            continue
        assert got["errs"] == 0, what
        assert np.array_equal(got["edge"], got["ref_edge"]), what + ": edge bins"
        assert np.array_equal(got["hist"], got["ref_hist"]), what + ": histograms"
        assert np.array_equal(got["plane"], got["ref_plane"]), what + ": edge plane"
        # the sums, and what the function leaves alone
        sizes = [p.size for p in got["planes"]]
        assert int(got["ref_edge"].sum()) == w * h
        for k in range(3):
            if k < len(sizes):
                assert int(got["ref_hist"][k].sum()) == sizes[k], what
            else:
                assert np.all(got["ref_hist"][k] == -7) and np.all(got["hist"][k] == -7), what + ": planes of a 4:0:0 picture are not touched"
        if kind == "flat":
            assert all(int(got["ref_hist"][k].max()) == sizes[k] for k in range(len(sizes))), what
            assert int(got["ref_edge"][1]) == 0
        if kind == "rails" and pic == build:
            assert int(got["ref_hist"][0][0]) + int(got["ref_hist"][0][-1]) == w * h and int(got["ref_hist"][0][-1]) > 0, what
            assert int(got["ref_edge"][1]) > 0
        if kind == "ramp" and pic == build:
            assert int((got["ref_hist"][0] > 0).sum()) == min(bins_of(build), w * h), what


@pytest.mark.parametrize("build", (8, 10, 12))
def test_host_path_is_the_reference_compute_edge(work, build):
    """the --rskip 2 form: the interior equal, the ring and what lies beside the picture keep the sentinel"""
    res = bits_results(work, build)
    for case in bits_cases():
        if case[0] != build:
            continue
        what, got = bits_key(case), res[bits_key(case)]
        _, w, h, kind = case
        assert np.array_equal(got["mine"], got["ref"]), what
        ring = np.ones(got["ref"].shape, bool)
        ring[1:h - 1, 1:w - 1] = False
        assert np.all(got["ref"][ring] == SENTINEL) and np.all(got["ref"][~ring] <= 1), what
        if build < 12 and kind in ("flat", "rails", "ramp", "threshold"):
            # the same pixels (these kinds draw nothing at random) through computeHistograms' packed call
            other = hist_results(work, build)[hist_key((build, build, "i420", w, h, kind))]
            assert np.array_equal(got["ref"][1:h - 1, 1:w - 1], other["ref_plane"][1:-1, 1:-1]), what


@pytest.mark.parametrize("build", (8, 10, 12))
def test_golden_file_is_what_the_driver_gives(work, golden, build):
    """tests/golden/scenestats.json (what the GPU tier compares against) against the reference here"""
    if build < 12:
        res = hist_results(work, build)
        for case in hist_cases():
            if case[0] == build:
                assert golden["cases"][hist_key(case)] == golden_hist_entry(case, res[hist_key(case)]), hist_key(case)
    res = bits_results(work, build)
    for case in bits_cases():
        if case[0] == build:
            assert golden["cases"][bits_key(case)] == golden_bits_entry(case, res[bits_key(case)]), bits_key(case)
    assert len(golden["cases"]) == len(hist_cases()) + len(bits_cases())


# ---- the encoder cases -------------------------------------------------------------------------------------------------------------------------------

ENC = {
    "hist": (8, 8, ["--hist-scenecut"]),
    "hist-rskip2": (8, 8, ["--hist-scenecut", "--rskip", "2"]),
    "rskip2": (8, 8, ["--rskip", "2"]),
    "rskip2-ctu32": (8, 8, ["--rskip", "2", "--ctu", "32"]),
    "main10-hist": (10, 10, ["--hist-scenecut"]),
    "main10-hist-rskip2": (10, 10, ["--hist-scenecut", "--rskip", "2"]),
    "main10-hist-input8": (10, 8, ["--hist-scenecut"]),
    "main10-rskip2": (10, 10, ["--rskip", "2"]),
    "main10-rskip2-ctu32": (10, 10, ["--rskip", "2", "--ctu", "32"]),
}
FRAMES = 12


def joined_clip(path, input_depth):
    """two clips of different seeds, six frames each; the second half's chroma planes are replaced (U by its complement, V by a constant) so that the edge
    histogram and both chroma histograms jump at the join"""
    import test_saostats_formats as sf
    w, h, half = 328, 200, FRAMES // 2
    dt, pmax = (np.uint8, 255) if input_depth == 8 else ("<u2", 1023)
    sf._clip(path + ".a", w, h, half, input_depth, "i420", 101)
    sf._clip(path + ".b", w, h, half, input_depth, "i420", 202)
    a, b = np.fromfile(path + ".a", dt), np.fromfile(path + ".b", dt).copy()
    ysz, csz = w * h, (w // 2) * (h // 2)
    b = b.reshape(half, ysz + 2 * csz)
    b[:, ysz:ysz + csz] = pmax - b[:, ysz:ysz + csz]
    b[:, ysz + csz:] = pmax // 5
    np.concatenate([a, b.reshape(-1)]).astype(dt).tofile(path)
    os.remove(path + ".a")
    os.remove(path + ".b")


def enc_args(yuv, input_depth, extra):
    return ["--input", yuv, "--input-res", "328x200", "--input-depth", str(input_depth), "--fps", "30", "--frames", str(FRAMES), "--preset", "medium", "--hash", "1",
            "--pools", "4", "-F", "2"] + extra


def test_the_options_change_the_reference_bitstream(tmp_path):
    """the condition of the encoder cases: on the joined clip the reference's bytes with --hist-scenecut differ from those without, and --rskip 2 from
    --rskip 1; otherwise a byte-identical bound encoder would show nothing"""
    import test_cuserve_denoise as tcd
    import test_saostats_formats as sf
    ref = os.path.join(REF, "x265_8bit")
    sf._need(ref)
    yuv = str(tmp_path / "clip.yuv")
    joined_clip(yuv, 8)
    plain = tcd._run(ref, enc_args(yuv, 8, []), str(tmp_path / "plain.hevc"))[1]
    assert tcd._run(ref, enc_args(yuv, 8, ["--hist-scenecut"]), str(tmp_path / "hist.hevc"))[1] != plain, "--hist-scenecut does not change this encode"
    rskip1 = tcd._run(ref, enc_args(yuv, 8, ["--rskip", "1"]), str(tmp_path / "r1.hevc"))[1]
    assert tcd._run(ref, enc_args(yuv, 8, ["--rskip", "2"]), str(tmp_path / "r2.hevc"))[1] != rskip1, "--rskip 2 does not change this encode"


def test_emulated_encoder_keeps_every_frame_on_the_host(tmp_path):
    """the emulated ABI has no x265hip_scene_stats: a --rskip 2 encode through the bound emulated encoder, asked for the pass, is byte-identical and reports
    every frame's edge bits kept on the host (the emulated encoders link the reference's own encoder.o: they have no computeHistograms seam)"""
    import test_saostats_formats as sf
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    sf._need(ref, emul)
    yuv = str(tmp_path / "clip.yuv")
    joined_clip(yuv, 8)
    err = sf._encode_pair(tmp_path, ref, emul, enc_args(yuv, 8, ["--rskip", "2"]), dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_SCENESTATS="1"))
    m = re.search(BITS_RE, err)
    assert "OFF" not in err and "VERIFY FAILED" not in err and m, err[-1200:]
    assert int(m.group(1)) == 0 and int(m.group(2)) == FRAMES, m.groups()


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def run_library(hp, L, build, planes, conv, want_hist=True, want_bits=True, out_stride=None, width=None):
    """x265hip_scene_stats on host planes (plane 0 `width` wide inside its rows when given): (return code, range errors, edge bins, histograms [3][bins]
    prefilled with -7, edge plane prefilled with the sentinel)"""
    n = len(planes)
    h, w = planes[0].shape[0], width or planes[0].shape[1]
    widths = (C.c_int * 3)(*([w] + [p.shape[1] for p in planes[1:]] + [0] * (3 - n)))
    heights = (C.c_int * 3)(*([p.shape[0] for p in planes] + [0] * (3 - n)))
    st = (C.c_int64 * 3)(*([p.shape[1] for p in planes] + [0] * (3 - n)))
    ptrs = (C.c_void_p * 3)(*([p.ctypes.data for p in planes] + [None] * (3 - n)))
    out_stride = out_stride or w
    pix = np.uint8 if build == 8 else np.uint16
    bits = np.full((h, out_stride), SENTINEL, pix)
    edge = np.full(2, -7, np.int32)
    hist = np.full((3, bins_of(build)), -7, np.int32)
    errs = C.c_uint32(0xFFFFFFFF)
    rc = L.x265hip_scene_stats(build, n, ptrs, widths, heights, st, planes[0].itemsize, conv[0], conv[1], conv[2], int(want_hist),
                               bits.ctypes.data if want_bits else None, out_stride, edge.ctypes.data, hist.ctypes.data if want_hist else None, C.byref(errs), None)
    return rc, errs.value, edge, hist, bits


def conversion_of(build, pic):
    mask = (1 << build) - 1
    if pic == build:
        return (0, 0, mask)
    if pic == 8:
        return (1, build - 8, mask)
    return (2, pic - build, mask) if pic > build else (3, build - pic, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("build", (8, 10))
def test_library_statistics_match_the_recorded_reference(golden, build):
    """every computeHistograms case against the golden file: the edge bins, every histogram bin, the edge plane with its zero ring (the caller's zeros: the
    call writes the interior only); again without the bits; the range-error count of the dirty picture"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    for case in hist_cases():
        if case[0] != build:
            continue
        _, pic, csp, w, h, kind = case
        what, g = hist_key(case), golden["cases"][hist_key(case)]
        planes, bad = planes_of(case)
        rc, errs, edge, hist, bits = run_library(hp, L, build, planes, conversion_of(build, pic))
        hp.check(rc)
        assert errs == g["range_errors"], what
        if kind == "dirty":
            assert errs == bad > 0
            continue
        bits[0, :] = 0; bits[-1, :] = 0; bits[:, 0] = 0; bits[:, -1] = 0                   # the ring as computeHistograms' memset leaves it
        assert np.all(bits[1:-1, 1:-1] <= 1), what
        assert [int(v) for v in edge] == g["edge_hist"], what + ": edge bins"
        assert sha(hist) == g["hist_sha"], what + ": histograms"
        assert sha(bits) == g["plane_sha"], what + ": edge plane"
        if (w, h) in FULL:
            assert np.array_equal(hist, unpack(g["hist"], hist.shape)) and np.array_equal(bits, unpack(g["plane"], bits.shape)), what
        rc, errs2, edge2, hist2, bits2 = run_library(hp, L, build, planes, conversion_of(build, pic), want_bits=False)
        hp.check(rc)
        assert errs2 == 0 and np.array_equal(edge2, edge) and np.array_equal(hist2, hist) and np.all(bits2 == SENTINEL), what + ": without the bits"


@pytest.mark.gpu
@pytest.mark.parametrize("build", (8, 10, 12))
def test_library_edge_bits_of_a_strided_picture(golden, build):
    """the --rskip 2 form (one strided plane, no histograms) against the golden file: an output pitch larger than the width, the ring and the bytes between
    the rows keep what they held; the histogram output is not touched"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    for case in bits_cases():
        if case[0] != build:
            continue
        _, w, h, kind = case
        what, g = bits_key(case), golden["cases"][bits_key(case)]
        src = strided_plane(case)
        rc, errs, edge, hist, bits = run_library(hp, L, build, [src], (0, 0, (1 << build) - 1), want_hist=False, out_stride=w + BITS_PAD, width=w)
        hp.check(rc)
        assert errs == 0 and np.all(hist == -7), what
        assert sha(bits) == g["plane_sha"], what
        if (w, h) in FULL:
            assert np.array_equal(bits, unpack(g["plane"], bits.shape)), what
        assert int(edge[1]) == int((bits[1:h - 1, 1:w - 1] == 1).sum()) and int(edge[0]) + int(edge[1]) == w * h, what


@pytest.mark.gpu
def test_library_refuses_what_it_cannot_serve():
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    p = [np.zeros((16, 16), np.uint16)]
    assert run_library(hp, L, 12, p, (0, 0, 4095))[0] == -1                              # the Main12 build's histograms: 4096 values, 1024 bins
    assert run_library(hp, L, 10, p, (0, 0, 1023), want_hist=False, want_bits=False)[0] == -1
    assert run_library(hp, L, 8, p, (0, 0, 255))[0] == -1                                # unconverted 2-byte samples in the 8-bit build


def _bound(tmp_path, name):
    import test_saostats_formats as sf
    build, input_depth, extra = ENC[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % build), os.path.join(REF, "integration", "x265_hip_%dbit" % build)
    sf._need(ref, hip)
    yuv = str(tmp_path / "clip.yuv")
    joined_clip(yuv, input_depth)
    return ref, hip, enc_args(yuv, input_depth, extra), (SCENE_RE if "--hist-scenecut" in extra else BITS_RE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ENC))
def test_bound_encoders_serve_scene_statistics_byte_identical(tmp_path, name):
    """the product's encoders against the unmodified reference, 12 frames with a scene change in the middle, two frame threads: the same bytes under
    X265HIP_VERIFY (the reference's body runs beside every served picture; any difference aborts) and again without it; pictures served"""
    import test_cuserve_denoise as tcd
    ref, hip, base, line = _bound(tmp_path, name)
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    for verify in (True, False):
        env = dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_SCENESTATS="1")
        if verify:
            env["X265HIP_VERIFY"] = "1"
        err, got = tcd._run(hip, base, str(tmp_path / "hip.hevc"), env)
        assert got == want, "bitstreams differ (X265HIP_VERIFY %s)" % ("set" if verify else "not set")
        assert "VERIFY FAILED" not in err and "OFF" not in err, err[-1500:]
        m = re.search(line, err)
        assert m, err[-1500:]
        print("%s (verify %d): %s" % (name, verify, m.group(0)))
        assert int(m.group(1)) > 0 and int(m.group(1)) + int(m.group(2)) == FRAMES, m.groups()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ENC))
def test_switch_off_keeps_every_picture_on_the_host(tmp_path, name):
    import test_cuserve_denoise as tcd
    ref, hip, base, line = _bound(tmp_path, name)
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    err, got = tcd._run(hip, base, str(tmp_path / "off.hevc"), dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_SCENESTATS="0"))
    m = re.search(line, err)
    assert got == want and m and int(m.group(1)) == 0 and int(m.group(2)) == FRAMES, err[-1200:]
