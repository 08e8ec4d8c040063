"""The edge and angle planes of --aq-mode 4 (include/x265hip.h: x265hip_edge_planes; x265_amd/csrc/edgepass.h, edgepass.hip; the edgeFilter seam of
x265_amd/host/x265_hip_srcplanes.cpp).

What is compared is the reference's own edgeFilter (source/encoder/slicetype.cpp:151-215) on a Frame around the test's planes (tests/support/edge_ref.cpp,
built here against oracle/_ref/libx265ref<depth>.so): the edge plane in every sample of the buffer, the ring of source samples and the zeros of the memset
included; the angle plane in every sample outside the doubt list; the listed angles after resolution through the reference's computeEdge on the 3x3 patch.
Nothing has a tolerance.  The doubt list is capped at 0.5 % of a noise picture (the band of 2^-10 degrees around the 179 whole degrees that noise gradients
spread over gives 2 * 2^-10 = 0.2 %): a cap against a pass that lists everything, not a tolerance.

CPU tier: edgepass.h's host path against the reference (depths 8 / 10 / 12, eight kinds of picture, four sizes, margins that differ from the picture so that
the `!=` rows and columns of the Gaussian read them); the nine specials at every gradient magnitude 3x3 patches can produce; the recorded golden file
(tests/golden/edgeplanes.json, written by tests/golden/make_edgeplanes_golden.py from the same driver) against the driver; the emulated-ABI encoder.
GPU tier: the library against the golden file (no reference needed), the list's overflow, the output pitch; the bound encoders against the unmodified
reference.  The pass is on by default in the 8-bit build only: the tests say X265HIP_EDGEPLANES=1 / 0."""
import base64
import ctypes as C
import hashlib
import json
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "edgeplanes.json")

DEPTHS = (8, 10, 12)
SIZES = ((16, 16), (24, 20), (66, 34), (328, 200))
FULL = SIZES[:2]                                   # the golden file holds these sizes' planes in full
KINDS = ("noise", "flat", "checker", "stripes", "ramp45", "ramp135", "smooth", "noise-rail-margins")
MX, MY, CTU = 40, 24, 64
DOUBT_CAP = 0.005
EDGE_RE = r"edgeplanes: (\d+) frames served, (\d+) kept on the host, (\d+) doubtful pixels resolved"


def seed_of(kind, depth, w, h):
    return 1000 * KINDS.index(kind) + 100 * DEPTHS.index(depth) + 10 * [s[0] for s in SIZES].index(w) + 7


def geometry(w, h):
    """(rows, stride) of the buffers: Frame::create's stride * (maxHeight + 2 * marginY)"""
    return (h + CTU - 1) // CTU * CTU + 2 * MY, w + 2 * MX


def picture(kind, depth, w, h):
    """the source buffer with its margins (rows x stride; the picture's sample (0, 0) at [MY, MX])"""
    rng = np.random.default_rng(seed_of(kind, depth, w, h))
    pmax = (1 << depth) - 1
    rows, stride = geometry(w, h)
    y, x = np.mgrid[0:h, 0:w]
    if kind in ("noise", "noise-rail-margins"):
        p = rng.integers(0, pmax + 1, (h, w))
    elif kind == "flat":
        p = np.full((h, w), pmax // 3)
    elif kind == "checker":
        p = (((x // 4) + (y // 4)) & 1) * pmax                   # 0 / pmax: the largest gradients, |h|, |v| up to 16 * pmax
    elif kind == "stripes":
        p = ((x // 3) & 1) * pmax
    elif kind == "ramp45":
        p = ((x + y) * 3) % (pmax + 1)                           # |h| == |v| wherever the ramp does not wrap
    elif kind == "ramp135":
        p = ((x - y) * 3) % (pmax + 1)
    else:
        p = np.clip(pmax * (0.5 + 0.22 * np.sin(x / 9.0) + 0.22 * np.cos(y / 7.0)) + rng.integers(-4, 5, (h, w)), 0, pmax)
    if kind == "noise-rail-margins":
        buf = np.where((np.add.outer(np.arange(rows), np.arange(stride)) & 1) == 1, pmax, 0)
    else:
        buf = rng.integers(0, pmax + 1, (rows, stride))
    buf[MY:MY + h, MX:MX + w] = p
    return np.ascontiguousarray(buf.astype(np.uint8 if depth == 8 else np.uint16))


def region(buf, w, h):
    return np.ascontiguousarray(buf[MY:MY + h, MX:MX + w])


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype("<u2").tobytes() if a.dtype != np.uint8 else a.tobytes()).hexdigest()


def masked(plane, doubts):
    """the plane with the listed pixels zeroed"""
    out = plane.copy()
    for d in doubts:
        out[d >> 16, d & 0xffff] = 0
    return out


def reference_source():
    mk = open(os.path.join(ROOT, "oracle", "reference.mk")).read()
    return os.path.join(os.environ.get("X265_REFERENCE") or re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1), "source")


_drivers = {}


def build_driver(tmp_dir, depth):
    """tests/support/edge_ref.cpp against oracle/_ref/libx265ref<depth>.so; skips where the reference is not there"""
    if depth in _drivers:
        return _drivers[depth]
    lib, src = os.path.join(REF, "libx265ref%d.so" % depth), reference_source()
    if not (os.path.exists(lib) and os.path.exists(os.path.join(src, "encoder", "slicetype.h")) and os.path.exists(os.path.join(REF, "x265_config.h"))):
        pytest.skip("the reference (its sources, oracle/_ref/libx265ref%d.so) is not here" % depth)
    exe = os.path.join(str(tmp_dir), "edge_ref%d" % depth)
    defs = ["-DEXPORT_C_API=1", "-DX265_ARCH_X86=1", "-DX86_64=1", "-DHAVE_INT_TYPES_H=1", "-DHAVE_STRTOK_R=1", "-DENABLE_LIBNUMA=0", "-D__STDC_LIMIT_MACROS=1",
            "-DX265_DEPTH=%d" % depth, "-DHIGH_BIT_DEPTH=%d" % int(depth > 8), "-DX265_NS=x265"]
    subprocess.check_call(["g++", "-O2", "-std=gnu++11", "-w"] + defs + ["-I" + REF, "-I" + src, "-I" + os.path.join(src, "common"), "-I" + os.path.join(src, "encoder"),
                           os.path.join(ROOT, "tests", "support", "edge_ref.cpp"), "-o", exe, lib, "-Wl,-rpath," + REF, "-lpthread", "-ldl"])
    _drivers[depth] = exe
    return exe


def drive(exe, tmp_dir, depth, w, h, buf):
    """the driver on one picture: dict of the five buffers, the doubt list and the specials"""
    fin, fout = os.path.join(str(tmp_dir), "in.raw"), os.path.join(str(tmp_dir), "out.raw")
    buf.tofile(fin)
    r = subprocess.run([exe, "planes", str(w), str(h), str(MX), str(MY), str(CTU), fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    raw = open(fout, "rb").read()
    n = buf.size * buf.itemsize
    planes = [np.frombuffer(raw[i * n:(i + 1) * n], buf.dtype).reshape(buf.shape) for i in range(5)]
    nd = int(np.frombuffer(raw[5 * n:5 * n + 4], "<u4")[0])
    doubts = np.frombuffer(raw[5 * n + 4:5 * n + 4 + 4 * nd], "<u4").tolist()
    return dict(ref_edge=planes[0], ref_theta=planes[1], edge=planes[2], theta=planes[3], resolved=planes[4], doubts=doubts,
                specials=[int(v) for v in r.stdout.split()])


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("edgeplanes")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def case_key(depth, kind, w, h):
    return "%d/%s/%dx%d" % (depth, kind, w, h)


def assert_doubt_cap(counts):
    """counts: {case: (listed pixels, pixels)}.  The share of the noise pictures is at most 0.5 %: taken over all noise pictures of the run together, and for
    each noise picture on which 0.5 % is at least ten pixels (on 16x16 one pixel is 0.39 %: two listed pixels there are a count, not a share)"""
    noise = dict((k, v) for k, v in counts.items() if "/noise" in k)
    assert noise
    listed, pixels = sum(v[0] for v in noise.values()), sum(v[1] for v in noise.values())
    print("noise pictures together: %d of %d pixels listed (%.4f)" % (listed, pixels, listed / float(pixels)))
    assert listed <= DOUBT_CAP * pixels, (listed, pixels)
    for k, (n, px) in noise.items():
        if DOUBT_CAP * px >= 10:
            assert n <= DOUBT_CAP * px, (k, n, px)


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def test_abi_announces_the_optional_entry():
    """the header, the ctypes table and the library agree; the binding looks the symbol up weakly; the emulated library does not have it"""
    from x265_amd import hipprim as hp
    hdr = open(os.path.join(ROOT, "include", "x265hip.h")).read()
    assert int(re.search(r"#define X265HIP_EDGE_SPECIALS\s+(\d+)", hdr).group(1)) == 9
    assert len(hp.PROTOTYPES["x265hip_edge_planes"][1]) == 13
    assert hasattr(hp.lib(), "x265hip_edge_planes")
    host = open(os.path.join(ROOT, "x265_amd", "host", "x265_hip_srcplanes.cpp")).read()
    assert re.search(r"x265hip_edge_planes\([^;]*\)\s*__attribute__\(\(weak\)\);", host, flags=re.S)
    emul = os.path.join(ROOT, "tests", "support", "libx265hip_emul.so")
    if os.path.exists(emul):
        assert not hasattr(C.CDLL(emul), "x265hip_edge_planes")


@pytest.mark.parametrize("depth", DEPTHS)
def test_host_path_is_the_reference_edge_filter(work, depth):
    exe = build_driver(work, depth)
    shares, wh = {}, {}
    for (w, h) in SIZES:
        for kind in KINDS:
            wh[case_key(depth, kind, w, h)] = w * h
            got = drive(exe, work, depth, w, h, picture(kind, depth, w, h))
            what = case_key(depth, kind, w, h)
            assert np.array_equal(got["edge"], got["ref_edge"]), what + ": edge plane"
            rows, stride = geometry(w, h)
            listed = np.zeros((rows, stride), bool)
            for d in got["doubts"]:
                listed[MY + (d >> 16), MX + (d & 0xffff)] = True
            assert np.array_equal(got["theta"][~listed], got["ref_theta"][~listed]), what + ": angle outside the doubt list"
            assert np.array_equal(got["resolved"], got["ref_theta"]), what + ": listed angles after resolution"
            shares[what] = len(got["doubts"]) / float(w * h)
    print("doubt shares, depth %d: %s" % (depth, ", ".join("%s %.4f" % (k, v) for k, v in sorted(shares.items()))))
    assert_doubt_cap(dict((k, (int(round(v * wh[k])), wh[k])) for k, v in shares.items()))


@pytest.mark.parametrize("depth", DEPTHS)
def test_specials_do_not_depend_on_the_magnitude(work, depth):
    exe = build_driver(work, depth)
    r = subprocess.run([exe, "specials"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    rows = [[int(v) for v in l.split()] for l in r.stdout.splitlines()]
    assert [row[0] for row in rows] == list(range(9))
    made = drive(exe, work, depth, 16, 16, picture("flat", depth, 16, 16))["specials"]
    pmax = (1 << depth) - 1
    for idx, lo, hi, tried in rows:
        assert lo == hi == made[idx], (idx, lo, hi, made[idx])
        # an axis gradient with the other one 0 is even (6 a + 10 b <= 16 pmax), a diagonal one is 3 a + 10 b <= 13 pmax: all of them but the few
        # smallest and largest that a, b in 0..pmax do not reach
        assert tried >= (3 if idx == 4 else (8 * pmax - 16 if idx in (1, 3, 5, 7) else 13 * pmax - 32)), (idx, tried)
    assert made == [45, 90, 135, 180, 0, 0, 135, 90, 45], made


@pytest.mark.parametrize("depth", DEPTHS)
def test_golden_file_is_what_the_driver_gives(work, golden, depth):
    """tests/golden/edgeplanes.json (what the GPU tier compares against) against the reference here"""
    exe = build_driver(work, depth)
    for (w, h) in SIZES:
        for kind in KINDS:
            g = golden["cases"][case_key(depth, kind, w, h)]
            got = drive(exe, work, depth, w, h, picture(kind, depth, w, h))
            assert got["specials"] == golden["specials"][str(depth)]
            assert g["seed"] == seed_of(kind, depth, w, h)
            assert g["edge_sha"] == sha(region(got["ref_edge"], w, h)) and g["theta_sha"] == sha(region(got["ref_theta"], w, h))
            assert sorted(g["doubts"]) == sorted(got["doubts"])
            assert g["theta_masked_sha"] == sha(masked(region(got["ref_theta"], w, h), g["doubts"]))
            if (w, h) in FULL:
                assert np.array_equal(unpack(g["edge"], depth, w, h), region(got["ref_edge"], w, h))
                assert np.array_equal(unpack(g["theta"], depth, w, h), region(got["ref_theta"], w, h))


def pack(a):
    return base64.b64encode(np.ascontiguousarray(a).astype("<u2").tobytes()).decode()


def unpack(s, depth, w, h):
    return np.frombuffer(base64.b64decode(s), "<u2").reshape(h, w).astype(np.uint8 if depth == 8 else np.uint16)


def test_emulated_encoder_keeps_every_frame_on_the_host(tmp_path):
    """the emulated ABI has no x265hip_edge_planes: an --aq-mode 4 encode through the bound emulated encoder, asked for the pass, is byte-identical and
    reports every frame kept on the host"""
    import test_saostats_formats as sf
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    sf._need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=101)
    args = ["--input", yuv, "--input-res", "328x200", "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2", "--aq-mode", "4"]
    err = sf._encode_pair(tmp_path, ref, emul, args, dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_EDGEPLANES="1"))
    m = re.search(EDGE_RE, err)
    assert "OFF" not in err and "VERIFY FAILED" not in err and m, err[-1200:]
    assert int(m.group(1)) == 0 and int(m.group(2)) == 6 and int(m.group(3)) == 0, m.groups()
    with_option = open(str(tmp_path / "ref.hevc"), "rb").read()
    r = subprocess.run([ref] + args[:-2] + ["-o", str(tmp_path / "ref_plain.hevc")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and open(str(tmp_path / "ref_plain.hevc"), "rb").read() != with_option, "--aq-mode 4 does not change this encode: the case shows nothing"


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def run_library(hp, L, depth, w, h, buf, specials, cap=None, out_stride=None, fill=0xA5):
    """x265hip_edge_planes on the picture inside `buf`: (edge, theta) as out_stride-wide arrays, the list array (cap + 64 entries, sentinel-filled), the count"""
    out_stride = out_stride or w
    cap = w * h if cap is None else cap
    dt = buf.dtype
    edge = np.full((h, out_stride), fill, dt)
    theta = np.full((h, out_stride), fill, dt)
    lst = np.full(cap + 64, 0xFFFFFFFF, np.uint32)
    count = C.c_int(-1)
    sp = np.asarray(specials, np.uint16)
    stride = buf.shape[1]
    org = buf.ctypes.data + (MY * stride + MX) * buf.itemsize
    hp.check(L.x265hip_edge_planes(depth, org, stride, w, h, sp.ctypes.data, edge.ctypes.data, theta.ctypes.data, out_stride, lst.ctypes.data, cap, C.byref(count), None))
    return edge, theta, lst, count.value


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_library_planes_match_the_recorded_reference(golden, depth):
    """every picture and size against the golden file: the edge plane identical; angles identical outside the returned list; the list within the cap.  The
    larger sizes are held as digests: the angle digest is taken with the recorded (host) doubt list zeroed, and the returned list may differ from the
    recorded one only where two double-precision atan2 implementations disagree about a value sitting on the band's edge (at most 2 pixels a picture)."""
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    specials = golden["specials"][str(depth)]
    counts = {}
    for (w, h) in SIZES:
        for kind in KINDS:
            what = case_key(depth, kind, w, h)
            g = golden["cases"][what]
            edge, theta, lst, n = run_library(hp, L, depth, w, h, picture(kind, depth, w, h), specials)
            assert 0 <= n <= w * h and np.all(lst[n:] == 0xFFFFFFFF), what
            mine = sorted(int(v) for v in lst[:n])
            assert len(set(mine)) == n and all((d & 0xffff) < w and (d >> 16) < h for d in mine), what
            assert sha(edge) == g["edge_sha"], what + ": edge plane"
            odd = set(mine) ^ set(g["doubts"])
            print("%s: %d doubtful pixels (%.4f), %d not in the recorded list or missing from it" % (what, n, n / float(w * h), len(odd)))
            assert len(odd) <= 2, (what, sorted(odd))
            if (w, h) in FULL:
                want_e, want_t = unpack(g["edge"], depth, w, h), unpack(g["theta"], depth, w, h)
                assert np.array_equal(edge, want_e), what
                keep = np.ones((h, w), bool)
                for d in mine:
                    keep[d >> 16, d & 0xffff] = False
                assert np.array_equal(theta[keep], want_t[keep]), what + ": angle outside the returned list"
            else:
                # (a band-edge pixel is listed on one side only and holds (int)degrees on both: the digest with every recorded pixel zeroed still has to hold)
                assert sha(masked(theta, g["doubts"])) == g["theta_masked_sha"], what + ": angle plane outside the recorded list"
            counts[what] = (n, w * h)
    assert_doubt_cap(counts)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", (8, 10))
def test_library_list_overflow_and_output_pitch(golden, depth):
    """a doubtCap of 4 on a noise picture reports more than 4 and writes nothing past the fourth entry, the planes are the ones of a complete list; with
    outStride > width what lies between the rows keeps its bytes"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    w, h = SIZES[3]
    specials = golden["specials"][str(depth)]
    buf = picture("noise", depth, w, h)
    g = golden["cases"][case_key(depth, "noise", w, h)]
    edge0, theta0, lst0, n0 = run_library(hp, L, depth, w, h, buf, specials)
    edge, theta, lst, n = run_library(hp, L, depth, w, h, buf, specials, cap=4)
    assert n == n0 > 4 and np.all(lst[4:] == 0xFFFFFFFF), (n, n0)
    assert set(int(v) for v in lst[:4]) <= set(int(v) for v in lst0[:n0])
    assert np.array_equal(edge, edge0) and np.array_equal(theta, theta0)
    edge, theta, lst, n = run_library(hp, L, depth, w, h, buf, specials, out_stride=w + 37, fill=0x5A)
    assert n == n0 and np.array_equal(edge[:, :w], edge0) and np.array_equal(theta[:, :w], theta0)
    assert np.all(edge[:, w:] == 0x5A) and np.all(theta[:, w:] == 0x5A)
    assert sha(edge0) == g["edge_sha"]


BOUND = {
    "alone": (328, 200, []),
    "rskip2": (328, 200, ["--rskip", "2"]),
    "qg8": (328, 200, ["--qg-size", "8"]),
    "ctu32": (328, 200, ["--ctu", "32"]),
    "aligned-320x192": (320, 192, []),            # a multiple of 16: copyFromPicture pads one column only, column width + 1 is what the buffer held before
}


def _bound(tmp_path, depth, name, frames=10):
    import test_saostats_formats as sf
    w, h, extra = BOUND[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % depth), os.path.join(REF, "integration", "x265_hip_%dbit" % depth)
    sf._need(ref, hip)
    yuv = str(tmp_path / "clip.yuv")
    sf._clip(yuv, w, h, frames, depth, "i420", 101)
    base = ["--input", yuv, "--input-res", "%dx%d" % (w, h), "--input-depth", str(depth), "--fps", "30", "--frames", str(frames), "--preset", "medium",
            "--hash", "1", "--pools", "4", "-F", "2", "--aq-mode", "4"] + extra
    return ref, hip, base


@pytest.mark.gpu
@pytest.mark.parametrize("depth", (8, 10))
@pytest.mark.parametrize("name", sorted(BOUND))
def test_bound_encoders_serve_edge_planes_byte_identical(tmp_path, name, depth):
    """the product's encoders with --aq-mode 4 against the unmodified reference, 10 frames, two frame threads: the same bytes under X265HIP_VERIFY (the
    reference's edgeFilter runs beside every served frame; a difference anywhere in the two buffers aborts) and again without it; frames served"""
    import test_cuserve_denoise as tcd
    ref, hip, base = _bound(tmp_path, depth, name)
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    for verify in (True, False):
        env = dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_EDGEPLANES="1")
        if verify:
            env["X265HIP_VERIFY"] = "1"
        err, got = tcd._run(hip, base, str(tmp_path / "hip.hevc"), env)
        assert got == want, "bitstreams differ (X265HIP_VERIFY %s)" % ("set" if verify else "not set")
        assert "VERIFY FAILED" not in err and "OFF" not in err, err[-1500:]
        m = re.search(EDGE_RE, err)
        assert m, err[-1500:]
        print("%s, %d bit (verify %d): %s frames served, %s kept on the host, %s doubtful pixels resolved" % ((name, depth, verify) + m.groups()))
        assert int(m.group(1)) > 0 and int(m.group(1)) + int(m.group(2)) == 10, m.groups()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", (8, 10))
def test_switch_off_keeps_every_frame_on_the_host(tmp_path, depth):
    import test_cuserve_denoise as tcd
    ref, hip, base = _bound(tmp_path, depth, "alone")
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    err, got = tcd._run(hip, base, str(tmp_path / "off.hevc"), dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_EDGEPLANES="0"))
    m = re.search(EDGE_RE, err)
    assert got == want and m and int(m.group(1)) == 0 and int(m.group(2)) == 10, err[-1200:]
