"""The frame encoder's weighted-prediction analysis on the GPU (x265hip_wpcost_*, x265_amd/csrc/wpcost.hip; the arithmetic in x265_amd/csrc/wpcost.h; the seam in
x265_amd/host/x265_hip_weightp.cpp).

CPU tier (skips where oracle/_ref is absent): tests/support/wpcost_ref.cpp runs the reference's real weightAnalyse (source/encoder/weightPrediction.cpp) on a
Frame / Slice / two Lowres around the planes made here, with the table slots the function calls wrapped, and logs every evaluation it makes: plane, list,
weight, offset, denominator, the value of every block, the total, and the slice's final weights.  wpcost.h on the host must reproduce every logged block and
total.  Witnesses are asserted from the reference's own log: each branch of the compensation, each side of the clip, the weights' clips, the offset loop ending
both ways, the lists, the chroma formats, the depths.  Everything is integer: every value is compared for equality, nothing has a tolerance.

GPU tier: the library against tests/golden/wpcost.json (no reference needed), guard cells, two contexts on two threads, refusals, the bound encoders on fade
clips against the unmodified reference.  Unset, the switch serves the 8-bit and Main10 builds: the tests say X265HIP_WEIGHTP=1 / 0, and one test
pins the default."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wpcost.json")

DEPTHS = (8, 10, 12)
MARGIN_X, MARGIN_Y = 32, 24                          # lowres margins of the cases; the pictures' are twice that, the chroma's shifted
CSPS = {"i400": 0, "i420": 1, "i422": 2, "i444": 3}
SHIFTS = {"i400": (0, 0), "i420": (1, 1), "i422": (1, 0), "i444": (0, 0)}          # (horizontal, vertical) chroma shifts
WPCOST_RE = (r"weightp: (\d+) analyses served, (\d+) evaluations, (\d+) launches, ([\d.]+) ms on the device, (\d+) took the early exit, "
             r"(\d+) left to the host")

def _case(w, h, csp, scale64, offset8=0, mv="mixed", is_b=0, bframes=3, poc=4, lists=((0, 1),), gain=1.0, bias=0.0, chroma_same=False):
    """picture width, height, chroma format; the reference's brightness = the frame's * scale64 / 64 + offset8 (8-bit units); the kind of the vectors; the slice;
    per list (reference poc, vectors searched); gain / bias (of the range): the frame is the texture * gain + bias, saturated at the rails; chroma_same: the
    reference's chroma is the frame's"""
    return dict(w=w, h=h, csp=csp, scale64=scale64, offset8=offset8, mv=mv, is_b=is_b, bframes=bframes, poc=poc, lists=lists, gain=gain, bias=bias,
                chroma_same=chroma_same)


#   208x128: a 104x64 lowres, 13 block columns.  mcChroma compensates only blocks whose PIXEL origin lies inside (lowresWidthInCU, lowresHeightInCU): two
#            blocks of a 208x128 picture, twelve of a 416x272 one (4:4:4: four) — the larger cases carry the four filter branches
#   200x120: width no multiple of 16 — the chroma extents are clamped (4:2:0: 96 of 100 columns); lowres 100x60 rounds up to 104x64 as Lowres::create does
CASES = {
    "p-208x128-i420": _case(208, 128, "i420", 48),
    "p-64x64-i420": _case(64, 64, "i420", 80, poc=1),
    "p-200x120-i420": _case(200, 120, "i420", 40, 6, mv="wild", poc=2),
    "p-416x272-i420": _case(416, 272, "i420", 46),
    "p-416x272-i422": _case(416, 272, "i422", 52),
    "p-416x272-i444": _case(416, 272, "i444", 44, 4),
    "p-208x128-i400": _case(208, 128, "i400", 48),
    "b-208x128-i420": _case(208, 128, "i420", 50, is_b=1, poc=2, lists=((0, 1), (4, 1))),
    "p-far-208x128-i420": _case(208, 128, "i420", 48, poc=8),                        # diffPoc > bframes + 1: no compensation
    "p-unsearched-208x128-i420": _case(208, 128, "i420", 56, lists=((0, 0),)),       # mvs[0].x == 0x7FFF: no compensation
    "p-lumaonly-208x128-i420": _case(208, 128, "i420", 48, chroma_same=True),        # luma weighted, chroma not
    "p-high-208x128-i420": _case(208, 128, "i420", 36, mv="zero", gain=1.7),          # a frame saturated at the maximum: weights that clip there
    "p-low-208x128-i420": _case(208, 128, "i420", 58, mv="zero", gain=1.8, bias=-0.6),   # a frame saturated at 0: weights that clip at 0
    "p-half-208x128-i420": _case(208, 128, "i420", 128, mv="zero"),                  # the frame at half the reference's brightness
    "p-same-208x128-i420": _case(208, 128, "i420", 64),                              # no change of brightness: the early exit
}
CORNER_VECTORS = [(8, 8), (2, 0), (0, 2), (2, 2), (1, 3)]      # after mcChroma's doubling and shifts: full-pel copy, filter_hpp, filter_vpp, and twice both filters


def key_of(depth, name):
    return "d%d/%s" % (depth, name)


def seed_of(key):
    return int.from_bytes(hashlib.sha256(key.encode()).digest()[:4], "little")


def _smooth(rng, h, w, pmax):
    """a textured plane: low-frequency structure plus noise, inside [0.15, 0.85] of the range"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = 0.5 + 0.2 * np.sin(xx / 7.0 + rng.uniform(0, 6)) * np.cos(yy / 5.0 + rng.uniform(0, 6)) + 0.1 * np.sin((xx + yy) / 3.0)
    a = a + rng.normal(0, 0.04, (h, w))
    return np.clip(a, 0.15, 0.85) * pmax


def _pad(a, my, mx, dt, extend):
    """the plane inside a buffer with margins: borders extended (the lowres planes), or poisoned with a ramp the function must overwrite (reference chroma)"""
    if extend:
        return np.pad(a, ((my, my), (mx, mx)), mode="edge").astype(dt)
    buf = ((np.arange((a.shape[0] + 2 * my) * (a.shape[1] + 2 * mx)) * 7) % 200 + 20).reshape(a.shape[0] + 2 * my, a.shape[1] + 2 * mx).astype(dt)
    buf[my:my + a.shape[0], mx:mx + a.shape[1]] = a
    return buf


def make_case(depth, name):
    """everything the analysis reads, made from the case's name: dict with the padded buffers (numpy), the sums, the vectors and the geometry"""
    cs = CASES[name]
    w, h, csp, is_b, bframes, poc, lists, scale64, offset8, mvkind = (cs[k] for k in ("w", "h", "csp", "is_b", "bframes", "poc", "lists", "scale64", "offset8", "mv"))
    rng = np.random.default_rng(seed_of(key_of(depth, name)))
    dt, pmax = (np.uint8, 255) if depth == 8 else (np.uint16, (1 << depth) - 1)
    hs, vs = SHIFTS[csp]
    lw, ll = -(-(w // 2) // 8) * 8, -(-(h // 2) // 8) * 8                       # Lowres::create rounds both up to whole 8x8 blocks
    cw, ch = w >> hs, h >> vs
    cmx, cmy = MARGIN_X * 2 >> hs, MARGIN_Y * 2 >> vs
    ncu = (lw // 8) * (ll // 8)
    nplanes = 1 if csp == "i400" else 3

    base_l = _smooth(rng, ll, lw, pmax)
    base_c = [_smooth(rng, ch, cw, pmax) for _ in range(2)]
    def shaped(a):
        return np.clip(np.rint(a * cs["gain"] + cs["bias"] * pmax), 0, pmax).astype(np.int64)
    fl = shaped(base_l)
    fc = [shaped(b) for b in base_c]
    # the means weightAnalyse forms divide by the 16-aligned picture size: the sums are scaled to it so that mean = sum / numpixels holds
    w16, h16 = -(-w // 16) * 16, -(-h // 16) * 16
    npix = [w16 * h16, (w16 * h16) >> (hs + vs), (w16 * h16) >> (hs + vs)]

    def sums_of(planes):
        out_s, out_v = [0, 0, 0], [0, 0, 0]
        for k, p in enumerate(planes):
            a = p.astype(np.float64)
            out_s[k] = int(round(a.mean() * npix[k]))
            out_v[k] = max(1, int(round(a.var() * npix[k])))
        return out_s, out_v

    case = dict(name=name, depth=depth, w=w, h=h, csp=csp, is_b=is_b, bframes=bframes, poc=poc, lw=lw, ll=ll, cw=cw, ch=ch, cmx=cmx, cmy=cmy, ncu=ncu,
                nplanes=nplanes, lstride=lw + 2 * MARGIN_X, cstride=cw + 2 * cmx)
    case["fenc_low"] = _pad(fl, MARGIN_Y, MARGIN_X, dt, True)
    case["fenc_c"] = [_pad(c, cmy, cmx, dt, True) for c in fc] if nplanes == 3 else []
    case["intra"] = rng.integers(300 << (depth - 8), 4000 << (depth - 8), ncu).astype(np.int32)       # some below, some above a block's SATD
    case["fenc_sums"] = sums_of([fl] + (fc if nplanes == 3 else []))
    case["lists"] = []
    for li, (rpoc, searched) in enumerate(lists):
        sc = scale64 / 64.0 if li == 0 else 64.0 / scale64
        off = offset8 * (1 << (depth - 8)) * (1 if li == 0 else -1)
        def dim(a):
            return np.clip(np.rint(a * sc + off + rng.normal(0, 0.004 * pmax, a.shape)), 0, pmax).astype(np.int64)
        low = [dim(np.roll(base_l, (i >> 1, i & 1), (0, 1))) for i in range(4)]           # four planes that differ: a wrong plane index shows
        rc = ([c.copy() for c in fc] if cs["chroma_same"] else [dim(c) for c in base_c]) if nplanes == 3 else []
        mv = np.zeros((ncu, 2), np.int32)
        if mvkind == "mixed":
            mv = rng.integers(-9, 10, (ncu, 2)).astype(np.int32)
            mv[::5] &= ~1                                                           # some half-pel-plane vectors, the rest averaged
            mv[::7] = 0
        elif mvkind == "wild":
            mv = rng.integers(-9, 10, (ncu, 2)).astype(np.int32)
            mv[2::6] = rng.integers(-700, 700, (len(mv[2::6]), 2))                # one block in six far outside: clipped at every side
        if mvkind != "zero":
            # the blocks of the chroma corner read entry y * lowresWidthInCU + x / blockWidth (y in chroma pixel rows): the four branches among them
            bw, bh, wcu, i = 16 >> hs, 16 >> vs, lw // 8, 0
            for y in range(0, ll // 8, bh):
                for x in range(0, wcu, bw):
                    mv[y * wcu + x // bw] = CORNER_VECTORS[i % len(CORNER_VECTORS)]
                    i += 1
        if mvkind == "wild":
            mv[0], mv[1] = (-700, 700), (700, -700)                                # the chroma corner clipped at every side, too
        sums = sums_of([low[0]] + rc)
        case["lists"].append(dict(poc=rpoc, searched=searched, low=[_pad(p, MARGIN_Y, MARGIN_X, dt, True) for p in low],
                                  c=[_pad(c, cmy, cmx, dt, False) for c in rc], mvs=mv, sums=sums))
    return case


def case_blob(case):
    """the case as tests/support/wpcost_ref.cpp reads it"""
    words = [CSPS[case["csp"]], case["w"], case["h"], MARGIN_X, MARGIN_Y, case["is_b"], case["bframes"], case["poc"], len(case["lists"])]
    words += case["fenc_sums"][0] + case["fenc_sums"][1]
    for l in case["lists"]:
        words += [l["poc"], l["searched"]] + l["sums"][0] + l["sums"][1]
    parts = [np.array(words, np.int64).tobytes(), case["fenc_low"].tobytes()] + [c.tobytes() for c in case["fenc_c"]] + [case["intra"].tobytes()]
    for l in case["lists"]:
        parts += [p.tobytes() for p in l["low"]] + [c.tobytes() for c in l["c"]] + [l["mvs"].tobytes()]
    return b"".join(parts)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------

def reference_source():
    mk = open(os.path.join(ROOT, "oracle", "reference.mk")).read()
    return os.path.join(os.environ.get("X265_REFERENCE") or re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1), "source")


def build_driver(tmp_dir, depth):
    """tests/support/wpcost_ref.cpp against oracle/_ref/libx265ref<depth>.so; skips where the reference is not there"""
    lib, src = os.path.join(REF, "libx265ref%d.so" % depth), reference_source()
    if not (os.path.exists(lib) and os.path.exists(os.path.join(src, "common", "lowres.h")) and os.path.exists(os.path.join(REF, "x265_config.h"))):
        pytest.skip("the reference (its sources, oracle/_ref/libx265ref%d.so) is not here" % depth)
    exe = os.path.join(str(tmp_dir), "wpcost_ref%d" % depth)
    defs = ["-DEXPORT_C_API=1", "-DX265_ARCH_X86=1", "-DX86_64=1", "-DHAVE_INT_TYPES_H=1", "-DHAVE_STRTOK_R=1", "-DENABLE_LIBNUMA=0", "-D__STDC_LIMIT_MACROS=1",
            "-DX265_DEPTH=%d" % depth, "-DHIGH_BIT_DEPTH=%d" % int(depth > 8), "-DX265_NS=x265"]
    subprocess.check_call(["g++", "-O2", "-std=gnu++11", "-w"] + defs + ["-I" + REF, "-I" + src, "-I" + os.path.join(src, "common"), "-I" + os.path.join(src, "encoder"),
                           os.path.join(ROOT, "tests", "support", "wpcost_ref.cpp"), "-o", exe, lib, "-Wl,-rpath," + REF, "-lpthread", "-ldl"])
    return exe


_memo = {}


def driver_results(tmp_dir, depth):
    """the driver's output for every case of a depth: computed once, shared by the tests, not modified"""
    if depth not in _memo:
        exe = build_driver(tmp_dir, depth)
        files = []
        for name in CASES:
            path = os.path.join(str(tmp_dir), "d%d-%s" % (depth, name))
            with open(path, "wb") as f:
                f.write(case_blob(make_case(depth, name)))
            files.append(path)
        fout = os.path.join(str(tmp_dir), "out%d.json" % depth)
        r = subprocess.run([exe, fout] + files, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-800:]
        res = json.load(open(fout))
        _memo[depth] = {name: res["d%d-%s" % (depth, name)] for name in CASES}
    return _memo[depth]


def block_digest(blocks):
    return hashlib.sha256(np.array(blocks, np.uint32).tobytes()).hexdigest()[:16]


def golden_entry(res):
    """per (plane, list) in the function's order: [plane, list, blocks per evaluation, digest of all its block values, [[wtPresent, weight, offset, denominator,
    total] per evaluation]]; and the final weights"""
    planes = []
    for e in res["evals"]:
        if not planes or planes[-1][:2] != [e["plane"], e["list"]]:
            planes.append([e["plane"], e["list"], len(e["blocks"]), [], []])
        assert len(e["blocks"]) == planes[-1][2]
        planes[-1][3] += e["blocks"]
        planes[-1][4].append([e["present"], e["w"], e["o"], e["d"], e["total"]])
    return {"planes": [[p, l, nb, block_digest(blocks), evs] for p, l, nb, blocks, evs in planes], "table": res["table"]}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("wpcost")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def offset_runs(evals):
    """the lengths of the runs of consecutive offsets at one (plane, list, weight, denominator): the offset loop of one scale"""
    runs, prev = [], None
    for e in evals:
        if not e["present"]:
            prev = None
            continue
        key = (e["plane"], e["list"], e["w"], e["d"])
        if prev and prev[0] == key and e["o"] == prev[1] + 1:
            runs[-1] += 1
        else:
            runs.append(1)
        prev = (key, e["o"])
    return runs


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", DEPTHS)
def test_host_path_reproduces_every_logged_block(work, depth):
    """wpcost.h on the host, over the same planes, gives every block value and every total the reference's weightAnalyse saw; the golden file holds the same"""
    res = driver_results(work, depth)
    g = json.load(open(GOLDEN))["cases"] if os.path.exists(GOLDEN) else None
    n = 0
    for name in CASES:
        for i, e in enumerate(res[name]["evals"]):
            assert e["blocks"] == e["host_blocks"], (name, i, e["plane"], e["list"], e["w"], e["o"], e["d"])
            assert e["total"] == e["host_total"] == sum(e["blocks"]) & 0xFFFFFFFF, (name, i)
            n += 1
        assert g is not None and golden_entry(res[name]) == g[key_of(depth, name)], name
    assert n > 100


@pytest.mark.parametrize("depth", DEPTHS)
def test_reference_log_witnesses_every_branch(work, depth):
    """the cases reach what they are there for, by the reference's own log"""
    res = driver_results(work, depth)
    every = [e for name in CASES for e in res[name]["evals"]]
    # luma: half-pel-plane and averaged vectors; the averaging slot ran as often as wpcost.h finds averaged blocks, the copy slot once per block
    mixed = res["p-208x128-i420"]
    assert mixed["luma"]["branch"][0] > 0 and mixed["luma"]["branch"][1] > 0
    assert mixed["calls"][1] == mixed["luma"]["branch"][1] and mixed["calls"][0] == sum(mixed["luma"]["branch"]) == 13 * 8
    # chroma: the plain copy outside the corner and the four branches inside it, twice (cb, cr); slot calls agree with wpcost.h's reading of the vectors
    for name in ("p-416x272-i420", "p-416x272-i422", "p-416x272-i444"):
        r = res[name]
        br = r["chroma"]["branch"]
        assert all(v > 0 for v in br), (name, br)
        assert {e["plane"] for e in r["evals"]} == {0, 1, 2}, name                      # (the branches are counted per plane; cb and cr both ran)
        assert r["calls"][2:7] == [2 * (br[0] + br[1]), 2 * br[2], 2 * br[3], 2 * br[4], 2 * br[4]], (name, r["calls"], br)
        assert r["extended"][0] == 1, name
    # vectors clipped at each side, luma and chroma
    wild = res["p-200x120-i420"]
    assert all(v > 0 for v in wild["luma"]["clipped"]), wild["luma"]
    assert all(v > 0 for v in wild["chroma"]["clipped"]), wild["chroma"]
    # weights that clip at 0 and at the pixel maximum
    assert any(e["clip0"] > 0 for e in every) and any(e["clipmax"] > 0 for e in every)
    # the offset loop breaking early and running to its end
    runs = [r for name in CASES for r in offset_runs(res[name]["evals"])]
    assert 5 in runs and any(r < 5 for r in runs), sorted(set(runs))
    # luma weighted with chroma not, and with chroma weighted
    tables = [res[name]["table"][0] for name in CASES]
    assert any(t[0][3] and t[1][3] and t[2][3] for t in tables) and any(t[0][3] and not t[1][3] and not t[2][3] for t in tables), tables
    # list 1, from a B slice
    b = res["b-208x128-i420"]
    assert any(e["list"] == 1 and e["present"] for e in b["evals"]) and any(e["list"] == 0 for e in b["evals"]) and len(b["table"]) == 2
    # a reduced luma denominator: the chosen weight was evaluated at a larger denominator than the table holds
    reduced = 0
    for name in CASES:
        wt, _, den, present = res[name]["table"][0][0]
        tried = {(e["w"], e["d"]) for e in res[name]["evals"] if e["plane"] == 0 and e["list"] == 0 and e["present"]}
        reduced += bool(present and tried and den < min(d for _, d in tried) and any(w == wt << (d - den) for w, d in tried))
    assert reduced > 0
    assert any(t[0][3] and t[1][3] for t in tables)
    # no compensation: the distance beyond bframes + 1, vectors never searched
    for name in ("p-far-208x128-i420", "p-unsearched-208x128-i420"):
        r = res[name]
        assert r["calls"][:7] == [0] * 7 and len(r["evals"]) > 1 and r["extended"][0] == 0, (name, r["calls"])
    # 4:0:0: luma only; 4:4:4: 16x16 chroma blocks
    assert {e["plane"] for e in res["p-208x128-i400"]["evals"]} == {0}
    c444 = [e for e in res["p-416x272-i444"]["evals"] if e["plane"]]
    assert c444 and all(len(e["blocks"]) == (416 // 16) * (272 // 16) for e in c444)
    c422 = [e for e in res["p-416x272-i422"]["evals"] if e["plane"]]
    assert c422 and all(len(e["blocks"]) == (208 // 8) * (272 // 8) for e in c422)
    # the clamped chroma extents: 200 x 120 -> 192 x 112 luma -> 96 x 56 chroma
    cw = [e for e in wild["evals"] if e["plane"]]
    assert cw and all(len(e["blocks"]) == 12 * 7 for e in cw)


@pytest.mark.parametrize("depth", DEPTHS)
def test_unchanged_brightness_takes_the_early_exit(work, depth):
    r = driver_results(work, depth)["p-same-208x128-i420"]
    assert r["evals"] == [] and r["calls"] == [0] * 8
    assert [t[3] for t in r["table"][0]] == [0, 0, 0]


def test_abi_announces_the_optional_entries():
    """the header, the ctypes table and the library agree; the binding looks the symbols up weakly"""
    from x265_amd import hipprim as hp
    hdr = open(os.path.join(ROOT, "include", "x265hip.h")).read()
    names = ("begin", "set_luma", "set_chroma", "blocks", "eval", "stats", "end")
    for n in names:
        assert re.search(r"\bx265hip_wpcost_%s\(" % n, hdr), n
        assert "x265hip_wpcost_%s" % n in hp.PROTOTYPES, n
        assert hasattr(hp.lib(), "x265hip_wpcost_%s" % n), n
    assert len(hp.PROTOTYPES["x265hip_wpcost_eval"][1]) == 6 and len(hp.PROTOTYPES["x265hip_wpcost_set_luma"][1]) == 8
    host = open(os.path.join(ROOT, "x265_amd", "host", "x265_hip_weightp.cpp")).read()
    assert re.search(r"x265hip_wpcost_eval\([^;]*\)\s*__attribute__\(\(weak\)\);", host, flags=re.S)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

class WeightParam(C.Structure):
    _fields_ = [("inputWeight", C.c_int32), ("inputOffset", C.c_int32), ("log2WeightDenom", C.c_int32), ("wtPresent", C.c_int32)]


GUARD = 0xC3C3C3C3


def _library():
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    return L


def _org(buf, my, mx):
    """the address of sample (0, 0) inside a padded buffer"""
    return buf.ctypes.data + (my * buf.shape[1] + mx) * buf.itemsize


def set_plane(L, ctx, case, li, plane):
    """set_luma / set_chroma as the seam calls them for list li; the reference's chroma borders extended first, as the function has done by then"""
    l = case["lists"][li]
    comp = l["searched"] and abs(case["poc"] - l["poc"]) <= case["bframes"] + 1
    mvs = l["mvs"].ctypes.data if comp else None
    if plane == 0:
        refs = (C.c_void_p * 4)(*[_org(p, MARGIN_Y, MARGIN_X) for p in l["low"]])
        return L.x265hip_wpcost_set_luma(ctx, _org(case["fenc_low"], MARGIN_Y, MARGIN_X), refs, case["lstride"], case["lw"], case["ll"], case["intra"].ctypes.data, mvs)
    hs, vs = SHIFTS[case["csp"]]
    cmy, cmx = case["cmy"], case["cmx"]
    if comp and not l.get("extended"):
        for k in range(2):
            inner = l["c"][k][cmy:cmy + case["ch"], cmx:cmx + case["cw"]].copy()
            l["c"][k][...] = np.pad(inner, ((cmy, cmy), (cmx, cmx)), mode="edge")
        l["extended"] = True
    return L.x265hip_wpcost_set_chroma(ctx, plane, _org(case["fenc_c"][plane - 1], cmy, cmx), _org(l["c"][plane - 1], cmy, cmx), case["cstride"],
                                       ((case["w"] >> 4) << 4) >> hs, ((case["h"] >> 4) << 4) >> vs, mvs, case["lw"] >> 3, case["ll"] >> 3)


def replay(L, depth, name, entry, batch):
    """every recorded evaluation of a case through the library, `batch` candidates per call; the entry's "planes" as the library gives them"""
    case = make_case(depth, name)
    ctx = C.c_void_p()
    assert L.x265hip_wpcost_begin(depth, CSPS[case["csp"]], C.byref(ctx)) == 0
    out = []
    try:
        for plane, li, _, _, evals in entry["planes"]:
            assert set_plane(L, ctx, case, li, plane) == 0, (name, plane, li)
            nb = L.x265hip_wpcost_blocks(ctx, plane)
            every, got = [], []
            for k0 in range(0, len(evals), batch):
                grp = evals[k0:k0 + batch]
                cands = (WeightParam * len(grp))(*[WeightParam(e[1], e[2], e[3], e[0]) for e in grp])
                blocks = np.full(len(grp) * nb + 16, GUARD, np.uint32)
                totals = np.full(len(grp) + 2, GUARD, np.uint32)
                rc = L.x265hip_wpcost_eval(ctx, plane, cands, len(grp), blocks[8:].ctypes.data, totals[1:].ctypes.data)
                assert rc == 0, (name, plane, li, rc)
                assert (blocks[:8] == GUARD).all() and (blocks[8 + len(grp) * nb:] == GUARD).all() and totals[0] == GUARD and totals[-1] == GUARD, "guard cells"
                every.append(blocks[8:8 + len(grp) * nb])
                got += [e[:4] + [int(totals[1 + q])] for q, e in enumerate(grp)]
            out.append([plane, li, nb, block_digest(np.concatenate(every)), got])
    finally:
        L.x265hip_wpcost_end(ctx)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_library_matches_the_recorded_reference(golden, depth):
    """every recorded candidate of every case, blocks and totals, one candidate per launch and five; guard cells around both outputs stay"""
    L = _library()
    seen = 0
    for name in CASES:
        entry = golden["cases"][key_of(depth, name)]
        for batch in (1, 5):
            assert replay(L, depth, name, entry, batch) == entry["planes"], (name, batch)
        seen += sum(len(p[4]) for p in entry["planes"])
    assert seen > 100


@pytest.mark.gpu
def test_two_contexts_on_two_threads(golden):
    L = _library()
    jobs = [(8, "p-416x272-i444"), (10, "b-208x128-i420")]
    bad = []

    def work_of(depth, name):
        entry = golden["cases"][key_of(depth, name)]
        for it in range(6):
            if replay(L, depth, name, entry, 1 + it % 5) != entry["planes"]:
                bad.append((depth, name, it))

    threads = [threading.Thread(target=work_of, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


@pytest.mark.gpu
def test_library_refuses_what_it_cannot_serve():
    """depth 9, csp 4, lines no multiple of 8, chroma on a 4:0:0 context, an evaluation of a plane never set, 17 candidates: X265HIP_EINVAL (-1)"""
    L = _library()
    ctx = C.c_void_p()
    assert L.x265hip_wpcost_begin(9, 1, C.byref(ctx)) == -1 and L.x265hip_wpcost_begin(8, 4, C.byref(ctx)) == -1
    assert L.x265hip_wpcost_begin(8, 0, C.byref(ctx)) == 0
    try:
        case = make_case(8, "p-64x64-i420")
        l = case["lists"][0]
        refs = (C.c_void_p * 4)(*[_org(p, MARGIN_Y, MARGIN_X) for p in l["low"]])
        fo = _org(case["fenc_low"], MARGIN_Y, MARGIN_X)
        assert L.x265hip_wpcost_set_luma(ctx, fo, refs, case["lstride"], 32, 28, case["intra"].ctypes.data, None) == -1
        assert L.x265hip_wpcost_set_chroma(ctx, 1, fo, fo, case["lstride"], 16, 16, None, 4, 4) == -1
        cands = (WeightParam * 17)()
        totals = np.zeros(17, np.uint32)
        assert L.x265hip_wpcost_eval(ctx, 0, cands, 1, None, totals.ctypes.data) == -1
        assert L.x265hip_wpcost_set_luma(ctx, fo, refs, case["lstride"], 32, 32, case["intra"].ctypes.data, None) == 0
        assert L.x265hip_wpcost_eval(ctx, 0, cands, 17, None, totals.ctypes.data) == -1
        assert L.x265hip_wpcost_eval(ctx, 0, cands, 1, None, totals.ctypes.data) == 0
    finally:
        L.x265hip_wpcost_end(ctx)


FRAMES = 12
ENC = {
    "medium": ("i420", 8, ["--preset", "medium"]), "main10": ("i420", 10, ["--preset", "medium"]), "slow": ("i420", 8, ["--preset", "slow"]),
    "weightb": ("i420", 8, ["--preset", "medium", "--weightb"]), "i422": ("i422", 8, ["--preset", "medium"]), "i444": ("i444", 8, ["--preset", "medium"]), "ctu32": ("i420", 8, ["--preset", "medium", "--ctu", "32"]),
}


def _clip(tmp_path, csp, fade):
    """a 416 x 240 clip: fading in, or of unchanged brightness.  The second stands still under per-frame noise: at this size the moving tiles of the
    default clip shift a picture's mean by more than the early-termination test allows, and the reference itself then analyses some of its frames"""
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 416, 240, FRAMES, seed=77, fade=fade, csp=csp, vmax=9 if fade else 0)
    return yuv


def _enc_args(yuv, csp, extra):
    return ["--input", yuv, "--input-res", "416x240", "--input-depth", "8", "--input-csp", csp, "--fps", "30", "--frames", str(FRAMES), "--pools", "4", "-F", "2"] + extra


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ENC))
def test_bound_encoders_serve_the_analysis_byte_identical(tmp_path, name):
    """the product's encoders against the unmodified reference on a 416 x 240 fade clip: the same bytes under X265HIP_VERIFY (wpcost.h beside every evaluation,
    the reference's weightAnalyse beside every table; any difference aborts) and again without it; analyses served; the reference weights P frames on the clip"""
    import test_cuserve_denoise as tcd
    import test_saostats_formats as sf
    csp, build, extra = ENC[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % build), os.path.join(REF, "integration", "x265_hip_%dbit" % build)
    sf._need(ref, hip)
    base = _enc_args(_clip(tmp_path, csp, True), csp, extra)
    rerr, want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))
    m = re.search(r"Weighted P-Frames: Y:([\d.]+)%", rerr)
    assert m and float(m.group(1)) > 0, rerr[-1200:]
    for verify in (True, False):
        env = dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_WEIGHTP="1")
        if verify:
            env["X265HIP_VERIFY"] = "1"
        err, got = tcd._run(hip, base, str(tmp_path / "hip.hevc"), env)
        assert got == want, "bitstreams differ (X265HIP_VERIFY %s)" % ("set" if verify else "not set")
        assert "VERIFY FAILED" not in err and "OFF" not in err, err[-1500:]
        m = re.search(WPCOST_RE, err)
        assert m, err[-1500:]
        print("%s (verify %d): %s" % (name, verify, m.group(0)))
        assert int(m.group(1)) > 0 and int(m.group(2)) > 0 and int(m.group(6)) == 0, m.groups()


@pytest.mark.gpu
def test_unchanged_brightness_launches_nothing(tmp_path):
    """every analysis of the clip takes the reference's early exit: nothing served, nothing launched, and the exits counted"""
    import test_cuserve_denoise as tcd
    import test_saostats_formats as sf
    ref, hip = os.path.join(REF, "x265_8bit"), os.path.join(REF, "integration", "x265_hip_8bit")
    sf._need(ref, hip)
    base = _enc_args(_clip(tmp_path, "i420", False), "i420", ["--preset", "medium"])
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    err, got = tcd._run(hip, base, str(tmp_path / "hip.hevc"), dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_WEIGHTP="1"))
    m = re.search(WPCOST_RE, err)
    assert got == want and m, err[-1200:]
    assert int(m.group(1)) == 0 and int(m.group(3)) == 0 and int(m.group(5)) > 0, m.groups()


@pytest.mark.gpu
def test_switch_off_leaves_every_analysis_to_the_host(tmp_path):
    import test_cuserve_denoise as tcd
    import test_saostats_formats as sf
    ref, hip = os.path.join(REF, "x265_8bit"), os.path.join(REF, "integration", "x265_hip_8bit")
    sf._need(ref, hip)
    base = _enc_args(_clip(tmp_path, "i420", True), "i420", ["--preset", "medium"])
    want = tcd._run(ref, base, str(tmp_path / "ref.hevc"))[1]
    err, got = tcd._run(hip, base, str(tmp_path / "hip.hevc"), dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_WEIGHTP="0"))
    m = re.search(WPCOST_RE, err)
    assert got == want and m and int(m.group(1)) == 0 and int(m.group(3)) == 0 and int(m.group(6)) > 0, err[-1200:]


@pytest.mark.gpu
def test_default_serves_the_8_bit_build(tmp_path):
    """X265HIP_WEIGHTP unset: on where the fade A/B was ahead (profiles/r16_v1_wpcost_ab.txt)"""
    import test_saostats_formats as sf
    ref, hip = os.path.join(REF, "x265_8bit"), os.path.join(REF, "integration", "x265_hip_8bit")
    sf._need(ref, hip)
    base = _enc_args(_clip(tmp_path, "i420", True), "i420", ["--preset", "medium"])
    env = {k: v for k, v in os.environ.items() if k != "X265HIP_WEIGHTP"}
    env.update(X265HIP="require", X265HIP_VERBOSE="1")
    out = []
    for exe, name in ((ref, "ref.hevc"), (hip, "hip.hevc")):
        r = subprocess.run([exe] + base + ["-o", str(tmp_path / name)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-1200:]
        out.append((r.stderr, open(str(tmp_path / name), "rb").read()))
    m = re.search(WPCOST_RE, out[1][0])
    assert out[0][1] == out[1][1] and m and int(m.group(1)) > 0 and int(m.group(6)) == 0, out[1][0][-1200:]
