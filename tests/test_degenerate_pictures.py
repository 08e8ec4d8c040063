"""Device decisions on pictures full of exact ties: flat, periodic, letterboxed and rail-valued (degenerate_cases.degenerate_scenes).

Every kernel that DECIDES something claims to reproduce a sequential tie rule — the motion searches replay the reference's comparisons in the reference's
order with strict `<` (x265_amd/csrc/mesearch.h), the SAD surfaces keep the smaller vy, then the smaller vx among equals (oracle/x265_oracle_sadsurf.inc),
the lookahead replays its candidates in the reference's order, the lowres intra estimate takes planar only if strictly cheaper than DC — and textured pictures
plus noise never put two candidates at the same cost.  These pictures do: on a flat picture every vector has the same SAD, on stripes and checkers every
period repeats the minimum, in letterbox bars whole blocks are flat, and rail values push every sum to its largest.

CPU tier: the restatement (backends.Orc, the emulated SAD surfaces) against the REAL reference (backends.Ref over oracle/_ref) on these pictures, and a tie
witness: brute-force cost surfaces of the FULL-search windows must attain their minimum more than once in at least a quarter of the windows of each tie
class — a scene that lost its ties would otherwise still pass.  GPU tier: the device against the restatement, every value equal."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from backends import Orc, Ref, same                          # noqa: E402
from degenerate_cases import degenerate_scenes               # noqa: E402
from oracle import pyoracle as po                            # noqa: E402

DEPTHS = [8, 10, 12]
M = 80                                                       # margin of every scene here
ME_H, ME_W = 160, 192
METHODS = [0, 1, 2, 3, 5]                                    # DIA, HEX, UMH, STAR, FULL
SUBMES = [0, 2, 3, 7]
# four squares (the team kernels: motion2_kernel, with quarter-pel planes motion3_kernel for 8 / 16 / 32) and three other shapes (motion_kernel)
SHAPES = [(8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (32, 24), (12, 16)]
SEA_SHAPES = [(8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (32, 24), (24, 32), (64, 48), (48, 64), (64, 16), (16, 64),
              (16, 12), (12, 16), (16, 4), (4, 16)]          # test_hip_parity.SEA_SHAPES: the shapes whose four sub-blocks lie inside the PU
SEA_PAD = (80, 96)                                           # PicYuv's margins at CTU 64: what the reference's integral planes are laid out for
CHROMA_SHAPES = [(8, 8), (16, 16), (32, 24), (64, 64)]
TIE_CLASSES = ("flat-mid", "flat-rails", "stripes8", "checker16")
LA_SIZES = {(200, 136): ((9, 1), (3, 3)), (66, 50): ((4, 1), (2, 2))}      # (W, H): (rows per slice, slices) serial and cooperative


def _need_ref(depth):
    if not po.ref_available(depth):
        pytest.skip("oracle/_ref/libx265ref%d.so not built (make -C oracle ref)" % depth)


# ---- the searches: one list of groups per depth, shared by both tiers ------------------------------------------------------------------------------

def _draw_pus(rng, g, m_y, m_x, count, tight=True):
    """`count` PUs for group g: positions on the 4-sample grid, the window mvp +- merange as Search::setSearchRange lays it (search.cpp:2724).  Every second
    predictor lies half-way between full-pel vectors, = 2 (mod 4), on the diagonal: its four full-pel neighbours then cost the same on a flat picture, the two
    vertical ones on stripes, and on the checkerboard the minima (0, +-8) and (+-8, 0) are equally far from it.  Of the others every fourth has ONE such
    component (a tie of two neighbours only), the rest are unconstrained."""
    w, h, merange = g["w"], g["h"], g["merange"]
    for k in range(count):
        bx = m_x + int(rng.integers(0, (ME_W - w) // 4 + 1)) * 4
        by = m_y + int(rng.integers(0, (ME_H - h) // 4 + 1)) * 4
        qmvp = [int(rng.integers(-40, 41)), int(rng.integers(-40, 41))]
        if k % 2:
            qmvp = [4 * int(rng.integers(-8, 8)) + 2] * 2
        elif rng.integers(0, 4) == 0:
            qmvp[int(rng.integers(0, 2))] = 4 * int(rng.integers(-10, 10)) + 2
        mvmin = [(qmvp[0] >> 2) - merange, (qmvp[1] >> 2) - merange]
        mvmax = [(qmvp[0] >> 2) + merange, (qmvp[1] >> 2) + merange]
        if tight and rng.integers(0, 4) == 0:                # a tight vertical bound, as frame-parallel row lag makes
            mvmax[1] = max(min(mvmax[1], int(rng.integers(0, 6))), mvmin[1])
        g["pus"].append((bx, by)); g["mins"].append(tuple(mvmin)); g["maxs"].append(tuple(mvmax)); g["mvps"].append(tuple(qmvp))
        g["cands"].append([(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(g["numCand"])])


def _group(rng, cls, w, h, method, subme, merange):
    return dict(cls=cls, w=w, h=h, method=method, subme=subme, merange=merange, qp=int(rng.choice([22, 37])), numCand=int(rng.integers(0, 3)),
                pus=[], mins=[], maxs=[], mvps=[], cands=[])


@functools.lru_cache(maxsize=None)
def _me_scenes(depth):
    return degenerate_scenes(depth, (ME_H, ME_W), 8000 + depth, margin=M)


@functools.lru_cache(maxsize=None)
def _me_groups(depth):
    """six classes x five methods x four subme x seven shapes, two PUs each: 1 680 searches"""
    rng = np.random.default_rng(8100 + depth)
    groups = []
    for ci in range(len(_me_scenes(depth))):
        for method in METHODS:
            for subme in SUBMES:
                for (w, h) in SHAPES:
                    g = _group(rng, ci, w, h, method, subme, 8 if method == 5 else int(rng.choice([16, 32])))
                    _draw_pus(rng, g, M, M, 2)
                    groups.append(g)
    return groups


def _me_results(o, depth, groups):
    scenes = _me_scenes(depth)
    out = []
    for g in groups:
        _, refp, srcp = scenes[g["cls"]]
        out.append([o.motion_estimate(refp, srcp, g["pus"][i][0], g["pus"][i][1], g["w"], g["h"], g["mins"][i], g["maxs"][i], g["mvps"][i], g["cands"][i],
                                      g["merange"], g["method"], g["subme"], g["qp"]) for i in range(len(g["pus"]))])
    return out


@functools.lru_cache(maxsize=None)
def _me_want(depth):
    return _me_results(Orc(depth), depth, _me_groups(depth))


@functools.lru_cache(maxsize=None)
def _sea_scenes(depth):
    """the same pictures in PicYuv's layout (margins replicated, 80 rows x 96 columns)"""
    pad = ((SEA_PAD[0], SEA_PAD[0]), (SEA_PAD[1], SEA_PAD[1]))
    return [(name, np.ascontiguousarray(np.pad(r[M:M + ME_H, M:M + ME_W], pad, mode="edge")), np.ascontiguousarray(np.pad(s[M:M + ME_H, M:M + ME_W], pad, mode="edge")))
            for name, r, s in _me_scenes(depth)]


@functools.lru_cache(maxsize=None)
def _sea_groups(depth):
    """six classes x twenty shapes, subme 0 / 2 / 3 in turn, four PUs each: 480 searches"""
    rng = np.random.default_rng(8200 + depth)
    groups = []
    for ci in range(len(_sea_scenes(depth))):
        for k, (w, h) in enumerate(SEA_SHAPES):
            g = _group(rng, ci, w, h, 4, (0, 2, 3)[(k + ci) % 3], int(rng.choice([8, 16])))
            _draw_pus(rng, g, SEA_PAD[0], SEA_PAD[1], 4)
            groups.append(g)
    return groups


@functools.lru_cache(maxsize=None)
def _sea_want(depth):
    o = Orc(depth)
    planes = [o.integral_planes(r) for _, r, _ in _sea_scenes(depth)]
    out = []
    for g in _sea_groups(depth):
        _, refp, srcp = _sea_scenes(depth)[g["cls"]]
        out.append([o.motion_estimate_sea(refp, srcp, g["pus"][i][0], g["pus"][i][1], g["w"], g["h"], g["mins"][i], g["maxs"][i], g["mvps"][i], g["cands"][i],
                                          g["merange"], g["subme"], g["qp"], planes=planes[g["cls"]]) for i in range(len(g["pus"]))])
    return planes, out


@functools.lru_cache(maxsize=None)
def _chroma_scenes(depth):
    return degenerate_scenes(depth, (ME_H, ME_W), 8000 + depth, margin=M, chroma=True)


@functools.lru_cache(maxsize=None)
def _chroma_groups(depth):
    """six classes x DIA / HEX / STAR x subme 3 / 7 x four shapes, two PUs each: 288 searches with the chroma SATD term of subpelCompare"""
    rng = np.random.default_rng(8300 + depth)
    groups = []
    for ci in range(len(_chroma_scenes(depth))):
        for method in (0, 1, 3):
            for subme in (3, 7):
                for (w, h) in CHROMA_SHAPES:
                    g = _group(rng, ci, w, h, method, subme, 16)
                    _draw_pus(rng, g, M, M, 2)
                    groups.append(g)
    return groups


def _chroma_results(o, depth):
    scenes = _chroma_scenes(depth)
    out = []
    for g in _chroma_groups(depth):
        _, ref, src = scenes[g["cls"]]
        out.append([o.motion_estimate_chroma(ref, src, g["pus"][i][0], g["pus"][i][1], g["w"], g["h"], g["mins"][i], g["maxs"][i], g["mvps"][i], g["cands"][i],
                                             g["merange"], g["method"], g["subme"], g["qp"]) for i in range(len(g["pus"]))])
    return out


@functools.lru_cache(maxsize=None)
def _chroma_want(depth):
    return _chroma_results(Orc(depth), depth)


def _label(scenes, g, i):
    return (scenes[g["cls"]][0], "method %d subme %d %dx%d merange %d qp %d" % (g["method"], g["subme"], g["w"], g["h"], g["merange"], g["qp"]),
            "pu", g["pus"][i], "mvp", g["mvps"][i], "window", g["mins"][i], g["maxs"][i], "cands", g["cands"][i])


# ---- CPU tier: the restatement against the real reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", DEPTHS)
def test_restated_searches_are_the_reference_on_degenerate_pictures(depth):
    _need_ref(depth)
    groups, scenes = _me_groups(depth), _me_scenes(depth)
    want, got = _me_results(Ref(depth), depth, groups), _me_want(depth)
    bad = [(_label(scenes, g, i), "ref", want[k][i], "restatement", got[k][i]) for k, g in enumerate(groups) for i in range(len(g["pus"])) if want[k][i] != got[k][i]]
    assert not bad, (len(bad), bad[:4])
    assert sum(len(g["pus"]) for g in groups) == 1680


@pytest.mark.parametrize("depth", DEPTHS)
def test_full_search_windows_hold_exact_ties(depth):
    """The tie witness.  sad + mvcost of every vector of each FULL-search window (merange 8), by Orc.sad and the cost table around its centre 65536: in each
    of the four tie classes the minimum is attained by more than one vector in at least a quarter of the windows."""
    o = Orc(depth)
    scenes = _me_scenes(depth)
    tabs = {qp: o.mvcost_table(qp).astype(np.int64) for qp in (22, 37)}
    tied, windows = {}, {}
    for g in _me_groups(depth):
        name, refp, srcp = scenes[g["cls"]]
        if g["method"] != 5 or name not in TIE_CLASSES:
            continue
        tab = tabs[g["qp"]]
        for i, (bx, by) in enumerate(g["pus"]):
            costs = [o.sad(g["w"], g["h"], srcp, (by, bx), refp, (by + vy, bx + vx)) +
                     int(tab[po.MVCOST_CENTRE + 4 * vx - g["mvps"][i][0]]) + int(tab[po.MVCOST_CENTRE + 4 * vy - g["mvps"][i][1]])
                     for vy in range(g["mins"][i][1], g["maxs"][i][1] + 1) for vx in range(g["mins"][i][0], g["maxs"][i][0] + 1)]
            windows[name] = windows.get(name, 0) + 1
            tied[name] = tied.get(name, 0) + (costs.count(min(costs)) > 1)
    print("windows whose minimum is attained more than once:", {n: "%d of %d" % (tied[n], windows[n]) for n in windows})
    assert sorted(windows) == sorted(TIE_CLASSES) and po.MVCOST_CENTRE == 65536
    for name in TIE_CLASSES:
        assert 4 * tied[name] >= windows[name], (name, tied[name], windows[name])


@pytest.mark.parametrize("depth", DEPTHS)
def test_restated_sea_searches_are_the_reference_on_degenerate_pictures(depth):
    _need_ref(depth)
    r = Ref(depth)
    groups, scenes = _sea_groups(depth), _sea_scenes(depth)
    oplanes, got = _sea_want(depth)
    rplanes = [r.integral_planes(refp, SEA_PAD) for _, refp, _ in scenes]
    for ci, (name, refp, _) in enumerate(scenes):
        for k, (w, h) in enumerate(Orc.SEA_WINDOWS):
            assert np.array_equal(oplanes[ci][k][:refp.shape[0] - h - 1, :refp.shape[1] - w], rplanes[ci][k][:refp.shape[0] - h - 1, :refp.shape[1] - w]), (name, w, h)
    n = 0
    for k, g in enumerate(groups):
        _, refp, srcp = scenes[g["cls"]]
        for i, (bx, by) in enumerate(g["pus"]):
            want = r.motion_estimate_sea(refp, srcp, bx, by, g["w"], g["h"], g["mins"][i], g["maxs"][i], g["mvps"][i], g["cands"][i], g["merange"], g["subme"], g["qp"],
                                         planes=rplanes[g["cls"]], pad=SEA_PAD)
            assert want == got[k][i], (_label(scenes, g, i), want, got[k][i])
            n += 1
    assert n == 480


@pytest.mark.parametrize("depth", DEPTHS)
def test_restated_chroma_searches_are_the_reference_on_degenerate_pictures(depth):
    _need_ref(depth)
    groups, scenes = _chroma_groups(depth), _chroma_scenes(depth)
    want, got = _chroma_results(Ref(depth), depth), _chroma_want(depth)
    bad = [(_label(scenes, g, i), want[k][i], got[k][i]) for k, g in enumerate(groups) for i in range(len(g["pus"])) if want[k][i] != got[k][i]]
    assert not bad, (len(bad), bad[:4])
    assert sum(len(g["pus"]) for g in groups) == 288


# ---- the lookahead ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _la_scenes(depth, w, h):
    return degenerate_scenes(depth, (h, w), 8400 + depth + w, margin=M, lookahead=True)


def _la_results(b, depth, w, h):
    """{(class, what): result tuple}: Lowres::init + intra estimate of both pictures, the P cost pass serial and in slices, the B cost pass of the source
    between two copies of the reference (both lists then cost the same wherever the pictures tie) with list 0 searched and reused"""
    out = {}
    for name, s0, s1 in _la_scenes(depth, w, h):
        for k, s in enumerate((s0, s1)):
            r = b.lowres_pass(s, (M, M), w, h, M, M)
            lw = r[5][1]
            out[name, "lowres", k] = (r[0], r[1], r[2], r[3]) + tuple(np.ascontiguousarray(p[:, :lw + 2 * M]) for p in r[4]) + r[5]
        for rps, ns in LA_SIZES[w, h]:
            out[name, "P", rps, ns] = b.lookahead_cost_p(s0, s1, (M, M), w, h, M, M, rps, ns)
        for prefill in (0, 1):
            rps, ns = LA_SIZES[w, h][1 - prefill]
            out[name, "B", rps, ns, prefill] = b.lookahead_cost_b(s0, s1, s0, (M, M), w, h, M, M, rps, ns, prefill)
    return out


@functools.lru_cache(maxsize=None)
def _la_want(depth, w, h):
    return _la_results(Orc(depth), depth, w, h)


def _same_results(want, got):
    assert set(want) == set(got)
    for k in want:
        assert len(want[k]) == len(got[k])
        for j, (x, y) in enumerate(zip(want[k], got[k])):
            assert same(x, y), (k, j, x if np.isscalar(x) else np.argwhere(np.asarray(x) != np.asarray(y))[:4], y if np.isscalar(y) else None)


@pytest.mark.parametrize("depth", DEPTHS)
def test_restated_lookahead_is_the_reference_on_degenerate_pictures(depth):
    _need_ref(depth)
    _same_results(_la_results(Ref(depth), depth, 200, 136), _la_want(depth, 200, 136))


# ---- SAD surfaces ----------------------------------------------------------------------------------------------------------------------------------

SURFACE_FORMS = [
    # depth, S, w, h, MX, MY, ctu — and the kernel that builds the windows on the device
    (8, 32, 136, 72, 96, 80, 64),         # sadsurf_ctu_kernel: the CTU's surface in LDS
    (10, 16, 136, 72, 96, 80, 64),        # sadsurf_ctu16_kernel
    (12, 32, 136, 72, 96, 80, 64),        # sadsurf_ctu16_wide_kernel: the surface in a pooled device buffer
    (8, 32, 200, 136, 48, 32, 16),        # --ctu 16: PicYuv pads 48 x 32 only, the window reaches the end of the buffer
]
WIN = 16


@functools.lru_cache(maxsize=None)
def _surface_pictures(form):
    """per class: (name, reference picture in PicYuv's buffer layout with replicated margins, stride, rows, source picture)"""
    depth, S, w, h, MX, MY, ctu = SURFACE_FORMS[form]
    rows, stride = ((h + ctu - 1) // ctu) * ctu + 2 * MY, ((w + 2 * MX + 63) // 64) * 64
    out = []
    for name, r, s in degenerate_scenes(depth, (h, w), 8500 + form, margin=16):
        buf = np.zeros((rows, stride), r.dtype)
        buf[:h + 2 * MY, :w + 2 * MX] = np.pad(r[16:16 + h, 16:16 + w], ((MY, MY), (MX, MX)), mode="edge")
        out.append((name, buf, stride, rows, np.ascontiguousarray(s[16:16 + h, 16:16 + w])))
    return out


def _run_complete(hp, L, depth, w, h, buf, stride, rows, src, S, lam, levels, MX, MY):
    """test_sadsurf_range16._run_complete for one source picture and any margins: the reference picture complete first, then the surface attached; -> its view"""
    from test_sadsurf import _read_view
    rp = L.x265hip_refpic_create(depth, w, h, stride, MX, MY, rows, buf.ctypes.data)
    assert rp, L.x265hip_last_error()
    assert L.x265hip_refpic_rows_final(rp, h) == 0 and L.x265hip_refpic_wait(rp) == 0
    sp = L.x265hip_srcpic_create(depth, w, h)
    assert sp and L.x265hip_srcpic_upload(sp, src.ctypes.data, src.shape[1]) == 0, L.x265hip_last_error()
    ss = L.x265hip_sadsurf_attach_levels(sp, rp, S, lam, levels)
    assert ss, L.x265hip_last_error()
    assert L.x265hip_refpic_wait(rp) == 0, L.x265hip_last_error()
    view = _read_view(hp, L, ss, w, h)
    L.x265hip_sadsurf_release(ss)
    L.x265hip_refpic_wait(rp)
    L.x265hip_refpic_destroy(rp)
    L.x265hip_srcpic_destroy(sp)
    return view


def _surfaces(hp, L, form, lam):
    """{class: {level: (origins, tables, sub-pel entries)}} of one library: the 8x8 windows too at 8 bit (16-bit pictures never have them), sub-pel tables always"""
    depth, S, w, h, MX, MY, ctu = SURFACE_FORMS[form]
    return {name: _run_complete(hp, L, depth, w, h, buf, stride, rows, src, S, lam, 31 if depth == 8 else 30, MX, MY)
            for name, buf, stride, rows, src in _surface_pictures(form)}


@pytest.mark.parametrize("form", range(len(SURFACE_FORMS)))
def test_restated_surfaces_follow_their_rule_on_degenerate_pictures(form):
    """Sampled entries of every window of the emulated surfaces against the real sad<N, N>, the windows' legality, and the documented rule (oracle/
    x265_oracle_sadsurf.inc: smallest cost, ties to the smaller vy, then the smaller vx) where it can be read off the picture:
      flat pictures, lambda 0   every vector costs the same: the first one, (-S, -S), wins everywhere and the origin is (-S, -S)
      flat pictures, lambda 180 the vector cost alone decides: (0, 0) from the top level down, origin (-8, -8)
      stripes8, lambda 0        the first row of vectors holds a minimum: every window starts at -S vertically"""
    import x265_amd.hipprim as hp
    from test_sadsurf import _emul
    em = _emul(hp)
    depth, S, w, h, MX, MY, ctu = SURFACE_FORMS[form]
    try:
        o = Ref(depth)
    except Exception:
        o = Orc(depth)                 # pinned to it by tests/test_oracle_vs_ref.py
    rng = np.random.default_rng(form)
    pictures = {p[0]: p for p in _surface_pictures(form)}
    for lam in (0, 180):
        views = _surfaces(hp, em, form, lam)
        for name, view in views.items():
            _, buf, stride, rows, src = pictures[name]
            assert sorted(view) == ([0, 1, 2, 3] if depth == 8 else [1, 2, 3])
            for l in (1, 2, 3):
                org, tab, sub = view[l]
                n = 8 << l
                assert sub is not None
                for by in range(org.shape[0]):
                    for bx in range(org.shape[1]):
                        ox, oy = int(org[by, bx, 0]), int(org[by, bx, 1])
                        x, y = bx * n, by * n
                        assert -S <= ox <= S - WIN and -S <= oy <= S - WIN
                        assert x + ox >= -MX and x + ox + WIN - 1 + n <= w + MX and y + oy >= -MY and y + oy + WIN - 1 + n <= h + MY
                        for k in rng.integers(0, WIN * WIN, 6):
                            j, i = divmod(int(k), WIN)
                            assert tab[by, bx, k] == o.sad(n, n, src, (y, x), buf, (MY + y + oy + j, MX + x + ox + i)), (name, lam, l, bx, by, i, j)
                if name in ("flat-mid", "flat-rails"):
                    assert (org == (-S if lam == 0 else -8)).all(), (name, lam, l, org.reshape(-1, 2)[:6])
                    assert (tab == tab[0, 0, 0]).all() and (sub == sub[0, 0, 0]).all()
                if name == "stripes8" and lam == 0:
                    assert (org[:, :, 1] == -S).all(), (l, org.reshape(-1, 2)[:6])
        if lam == 0 and form == 0:
            # Stripes against themselves match at every multiple of 8 that stays inside the picture (the replicated margin left of it is flat): the first such
            # vector is -32 for a block at x >= 32, -16 at x = 16, 0 at x = 0, the origin 8 less, clamped to -32.  stripes8's source lies 4 columns further
            # and so do its matches: -28, -12, 4.
            _, buf, stride, rows, src = pictures["stripes8"]
            own = np.ascontiguousarray(buf[MY:MY + h, MX:MX + w])
            unshifted = _run_complete(hp, em, depth, w, h, buf, stride, rows, own, S, 0, 31, MX, MY)
            origins = lambda view: {tuple(int(v) for v in o_) for o_ in view[1][0].reshape(-1, 2)}       # noqa: E731
            assert origins(unshifted) == {(-32, -32), (-24, -32), (-8, -32)}
            assert origins(views["stripes8"]) == {(-32, -32), (-20, -32), (-4, -32)}
        if depth == 12:
            assert int(views["flat-rails"][3][1].max()) == 4095 * 64 * 64 == 16773120           # the largest entry a surface can hold


# ---- the lookahead session ---------------------------------------------------------------------------------------------------------------------------

def _padded_with_stats(cores, margin):
    """pictures as test_la_session._frames returns them (replicated margins, 8 more columns on the right) + their weighted-prediction statistics"""
    pics, stats = [], []
    for p in cores:
        core = p.astype(np.int64)
        n = core.size
        sm, sq = int(core.sum()), int((core * core).sum())
        stats.append(((sq - (sm * sm + n // 2) // n) // 4, sm // 4))
        pics.append(np.ascontiguousarray(np.pad(p, ((margin, margin), (margin, margin + 8)), mode="edge")))
    return pics, stats


def _frames_cut_to_black(textured):
    """the session script's own moving texture behind letterbox bars (top and bottom 48 rows at 16 << (depth - 8)), a cut to two black frames after the third, and
    back: whole frames and the bars of the others are flat, every vector of a block in them costs the same"""
    def frames(depth, seed, count, W, H, margin, fade):
        pics, _ = textured(depth, seed, count, W, H, margin, fade)
        black = 16 << (depth - 8)
        cores = []
        for t, p in enumerate(pics):
            core = p[margin:margin + H, margin:margin + W].copy()
            core[:48] = black
            core[H - 48:] = black
            if t in (3, 4):
                core[:] = black
            cores.append(core)
        return _padded_with_stats(cores, margin)
    return frames


def _frames_static_checker32(depth, seed, count, W, H, margin, fade):
    """the same checkerboard of 16 x 16 squares in every frame: the zero vector matches exactly, and so does every vector that moves by whole periods"""
    ref = {name: r for name, r, _ in degenerate_scenes(depth, (H, W), seed, margin=margin, lookahead=True)}["checker32"]
    return _padded_with_stats([ref[margin:margin + H, margin:margin + W]] * count, margin)


SESSIONS = {
    # test_la_session.CONFIGS rows (depth, W, H, frames, bframes, fade, seed) + the pictures the script runs on
    "cut-to-black": ((8, 200, 136, 7, 3, False, 17), _frames_cut_to_black),            # letterboxed motion x 3, black x 2, letterboxed x 2
    "static-checker32": ((10, 176, 144, 6, 2, False, 18), lambda textured: _frames_static_checker32),
}


def _drive_session(monkeypatch, name, device):
    """test_la_session's randomised script (frames entering and leaving slots, batches, searches ahead, cooperative slices, vector uploads) on one of SESSIONS:
    its configuration list and its picture source are replaced for the call, the script itself is the one the textured configurations run"""
    import test_la_session as tls
    hp, hip, em = tls._libs()
    cfg, source = SESSIONS[name]
    monkeypatch.setattr(tls, "CONFIGS", [cfg])
    monkeypatch.setattr(tls, "_frames", source(tls._frames))
    tls._drive(hp, hip if device else em, em, 0)


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_session_script_is_deterministic_on_degenerate_pictures(monkeypatch, name):
    """CPU tier: the emulation on both sides, as test_la_session keeps its script honest without a GPU"""
    _drive_session(monkeypatch, name, False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_session_matches_emulation_on_degenerate_pictures(monkeypatch, name):
    """x265hip_la_* of the device against the emulated session, every output array of every call"""
    _drive_session(monkeypatch, name, True)


# ---- one degenerate clip through the bound encoder -------------------------------------------------------------------------------------------------

CLIP_W, CLIP_H, CLIP_FRAMES = 256, 192, 8


def _write_clip(path):
    """8-bit 4:2:0: three letterboxed frames of a texture that moves, a cut to two black frames, three static frames of stripes8 with a flat right half"""
    from cases import textured_frame
    rng = np.random.default_rng(8600)
    big = textured_frame(rng, CLIP_H + 32, CLIP_W + 32, 8, sigma=2.0)
    yy, xx = np.mgrid[0:CLIP_H, 0:CLIP_W]
    with open(path, "wb") as f:
        for t in range(CLIP_FRAMES):
            c = np.full((CLIP_H // 2, CLIP_W // 2), 128, np.uint8)
            if t < 3:
                y = big[8 + 2 * t:8 + 2 * t + CLIP_H, 8 + 3 * t:8 + 3 * t + CLIP_W].copy()
                y[:48] = 16
                y[CLIP_H - 48:] = 16
                sub = (y[0::2, 0::2].astype(np.int64) + y[1::2, 0::2] + y[0::2, 1::2] + y[1::2, 1::2] + 2) >> 2
                c = (128 + (sub - 128) // 2).astype(np.uint8)
                c[:24] = 128
                c[CLIP_H // 2 - 24:] = 128
            elif t < 5:
                y = np.full((CLIP_H, CLIP_W), 16, np.uint8)
            else:
                y = np.where(xx < CLIP_W // 2, (xx % 8 < 4) * 255, 127).astype(np.uint8)
            f.write(np.ascontiguousarray(y).tobytes() + c.tobytes() + (255 - c).tobytes())


def _served(err):
    """the three modules the clip must really reach (regexes of test_sadsurf_range16 / test_sadsurf / test_cuserve)"""
    from test_sadsurf_range16 import SERVED_RE
    sads = re.search(SERVED_RE, err)
    subpel = re.search(r"sadplanes: (\d+) sub-pel SATDs of the motion search", err)
    answers = re.search(r"cuserve: (\d+) sse_pp and (\d+) psy-cost \(source, reconstruction\) answers", err)
    assert sads and subpel and answers, err[-1500:]
    counts = (int(sads.group(1)), int(subpel.group(1)), int(answers.group(1)), int(answers.group(2)))
    print("served: %d integer-pel SADs, %d sub-pel SATDs, %d sse_pp and %d psy-cost answers" % counts)
    assert all(c > 0 for c in counts), counts


@pytest.mark.parametrize("bits", [8, 10])
def test_emulated_encoder_is_byte_identical_on_a_degenerate_clip(tmp_path, bits):
    """x265_emul_{8,10}bit against the unmodified reference at preset medium, every served value recomputed by the reference's function (X265HIP_VERIFY)"""
    import test_places as tp
    ref, emul = tp._need("x265_%dbit" % bits), tp._need("x265_emul_%dbit" % bits)
    yuv = str(tmp_path / "clip.yuv")
    _write_clip(yuv)
    want, _ = tp._encode(ref, yuv, CLIP_W, CLIP_H, CLIP_FRAMES, str(tmp_path / "ref.hevc"), {})
    got, err = tp._encode(emul, yuv, CLIP_W, CLIP_H, CLIP_FRAMES, str(tmp_path / "emul.hevc"), {"X265HIP_VERIFY": "1"})
    assert len(want) > 1000 and got == want, "bitstreams differ"
    _served(err)


# ---- GPU tier: the device against the restatement --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hipmod():
    import hipbackend
    from x265_amd import hipprim as hp
    assert hp.lib().x265hip_device_count() > 0, "no HIP device: the -m gpu tests need a real MI355X"
    hp.check(hp.lib().x265hip_init(0))
    return hipbackend


def _hip(hipmod, depth):
    g = hipmod.Hip(depth)
    for qp in (22, 37):
        g.set_mvcost_table(qp, Orc(depth).mvcost_table(qp))
    return g


def _report(scenes, groups, want, got):
    """every mismatch of a run, grouped by class / method / shape: one GPU run tells the whole story"""
    bad = [(_label(scenes, g, i), "want", want[k][i], "got", got[k][i]) for k, g in enumerate(groups) if got[k] is not None
           for i in range(len(g["pus"])) if want[k][i] != got[k][i]]
    total = sum(len(g["pus"]) for k, g in enumerate(groups) if got[k] is not None)
    assert not bad, ("%d / %d searches differ" % (len(bad), total), bad[:6])
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [0, 1], ids=["filter", "planes"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_device_searches_match_restatement_on_degenerate_pictures(hipmod, depth, method, planes):
    """x265hip_motion_estimate_planes_batch, a launch per (class, subme, shape): motion_kernel for the three non-square shapes, motion2_kernel for the squares
    (with quarter-pel planes for 64x64 only), motion3_kernel for 8x8 / 16x16 / 32x32 with planes"""
    g = _hip(hipmod, depth)
    groups, scenes, want = _me_groups(depth), _me_scenes(depth), _me_want(depth)
    got = [None] * len(groups)
    for k, gr in enumerate(groups):
        if gr["method"] != method:
            continue
        _, refp, srcp = scenes[gr["cls"]]
        cost, mv = g.motion_estimate_batch(refp, srcp, gr["w"], gr["h"], gr["pus"], gr["mins"], gr["maxs"], gr["mvps"], gr["cands"] if gr["numCand"] else [],
                                           gr["merange"], method, gr["subme"], gr["qp"], planes_margin=M if planes else 0)
        hipmod._release()
        got[k] = [(int(cost[i]), (int(mv[i, 0]), int(mv[i, 1]))) for i in range(len(gr["pus"]))]
    assert _report(scenes, groups, want, got) == 336


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_device_sea_searches_match_restatement_on_degenerate_pictures(hipmod, depth):
    g = _hip(hipmod, depth)
    groups, scenes = _sea_groups(depth), _sea_scenes(depth)
    planes, want = _sea_want(depth)
    for ci, (name, refp, _) in enumerate(scenes):
        for k, p in enumerate(g.integral_planes(refp)):
            assert np.array_equal(p, planes[ci][k]), (name, Orc.SEA_WINDOWS[k])
    got = []
    for gr in groups:
        _, refp, srcp = scenes[gr["cls"]]
        cost, mv = g.motion_estimate_sea_batch(refp, srcp, gr["w"], gr["h"], gr["pus"], gr["mins"], gr["maxs"], gr["mvps"], gr["cands"] if gr["numCand"] else [],
                                               gr["merange"], gr["subme"], gr["qp"])
        hipmod._release()
        got.append([(int(cost[i]), (int(mv[i, 0]), int(mv[i, 1]))) for i in range(len(gr["pus"]))])
    assert _report(scenes, groups, want, got) == 480


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_device_chroma_searches_match_restatement_on_degenerate_pictures(hipmod, depth):
    g = _hip(hipmod, depth)
    groups, scenes, want = _chroma_groups(depth), _chroma_scenes(depth), _chroma_want(depth)
    got = []
    for gr in groups:
        _, ref, src = scenes[gr["cls"]]
        cost, mv = g.motion_estimate_chroma_batch(ref, src, gr["w"], gr["h"], gr["pus"], gr["mins"], gr["maxs"], gr["mvps"], gr["cands"] if gr["numCand"] else [],
                                                  gr["merange"], gr["method"], gr["subme"], gr["qp"])
        hipmod._release()
        got.append([(int(cost[i]), (int(mv[i, 0]), int(mv[i, 1]))) for i in range(len(gr["pus"]))])
    assert _report(scenes, groups, want, got) == 288


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(LA_SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("depth", DEPTHS)
def test_device_lookahead_matches_restatement_on_degenerate_pictures(hipmod, depth, size):
    """lowres planes and intra estimate, lookahead_p_kernel serial and in slices, lookahead_bidir_kernel behind both list searches (and behind a reused list 0),
    one class at a time; then all classes as the pairs of ONE launch of the P cost pass"""
    w, h = size
    g = hipmod.Hip(depth)
    want = _la_want(depth, w, h)
    got = _la_results(g, depth, w, h)
    hipmod._release()
    _same_results(want, got)
    scenes = _la_scenes(depth, w, h)
    rps, ns = LA_SIZES[size][1]
    batch = g.lookahead_cost_p_batch([(s0, s1) for _, s0, s1 in scenes], (M, M), w, h, M, M, rps, ns)
    hipmod._release()
    _same_results({name: want[name, "P", rps, ns] for name, _, _ in scenes}, {name: batch[i] for i, (name, _, _) in enumerate(scenes)})


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_device_intra_scan_matches_restatement_on_flat_and_striped_blocks(hipmod, depth):
    """x265hip_intra_scan_batch on blocks whose 35 predictions all cost the same (flat block, flat neighbours: equal or at the rails) and on stripes8, composed
    from the pinned intra_pred + sa8d like test_hip_parity's; these are the costs the host's own `<` then decides on"""
    o, g = Orc(depth), hipmod.Hip(depth)
    rng = np.random.default_rng(8700 + depth)
    scenes = {name: (r, s) for name, r, s in _me_scenes(depth)}
    for name in ("flat-mid", "flat-rails", "stripes8"):
        nbr, plane = scenes[name]              # neighbours out of the reference picture, the block out of the source picture
        for n in (8, 16, 32):
            xy = [(int(rng.integers(1, plane.shape[0] - n)), int(rng.integers(1, plane.shape[1] - 2 * n))) for _ in range(5)]
            lines = np.zeros((len(xy), 4 * n + 1), o.pix)
            for i, (y, x) in enumerate(xy):
                lines[i, 0] = nbr[y - 1, x - 1]
                lines[i, 1:2 * n + 1] = np.resize(nbr[y - 1, x:x + 2 * n], 2 * n)
                lines[i, 2 * n + 1:] = np.resize(nbr[y:y + 2 * n, x - 1], 2 * n)
            filt = np.stack([o.intra_filter(n, lines[i]) for i in range(len(xy))])
            got = g.intra_scan(n, lines, filt, plane, xy)
            hipmod._release()
            for i, (y, x) in enumerate(xy):
                want = [o.sa8d(n, plane, (y, x), o.intra_pred(n, mode, filt[i] if o.intra_uses_filtered(n, mode) else lines[i], 1 if n <= 16 else 0), (0, 0))
                        for mode in range(35)]
                assert [int(v) for v in got[i]] == want, (name, n, i)
                if name != "stripes8":
                    assert len(set(want)) == 1, (name, n, want)
                if name == "flat-rails":
                    assert want[0] > 0


def _same_surfaces(got, want):
    n = 0
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for l in want[name]:
            for k, what in enumerate(("origins", "tables", "sub-pel")):
                if want[name][l][k] is None:
                    assert l == 0 and got[name][l][k] is None
                    continue
                assert np.array_equal(got[name][l][k], want[name][l][k]), (name, what, l, np.argwhere(got[name][l][k] != want[name][l][k])[:4])
                n += want[name][l][k].size
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("lam", [0, 180])
@pytest.mark.parametrize("form", range(len(SURFACE_FORMS)))
def test_device_surfaces_match_restatement_on_degenerate_pictures(form, lam):
    """sadsurf_ctu_kernel / sadsurf_ctu16_kernel / sadsurf_ctu16_wide_kernel and the sub-pel kernels (subpel_satd_kernel_lds at 8 and 10 bit): origins, tables and
    the 49 sub-pel entries of every block of every class"""
    import x265_amd.hipprim as hp
    from test_sadsurf import _emul
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    assert _same_surfaces(_surfaces(hp, L, form, lam), _surfaces(hp, _emul(hp), form, lam)) > 10000


@pytest.mark.gpu
def test_device_wide_surfaces_on_five_workgroups_match_restatement_on_degenerate_pictures(monkeypatch):
    """the wide form with each workgroup walking several CTUs out of one region of the pooled buffer (X265HIP_SADSURF_WIDE_GROUPS, read per launch)"""
    import x265_amd.hipprim as hp
    from test_sadsurf import _emul
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    want = _surfaces(hp, _emul(hp), 2, 180)
    monkeypatch.setenv("X265HIP_SADSURF_WIDE_GROUPS", "5")
    assert _same_surfaces(_surfaces(hp, L, 2, 180), want) > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 10])
def test_bound_encoder_is_byte_identical_on_a_degenerate_clip(tmp_path, bits):
    """oracle/_ref/integration/x265_hip_{8,10}bit on the clip of the CPU tier: the reference's bytes, every served value recomputed beside it (X265HIP_VERIFY)"""
    import test_places as tp
    from test_x265_dropin import _need
    ref, hip = _need("x265_%dbit" % bits), _need("x265_hip_%dbit" % bits)
    yuv = str(tmp_path / "clip.yuv")
    _write_clip(yuv)
    want, _ = tp._encode(ref, yuv, CLIP_W, CLIP_H, CLIP_FRAMES, str(tmp_path / "ref.hevc"), {})
    got, err = tp._encode(hip, yuv, CLIP_W, CLIP_H, CLIP_FRAMES, str(tmp_path / "hip.hevc"), {"X265HIP_VERIFY": "1"})
    assert len(want) > 1000 and got == want, "bitstreams differ"
    _served(err)
