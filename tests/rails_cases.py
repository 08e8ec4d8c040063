"""Inputs at the pixel rails and at both ends of the QP range, shared by tests/test_cuserve_rails.py: residual patterns as (source, prediction) planes, the
QP list, levels "made elsewhere" for the inverse half, and the chain form of cuserve.hip that serves a unit.

Every pattern is a function of a plane's size, the size `n` of the transform units it is meant for (the pattern repeats per n x n unit, so every unit of that
size sees it whole) and the bit depth.  Source and prediction are the positive and the negative part of the residual, so a residual of +-pmax puts one of
them on each rail."""
import numpy as np

# the block kinds; "same:*" have source == prediction (every unit numSig == 0)
KINDS = ("rail+", "rail-", "same:random", "same:zero", "same:max", "rail+dither", "checker", "cols1", "cols2", "rows1", "rows2",
         "basis:1,1", "basis:N-1,N-1", "basis:1,0", "spike+0", "spike-1", "spike+2", "spike-3", "spike-0", "spike+1", "spike-2", "spike+3",
         "clip-recon:hi", "clip-recon:lo")
BARE_KINDS = tuple(k for k in KINDS if not k.startswith(("same", "clip-recon")))      # the kinds that are a bare residual


def qps(depth):
    """internal QPs (as test_cuserve._job_header takes them): the low end, where levels clip, and the last steps of the range"""
    bd = 6 * (depth - 8)
    return (0, 1, 5, 6, 11, 12, 17, 18, bd + 4, bd + 46, bd + 48, bd + 51)


def dct_sign(n, k):
    """the signs of row k of the n-point DCT-II matrix (cos((2j + 1) k pi / 2n)): the +-1 vector that maximises coefficient k"""
    return np.where(np.cos((2 * np.arange(n) + 1) * k * np.pi / (2 * n)) >= 0, 1, -1)


def dither(n, depth, seed):
    """(source, prediction) of one n x n unit: source in [pmax - 3, pmax], prediction in [0, 3]"""
    rng = np.random.default_rng([seed, depth, n])
    pmax = (1 << depth) - 1
    return pmax - rng.integers(0, 4, (n, n)), rng.integers(0, 4, (n, n))


def planes(kind, h, w, n, depth, seed=1):
    """(source, prediction) of an h x w plane, int64 in [0, pmax]"""
    pmax = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if kind.startswith("same"):
        what = kind.split(":")[1]
        s = np.random.default_rng([seed, depth, h, w]).integers(0, pmax + 1, (h, w)) if what == "random" else np.full((h, w), 0 if what == "zero" else pmax)
        return s, s.copy()
    if kind == "rail+dither":
        s, p = dither(n, depth, seed)
        return np.tile(s, (h // n, w // n)), np.tile(p, (h // n, w // n))
    if kind.startswith("clip-recon"):
        step = np.random.default_rng([seed, depth, h, w, 7]).integers(0, 7, (h, w))
        if kind.endswith("hi"):
            return pmax - step, np.full((h, w), pmax)
        return step, np.zeros((h, w), np.int64)
    if kind == "rail+":
        r = np.full((h, w), pmax)
    elif kind == "rail-":
        r = np.full((h, w), -pmax)
    elif kind == "checker":
        r = pmax * (1 - 2 * ((xx + yy) & 1))
    elif kind in ("cols1", "cols2"):
        r = pmax * (1 - 2 * ((xx // int(kind[-1])) & 1))
    elif kind in ("rows1", "rows2"):
        r = pmax * (1 - 2 * ((yy // int(kind[-1])) & 1))
    elif kind.startswith("basis"):
        k, k2 = (n - 1 if v == "N-1" else int(v) for v in kind.split(":")[1].split(","))
        r = pmax * np.tile(np.outer(dct_sign(n, k), dct_sign(n, k2)), (h // n, w // n))
    elif kind.startswith("spike"):
        corner = int(kind[-1])
        cy, cx = (n - 1) * (corner >> 1), (n - 1) * (corner & 1)
        r = np.where((yy % n == cy) & (xx % n == cx), pmax if kind[5] == "+" else -pmax, 0)
    else:
        raise ValueError(kind)
    return np.maximum(r, 0), np.maximum(-r, 0)


def residual(kind, n, depth, seed=1):
    """the n x n residual of a bare kind, int16"""
    s, p = planes(kind, n, n, n, depth, seed)
    return np.ascontiguousarray((s - p).astype(np.int16))


def job_pixels(kind, dims, tiles, depth, seed=1):
    """the pixel block of a job: the sources of Y, Cb, Cr, then the predictions; dims [(h, w)] and tiles [n] per plane; seed: one, or one per plane"""
    dt = np.uint8 if depth == 8 else np.uint16
    seeds = seed if isinstance(seed, (list, tuple)) else [seed] * len(dims)
    both = [planes(kind, h, w, n, depth, sd) for (h, w), n, sd in zip(dims, tiles, seeds)]
    return np.ascontiguousarray(np.concatenate([s.astype(dt).ravel() for s, _ in both] + [p.astype(dt).ravel() for _, p in both]))


# ---- levels made elsewhere (what Quant::rdoQuant may hand to the inverse half) ------------------------------------------------------------------------

LEVEL_SETS = ("random", "all+", "all-", "dc+", "dc-", "last+", "last-", "dense1%")


def level_limit(scale, shift):
    """the largest |level| whose dequantisation is defined in the reference: dequant_normal computes level * scale + add in int, add = 1 << (shift - 1)"""
    return min(32767, ((1 << 31) - 1 - (1 << (shift - 1))) // scale)


def levels(name, n, limit, seed=1):
    """n * n int16 levels of the named set, every |level| <= limit (-32768 where the limit allows it)"""
    rng = np.random.default_rng([seed, n, limit])
    lo = -32768 if limit == 32767 else -limit
    lv = np.zeros(n * n, np.int64)
    if name == "random":
        lv = rng.integers(lo, limit + 1, n * n)
    elif name == "all+":
        lv[:] = limit
    elif name == "all-":
        lv[:] = lo
    elif name in ("dc+", "dc-"):
        lv[0] = limit if name == "dc+" else lo
    elif name in ("last+", "last-"):
        lv[-1] = limit if name == "last+" else lo
    elif name == "dense1%":
        at = rng.choice(n * n, max(2, n * n // 100), replace=False)
        lv[at] = rng.integers(lo, limit + 1, at.size)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(lv.astype(np.int16))


# ---- which chain of x265_amd/csrc/cuserve.hip serves a unit (run_tiles, with the team form on: the default) ---------------------------------------------

CHAINS = ("team32", "tile32", "tile16", "tile8", "solo16")


def chain_of(plane, n, units_in_plane):
    """32x32 luma units go to the four-wave team chain; a chroma plane's lone 16x16 unit (a 32x32 CU at 4:2:0) to the solo chain; everything else to
    tile_chain<n>: 32x32 chroma (4:4:4), 16x16 luma and chroma of more than one unit, 8x8 chroma"""
    if n == 32:
        return "team32" if plane == 0 else "tile32"
    if n == 16:
        return "solo16" if plane and units_in_plane == 1 else "tile16"
    return "tile8"
