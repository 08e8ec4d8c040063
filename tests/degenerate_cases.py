"""Seeded pictures full of exact ties and rail values for tests/test_degenerate_pictures.py; a module beside tests/cases.py (whose generators and rng
streams it leaves alone) built on that module's scenes."""
import numpy as np

from cases import lookahead_scene, me_scene, me_scene_yuv


def degenerate_scenes(depth, shape, seed, margin=80, lookahead=False, chroma=False):
    """Pictures on which many candidates of a search cost exactly the same, or on which every sum sits at its rail: what black frames, letterbox
    bars, static graphics and periodic textures give an encoder.  Returns a list of (name, reference, source); shape = (H, W) of the picture area.
    With pmax the largest sample value:
      flat-mid    both pictures pmax // 2 everywhere
      flat-rails  reference 0, source pmax
      stripes8    (x % 8 < 4) * pmax, the source half a period (4 columns) further: the equal minima lie at +-4, +-12, ...
      checker16   ((x // 8 + y // 8) & 1) * pmax, the source 8 rows further
      railnoise   independent draws from {0, pmax}: no ties, saturating sums
      letterbox   an me_scene pair whose top and bottom 48 rows (a quarter of the height in pictures below 128 rows), and the margins beyond
                  them, are 16 << (depth - 8) in both pictures
    The planes are me_scene's: (H + 2 margin, W + 2 margin), the pattern running through the margins.  lookahead=True gives lookahead_scene's
    instead (the picture area padded by replication, 8 more columns on the right) with the periods doubled, stripes16 and checker32: a period
    below 16 luma samples averages to a flat picture in the half-resolution planes.  chroma=True returns (Y, Cb, Cr) triples in me_scene_yuv's
    layout, the chroma planes flat or periodic like the luma (letterbox: the bars are black, chroma at mid level)."""
    H, W = shape
    m = margin
    pmax = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    per = 16 if lookahead else 8
    rng = np.random.default_rng(seed)

    def finish(p, mm):
        p = np.asarray(p).astype(dt)
        return np.ascontiguousarray(np.pad(p, ((mm, mm), (mm, mm + 8)), mode="edge") if lookahead else p)

    def patterns(h, w, mm):
        rows, cols = (h, w) if lookahead else (h + 2 * mm, w + 2 * mm)
        yy, xx = np.mgrid[0:rows, 0:cols]
        half = per // 2
        flat = lambda v: np.full((rows, cols), v, np.int64)        # noqa: E731
        out = [("flat-mid", flat(pmax // 2), flat(pmax // 2)),
               ("flat-rails", flat(0), flat(pmax)),
               ("stripes%d" % per, (xx % per < half) * pmax, ((xx - half) % per < half) * pmax),
               ("checker%d" % (2 * per), ((xx // per + yy // per) & 1) * pmax, ((xx // per + (yy - per) // per) & 1) * pmax),
               ("railnoise", rng.integers(0, 2, (rows, cols)) * pmax, rng.integers(0, 2, (rows, cols)) * pmax)]
        return [(name, finish(r, mm), finish(s, mm)) for name, r, s in out]

    def bars(p, h, mm, value):
        bar = (48 if H >= 128 else H // 4) * h // H
        p = p.copy()
        p[:mm + bar] = value
        p[mm + h - bar:] = value
        return p

    black = 16 << (depth - 8)
    if chroma:
        assert not lookahead
        luma, cb, cr = patterns(H, W, m), patterns(H // 2, W // 2, m // 2), patterns(H // 2, W // 2, m // 2)
        scenes = [(y[0], (y[1], b[1], r[1]), (y[2], b[2], r[2])) for y, b, r in zip(luma, cb, cr)]
        ref, src, _ = me_scene_yuv(depth, seed, H, W, m)
        mid = 1 << (depth - 1)
        lb = [tuple(bars(p, H >> (k > 0), m >> (k > 0), mid if k else black) for k, p in enumerate(t)) for t in (ref, src)]
        return scenes + [("letterbox", lb[0], lb[1])]
    scenes = patterns(H, W, m)
    if lookahead:
        ref, src, _ = lookahead_scene(depth, seed, H, W, m)
    else:
        ref, src, _ = me_scene(depth, seed, H, W, m)
    return scenes + [("letterbox", bars(ref, H, m, black), bars(src, H, m, black))]
