"""What the tests of the lookahead's HME levels (tests/test_lookahead_hme.py) and tools/lookahead_hme_time.py share: the planes of Lowres::create / init with
bEnableHME built in numpy, the two level descriptions of x265hip_lookahead_cost_hme_batch, and the lookahead's cost table on the device."""
import numpy as np

MARGIN = 80                                             # of the pictures and of the half-resolution planes, as in the other lookahead tests


def _downscale(src, oy, ox, w, h):
    """frame_init_lowres_core (common/pixel.cpp:605-628): the four half-pel planes of a w x h downscale of src at origin (oy, ox)"""
    s = src.astype(np.int64)
    r = [s[oy + k:oy + k + 2 * h:2] for k in range(3)]

    def col(rows, k):
        return rows[:, ox + k:ox + k + 2 * w:2]

    def filt(a, b, c, d):
        return ((((a + b + 1) >> 1) + ((c + d + 1) >> 1) + 1) >> 1)
    return [filt(col(r[0], 0), col(r[1], 0), col(r[0], 1), col(r[1], 1)), filt(col(r[0], 1), col(r[1], 1), col(r[0], 2), col(r[1], 2)),
            filt(col(r[1], 0), col(r[2], 0), col(r[1], 1), col(r[2], 1)), filt(col(r[1], 1), col(r[2], 1), col(r[1], 2), col(r[2], 2))]


def host_planes(pic, W, H):
    """Lowres::create + init with bEnableHME (common/lowres.cpp:50-161, :293-316) of one padded picture: the half-resolution buffer (4 planes of
    `planesize`), the quarter-resolution buffer (4 planes of planesize / 2, stride lumaStride / 2, origin at padoffset / 2) and the geometry"""
    dt = pic.dtype
    lw, lh = ((W // 2 + 7) // 8) * 8, ((H // 2 + 7) // 8) * 8
    stride = lw + 2 * MARGIN
    stride += (32 - stride % 32) % 32
    rows = lh + 2 * MARGIN
    planesize, padoffset = stride * rows, stride * MARGIN + MARGIN
    buf = np.zeros((4, rows, stride), dt)
    for k, p in enumerate(_downscale(pic, MARGIN, MARGIN, lw, lh)):
        buf[k, :, :lw + 2 * MARGIN] = np.pad(p, MARGIN, mode="edge")
    # the quarter resolution is the same filter over half-resolution plane 0, borders included (its right and bottom taps reach into them)
    s2, m2 = stride // 2, MARGIN // 2
    low = np.zeros((4, planesize // 2), dt)
    org = padoffset // 2
    for k, p in enumerate(_downscale(buf[0], MARGIN, MARGIN, lw // 2, lh // 2)):
        ext = np.pad(p, m2, mode="edge")
        view = low[k, org - m2 * s2 - m2:]
        for y in range(ext.shape[0]):
            view[y * s2:y * s2 + ext.shape[1]] = ext[y]
    geom = dict(stride=stride, lw=lw, lh=lh, planesize=planesize, padoffset=padoffset, W8=lw // 8, H8=lh // 8, W4=(lw // 2 + 7) // 8, H4=(lh // 2 + 7) // 8)
    return np.ascontiguousarray(buf.reshape(-1)), np.ascontiguousarray(low.reshape(-1)), geom


def mvcost_table(L, depth, cache={}):
    from hipbackend import MVCOST_HALF
    from x265_amd.hipprim import DevBuf, check
    if depth not in cache:
        tab = np.zeros(2 * MVCOST_HALF + 1, np.uint16)
        check(L.x265hip_mvcost_table(12 + 6 * (depth - 8), depth, tab.ctypes.data, MVCOST_HALF))
        cache[depth] = DevBuf(tab)
    return cache[depth].at(MVCOST_HALF)


def levels_of(hp, geom, methods, ranges, rows8, rows4, n):
    lv1 = hp.LookaheadHmeLevel(geom["stride"], geom["planesize"], geom["padoffset"], geom["W8"], geom["H8"], methods[1], ranges[1], rows8, n)
    lv0 = hp.LookaheadHmeLevel(geom["stride"] // 2, geom["planesize"] // 2, geom["padoffset"] // 2, geom["W4"], geom["H4"], methods[0], ranges[0], rows4, n)
    return lv0, lv1
