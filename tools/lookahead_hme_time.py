"""Kernel and call time of the lookahead's two HME levels (x265hip_lookahead_cost_hme_batch) for a batch of 1080p (frame, reference) pairs, per method pair,
beside the one-level entry (HEX at range 16) that non-HME encodes launch.  Device time = HIP events around the launches of one batch (level 0 + level 1);
call time = wall clock of the same calls including the final synchronise.  Not the contract bench.
    python tools/lookahead_hme_time.py [--pairs 8] [--iters 10]      (DEPTH=10 for the 16-bit kernels)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from x265_amd import hipprim as hp                      # noqa: E402
from x265_amd.hipprim import DevBuf, check              # noqa: E402
import hme_planes as t                                  # noqa: E402  (the planes of Lowres::init with bEnableHME, in numpy)

NAMES = {0: "dia", 1: "hex", 2: "umh", 3: "star"}
PAIRS = [((1, 2), (16, 32)), ((1, 1), (16, 32)), ((0, 1), (16, 32)), ((2, 2), (16, 32)), ((2, 3), (16, 32)), ((3, 3), (16, 32))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    L = hp.lib()
    check(L.x265hip_init(0))
    depth = int(os.environ.get("DEPTH", "8"))
    W, H = 1920, 1080
    from cases import lookahead_scene
    s0, s1, m = lookahead_scene(depth, 4321, H, W, t.MARGIN)
    host = [t.host_planes(p, W, H) for p in (s0, s1)]
    geom = host[0][2]
    bufs, lows = [DevBuf(h[0]) for h in host], [DevBuf(h[1]) for h in host]
    W8, H8, W4, H4 = geom["W8"], geom["H8"], geom["W4"], geom["H4"]
    n, n1, n0 = a.pairs, W8 * H8, W4 * H4
    icost = DevBuf(np.full(n1, 1 << 20, np.int32))
    mv = t.mvcost_table(L, depth)
    out1 = [(DevBuf.zeros((2 * n1,), np.int32), DevBuf.zeros((n1,), np.int32), DevBuf.zeros((n1,), np.uint16), DevBuf.zeros((H8,), np.int32),
             DevBuf.zeros((n1,), np.uint64)) for _ in range(n)]
    out0 = [(DevBuf.zeros((2 * n0,), np.int32), DevBuf.zeros((n0,), np.int32), DevBuf.zeros((n0,), np.uint64)) for _ in range(n)]
    p0, p1, pold = (hp.LookaheadHmePair * n)(), (hp.LookaheadHmePair * n)(), (hp.LookaheadPair * n)()
    for i in range(n):
        p0[i].fenc, p0[i].ref = lows[1].at(geom["padoffset"] // 2), lows[0].at(geom["padoffset"] // 2)
        p0[i].mvs, p0[i].mvCosts, p0[i].sync = out0[i][0].ptr, out0[i][1].ptr, out0[i][2].ptr
        for p in (p1[i], pold[i]):
            p.fenc, p.ref, p.intraCost = bufs[1].at(geom["padoffset"]), bufs[0].at(geom["padoffset"]), icost.ptr
            p.mvs, p.mvCosts, p.lowresCosts, p.rowSatds, p.sync = out1[i][0].ptr, out1[i][1].ptr, out1[i][2].ptr, out1[i][3].ptr, out1[i][4].ptr
        p1[i].lowerMvs, p1[i].lowerMvCosts, p1[i].lowerCount = out0[i][0].ptr, out0[i][1].ptr, n0
    d0, d1, dold = (DevBuf(np.frombuffer(bytes(x), np.uint8)) for x in (p0, p1, pold))
    est = DevBuf.zeros((4 * n,), np.int64)
    epoch = [0x100000]

    def measure(fn):
        fn()
        check(L.x265hip_stream_sync(None))
        tm = hp.Timer(None)
        tm.start()
        for _ in range(a.iters):
            fn()
        dev = tm.stop_ms() / a.iters
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
            check(L.x265hip_stream_sync(None))
        return dev, (time.perf_counter() - t0) * 1e3 / a.iters

    def one_level():
        epoch[0] += 1
        check(L.x265hip_lookahead_cost_p_batch(depth, dold.ptr, n, geom["stride"], geom["planesize"], W8, H8, H8, 1, mv, epoch[0], est.ptr, None))
    dev, call = measure(one_level)
    print(json.dumps(dict(what="one level (non-HME launch)", depth=depth, pairs=n, grid=[W8, H8], device_ms=round(dev, 3), call_ms=round(call, 3))))
    for methods, ranges in PAIRS:
        lv0, lv1 = t.levels_of(hp, geom, methods, ranges, H8, H4, 1)

        def two_levels():
            epoch[0] += 1
            check(L.x265hip_lookahead_cost_hme_batch(depth, d0.ptr, n, 0, C.byref(lv0), None, mv, epoch[0], est.ptr, None))
            check(L.x265hip_lookahead_cost_hme_batch(depth, d1.ptr, n, 1, C.byref(lv1), C.byref(lv0), mv, epoch[0], est.ptr, None))

        def level0():
            epoch[0] += 1
            check(L.x265hip_lookahead_cost_hme_batch(depth, d0.ptr, n, 0, C.byref(lv0), None, mv, epoch[0], est.ptr, None))
        dev0, _ = measure(level0)
        dev, call = measure(two_levels)
        assert not est.get().reshape(n, 4)[:, 3].any()
        print(json.dumps(dict(what="hme %s,%s ranges %d,%d" % (NAMES[methods[0]], NAMES[methods[1]], ranges[0], ranges[1]), depth=depth, pairs=n, grids=[[W4, H4], [W8, H8]],
                              level0_device_ms=round(dev0, 3), device_ms=round(dev, 3), call_ms=round(call, 3))))


if __name__ == "__main__":
    main()
