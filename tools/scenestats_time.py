#!/usr/bin/env python3
"""Times x265hip_scene_stats (x265_amd/csrc/scenestats.hip) on 1920x1080 4:2:0 pictures: device time per call (HIP events around the launch group, clock
X265HIP_CLK_SCENE) and the wall time of the whole call (staging memcpy, upload, kernel, download, copies out), for a noise picture and for a flat one (every
sample of a plane in one bin), in the computeHistograms form (three planes, histograms, with and without the edge plane) and in the --rskip 2 form (one
strided plane, bits only).
    python tools/scenestats_time.py [--calls 20] [--res 1920x1080]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLK_SCENE = 8


def device_time(L):
    spans, ns, by = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.x265hip_device_time(CLK_SCENE, C.byref(spans), C.byref(ns), C.byref(by))
    return spans.value, ns.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--res", default="1920x1080")
    a = ap.parse_args()
    w, h = map(int, a.res.split("x"))
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    rng = np.random.default_rng(5)
    for depth in (8, 10):
        dt, bins, pmax = (np.uint8, 256, 255) if depth == 8 else (np.uint16, 1024, 1023)
        for kind in ("noise", "flat"):
            shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
            planes = [np.ascontiguousarray((rng.integers(0, pmax + 1, s) if kind == "noise" else np.full(s, pmax // 3)).astype(dt)) for s in shapes]
            for form in ("histograms + bits", "histograms", "bits of a strided plane"):
                n = 1 if form.startswith("bits") else 3
                if n == 1:
                    wide = np.zeros((h, w + 64), dt)
                    wide[:, :w] = planes[0]
                    use = [wide]
                else:
                    use = planes
                widths = (C.c_int * 3)(w, w // 2, w // 2)
                heights = (C.c_int * 3)(h, h // 2, h // 2)
                strides = (C.c_int64 * 3)(use[0].shape[1], w // 2, w // 2)
                ptrs = (C.c_void_p * 3)(*([p.ctypes.data for p in use] + [None] * (3 - n)))
                bits = np.zeros((h, w), dt)
                edge = np.zeros(2, np.int32)
                hist = np.zeros((3, bins), np.int32)
                errs = C.c_uint32()

                def call():
                    hp.check(L.x265hip_scene_stats(depth, n, ptrs, widths, heights, strides, planes[0].itemsize, 0, 0, pmax, int(n == 3),
                                                   bits.ctypes.data if "bits" in form else None, w, edge.ctypes.data, hist.ctypes.data if n == 3 else None,
                                                   C.byref(errs), None))
                for _ in range(3):
                    call()
                s0, ns0 = device_time(L)
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                wall = (time.perf_counter() - t0) / a.calls
                s1, ns1 = device_time(L)
                if n == 3:
                    assert int(hist[0].sum()) == w * h and int(hist[1].sum()) == (w // 2) * (h // 2) and errs.value == 0
                    if kind == "flat":
                        assert int(hist[0].max()) == w * h
                print("%2d bit %-5s %dx%d %-24s kernel %6.1f us per call (HIP events, mean of %d launch groups), whole call %.3f ms, %d edge pixels"
                      % (depth, kind, w, h, form + ":", (ns1 - ns0) * 1e-3 / max(s1 - s0, 1), s1 - s0, wall * 1e3, int(edge[1])))


if __name__ == "__main__":
    main()
