#!/usr/bin/env python3
"""Times x265hip_picture_hash (x265_amd/csrc/pichash.hip) on 1920x1080 4:2:0 pictures: device time per call (HIP events around the launch, clock
X265HIP_CLK_PICHASH) and the wall time of the whole call (staging memcpy, upload, kernel, download of the result words), for a noise picture and for a flat
one (every workgroup of a plane leaves the same words: the atomics are one per workgroup, so flat must not be slower), for the CRC and the checksum, in the
per-row form (a band of 64 luma rows, three planes: what a one-slice encode asks per CTU row) and in the whole-picture form (--slices > 1).  The time of the
reference's own body per row is not measured here: the seam prints it (X265HIP_VERBOSE, the pichash line of an encode with X265HIP_PICHASH=0).
    python tools/pichash_time.py [--calls 50] [--res 1920x1080]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLK_PICHASH = 9


class HashPlane(C.Structure):
    _fields_ = [("plane", C.c_void_p), ("stride", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("y0", C.c_int32)]


def device_time(L):
    spans, ns, by = C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.x265hip_device_time(CLK_PICHASH, C.byref(spans), C.byref(ns), C.byref(by))
    return spans.value, ns.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--res", default="1920x1080")
    a = ap.parse_args()
    w, h = map(int, a.res.split("x"))
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    rng = np.random.default_rng(5)
    pad = 160                                          # the reconstructed picture's rows are wider than the picture
    for depth in (8, 10):
        dt, pmax = (np.uint8, 255) if depth == 8 else (np.uint16, 1023)
        for kind in ("noise", "flat"):
            planes = []
            for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
                buf = np.zeros((s[0], s[1] + pad), dt)
                buf[:, :s[1]] = rng.integers(0, pmax + 1, s) if kind == "noise" else pmax // 3
                planes.append(buf)
            for method, mname in ((2, "CRC"), (3, "checksum")):
                for form, rows in (("row of 64", 64), ("whole picture", h)):
                    arr = (HashPlane * 3)()
                    for k, p in enumerate(planes):
                        arr[k] = HashPlane(p.ctypes.data + (64 >> (k > 0)) * p.strides[0], p.shape[1], p.shape[1] - pad, rows >> (k > 0), 64 >> (k > 0))
                    if rows == h:
                        for k, p in enumerate(planes):
                            arr[k].plane, arr[k].y0 = p.ctypes.data, 0
                    state = np.zeros(3, np.uint32)

                    def call():
                        state[:] = 0xFFFF if method == 2 else 0
                        hp.check(L.x265hip_picture_hash(depth, method, arr, 3, state.ctypes.data, None))
                    for _ in range(3):
                        call()
                    s0, ns0 = device_time(L)
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        call()
                    wall = (time.perf_counter() - t0) / a.calls
                    s1, ns1 = device_time(L)
                    print("%2d bit %-5s %dx%d %-8s %-14s kernel %6.1f us per call (HIP events, mean of %d launches), whole call %.3f ms, state %s"
                          % (depth, kind, w, h, mname, form + ":", (ns1 - ns0) * 1e-3 / max(s1 - s0, 1), s1 - s0, wall * 1e3, " ".join("%08x" % v for v in state)))


if __name__ == "__main__":
    main()
