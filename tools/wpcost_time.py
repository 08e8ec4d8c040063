#!/usr/bin/env python3
"""Times x265hip_wpcost_* (x265_amd/csrc/wpcost.hip) on the planes of a 1920x1080 picture: the wall time of set_luma / set_chroma (staging memcpy, upload,
the compensation launch; no synchronisation) and of eval with 1 and with 5 candidates (launch, download of the block costs, synchronisation, the host's
totals), and the device time per launch from the context's own events (x265hip_wpcost_stats), for the 960x544 lowres luma and a 960x536 4:2:0 chroma plane,
with and without vectors, 8 and 10 bit.  The time of the reference's own body per analysis is not measured here: the seam prints it (X265HIP_VERBOSE, the
weightp line of an encode with X265HIP_WEIGHTP=0).
    python tools/wpcost_time.py [--calls 30]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class WeightParam(C.Structure):
    _fields_ = [("inputWeight", C.c_int32), ("inputOffset", C.c_int32), ("log2WeightDenom", C.c_int32), ("wtPresent", C.c_int32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    from x265_amd import hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    rng = np.random.default_rng(5)
    lw, ll, cw, ch, m = 960, 544, 960, 536, 48
    for depth in (8, 10):
        dt, pmax = (np.uint8, 255) if depth == 8 else (np.uint16, 1023)
        low = [rng.integers(0, pmax + 1, (ll + 2 * m, lw + 2 * m)).astype(dt) for _ in range(5)]
        chroma = [rng.integers(0, pmax + 1, (ch + 2 * m, cw + 2 * m)).astype(dt) for _ in range(2)]
        ncu = (lw // 8) * (ll // 8)
        intra = rng.integers(100, 4000, ncu).astype(np.int32)
        mvs = rng.integers(-40, 41, (ncu, 2)).astype(np.int32)
        org = lambda b: b.ctypes.data + (m * b.shape[1] + m) * b.itemsize
        ctx = C.c_void_p()
        hp.check(L.x265hip_wpcost_begin(depth, 1, C.byref(ctx)))
        refs = (C.c_void_p * 4)(*[org(p) for p in low[1:]])
        for vectors in (True, False):
            mv = mvs.ctypes.data if vectors else None
            for plane, name in ((0, "luma 960x544"), (1, "chroma 960x536")):
                def set_plane():
                    if plane == 0:
                        hp.check(L.x265hip_wpcost_set_luma(ctx, org(low[0]), refs, lw + 2 * m, lw, ll, intra.ctypes.data, mv))
                    else:
                        hp.check(L.x265hip_wpcost_set_chroma(ctx, 1, org(chroma[0]), org(chroma[1]), cw + 2 * m, cw, ch, mv, lw // 8, ll // 8))
                nb = 0
                line = "%2d bit %-15s %-12s" % (depth, name, "vectors" if vectors else "no vectors")
                for n in (1, 5):
                    cands = (WeightParam * n)(*[WeightParam(60 + i, i - 2, 6, 1) for i in range(n)])
                    set_plane()
                    nb = L.x265hip_wpcost_blocks(ctx, plane)
                    blocks = np.zeros(n * nb, np.uint32)
                    totals = np.zeros(n, np.uint32)
                    for _ in range(3):
                        hp.check(L.x265hip_wpcost_eval(ctx, plane, cands, n, blocks.ctypes.data, totals.ctypes.data))
                    l0, n0 = C.c_uint64(), C.c_uint64()
                    L.x265hip_wpcost_stats(ctx, C.byref(l0), C.byref(n0), None)
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        hp.check(L.x265hip_wpcost_eval(ctx, plane, cands, n, blocks.ctypes.data, totals.ctypes.data))
                    wall = (time.perf_counter() - t0) / a.calls
                    l1, n1 = C.c_uint64(), C.c_uint64()
                    L.x265hip_wpcost_stats(ctx, C.byref(l1), C.byref(n1), None)
                    line += "  eval x%d: kernel %6.1f us, call %.3f ms" % (n, (n1.value - n0.value) * 1e-3 / max(l1.value - l0.value, 1), wall * 1e3)
                # set + the evaluation that waits for it: what opening a plane costs
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    set_plane()
                    t1 = time.perf_counter()
                    hp.check(L.x265hip_wpcost_eval(ctx, plane, cands, 1, blocks.ctypes.data, totals.ctypes.data))
                both = (time.perf_counter() - t0) / a.calls
                print("%s  open (set + first eval): %.3f ms  (%d blocks, total %d)" % (line, both * 1e3, nb, int(totals[0])))
        L.x265hip_wpcost_end(ctx)


if __name__ == "__main__":
    main()
