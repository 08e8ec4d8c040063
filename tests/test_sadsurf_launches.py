"""How the SAD-surface builder (x265_amd/csrc/surfbuild.hip progress_multi) cuts one pass into launches: more surfaces in a group than a launch has jobs
(kMaxJobs = 16), and one launch's LDS sized by the largest of mixed search ranges.  GPU tier only; the device surfaces against the restatement
(tests/support/libx265hip_emul.so), entry for entry, and the launch count of x265hip_sadsurf_stats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_sadsurf import MX, MY, _emul, _pictures, _read_view      # noqa: E402


def _launches(L):
    st = (C.c_uint64 * 4)()
    L.x265hip_sadsurf_stats(C.byref(st, 0), C.byref(st, 8), C.byref(st, 16), C.byref(st, 24))
    return int(st[2])


def _run_attached_first(hp, L, depth, w, h, buf, stride, rows, srcs, ranges, lam, levels):
    """Source k attached with range ranges[k] before any row of the reference picture is final, then all rows final in one call; -> views"""
    rp = L.x265hip_refpic_create(depth, w, h, stride, MX, MY, rows, buf.ctypes.data)
    assert rp, L.x265hip_last_error()
    sps, sss = [], []
    for s, S in zip(srcs, ranges):
        sp = L.x265hip_srcpic_create(depth, w, h)
        assert sp and L.x265hip_srcpic_upload(sp, s.ctypes.data, s.shape[1]) == 0, L.x265hip_last_error()
        sps.append(sp)
        ss = L.x265hip_sadsurf_attach_levels(sp, rp, S, lam, levels)
        assert ss, L.x265hip_last_error()
        sss.append(ss)
    assert L.x265hip_refpic_rows_final(rp, h) == 0
    assert L.x265hip_refpic_wait(rp) == 0, L.x265hip_last_error()
    views = [_read_view(hp, L, ss, w, h) for ss in sss]
    for ss in sss:
        L.x265hip_sadsurf_release(ss)
    L.x265hip_refpic_wait(rp)
    L.x265hip_refpic_destroy(rp)
    for sp in sps:
        L.x265hip_srcpic_destroy(sp)
    return views


@pytest.mark.gpu
@pytest.mark.parametrize("depth,ranges", [(8, (8, 32)), (10, (8, 16)), (10, (20, 32))])
def test_eighteen_surfaces_of_mixed_ranges_take_two_launches(depth, ranges):
    """18 source pictures attached to one reference picture before any of its rows is final, their ranges alternating; then all rows final in one call: the
    builder's one pass has 18 surfaces in one group and cuts it into launches of 16 and 2 jobs, each sized by the largest range among its jobs — at 10 bit
    once in the LDS form (8 / 16) and once in the wide form (20 / 32).  Every origin and entry of every surface equals the restatement's, the sub-pel tables
    too."""
    import x265_amd.hipprim as hp
    L = hp.lib()
    hp.check(L.x265hip_init(0))
    em = _emul(hp)
    w, h, n = 200, 136, 18
    S = [ranges[k & 1] for k in range(n)]
    levels = 31 if depth == 8 else 30
    buf, stride, rows, srcs = _pictures(w, h, 29, count=n, depth=depth)
    before = _launches(L)
    got = _run_attached_first(hp, L, depth, w, h, buf, stride, rows, srcs, S, 180, levels)
    launches = _launches(L) - before
    want = _run_attached_first(hp, em, depth, w, h, buf, stride, rows, srcs, S, 180, levels)
    for k in range(n):
        assert sorted(got[k]) == sorted(want[k]) == ([0, 1, 2, 3] if depth == 8 else [1, 2, 3])
        for l in got[k]:
            assert np.array_equal(got[k][l][0], want[k][l][0]), ("origins", k, l)
            assert np.array_equal(got[k][l][1], want[k][l][1]), ("tables", k, l)
            if l:
                assert got[k][l][2] is not None and np.array_equal(got[k][l][2], want[k][l][2]), ("sub-pel", k, l)
    assert launches == 2, launches
