"""Every batched entry point with many jobs per call: job i must read off[i] and write out[i], whatever n is.

The per-primitive sweeps of test_hip_parity.py launch one job per call, so a kernel that used off[0] for every job, split a wave
over the wrong number of jobs, let its clamped tail lanes store, dropped the pitch of a dense output or forgot to accumulate across
jobs would pass them.  The launches here (tests/batch_cases.py) have shuffled per-job offsets, pitches that all differ, sentinel
guard cells around every output cell, and are compared exactly with the pinned oracle called once per job.

  entry point                                   family (test id)          what the launches vary
  --------------------------------------------  ------------------------  ----------------------------------------------------------------
  sse_pp_batch, sad_xn_batch (K 3, 4)           wave_packed-{8,10,12}     8 shapes x n = bpw + 1 and 8 bpw + 3; rail jobs (sums above 2^32)
  sse_ss_batch (also as ssd_s, planeB NULL)     wave_packed_int16         the same shapes and counts
  sub_ps, add_ps, addavg, pixelavg_pp,          elementwise-{8,10,12}     2x4, 6x8 (V = 2), 4x4, 12x16, 24x32, 64x64 x n = 7, 67, 530; three
  copy (pp, sp, ps, ss), p2s _batch                                       planes with three pitches and three offset arrays
  sub_ps, sse_pp, sad_xn past grid_for()'s cap  past_the_cap-8            the second trip of the grid-stride loops of ew_kernel, sse_kernel,
                                                                          pixcmp_kernel
  nquant_batch, dequant_scaling_batch,          quant_denoise             sizes 4 .. 32 x n = 7, 67, 530; numSig 0 and numCoeff, both dequant
  denoise_dct_batch                                                       branches with saturation, resSum accumulated over the units
  dct_batch / idct_batch with dst4 = 1          dst4-{8,10,12}            n = 7, 67, 530
  var, transpose, scale1d_128to64,              smallops-{8,10,12}        every size x n = 7, 67, 530; an all-pmax var job
  scale2d_64to32 _batch
  intra_filter_batch, intra_allangs_batch       intra-{8,10,12}           N = 4 .. 32 x count = 7, 67; bLuma 0 and 1; all-pmax and all-zero lines
  interp_batch, taps = 4                        interp4-{8,10,12}         7 chroma shapes x every kind but HV (+ HPS row extension), coeffIdx 0 .. 7
  interp_batch, taps = 8                        interp8-{8,10,12}         the shapes of test_interp_batches x all kinds (+ HPS row extension),
                                                                          coeffIdx 0 .. 3
  pel_filter_chroma_batch                       loopfilter-{8,10,12}      both edge directions x n = 7, 67, 530; the four maskP / maskQ combinations, tc 0 .. 24
  deblock_chroma_batch                          loopfilter-{8,10,12}      the chroma planes of a 200x136 picture: all vertical edges, then all horizontal ones;
                                                                          bs 0 / 1 / 2, per-unit QPs, bypass flags
  sao_apply_batch kinds 0-4,                    loopfilter-{8,10,12}      every 64x64 CTU of the picture (ragged ones too) in one launch; per-job sign buffers in
  sao_stats_batch kinds 0-4                                               one array, signLeft, offsets; stats / count start non-zero
  pixcmp, dct / idct / quant / count_nonzero,   test_parity_batches_at_    test_hip_parity.py's four many-job tests (8 and 10 bit there) run as they
  interp, cpy_shift, copy_cnt, rdoq_cost        twelve_bit                stand at depth 12

The other _batch entry points have their many-job launches in test_hip_parity.py (pixcmp, dct / idct / quant / count_nonzero, residual_chain,
cpy_shift / copy_cnt / blockfill_s / rdoq_cost, the coefficient-scan costs, pel_filter_luma_strong, deblock_luma, sao_apply kind 5, intra_pred,
intra_scan, the motion-estimation and lookahead launches).  weight_pp, weight_sp, sao_sign and dequant_normal take no job list: nothing to batch.

The CPU tier (unmarked) checks the tables themselves: the oracle against an independent numpy restatement, the builder's promises
(distinct shuffled offsets, disjoint guarded destinations, differing pitches), witnesses that each case still reaches the branch it
is there for, and that the batching faults named above — applied to the restatement — are caught by a named case."""
import collections

import numpy as np
import pytest

import batch_cases as bc


@pytest.fixture(scope="module", params=bc.TABLES, ids=lambda t: "%s-%s" % t if t[1] else t[0])
def table(request):
    """(family, depth, promised launch count, [(case, expected outputs)]): built once, shared by both tiers; nothing a test calls on a case changes it."""
    family, depth = request.param
    _, count, gen = bc.FAMILIES[family]
    rows = []
    for c in gen(depth):
        want = c.want()
        if c.big:                       # expected = chunked numpy; the oracle vouches for every 97th job
            for k, idx, val in c.placements(range(0, c.n, 97)):
                assert np.array_equal(want[k][idx], val), (c.label, k, idx)
        rows.append((c, want))
    return family, depth, count, rows


def _mismatches(c, got, want):
    out = []
    for k in c.outs:
        bad = got[k] != want[k]
        if bad.any():
            inside, outside = int((bad & c.cells[k]).sum()), int((bad & ~c.cells[k]).sum())
            out.append((c, "%s[%s]: %d wrong in the jobs' cells, %d sentinel cells overwritten, first at %s" % (
                c.label, k, inside, outside, tuple(int(v) for v in np.argwhere(bad)[0]))))
    return out


def _report(bad, total):
    """Like _report of test_hip_parity.py: every mismatch, grouped by (entry, shape, n), the first few spelled out."""
    if not bad:
        return
    groups = collections.Counter((c.entry, c.shape, c.n) for c, _ in bad)
    pytest.fail("%d mismatches in %d launches; by (entry, shape, n): %s; first: %s" % (len(bad), total, dict(groups.most_common(40)), [m for _, m in bad[:6]]))


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------
def test_tables_keep_the_builder_promises(table):
    family, depth, count, rows = table
    assert len(rows) == count, "the table of %s promises %d launches" % (family, count)
    for c, want in rows:
        for off, pitch in c.offsets:
            assert len(np.unique(off)) == len(off), (c.label, "offsets repeat")
            d = np.diff(off.astype(np.int64))
            assert len(off) < 3 or ((d < 0).any() and (d > 0).any()), (c.label, "offsets are monotone")
            if pitch:
                assert ((off % pitch) % 2 == 1).all(), (c.label, "an origin at even x")
        assert len(set(c.pitches)) == len(c.pitches) and c.width not in c.pitches, (c.label, "pitches", c.pitches, c.width)
        for k in c.outs:
            m, buf = c.cells[k], c.bufs[k]
            assert m.shape == buf.shape and (want[k][~m] == buf[~m]).all(), (c.label, k, "the reference writes outside the cells")
            if family != "loopfilter":              # pure outputs start as sentinels; the loop filters work in place on a picture
                assert (buf[~m] == bc.sentinel(buf.dtype)).all(), (c.label, k, "sentinels")
            if not c.guarded:
                continue
            if m.ndim == 2 and not m[0].any():      # a scattered plane: n separate rectangles, each with a guard band, none at the rim
                pad = np.pad(m, 1)
                corners = m & ~pad[:-2, 1:-1] & ~pad[1:-1, :-2] & ~pad[:-2, :-2] & ~pad[:-2, 2:]
                assert corners.sum() == c.n and not (m[-1].any() or m[:, 0].any() or m[:, -1].any()), (c.label, k, "guard bands")
            elif m.ndim == 1 and not m[0]:           # slots scattered over a 1-D array: n separate runs, sentinels before, between and behind them
                assert (m[1:] & ~m[:-1]).sum() == c.n and not m[-bc.GUARD_ROWS:].any(), (c.label, k, "guard gaps")
            else:                                    # dense: n rows (or elements), then the guard rows
                assert not m[-bc.GUARD_ROWS:].any() and m[:min(c.n, len(m) - bc.GUARD_ROWS)].all(), (c.label, k, "guard rows")


def test_oracle_equals_numpy_restatement(table):
    family, depth, count, rows = table
    bad, n = [], 0
    for c, want in rows:
        if c.restate is None or c.big:              # past_the_cap: the restatement IS the expectation, spot-checked in the fixture
            continue
        n += 1
        bad += _mismatches(c, c.restate(), want)
    _report(bad, n)
    need = {"elementwise": count, "wave_packed": count, "wave_packed_int16": count, "quant_denoise": count, "smallops": len(bc.NS) * (len(bc.SQUARE) + 2)}
    assert n == need.get(family, 0)


def test_cases_reach_their_branches(table):
    """Witnesses from the reference side alone: a case cannot quietly stop exercising what it is there for."""
    family, depth, count, rows = table
    seen = collections.defaultdict(set)
    for c, want in rows:
        w = c.witness(want)
        if c.entry == "add_ps":
            assert w["clips_low"] and w["clips_high"], c.label
        if c.entry in ("sse_ss", "ssd_s") or (c.entry == "sse_pp" and depth == 12):
            assert w["above_2^32"] or c.shape != "64x64", c.label
        if c.entry == "nquant":
            assert w["numSig_0"] and w["numSig_all"], c.label
        if c.entry == "dequant_scaling":
            assert w["saturates"], c.label
            seen["dequant"].add(w["branch"])
        if c.entry == "denoise_dct":
            assert w["zeroed"] and w["resSum_changes"] and w["start_nonzero"], c.label
        if c.entry.startswith("interp"):
            assert w["coeffIdx_0"], c.label
        if c.entry == "pel_filter_chroma":
            assert w["mask_combos"] == 4 and w["filtered"], c.label
        if c.entry == "deblock_chroma":
            assert w["filtered"] and w["skipped"] and w["bypassed"], c.label
        if c.entry == "sao_apply":
            assert w["changed"] and w["signs_written"], c.label
        if c.entry == "sao_stats" and c.shape != "kind0":
            assert (w["classes"] > 0).all(), (c.label, w["classes"])      # every edge class 0 .. 4 counted over the launch
    if family == "quant_denoise":
        assert seen["dequant"] == {"shift>per", "shift<=per"}


def test_sao_job_layouts_match_the_abi():
    import ctypes as C
    from x265_amd import hipprim as hp
    for dt, st in ((bc.SAO_JOB, hp.SaoJob), (bc.SAO_STATS_JOB, hp.SaoStatsJob)):
        assert dt.itemsize == C.sizeof(st) and [dt.fields[f[0]][1] for f in st._fields_] == [getattr(st, f[0]).offset for f in st._fields_]


def test_batching_faults_are_caught():
    """The faults of the issue, applied to the numpy restatement: the named case tells each from the oracle."""
    for c, mut in ((bc.sad_xn_case(3, 8, 8, 8, bc.jobs_per_wave(8, 8) + 1, 1), "offF[0]"),          # offA[jc / divA] -> offA[0]
                   (bc.ew_case("sub_ps", 10, 12, 16, 7, 2), "offD[0]"),                              # offD[job] -> offD[0] in ew_kernel
                   (bc.ew_case("add_ps", 8, 6, 8, 7, 3), "off0[0]"),
                   (bc.sse_case("sse_pp", 8, 8, 8, bc.jobs_per_wave(8, 8) + 1, 4), "tail lanes write"),   # jobOk dropped from sse_kernel's store
                   (bc.sse_case("sse_ss", None, 16, 16, 5, 5), "offA[0]"),
                   (bc.denoise_case(8, 7, 6), "resSum of one unit")):                                 # no accumulation of resSum across units
        want = c.oracle()
        assert not _mismatches(c, c.restate(), want), c.label
        assert _mismatches(c, c.restate(mut), want), (c.label, mut)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hipmod():
    import hipbackend
    from x265_amd import hipprim as hp
    assert hp.lib().x265hip_device_count() > 0, "no HIP device: the -m gpu tests need a real MI355X"
    hp.check(hp.lib().x265hip_init(0))
    return hipbackend


def _launch(c):
    """Upload the case's arrays, call its entry point through the C ABI, return the output arrays it names."""
    from x265_amd import hipprim as hp
    dev = {k: hp.DevBuf(v) for k, v in c.bufs.items()}
    hp.check(getattr(hp.lib(), c.fn)(*[dev[a.name].ptr if isinstance(a, bc.Buf) else a for a in c.args]))
    return {k: dev[k].get() for k in c.outs}


@pytest.mark.gpu
def test_many_job_launches_match_oracle(table, hipmod):
    family, depth, count, rows = table
    bad, launched = [], 0
    for c, want in rows:
        try:
            got = _launch(c)
        except Exception as e:  # noqa: BLE001 - report and continue
            bad.append((c, "%s !! %s" % (c.label, str(e)[:80])))
            continue
        launched += 1
        bad += _mismatches(c, got, want)
    _report(bad, launched)
    assert launched == count, "%d of the %d launches the table of %s promises were compared" % (launched, count, family)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["test_pixcmp_batches", "test_transform_batches", "test_interp_batches", "test_misc_batches"])
def test_parity_batches_at_twelve_bit(hipmod, name):
    """The many-job tests of test_hip_parity.py (parametrised there over 8 and 10 bit) as they stand, at depth 12; each takes under a second."""
    import test_hip_parity
    getattr(test_hip_parity, name)(hipmod, 12)
