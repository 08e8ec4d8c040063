"""Random encoder-option sets through the x265-side bindings (tools/fuzz_encoder.py): for each pinned seed the reference encoder and the bound
encoder get the same drawn clip (size, chroma format, fade) and the same drawn options (preset, search method, reference count, B structure,
rate control, CTU / TU sizes, slices, WPP, tunes ...) and must produce the same bytes.  The seeds below were picked from a sweep of 200 for what
they cover and for running in about a second each; the whole sweep is clean (2 of 200 are not test cases: one the reference rejects, one where
the reference's own output moves when a 2 ms sleep is added to FrameFilter::processPostRow with every seam off — the fuzzer detects both).

CPU tier: oracle/_ref/x265_emul_8bit (the C ABI emulated by the oracle — test infrastructure).  GPU tier: oracle/_ref/integration/x265_hip_8bit."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref")

CPU_SEEDS = [19, 29, 33, 38, 40, 42, 45, 47, 50, 54, 59, 61, 63, 64, 65, 70, 74, 79, 82, 83, 84, 86, 90, 91, 95, 100, 101, 106, 109, 114, 130, 136, 145, 161, 162, 181]
GPU_SEEDS = [19, 29, 40, 45, 59, 61, 63, 64, 70, 74, 82, 84, 86, 95, 109, 130, 136, 145, 162, 181]


def _need(name):
    # the product's integration builds (reference objects + the binding + libx265hip.so) live in oracle/_ref/integration, the reference alone and the
    # emulated-ABI test binaries in oracle/_ref
    p = os.path.join(REF, "integration", name) if "_hip" in name else os.path.join(REF, name)
    if not os.path.exists(p):
        pytest.skip("%s not built (needs /root/reference at build time: make -C oracle ref emul; make -C integration hip)" % name)
    return p


def _check(seed, bound, tmp_path, bits=8):
    import fuzz_encoder as fz
    r = fz.run_case(fz.draw(seed), bound, _need("x265_%dbit" % bits), str(tmp_path), bits=bits)
    assert r["encoded"], "seed %d is pinned as a case the reference encodes: %s" % (seed, r)
    if "reference_timing_dependent" in r:
        pytest.skip("seed %d: the reference's own output moved under a timing perturbation with every seam off (%s)" % (seed, r["reference_timing_dependent"]))
    assert r["ok"], "seed %d: bitstreams differ\n%s" % (seed, r["cmd"])
    return r


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_random_option_set_is_byte_identical_with_emulated_abi(tmp_path, seed):
    _check(seed, _need("x265_emul_8bit"), tmp_path)


# Explicit cases (not drawn): option COMBINATIONS the table only ever draws one at a time.  The first two are round 4's advisor finding — with
# --max-tu-size 16 and --tu-inter-depth 3 / 4 a 32x32 CU's residual tree goes below the CU job's smallest transform size, and the CU's final sse / psy answers
# must not be put together from the job's 16x16 units (x265_hip_cuserve.cpp final_sum); run under X265HIP_VERIFY, which aborts on a wrong served value.
EXPLICIT = [
    dict(width=416, height=240, frames=10, csp="i420", fade=False, seed=9001, args=["--preset", "medium", "--max-tu-size", "16", "--tu-inter-depth", "3", "--rdoq-level", "0", "-F", "2", "--pools", "4"]),
    dict(width=416, height=240, frames=10, csp="i420", fade=False, seed=9002, args=["--preset", "medium", "--max-tu-size", "16", "--tu-inter-depth", "4", "--tu-intra-depth", "4", "-F", "2", "--pools", "4"]),
    dict(width=352, height=288, frames=8, csp="i420", fade=False, seed=9003, args=["--preset", "fast", "--max-tu-size", "8", "--tu-inter-depth", "2", "-F", "1", "--pools", "4"]),
    dict(width=416, height=240, frames=8, csp="i420", fade=False, seed=9004, args=["--preset", "medium", "--ctu", "32", "--max-tu-size", "16", "--tu-inter-depth", "2", "--psy-rd", "0", "-F", "2", "--pools", "4"]),
]


def _explicit(case, bound, tmp_path):
    import fuzz_encoder as fz
    os.environ["X265HIP_VERIFY"] = "1"
    try:
        r = fz.run_case(case, bound, _need("x265_8bit"), str(tmp_path), bits=8)
    finally:
        del os.environ["X265HIP_VERIFY"]
    assert r["encoded"], r
    assert r["ok"], "explicit case %d: bitstreams differ\n%s" % (case["seed"], r["cmd"])


@pytest.mark.parametrize("case", EXPLICIT, ids=lambda c: str(c["seed"]))
def test_explicit_option_combination_is_byte_identical_with_emulated_abi(tmp_path, case):
    _explicit(case, _need("x265_emul_8bit"), tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXPLICIT, ids=lambda c: str(c["seed"]))
def test_explicit_option_combination_is_byte_identical_on_gpu(tmp_path, case):
    _explicit(case, _need("x265_hip_8bit"), tmp_path)


MAIN10_SEEDS = [202, 203, 205, 206, 207, 209, 210, 213, 214, 217]


@pytest.mark.parametrize("seed", MAIN10_SEEDS)
def test_random_option_set_main10_with_emulated_abi(tmp_path, seed):
    _check(seed, _need("x265_emul_10bit"), tmp_path, bits=10)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", MAIN10_SEEDS[:6])
def test_random_option_set_main10_on_gpu(tmp_path, seed):
    _check(seed, _need("x265_hip_10bit"), tmp_path, bits=10)


MAIN12_SEEDS = [700, 703, 705, 709, 713, 717, 719]


@pytest.mark.parametrize("seed", MAIN12_SEEDS)
def test_random_option_set_main12_with_emulated_abi(tmp_path, seed):
    _check(seed, _need("x265_emul_12bit"), tmp_path, bits=12)


def test_draw_is_a_pure_function_of_the_seed():
    import fuzz_encoder as fz
    assert fz.draw(7) == fz.draw(7) and fz.draw(7) != fz.draw(8)
    kinds = {fz.draw(s)["csp"] for s in range(60)}
    assert kinds == {"i420", "i422", "i444", "i400"}
    # the rules that keep draws inside what the reference encodes deterministically (tools/fuzz_encoder.py explains each)
    for s in range(1200):
        c = fz.draw(s)
        a = c["args"]
        if c["height"] <= 64:
            assert "--no-weightp" in a and "--no-weightb" in a, (s, a)       # (presets slower / veryslow imply --weightb: seed 1018)
        if "--vbv-bufsize" in a:
            assert a[a.index("-F") + 1] == "1" and "--no-wpp" in a, (s, a)
        if "--bframes" in a:
            la = [int(a[i + 1]) for i, w in enumerate(a) if w == "--rc-lookahead"]
            default = {"ultrafast": 5, "superfast": 10, "veryfast": 15, "faster": 15, "fast": 15, "medium": 20, "slow": 25, "slower": 40, "veryslow": 40}[a[1]]
            assert (la[-1] if la else default) > int(a[a.index("--bframes") + 1]), (s, a)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_random_option_set_is_byte_identical_on_gpu(tmp_path, seed):
    r = _check(seed, _need("x265_hip_8bit"), tmp_path)
    assert any("x265hip:" in l for l in r["served"]), r
