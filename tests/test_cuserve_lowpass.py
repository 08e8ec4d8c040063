"""CU residual quad-tree jobs of --lowpass-dct encodes (include/x265hip.h: X265HIP_CUJOB_LOWPASS in x265hip_cujob::coefMode, x265hip_cujob_lowpass,
x265hip_cujob_features bit 3).

Statement: test_cuserve_denoise.statement with ONE change — where a unit's size is 16 or 32, be.dct(n, r) is the low-pass composition of the reference's
lowPassDct16_c / lowPassDct32_c (common/lowpassdct.cpp:64-112), written here in numpy around be.dct(n // 2, avg): 2x2 sums cast to int16, avg = sum >> 2, the
ordinary half-size transform in the top-left quadrant of zeros, entry 0 replaced by (int16)(total >> 1) (16) or (int16)(total >> 3) (32).  The same holds for
the source block's transform of a coefficient-mode job.  Without X265HIP_CUJOB_DENOISE the denoise step is left out.  Every comparison is exact.

CPU tier: the ABI; the composition against the REAL reference's cu[].dct after enableLowpassDCTPrimitives (a driver of this test's own, tests/support/
lowpass_ref.cpp) and against the digests recorded from it (tests/golden/lowpass_dct.json); the statement against itself; the emulated-ABI encoder with
--lowpass-dct (the emulated library has no low-pass forms: no CU job, the reference's bytes).
GPU tier: device jobs against the statement in both server modes, the limits of the mode word, and the bound encoders against the unmodified reference, each
under X265HIP_VERIFY and again without it.  The jobs are on by default in the Main10 build only (the measured default: profiles/r11_v1_cujob_lowpass_ab.txt), so
the tests say X265HIP_CUSERVE_LOWPASS=1 / 0 where they need them / need them gone."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lowpass_dct.json")
vp, u32 = C.c_void_p, C.c_uint32

DENOISE, LOWPASS = 16, 32
LOWPASS_RE = r"cuserve: lowpass dct: (\d+) jobs carried the flag, (\d+) CUs kept on the host because of it"


# ---- the composition -----------------------------------------------------------------------------------------------------------------------------------

def lowpass_dct(be, n, block, seen=None):
    """lowPassDct16_c / lowPassDct32_c of an n x n int16 block: n * n int16, rows contiguous.  seen["wrapped"] counts DCs the int16 cast changed"""
    assert n in (16, 32) and block.shape == (n, n) and block.dtype == np.int16
    b = block.astype(np.int32)
    sums = (b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2]).astype(np.int16)           # int16_t sum = ...: the assignment truncates
    avg = np.ascontiguousarray(sums >> 2)                                                             # arithmetic shift
    total = int(sums.astype(np.int64).sum())                                                          # int32_t totalSum (|total| <= 1024 * 4 * 4095)
    coef = be.dct(n // 2, avg, (0, 0)).reshape(n // 2, n // 2)
    dst = np.zeros((n, n), np.int16)
    dst[:n // 2, :n // 2] = coef
    dc = total >> (1 if n == 16 else 3)
    dst[0, 0] = np.array([dc], np.int64).astype(np.int16)[0]                                          # static_cast<int16_t>: wraps
    if seen is not None and not -32768 <= dc <= 32767:
        seen["wrapped"] = seen.get("wrapped", 0) + 1
    return dst.ravel()


def forward(be, n, block, lowpass, seen=None):
    """cu[].dct of the process: the low-pass composition for 16 and 32 when the flag is set, the standard transform otherwise (8x8 always)"""
    if lowpass and n >= 16:
        return lowpass_dct(be, n, block, seen)
    return be.dct(n, block, (0, 0))


def plain(hp, j):
    """a copy of the header with both flags cleared: what the helpers of the other test files (which test coefMode for truth) are given"""
    c = hp.CuJob.from_buffer_copy(j)
    c.coefMode &= ~(DENOISE | LOWPASS)
    return c


# ---- the statement -------------------------------------------------------------------------------------------------------------------------------------

def statement(hp, O, j, pix, q, dq, tables=None, seen=None):
    """the job with the table set (q, dq) and, for a denoise job, the offset tables: ({unitIndex: (numSig, zeroDist, codedDist, codedEnergy)}, levels, resi,
    absCoef).  seen counts coded units ("coded"), lone-DC units ("dc"), units whose levels sign hiding changed ("hidden"), wrapped DCs ("wrapped")"""
    import test_cuserve_formats as tcf
    import test_cuserve_scaling as tcs
    from backends import Orc
    depth, fmt = j.bitDepth, j.chroma
    be = Orc(depth)
    pmax = (1 << depth) - 1
    dims = tcf.plane_dims(j.log2CUSize, fmt)
    half = sum(h * w for h, w in dims)
    src, prd, at = [], [], 0
    for (h, w) in dims:
        src.append(pix[at:at + h * w].reshape(h, w))
        prd.append(pix[half + at:half + at + h * w].reshape(h, w))
        at += h * w
    levels, resi = np.zeros(hp.CUJOB_MAX_ELEMS, np.int16), np.zeros(hp.CUJOB_MAX_ELEMS, np.int16)
    abs_coef = np.zeros(hp.CUJOB_MAX_ELEMS, np.uint16)
    units = {}
    seen = seen if seen is not None else {}
    coef_mode = j.coefMode & ~(DENOISE | LOWPASS)
    lowpass, denoise = bool(j.coefMode & LOWPASS), bool(j.coefMode & DENOISE)
    assert coef_mode in (0, 1) and denoise == (tables is not None)
    for (s, plane, tx, ty, ui, eo, n) in tcf.layout(j):
        log2n = n.bit_length() - 1
        f = np.ascontiguousarray(src[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        p = np.ascontiguousarray(prd[plane][ty * n:(ty + 1) * n, tx * n:(tx + 1) * n])
        r = np.ascontiguousarray((f.astype(np.int32) - p.astype(np.int32)).astype(np.int16))
        zero = be.sse_pp(n, f, (0, 0), p, (0, 0))
        coef = forward(be, n, r, lowpass, seen)                                                        # quant.cpp:432: the table's cu[].dct
        if denoise:
            coef, res_sum = be.denoise_dct(coef, np.zeros(n * n, np.uint32), tables[(int(plane != 0), log2n)])
            assert res_sum.max() <= 32768
            abs_coef[eo:eo + n * n] = res_sum
        if coef_mode:
            levels[eo:eo + n * n] = coef
            if j.sourceDct and plane == 0:
                resi[eo:eo + n * n] = forward(be, n, np.ascontiguousarray(f.astype(np.int16)), lowpass, seen)      # quant.cpp:436-442: the same table entry
            units[ui] = (0, zero, None, None)
            continue
        rem, per = j.qpRem[plane], j.qpPer[plane]
        tab = tcs.table_offset(log2n, plane, rem)
        qc, dqc = np.ascontiguousarray(q[tab:tab + n * n]), np.ascontiguousarray(dq[tab:tab + n * n])
        transform_shift = 15 - depth - log2n
        qbits = 14 + per + transform_shift
        lv, du, ns = be.quant(coef, qc, qbits, j.quantOffset << (qbits - 9))
        if ns >= 2 and j.signHide:
            before = lv.copy()
            ns = O.orc_sign_hide_hdq(lv.ctypes.data, du.ctypes.data, coef.ctypes.data, ns, log2n, 0)
            seen["hidden"] = seen.get("hidden", 0) + int(not np.array_equal(before, lv))
        assert ns == int(np.count_nonzero(lv))
        levels[eo:eo + n * n] = lv
        if not ns:
            units[ui] = (0, zero, None, None)
            continue
        seen["coded"] = seen.get("coded", 0) + 1
        back_c = be.dequant_scaling(lv, dqc, per, 20 - 14 - transform_shift)
        if ns == 1 and lv[0] != 0:
            dc = ((((int(back_c[0]) * (64 >> 6) + 1) >> 1) * (64 >> 3)) + (1 << (12 - (depth - 8) - 3 - 1))) >> (12 - (depth - 8) - 3)      # quant.cpp:588-597
            back = np.full((n, n), np.int16(dc), np.int16)
            seen["dc"] = seen.get("dc", 0) + 1
        else:
            back = be.idct(n, back_c)
        rec = np.ascontiguousarray(np.clip(p.astype(np.int32) + back, 0, pmax).astype(f.dtype))
        units[ui] = (ns, zero, be.sse_pp(n, f, (0, 0), rec, (0, 0)), be.psy_cost_pp(n, f, (0, 0), rec, (0, 0)))
        resi[eo:eo + n * n] = back.ravel()
    return units, levels, resi, abs_coef


def compare(hp, j, got, want, label):
    """units, levels and resi as test_cuserve_formats.compare compares them, and for a denoise job the absCoef block of every unit"""
    import test_cuserve_formats as tcf
    n, c = tcf.compare(plain(hp, j), got[:3], want[:3], label)
    if j.coefMode & DENOISE:
        for (s, plane, tx, ty, ui, eo, m) in tcf.layout(j):
            assert np.array_equal(got[3][eo:eo + m * m], want[3][eo:eo + m * m]), (label, s, plane, tx, ty, "absCoef")
    return n, c


def header(hp, tc, shape, fmt, depth, qps, sliceI, signHide, scaling, coef, source_dct):
    import test_cuserve_scaling as tcs
    j = tcs.job_header(hp, tc, shape, fmt, depth, qps, sliceI, signHide, scaling, coef=coef & 1, source_dct=source_dct)
    j.coefMode = coef
    return j


# ---- the inputs of the transform tests -------------------------------------------------------------------------------------------------------------------

KINDS = ("residual", "rail+", "rail-", "source", "bright")
CASES = [(depth, n, kind, 4100 + 100 * depth + n + k) for depth in (8, 10, 12) for n in (16, 32) for k, kind in enumerate(KINDS)]
BLOCKS = 3


def blocks_of(depth, n, kind, seed):
    """BLOCKS n x n int16 blocks: residuals in [-pmax, pmax], both rails, source samples in [0, pmax], the all-pmax source block"""
    pmax = (1 << depth) - 1
    rng = np.random.default_rng(seed)
    if kind == "residual":
        b = rng.integers(-pmax, pmax + 1, (BLOCKS, n, n))
    elif kind == "source":
        b = rng.integers(0, pmax + 1, (BLOCKS, n, n))
    else:
        b = np.full((BLOCKS, n, n), -pmax if kind == "rail-" else pmax)
    return np.ascontiguousarray(b.astype(np.int16))


def composed(depth, n, kind, seed, seen=None):
    from backends import Orc
    be = Orc(depth)
    return np.stack([lowpass_dct(be, n, b, seen) for b in blocks_of(depth, n, kind, seed)])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a.astype("<i2")).tobytes()).hexdigest()


def reference_source():
    """where the reference's sources lie: X265_REFERENCE, or the REF of oracle/reference.mk"""
    mk = open(os.path.join(ROOT, "oracle", "reference.mk")).read()
    return os.path.join(os.environ.get("X265_REFERENCE") or re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1), "source")


def build_driver(tmp_path, depth):
    """tests/support/lowpass_ref.cpp against oracle/_ref/libx265ref<depth>.so with the flags of oracle/reference.mk; skips where the reference is not there"""
    lib, src = os.path.join(REF, "libx265ref%d.so" % depth), reference_source()
    if not (os.path.exists(lib) and os.path.exists(os.path.join(src, "common", "primitives.h")) and os.path.exists(os.path.join(REF, "x265_config.h"))):
        pytest.skip("the reference (its sources, oracle/_ref/libx265ref%d.so) is not here" % depth)
    exe = str(tmp_path / ("lowpass_ref%d" % depth))
    defs = ["-DEXPORT_C_API=1", "-DX265_ARCH_X86=1", "-DX86_64=1", "-DHAVE_INT_TYPES_H=1", "-DHAVE_STRTOK_R=1", "-DENABLE_LIBNUMA=0", "-D__STDC_LIMIT_MACROS=1",
            "-DX265_DEPTH=%d" % depth, "-DHIGH_BIT_DEPTH=%d" % int(depth > 8), "-DX265_NS=x265"]
    subprocess.check_call(["g++", "-O1", "-std=gnu++11", "-w"] + defs + ["-I" + REF, "-I" + src, "-I" + os.path.join(src, "common"), "-I" + os.path.join(src, "encoder"),
                           os.path.join(ROOT, "tests", "support", "lowpass_ref.cpp"), "-o", exe, lib, "-Wl,-rpath," + REF, "-lpthread", "-ldl"])
    return exe


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def test_library_takes_lowpass_jobs_and_the_abi_agrees():
    """x265hip_cujob_features() bit 3 (needs no device), the flag's value in the header and in hipprim, the new entry point's prototype, and a job header that
    has not grown"""
    from x265_amd import hipprim as hp
    L = hp.lib()
    assert L.x265hip_cujob_features() & 8
    hdr = open(os.path.join(ROOT, "include", "x265hip.h")).read()
    assert int(re.search(r"#define X265HIP_CUJOB_LOWPASS\s+(\d+)u", hdr).group(1)) == LOWPASS == hp.CUJOB_LOWPASS
    assert re.search(r"int x265hip_cujob_lowpass\(x265hip_cuserve\* cs\);", hdr)
    res, args = hp.PROTOTYPES["x265hip_cujob_lowpass"]
    assert res is C.c_int and len(args) == 1
    assert hasattr(L, "x265hip_cujob_lowpass")
    body = re.search(r"typedef struct x265hip_cujob\s*\{(.*?)\}\s*x265hip_cujob;", hdr, flags=re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "uint32_t scaling" and hp.CuJob._fields_[-1][0] == "scaling" and C.sizeof(hp.CuJob) == 92
    # the binding looks the entry point up through a weak reference, like the other optional ones
    bh = open(os.path.join(ROOT, "x265_amd", "host", "x265_hip_cuserve.h")).read()
    assert re.search(r'extern "C" int x265hip_cujob_lowpass\(x265hip_cuserve\* cs\) __attribute__\(\(weak\)\);', bh)


def test_test_data_holds_wrapped_dcs():
    """at 10 and 12 bit the all-pmax source block's DC (and the rails') does not fit int16: at least one wrapped DC per size and depth >= 10, none at 8 bit"""
    for depth in (8, 10, 12):
        for n in (16, 32):
            seen = {}
            for (d, m, kind, seed) in CASES:
                if (d, m) == (depth, n):
                    composed(d, m, kind, seed, seen)
            assert (seen.get("wrapped", 0) > 0) == (depth >= 10), (depth, n, seen)
            if depth >= 10:
                seen = {}
                out = composed(depth, n, "bright", 0, seen)
                pmax, shift = (1 << depth) - 1, 1 if n == 16 else 3
                assert seen["wrapped"] == BLOCKS and int(out[0][0]) == ((((n * n * pmax) >> shift) + 32768) % 65536) - 32768 != (n * n * pmax) >> shift


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_composition_is_the_reference_lowpass_dct(tmp_path, depth):
    """the numpy composition against cu[BLOCK_16x16].dct / cu[BLOCK_32x32].dct of an EncoderPrimitives filled by setupCPrimitives + setupAliasPrimitives +
    enableLowpassDCTPrimitives of the real reference (the driver, run as a plain child process): entry for entry, and the recorded digests are these outputs'"""
    exe = build_driver(tmp_path, depth)
    gold = {(g["depth"], g["n"], g["kind"], g["seed"]): g for g in json.load(open(GOLDEN))["cases"]}
    done = 0
    for (d, n, kind, seed) in CASES:
        if d != depth:
            continue
        blocks = blocks_of(d, n, kind, seed)
        f = str(tmp_path / "blocks.bin")
        blocks.astype("<i2").tofile(f)
        r = subprocess.run([exe, str(n), f], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-800:]
        ref = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()], np.int64)
        assert ref.shape == (BLOCKS, n * n)
        mine = composed(d, n, kind, seed)
        assert np.array_equal(mine, ref), (d, n, kind, np.argwhere(mine != ref)[:4])
        # the three quadrants the reference's memset leaves
        q = ref.reshape(BLOCKS, n, n)
        assert not q[:, n // 2:, :].any() and not q[:, :, n // 2:].any()
        g = gold[(d, n, kind, seed)]
        assert g["input"] == digest(blocks) and g["output"] == digest(ref), (d, n, kind)
        done += 1
    assert done == 2 * len(KINDS)


def test_composition_matches_the_recorded_reference_outputs():
    """the same composition against the digests recorded from the reference's driver (tests/golden/lowpass_dct.json): runs with no reference present"""
    gold = json.load(open(GOLDEN))["cases"]
    assert sorted((g["depth"], g["n"], g["kind"], g["seed"]) for g in gold) == sorted(CASES)
    for g in gold:
        key = (g["depth"], g["n"], g["kind"], g["seed"])
        assert digest(blocks_of(*key)) == g["input"], key
        assert digest(composed(*key)) == g["output"], key


MODE_WORDS = ((LOWPASS, 0), (LOWPASS | 1, 1), (LOWPASS | DENOISE, 0), (LOWPASS | DENOISE | 1, 0), (LOWPASS | 1, 0), (LOWPASS | DENOISE | 1, 1))


def test_statement_checks_itself():
    """test_cuserve_scaling.SHAPES, formats 0-3, 8 / 10 / 12 bit, ordinary and coefficient mode, with and without DENOISE.  With the flag clear the statement is
    test_cuserve_formats.statement unit for unit; with it set every coefficient outside the top-left quadrant of a 16 / 32 unit is zero (coefficient mode: the
    levels block and the source transform; ordinary mode: the levels, which a zero coefficient cannot make) and 8x8 units equal the flag-clear statement.
    Floors (conditions of the test, from what this loop produces: 60 jobs, 1 656 units, 744 of them 16 / 32 units of coefficient-mode jobs, 454 coded units, 648
    8x8 units): more than 1 500 units, more than 500 quadrant checks on coefficients, more than 200 coded units, more than 100 8x8 units compared."""
    import test_cuserve as tc
    import test_cuserve_denoise as tcd
    import test_cuserve_formats as tcf
    import test_cuserve_scaling as tcs
    from x265_amd import hipprim as hp
    O = tcs._orc()
    q, dq = tcs.flat16_set()
    rng = np.random.default_rng(1901)
    total = units = coded = quadrants = small = 0
    for depth in (8, 10, 12):
        for shape in tcs.SHAPES:
            for fmt in (0, 1, 2, 3):
                qps = tcs.qps_of(depth, (22, 30, 37)[total % 3])
                coef, sdct = MODE_WORDS[total % len(MODE_WORDS)]
                j = header(hp, tc, shape, fmt, depth, qps, (total // 2) % 2, int(total % 3 != 0), 0, coef, sdct)
                pix = tcs.pixels(rng, shape[0], fmt, depth, (total // 4) % 4)
                tables = tcd.make_tables(rng, j, "plausible") if coef & DENOISE else None
                seen = {}
                want = statement(hp, O, j, pix, q, dq, tables, seen)
                # the flag clear and no denoise: the flat statement
                flat = plain(hp, j)
                clear = statement(hp, O, flat, pix, q, dq)
                n, c = tcf.compare(flat, clear[:3], tcf.statement(hp, O, flat, pix), (depth, shape, fmt, qps, coef))
                # the flag clear, denoise as the job has it: what 8x8 units must equal
                off = hp.CuJob.from_buffer_copy(j)
                off.coefMode &= ~LOWPASS
                std = statement(hp, O, off, pix, q, dq, tables)
                for (s, plane, tx, ty, ui, eo, m) in tcf.layout(j):
                    lv, sr = want[1][eo:eo + m * m].reshape(m, m), want[2][eo:eo + m * m].reshape(m, m)
                    if m == 8:
                        assert want[0][ui] == std[0][ui] and np.array_equal(want[1][eo:eo + 64], std[1][eo:eo + 64]) and np.array_equal(want[2][eo:eo + 64], std[2][eo:eo + 64]) \
                            and np.array_equal(want[3][eo:eo + 64], std[3][eo:eo + 64]), (depth, shape, fmt, s, plane, tx, ty)
                        small += 1
                        continue
                    assert not lv[m // 2:, :].any() and not lv[:, m // 2:].any(), (depth, shape, fmt, s, plane, tx, ty, "levels")
                    assert not want[3][eo:eo + m * m].reshape(m, m)[m // 2:, :].any() and not want[3][eo:eo + m * m].reshape(m, m)[:, m // 2:].any()
                    if coef & 1:
                        quadrants += 1
                        if sdct and plane == 0:
                            assert sr.any() and not sr[m // 2:, :].any() and not sr[:, m // 2:].any(), (depth, shape, fmt, s, plane, tx, ty, "source transform")
                total += 1; units += n; coded += seen.get("coded", 0)
    print("%d jobs, %d units, %d quadrant checks on coefficients, %d coded units, %d 8x8 units" % (total, units, quadrants, coded, small))
    assert total == 3 * len(tcs.SHAPES) * 4 and units > 1500 and quadrants > 500 and coded > 200 and small > 100


def test_emulated_encoder_keeps_lowpass_cus_on_the_host(tmp_path):
    """the emulated ABI has no x265hip_cujob_lowpass and its transforms are the standard ones: with --lowpass-dct the binding (asked for the jobs with
    X265HIP_CUSERVE_LOWPASS=1) hands it no CU job, says which CUs it kept, reports no failure, and the bytes are the reference's — which differ from the same
    encode without the option.  (Before the binding looked at the process's transform table this encode did not come that far: the private C tables of the
    binding left lowpassdct.cpp's pointers to the standard transforms on empty slots, and the encoder ended with a segmentation fault: profiles/
    r11_v1_cujob_lowpass_parent.txt.)"""
    import test_cuserve_formats as tcf
    import test_saostats_formats as sf
    ref, emul = os.path.join(REF, "x265_8bit"), os.path.join(REF, "x265_emul_8bit")
    sf._need(ref, emul)
    from x265_amd.synth import make_clip
    yuv = str(tmp_path / "clip.yuv")
    make_clip(yuv, 328, 200, 6, seed=101)
    args = ["--input", yuv, "--input-res", "328x200", "--fps", "30", "--frames", "6", "--preset", "medium", "--hash", "1", "--pools", "4", "-F", "2"]
    err = sf._encode_pair(tmp_path, ref, emul, args + ["--lowpass-dct"], dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_CUSERVE_LOWPASS="1"))
    assert "OFF" not in err and "did not come back" not in err and "VERIFY FAILED" not in err, err[-1200:]
    m = re.search(tcf.JOBS_RE, err)
    assert m is None or int(m.group(1)) == 0, err[-1200:]
    d = re.search(LOWPASS_RE, err)
    assert d and int(d.group(1)) == 0 and int(d.group(2)) > 0, err[-1200:]
    with_option = open(str(tmp_path / "ref.hevc"), "rb").read()
    r = subprocess.run([ref] + args + ["-o", str(tmp_path / "ref_plain.hevc")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and open(str(tmp_path / "ref_plain.hevc"), "rb").read() != with_option, "--lowpass-dct does not change this encode: the case shows nothing"
    # the 8-bit build's default (variable unset) keeps them on the host as well
    err = sf._encode_pair(tmp_path, ref, emul, args + ["--lowpass-dct"], dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1"))
    d = re.search(LOWPASS_RE, err)
    assert "VERIFY FAILED" not in err and d and int(d.group(1)) == 0 and int(d.group(2)) > 0, err[-1200:]


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def run_on(hp, L, cs, slot, j, pix, block=None):
    """the job through submit / poll (a denoise job with its offset block written in front of it): (units, levels, resi, absCoef or None)"""
    import test_cuserve_denoise as tcd
    import test_cuserve_formats as tcf
    if j.coefMode & DENOISE:
        return tcd.run_on(hp, L, cs, slot, j, pix, block)
    return tcf.run_on(hp, L, cs, slot, j, pix) + (None,)


def rail_pixels(j, source_high):
    import test_cuserve_denoise as tcd
    return tcd.rail_pixels(j, source_high)


def bright_pixels(rng, j):
    """an all-pmax source over a random prediction: the source transform's DC is the largest there is"""
    import test_cuserve_formats as tcf
    pmax = (1 << j.bitDepth) - 1
    n = sum(h * w for h, w in tcf.plane_dims(j.log2CUSize, j.chroma))
    dt = np.uint8 if j.bitDepth == 8 else np.uint16
    return np.ascontiguousarray(np.concatenate([np.full(n, pmax, dt), rng.integers(0, pmax + 1, n).astype(dt)]))


# (shape, format): the smallest jobs at which each kernel form exists — a 32x32 CU at 4:2:0 is the team 32x32 unit plus one 16x16 unit on a wave per chroma plane
# (sizes 32 + 16: tiles of four 16x16 luma units and 8x8 chroma that stays standard); at 4:4:4 one-wave 32x32 chroma; a lone 16x16 CU with 8x8 chroma; a 64x64
# CU at 4:2:2: four team units and tiles of four 16x16 chroma units, 4:2:2 rows
FORMS = (((5, 5, 5), 1), ((5, 5, 4), 1), ((5, 5, 5), 3), ((5, 5, 4), 3), ((4, 4, 4), 1))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_device_lowpass_jobs_match_the_statement(mode):
    """8 / 10 / 12 bit, the forms above twice each with the mode words 32, 33 (sourceDct 1 and 0), 48, 49 (sourceDct 0 and 1) round-robin and pixel kinds 0-3,
    the 64x64 4:2:2 job once per depth, two rail jobs per depth in coefficient mode (their DC wraps at 10 / 12 bit: asserted on the expected values), an
    all-bright source under 33 with sourceDct, one job per depth with a registered table set: units, levels, resi, absCoef.  In mode 0 the first job starts the
    resident server before x265hip_cujob_lowpass has the kernels replaced."""
    import test_cuserve as tc
    import test_cuserve_denoise as tcd
    import test_cuserve_scaling as tcs
    hp, L, tc, tcf, cs = tcs._device(mode)
    O = tcs._orc()
    try:
        rng = np.random.default_rng(1910 + mode)
        j0 = tc._job_header(hp, 5, 5, 5, 1, 8, (30, 29, 29), 0, 1)
        p0 = tc._job_pixels(rng, 5, 1, 8, 1)
        done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
        assert tc._compare(hp, j0, tc._run_on(hp, L, cs, 0, j0, p0), wu, wl, wr, "plain job before any low-pass job")[0] == done
        hp.check(L.x265hip_cujob_lowpass(cs))
        hp.check(L.x265hip_cujob_lowpass(cs))                                        # (once per service: the second call changes nothing)
        flat, named = tcs.flat16_set(), tcs.default_set()
        registered = False
        cases = []
        for depth in (8, 10, 12):
            for turn in range(2):
                for (shape, fmt) in FORMS:
                    cases.append((depth, fmt, shape, None, 0))
            cases.append((depth, 2, (6, 5, 4), None, 0))
            cases.append((depth, 1, (5, 5, 4), "rail", False))
            cases.append((depth, 3, (5, 5, 5), "rail", True))
            cases.append((depth, 1, (5, 5, 4), "bright", None))
            cases.append((depth, 1, (5, 5, 4), None, 1))                              # with the table set
        total = units = coded = sources = with_set = 0
        seen, words = {}, {}
        for (depth, fmt, shape, special, arg) in cases:
            sid = int(special is None and arg == 1)
            if special == "rail":
                coef, sdct = LOWPASS | 1, 0
            elif special == "bright":
                coef, sdct = LOWPASS | 1, 1
            elif sid:
                coef, sdct = (LOWPASS, 0) if depth != 10 else (LOWPASS | DENOISE, 0)
            else:
                coef, sdct = MODE_WORDS[total % len(MODE_WORDS)]
            qps = tcs.qps_of(depth, (22, 30, 37)[(total // 4) % 3])
            j = header(hp, tc, shape, fmt, depth, qps, (total // 2) % 2, int(total % 3 != 0), sid, coef, sdct)
            if special == "rail":
                pix = rail_pixels(j, arg)
            elif special == "bright":
                pix = bright_pixels(rng, j)
            else:
                pix = tcs.pixels(rng, shape[0], fmt, depth, (total // 3) % 4)
            if sid and not registered:
                assert tcs._add(hp, L, cs, named) == 1
                registered = True
            q, dq = named if sid else flat
            tables = tcd.make_tables(rng, j, "plausible") if coef & DENOISE else None
            mine = {}
            want = statement(hp, O, j, pix, q, dq, tables, mine)
            if special is not None and depth >= 10:
                assert mine.get("wrapped", 0) > 0, (depth, special, "the expected DC did not wrap")
            got = run_on(hp, L, cs, total % 4, j, pix, tcd.pack_block(j, tables) if tables else None)
            n, c = compare(hp, j, got, want, (mode, depth, fmt, shape, special, qps, sid, coef, sdct))
            for k, v in mine.items():
                seen[k] = seen.get(k, 0) + v
            words[(coef, sdct)] = words.get((coef, sdct), 0) + 1
            total += 1; units += n; with_set += sid
            if coef & 1:
                sources += c
            else:
                coded += c
        print("mode %d: %d jobs (%r), %d units, %d coded, %d source transforms, %d with a table set; %r" % (mode, total, words, units, coded, sources, with_set, seen))
        assert total == 3 * (2 * len(FORMS) + 5) and with_set == 3 and set(MODE_WORDS) <= set(words)
        # coded units, units with hidden signs, source transforms and wrapped DCs all occurred
        assert coded > 0 and sources > 0 and seen.get("hidden", 0) > 0 and seen.get("wrapped", 0) > 0, (coded, sources, seen)
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


@pytest.mark.gpu
def test_mode_word_limits():
    """8 | 32 is X265HIP_EINVAL (the inverse half has nothing low-pass about it), before and after the switch-over; the flag on a service that was not switched
    over is refused; the service goes on serving after each refusal; a flag-clear job on a switched-over service equals the flat statement"""
    import test_cuserve_scaling as tcs
    hp, L, tc, tcf, cs = tcs._device(0)
    O = tcs._orc()
    try:
        rng = np.random.default_rng(1920)
        job = vp()
        hp.check(L.x265hip_cuserve_slot(cs, 1, C.byref(job), None, None, None, None))
        seq = u32()

        def refused(mode_word, shape, fmt):
            bad = tc._job_header(hp, shape[0], shape[1], shape[2], fmt, 8, (30, 29, 29), 0, 1)
            bad.coefMode = mode_word
            C.memmove(job, C.byref(bad), C.sizeof(bad))
            return L.x265hip_cuserve_submit(cs, 1, C.byref(seq)) == -1            # X265HIP_EINVAL

        def flat_job_matches(label):
            j0 = tc._job_header(hp, 5, 5, 4, 1, 8, (30, 29, 29), 0, 1)
            p0 = tc._job_pixels(rng, 5, 1, 8, 1)
            done, wu, wl, wr = tc._oracle_job(hp, O, j0, p0)
            assert tc._compare(hp, j0, tc._run_on(hp, L, cs, 1, j0, p0), wu, wl, wr, label)[0] == done

        assert refused(LOWPASS, (5, 5, 4), 1) and refused(LOWPASS | 1, (5, 5, 4), 1), "the flag on a service that was not switched over"
        flat_job_matches("plain job after the refused ones")
        assert refused(8 | LOWPASS, (5, 5, 5), 0)
        flat_job_matches("plain job after the refused inverse job")
        hp.check(L.x265hip_cujob_lowpass(cs))
        assert refused(8 | LOWPASS, (5, 5, 5), 0) and refused(LOWPASS | 2, (5, 5, 4), 1) and refused(LOWPASS | DENOISE, (5, 5, 4), 1)      # (no x265hip_cujob_denoise call)
        flat_job_matches("flag-clear job on the switched-over service")
        j = header(hp, tc, (5, 5, 4), 1, 8, (26, 25, 25), 0, 1, 0, LOWPASS, 0)
        pix = tcs.pixels(rng, 5, 1, 8, 0)
        n, c = compare(hp, j, run_on(hp, L, cs, 1, j, pix), statement(hp, O, j, pix, *tcs.flat16_set()), "after the refused jobs")
        assert n == 15 and c > 0
    finally:
        hp.check(L.x265hip_cuserve_close(cs))


BOUND = {   # depth, csp, preset, extra arguments, extra environment
    "8bit": (8, "i420", "medium", [], {}),
    "main10-slow": (10, "i420", "slow", [], {}),                                   # psy-rdoq: the wrapping source DC inside a real encode
    "8bit-444": (8, "i444", "medium", [], {}),
    "8bit-ctu32": (8, "i420", "medium", ["--ctu", "32"], {}),
    "8bit-scaling-list": (8, "i420", "medium", ["--scaling-list", "default"], {}),
    "8bit-nr-inter": (8, "i420", "medium", ["--nr-inter", "400"], {"X265HIP_CUSERVE_DENOISE": "1"}),
    "main12": (12, "i420", "medium", [], {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND))
def test_bound_encoders_serve_lowpass_cus_byte_identical(tmp_path, name):
    """the product's encoders (oracle/_ref/integration) with --lowpass-dct against the unmodified reference, 328x200 with partial CTUs, 10 frames, two frame
    threads: the reference's bytes differ from the same encode without the option (or the case shows nothing); under X265HIP_VERIFY and again without it the
    same bytes, units served, every CU job carried the flag (J == the jobs of the cuserve line, J > 0).  The jobs are enabled with X265HIP_CUSERVE_LOWPASS=1 (the
    default of the Main10 build alone); with X265HIP_CUSERVE_LOWPASS=0: the same bytes and no flagged job."""
    import test_cuserve_denoise as tcd
    import test_cuserve_formats as tcf
    import test_saostats_formats as sf
    depth, csp, preset, extra, more = BOUND[name]
    ref, hip = os.path.join(REF, "x265_%dbit" % depth), os.path.join(REF, "integration", "x265_hip_%dbit" % depth)
    sf._need(ref, hip)
    yuv = str(tmp_path / "clip.yuv")
    sf._clip(yuv, 328, 200, 10, depth, csp, 101)
    base = ["--input", yuv, "--input-res", "328x200", "--input-depth", str(depth), "--input-csp", csp, "--fps", "30", "--frames", "10", "--preset", preset,
            "--hash", "1", "--pools", "4", "-F", "2"] + extra
    want = tcd._run(ref, base + ["--lowpass-dct"], str(tmp_path / "ref.hevc"))[1]
    assert want != tcd._run(ref, base, str(tmp_path / "ref_plain.hevc"))[1], "--lowpass-dct does not change this encode: the case shows nothing"
    for verify in (True, False):
        env = dict(X265HIP="require", X265HIP_VERBOSE="1", X265HIP_CUSERVE_LOWPASS="1", **more)
        if verify:
            env["X265HIP_VERIFY"] = "1"
        err, got = tcd._run(hip, base + ["--lowpass-dct"], str(tmp_path / "hip.hevc"), env)
        assert got == want, "bitstreams differ (X265HIP_VERIFY %s)" % ("set" if verify else "not set")
        assert "VERIFY FAILED" not in err and "OFF" not in err and "did not come back" not in err, err[-1500:]
        m, d = re.search(tcf.JOBS_RE, err), re.search(LOWPASS_RE, err)
        assert m and d, err[-1500:]
        jobs, fwd, inv = (int(g) for g in m.groups())
        carried, kept = (int(g) for g in d.groups())
        print("%s (verify %d): %d jobs, %d carried the flag, %d CUs kept; %d forward units, %d inverse units" % (name, verify, jobs, carried, kept, fwd, inv))
        assert carried > 0 and carried == jobs and kept == 0 and fwd > jobs, (jobs, carried, kept, fwd, inv)
    err, got = tcd._run(hip, base + ["--lowpass-dct"], str(tmp_path / "off.hevc"),
                        dict(X265HIP="require", X265HIP_VERIFY="1", X265HIP_VERBOSE="1", X265HIP_CUSERVE_LOWPASS="0", **more))
    d = re.search(LOWPASS_RE, err)
    assert got == want, "X265HIP_CUSERVE_LOWPASS=0: bitstreams differ"
    assert d and int(d.group(1)) == 0 and int(d.group(2)) > 0, err[-1200:]
