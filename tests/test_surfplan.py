"""The integer rules of the SAD-surface builder (x265_amd/csrc/surfplan.h: which rows a launch takes, how large its grids are), compiled on their own by plain
g++ — the header has no HIP in it — into tests/support/surfplan_cases.cpp, which reads cases and prints results; every expectation is stated here.  With
-fsanitize=address,undefined where that links (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("surfplan") / "surfplan_cases")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "x265_amd", "csrc"), os.path.join(ROOT, "tests", "support", "surfplan_cases.cpp"), "-o", exe]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [[int(v) for v in l.split()] for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _trim_line(cus, cols, takes, arriving):
    return "trim %d %d %d " % (cus, cols, len(takes)) + " ".join("%d %d" % (t, a) for t, a in zip(takes, arriving))


# The whole-round rule, worked by hand: it applies when cols > 0 and cols <= cus and rows * cols > cus; rpr = cus // cols, excess = rows % rpr; it trims when
# 4 * excess < 3 * rpr and excess <= spare (the rows of arriving items); rows are taken from the last arriving item backwards.
TRIM_CASES = [
    # cus, cols, takes, arriving, result
    (224, 30, [17, 17, 17], [0, 0, 1], [17, 17, 15]),      # rpr 7, 51 rows: excess 2 (8 < 21), spare 17
    (224, 30, [17, 17, 17], [0, 0, 0], [17, 17, 17]),      # no spare
    (224, 30, [3, 3], [1, 1], [3, 3]),                     # 6 rows x 30 = 180 CTUs: one round holds it
    (224, 30, [6, 6], [1, 1], [6, 1]),                     # 12 rows: excess 5 (20 < 21)
    (224, 30, [6, 7], [1, 1], [6, 7]),                     # 13 rows: excess 6 (24 >= 21): the last round is at least 3/4 full
    (224, 240, [2, 2], [1, 1], [2, 2]),                    # a row exceeds the CUs
    (224, 60, [4, 1], [1, 1], [3, 0]),                     # rpr 3, 5 rows: excess 2 (8 < 9): one from the last item, one from the one before
    (224, 60, [1, 4], [1, 0], [1, 4]),                     # excess 2 > spare 1
]


def test_whole_round_trim_hand_worked_cases(program):
    got = _ask(program, [_trim_line(c[0], c[1], c[2], c[3]) for c in TRIM_CASES])
    for c, g in zip(TRIM_CASES, got):
        assert g == c[4], (c, g)


def test_whole_round_trim_properties_of_random_cases(program):
    rng = np.random.default_rng(20)
    cases = []
    for _ in range(400):
        n = int(rng.integers(1, 7))
        cus = int(rng.choice([8, 32, 224, 256]))
        cols = int(rng.integers(0, cus + 8)) if rng.random() < 0.2 else int(rng.integers(1, max(2, cus // 2)))
        cases.append((cus, cols, [int(v) for v in rng.integers(0, 20, n)], [int(v) for v in rng.integers(0, 2, n)]))
    got = _ask(program, [_trim_line(*c) for c in cases])
    trimmed = 0
    for (cus, cols, takes, arriving), out in zip(cases, got):
        assert len(out) == len(takes)
        assert all(o >= 0 for o in out), (cus, cols, takes, arriving, out)
        assert all(o <= t for o, t in zip(out, takes))
        assert all(o == t for o, t, a in zip(out, takes, arriving) if not a), "only arriving items shrink"
        # from the back: behind an arriving item that gave rows up, every arriving item has given up all of its rows
        gave = [k for k in range(len(takes)) if out[k] < takes[k]]
        if gave:
            assert all(out[k] == 0 for k in range(gave[0] + 1, len(takes)) if arriving[k]), (takes, arriving, out)
            assert 0 < cols <= cus and sum(out) % (cus // cols) == 0, "a trimmed launch is whole rounds"
            trimmed += 1
    assert 40 < trimmed < 360           # both outcomes are well represented


def test_wide_group_count(program):
    # min(freeCUs, cap if cap > 0, total)
    cases = [((224, 0, 510), 224),       # no cap, 510 CTUs: one workgroup per free CU
             ((224, 2, 12), 2),          # the tests' cap: 12 CTUs walked by 2 workgroups
             ((224, 0, 12), 12),         # fewer CTUs than CUs
             ((224, 300, 510), 224),     # a cap above the free CUs bounds nothing
             ((224, -1, 510), 224)]      # nor does a negative one
    got = _ask(program, ["wide %d %d %d" % c[0] for c in cases])
    assert [g[0] for g in got] == [c[1] for c in cases]


def test_subpel_grids(program):
    # first form: waves = ceil(jobs of 16x16 / 4) + jobs of 32x32 + jobs of 64x64; grid = min(waves // 4 + 1, 4096) rounded up to a multiple of 128
    first = [((0, 0, 0), (0, 128)),                       # 0 // 4 + 1 = 1 -> 128
             ((2044, 2044, 2044), (511, 128)),            # 16x16 blocks only: 2044 / 4 = 511 waves; 511 // 4 + 1 = 128 -> 128
             ((2048, 2048, 2048), (512, 256)),            # 512 waves; 512 // 4 + 1 = 129 -> 256
             # one CTU row of 1920 x 1080 (30 CTUs): 480 + 120 + 30 blocks x 49 vectors = 23520, 5880, 1470 jobs; waves = 5880 + 5880 + 1470 = 13230;
             # 13230 // 4 + 1 = 3308 -> 3328
             ((23520, 29400, 30870), (13230, 3328)),
             ((0, 0, 100000), (100000, 4096))]            # 25001 workgroups wanted: capped at 4096
    got = _ask(program, ["grid %d %d %d" % c[0] for c in first])
    assert [tuple(g) for g in got] == [c[1] for c in first]
    # second form: groups = 4 x (64x64 blocks) + (32x32 blocks) + ceil(16x16 blocks / 4); grid = min(groups, 16384) rounded up to a multiple of 128
    second = [((480, 120, 30), (360, 384)),               # the same CTU row: 120 + 120 + 120 = 360 -> 384
              ((3, 2, 1), (7, 128)),                      # 4 + 2 + 1 = 7 -> 128
              ((1, 0, 0), (1, 128)),
              ((0, 128, 0), (128, 128)),                  # a multiple of 128 stays
              ((0, 0, 5000), (20000, 16384))]             # capped
    got = _ask(program, ["ldsgrid %d %d %d" % c[0] for c in second])
    assert [tuple(g) for g in got] == [c[1] for c in second]


def test_rows_possible(program):
    # a 136-line picture (3 CTU rows) under a margin of 80, range 32: CTU row r wants the lines up to 64 (r + 1) + 32 on the device, lines of the bottom
    # margin included: uploaded - 80 >= 96 for row 0, >= 160 for row 1, >= 224 for row 2 — more than the buffer has (296 - 80 = 216), so the last row
    # comes with the complete buffer (80 + 136 + 80 = 296), which gives every row
    cases = [((0, 3, 32, 175, 80, 136), 0),
             ((0, 3, 32, 176, 80, 136), 1),
             ((0, 3, 32, 216, 80, 136), 1),              # the picture's last line is there, its bottom margin is not
             ((1, 3, 32, 239, 80, 136), 1),              # 159 < 160
             ((1, 3, 32, 295, 80, 136), 2),              # 215 >= 160, < 224
             ((1, 3, 32, 296, 80, 136), 3),
             ((2, 3, 32, 100, 80, 136), 2),              # never below what is built
             ((0, 17, 8, 80 + 72 + 64 * 5, 80, 1080), 6)]  # range 8: rows 0..5 want 72 + 64 r lines
    got = _ask(program, ["rows %d %d %d %d %d %d" % c[0] for c in cases])
    assert [g[0] for g in got] == [c[1] for c in cases]
