"""Writes tests/golden/pichash.json: for every case of tests/test_pichash.py the running values the reference's FrameEncoder::initDecodedPictureHashSEI
leaves after each per-row call and after the whole-picture call, and the digests crcFinish / checksumFinish make of them (tests/support/pichash_ref.cpp,
built against oracle/_ref).  The pictures themselves are not stored: the test makes them again from the case's name.

    python tests/golden/make_pichash_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_pichash as tp


def main():
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for depth in tp.DEPTHS:
            res = tp.driver_results(tmp, depth)
            for c in tp.cases(depth):
                cases[tp.key_of(depth, c)] = tp.golden_entry(res[c[0]])
    with open(tp.GOLDEN, "w") as f:
        json.dump({"what": "running values (rows, whole) and digests of --hash 2 (crc) and --hash 3 (sum) per case of tests/test_pichash.py", "cases": cases}, f,
                  indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases -> %s (%d bytes)" % (len(cases), os.path.relpath(tp.GOLDEN, ROOT), os.path.getsize(tp.GOLDEN)))


if __name__ == "__main__":
    main()
