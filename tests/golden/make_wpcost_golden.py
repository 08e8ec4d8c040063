"""Writes tests/golden/wpcost.json: for every case of tests/test_wpcost.py every evaluation the reference's weightAnalyse makes, grouped by (plane, list) in the
function's own order (wtPresent, weight, offset, denominator, total; per group the number of blocks and a digest of all block values), and the slice's final weights
(tests/support/wpcost_ref.cpp, built against oracle/_ref).  The planes themselves are not stored: the test makes them again from the case's name.

    python tests/golden/make_wpcost_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_wpcost as tw


def main():
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for depth in tw.DEPTHS:
            res = tw.driver_results(tmp, depth)
            for name in tw.CASES:
                cases[tw.key_of(depth, name)] = tw.golden_entry(res[name])
    what = ("per case of tests/test_wpcost.py: planes = [plane, list, blocks per evaluation, digest of all block values, [[wtPresent, weight, offset, "
            "denominator, total] per evaluation]] in the function's order; table = final [weight, offset, denominator, wtPresent] per list and plane")
    with open(tw.GOLDEN, "w") as f:
        # one case per line
        f.write('{"what": %s,\n"cases": {\n' % json.dumps(what))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(cases[k], separators=(",", ":"))) for k in sorted(cases)))
        f.write("\n}}\n")
    print("%d cases -> %s (%d bytes)" % (len(cases), os.path.relpath(tw.GOLDEN, ROOT), os.path.getsize(tw.GOLDEN)))


if __name__ == "__main__":
    main()
