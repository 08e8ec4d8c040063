"""Writes tests/golden/scenestats.json: what the reference's own Encoder::computeHistograms and computeEdge give for the pictures of tests/test_scenestats.py,
recorded through the same driver (tests/support/hist_ref.cpp against oracle/_ref/libx265ref<depth>.so) so that the GPU tier needs no reference.  Per
computeHistograms case the range-error count, the two edge bins and the digests of the histograms and of the edge plane; per --rskip 2 case the digest of
the sentinel-filled plane after computeEdge; for the two smallest sizes the arrays in full (base64 of deflated little-endian int32).

    python tests/golden/make_scenestats_golden.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_scenestats as ts   # noqa: E402


def main():
    out = {"sentinel": ts.SENTINEL, "bits_pad": ts.BITS_PAD, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in ts.hist_cases():
            out["cases"][ts.hist_key(case)] = ts.golden_hist_entry(case, ts.drive_hist(ts.build_driver(tmp, case[0]), tmp, case, rskip=2))
        for case in ts.bits_cases():
            out["cases"][ts.bits_key(case)] = ts.golden_bits_entry(case, ts.drive_bits(ts.build_driver(tmp, case[0]), tmp, case))
    with open(ts.GOLDEN, "w") as f:
        # one case per line
        cases = out.pop("cases")
        f.write(json.dumps(out, sort_keys=True)[:-1] + ', "cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(cases[k], sort_keys=True)) for k in sorted(cases)))
        f.write("\n}}\n")
    print("%s: %d cases" % (os.path.relpath(ts.GOLDEN, ROOT), len(cases)))


if __name__ == "__main__":
    main()
