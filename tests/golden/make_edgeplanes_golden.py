"""Writes tests/golden/edgeplanes.json: what the reference's own edgeFilter gives for the pictures of tests/test_edgeplanes.py, recorded through the same driver
(tests/support/edge_ref.cpp against oracle/_ref/libx265ref<depth>.so) so that the GPU tier needs no reference.  Per depth the nine specials; per case the
seed, the size, the digests of the picture region of both planes, the host path's doubt list and the digest of the angle plane with the listed pixels zeroed;
for the two smallest sizes both planes in full (base64 of little-endian uint16).

    python tests/golden/make_edgeplanes_golden.py
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_edgeplanes as te   # noqa: E402


def main():
    out = {"margins": [te.MX, te.MY], "ctu": te.CTU, "specials": {}, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for depth in te.DEPTHS:
            exe = te.build_driver(tmp, depth)
            for (w, h) in te.SIZES:
                for kind in te.KINDS:
                    got = te.drive(exe, tmp, depth, w, h, te.picture(kind, depth, w, h))
                    out["specials"][str(depth)] = got["specials"]
                    edge, theta = te.region(got["ref_edge"], w, h), te.region(got["ref_theta"], w, h)
                    case = {"seed": te.seed_of(kind, depth, w, h), "size": [w, h], "edge_sha": te.sha(edge), "theta_sha": te.sha(theta),
                            "doubts": sorted(got["doubts"]), "theta_masked_sha": te.sha(te.masked(theta, got["doubts"]))}
                    if (w, h) in te.FULL:
                        case["edge"], case["theta"] = te.pack(edge), te.pack(theta)
                    out["cases"][te.case_key(depth, kind, w, h)] = case
    with open(te.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases" % (os.path.relpath(te.GOLDEN, ROOT), len(out["cases"])))


if __name__ == "__main__":
    main()
