"""Regenerates tests/golden/hme_lookahead.json: the log of tests/support/hme_ref.cpp (the reference's own two-level lookahead estimate under --hme) for every
case of tests/test_lookahead_hme.py.  Needs the reference's sources and oracle/_ref/libx265ref{8,10,12}.so (the project's build makes them).
    python tests/golden/make_hme_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_lookahead_hme as t      # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for depth in (8, 10, 12):
            out.update(t.run_driver(tmp, depth))
    assert sorted(out) == sorted(t.key_of(*c) for c in t.all_cases())
    out = {k: out[k] for k in sorted(out)}
    assert t.unpack_log(t.pack_log(out)) == out
    with open(t.GOLDEN, "w") as f:
        json.dump(t.pack_log(out), f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d bytes" % (t.GOLDEN, len(out), os.path.getsize(t.GOLDEN)))


if __name__ == "__main__":
    main()
