#!/usr/bin/env python3
"""Writes tests/golden/solver_bits.json, the recording tests/test_solver_bits_gpu.py compares against: per case the SHA-256 digests
that test's digests() computes, from the library this tree builds.  Needs the MI355X.  A recording pins the commit it was made from:
make it from the commit whose bits are to be kept, twice, and commit it only if both agree.

  python tests/golden/make_solver_bits.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_solver_bits_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for case in T.CASES:
        rec[case] = T.digests(case)
        print("%s: %d digests" % (case, len(rec[case])), flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
