#!/usr/bin/env python3
"""Writes tests/golden/boundary_catalogue.json, the recording tests/test_boundary_catalogue_gpu.py compares against: per case what
that test's catalogue() collects, from the library this tree builds.  Needs the MI355X.  A recording pins the commit it was made from:
make it from the commit whose answers are to be kept, twice, and commit it only if both files are byte for byte the same.

  python tests/golden/make_boundary_catalogue.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_boundary_catalogue_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for case in sorted(T.CASES):
        rec[case] = T.catalogue(case)
        print("%s: %d moments" % (case, len(rec[case])), flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
