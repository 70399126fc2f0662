#!/usr/bin/env python3
"""Writes tests/golden/solver_catalogue.json, the recording tests/test_solver_catalogue_gpu.py compares against: per case what that
test's catalogue() collects, from the library this tree builds.  Needs the MI355X.  A recording pins the commit it was made from:
make it from the commit whose answers are to be kept, twice, and commit it only if both agree (a statistic's value that differs
between the two goes into the test's UNSTABLE_VALUES and is left out).

  python tests/golden/make_solver_catalogue.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_solver_catalogue_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for case in sorted(T.CASES):
        rec[case] = T.strip_unstable(T.catalogue(case), case)
        print("%s: %d arrays, %d statistics at %d moments" % (case, len(T.ARRAY_IDS), len(T.STAT_IDS), 3), flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
