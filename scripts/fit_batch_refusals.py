"""Writes tests/golden/fit_batch_refusals.json: the ValueError text of every case in the table of tests/test_fit_batch_refusals.py, as
the package in this tree words it.  Run once, on the tree whose wording is to be kept (the file in git was written before the three
host functions of the batched fits were folded); the test then holds every later tree to it.  Needs neither a GPU nor the library.

    python scripts/fit_batch_refusals.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as G                      # noqa: E402
import test_fit_batch_refusals as T              # noqa: E402


def main():
    pkg = G.load_package()
    T.no_library(pkg, setattr)
    out = {f"{T.FNS[m]}:{name}": T.refusal(pkg, m, name) for m, name in T.CASES}
    with open(T.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} refusals -> {os.path.relpath(T.GOLDEN, ROOT)}")


if __name__ == "__main__":
    main()
