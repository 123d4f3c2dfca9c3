#!/usr/bin/env python
"""Write the snapshot of what the launch-program compiler emits (tests/_plan_snapshot.py: 29 plans, compiled on the CPU):

    python tools/plan_snapshot.py [--out tests/golden/plan_programs.json]

``tests/test_plan_snapshot.py`` compares the compiler against the committed file.  Regenerate it only for a change that moves
records or dispatch ON PURPOSE, from a tree whose programs are known to be right, and show the diff (one plan per line).
Valid for 256 CUs (the library's figure without a device, and an MI355X's)."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "avid-cma_amd"), REPO):
    sys.path.insert(0, p)

import _plan_snapshot as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=S.GOLDEN)
    args = ap.parse_args()
    snap = S.snapshot()
    S.write(snap, args.out)
    print(f"{len(snap)} plans, {os.path.getsize(args.out)} bytes -> {os.path.relpath(args.out, REPO)}")


if __name__ == "__main__":
    main()
