#!/usr/bin/env python3
"""tests/golden/reference_draws.json: where the reference's training dataset consumes Python's `random`.

For every call of the table REFERENCE_DRAWS in tests/test_host_cpu.py, the numbers of the lines of the reference's
dataset.py that contain it.  test_training_item_draws_follow_the_reference_source_order checks its table against this
file, so the suite needs no reference checkout.

Run:  python tests/golden/make_golden_draws.py <reference checkout>       (CPU only)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    from test_host_cpu import REFERENCE_DRAWS
    with open(os.path.join(sys.argv[1], "dataset.py")) as fh:
        lines = fh.read().splitlines()
    found = {}
    for _, text, _ in REFERENCE_DRAWS:
        found[text] = [i + 1 for i, ln in enumerate(lines) if text in ln]
        if not found[text]:
            raise SystemExit("the reference's dataset.py has no line with %r" % text)
    with open(os.path.join(HERE, "reference_draws.json"), "w") as fh:
        json.dump({"file": "dataset.py", "lines_containing": found}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
