#!/usr/bin/env python
"""Writes tests/golden/bn_paths/ for tests/test_bn_paths_gpu.py: the results of that file's cases, with its runner and
seeds.  Run it in a checkout of the commit the goldens are to pin (the parent's ops.py and library; only this file and the
test are taken from the newer tree):
   python tools/bn_paths_golden.py [out_dir]"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SRK_ENV_LIVE", "1")   # (as tests/conftest.py: SRK_BN_RED16 is read at every call)
spec = importlib.util.spec_from_file_location("bn_paths_cases", os.path.join(ROOT, "tests", "test_bn_paths_gpu.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    hashes = {}
    for case in T.CASES:
        name, arrays = T.name_of(case), {}
        for k, v in T.run_case(case).items():
            a = T.to_numpy(v)
            if a.nbytes <= T.WHOLE_BYTES:
                arrays[k] = a
            else:
                arrays[k + "_corner"] = T.corner(a)
                hashes.setdefault(name, {})[k] = T.digest(a)
        np.savez(os.path.join(out, name + ".npz"), **arrays)
        print(name, sorted(arrays), "written")
    with open(os.path.join(out, "sha256.json"), "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
