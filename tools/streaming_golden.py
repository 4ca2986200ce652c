#!/usr/bin/env python
"""Writes tests/golden/streaming_bits/ for tests/test_streaming_bits_gpu.py: the results of that file's cases, with its
runner and inputs.  Run it with the library the goldens are to pin (SRK_LIB_PATH: the parent commit's; the cases call the
C ABI alone, so nothing else of the parent's tree is needed):
   SRK_LIB_PATH=/path/to/parent/libsrk.so python tools/streaming_golden.py [out_dir]"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # (streaming_ref)
spec = importlib.util.spec_from_file_location("streaming_bits_cases", os.path.join(ROOT, "tests", "test_streaming_bits_gpu.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    hashes = {}
    for name in T.NAMES:
        arrays = {}
        for k, a in T.run_case(name).items():
            if a.nbytes <= T.WHOLE_BYTES:
                arrays[k] = a
            else:
                arrays[k + "_corner"] = T.corner(a)
                hashes.setdefault(name, {})[k] = T.digest(a)
        np.savez(os.path.join(out, name + ".npz"), **arrays)
        print(name, sorted(arrays), "written", flush=True)
    with open(os.path.join(out, "sha256.json"), "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
