#!/usr/bin/env python
"""Writes tests/golden/espcn_pair_l1/ for tests/test_espcn_pair_l1_gpu.py: the output of k_espcn_pair for that file's
cases, net and seeds.  Run with the library the goldens are to pin (SRK_LIB_PATH: the parent commit's):
   SRK_LIB_PATH=/path/to/parent/libsrk.so python tools/pair_l1_golden.py [out_dir]"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("pair_l1_cases", os.path.join(ROOT, "tests", "test_espcn_pair_l1_gpu.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    for shape in T.CASES:
        y = T.run_pair(T.input_of(shape))
        name = T.name_of(shape)
        if y.numel() * 4 < T.WHOLE_BYTES:
            np.save(os.path.join(out, name + ".npy"), y.cpu().numpy())
        else:
            np.save(os.path.join(out, name + "_rows.npy"), T.pick_rows(y, T.rows_of(shape)).cpu().numpy())
            with open(os.path.join(out, name + ".json"), "w") as f:
                json.dump({"shape": list(y.shape), "layout": "NHWC float32 bytes", "rows": T.rows_of(shape).tolist(),
                           "sha256": hashlib.sha256(T.nhwc_bytes(y)).hexdigest()}, f)
                f.write("\n")
        print(name, tuple(y.shape), "written")


if __name__ == "__main__":
    main()
