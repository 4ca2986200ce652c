#!/usr/bin/env python3
"""k_espcn_pair's tile loop by phase at c2's shape (declared maximum), from a library built with tools/pair_l1_stamps.sh
(SRK_LIB_PATH): medians over launches x blocks x waves x own tiles, us, for ordinary tiles (nine fragments from the tile
above, no dead rows), split by the wave's first-layer form (four or five pixel fragments), and for fresh tiles (rows 0 ..
1 computed: three more fragments).  DESIGN 15.7."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import pytorch_super_resolution_model_collection_amd as pkg
from pytorch_super_resolution_model_collection_amd import _lib, ops

PHASES = ["staging signal -> first layer (staged tile awaited, bias read)", "first-layer MFMAs, rows 2 .. 9",
          "l1_store, its two counter waits (fresh: and rows 0 .. 1)", "wait in front of the second layer",
          "second layer (216 MFMAs)", "epilogue"]
NB, NW, NT = 256, 8, 64
torch.manual_seed(0)
net = pkg.ESPCNNet(3, 64, 4).cuda()
net.weight_init()
net.eval()
x = ops.declare_absmax(torch.rand(64, 3, 256, 256, device="cuda"), 1.0)
lib = _lib.load()
lib.srk_pair_l1_stamps.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_ulonglong * (NB * NW * NT * 8))()
kinds = {"ordinary, four fragments (64 MFMAs)": [], "ordinary, five fragments (80 MFMAs)": [], "fresh (column top)": []}
tile_time = []
with torch.no_grad():
    for it in range(8):
        ops.espcn_pair(x, net.layers[0], net.layers[1])
        torch.cuda.synchronize()
        assert lib.srk_pair_l1_stamps(buf) == 0
        if it < 2:
            continue   # warm
        arr = np.frombuffer(buf, dtype=np.uint64).reshape(NB, NW, NT, 8).tolist()
        for b in range(NB):
            for w in range(NW):
                grp, mh = w >> 2, w & 1
                prev6 = 0
                for own in range(NT):
                    st = arr[b][w][own][:7]
                    i = 2 * own + grp                # c2: 128 tiles per block, four columns of 32
                    if 0 in st:
                        prev6 = 0
                        continue                     # (a phase skipped: dead rows)
                    fresh, last = i % 32 == 0, i % 32 == 31
                    d = [(st[k + 1] - st[k]) / 100.0 for k in range(6)]
                    if prev6:
                        tile_time.append((st[6] - prev6) / 100.0)
                    prev6 = st[6]
                    if last:
                        continue
                    key = "fresh (column top)" if fresh else ("ordinary, five fragments (80 MFMAs)" if mh == (own & 1)
                                                               else "ordinary, four fragments (64 MFMAs)")
                    kinds[key].append(d)
print("k_espcn_pair tile loop by phase, c2, declared maximum: 6 launches x 256 blocks x 8 waves, us per wave and own tile")
print("own tile to own tile (end of epilogue to end of epilogue): median %.2f us over %d" % (statistics.median(tile_time), len(tile_time)))
for key, rows in kinds.items():
    print("%s: %d tiles" % (key, len(rows)))
    for p, name in enumerate(PHASES):
        col = sorted(r[p] for r in rows)
        print("  %-62s median %6.2f  p10 %6.2f  p90 %6.2f" % (name, statistics.median(col), col[len(col) // 10], col[len(col) * 9 // 10]))
    print("  %-62s median %6.2f" % ("sum of the six", statistics.median([sum(r) for r in rows])))
