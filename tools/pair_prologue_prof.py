#!/usr/bin/env python3
"""k_espcn_pair's prologue by phase, from a library built with tools/pair_prologue_stamps.sh (SRK_LIB_PATH): c2's shape,
once with max|x| measured in the launch and once with a declared maximum; median / maximum over the blocks, us."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import pytorch_super_resolution_model_collection_amd as pkg
from pytorch_super_resolution_model_collection_amd import _lib, ops

PHASES = ["arguments + |x| slice + arrival", "filter copy", "fragment loads, offsets, first tile's loads",
          "rendezvous wait + barrier", "scales"]
net = pkg.ESPCNNet(3, 64, 4).cuda()
net.weight_init()
net.eval()
x = torch.rand(64, 3, 256, 256, device="cuda")
xd = ops.declare_absmax(x.clone(), 1.0)
ops.PAIR_AMAX_IN_LAUNCH_BYTES = 1 << 62   # the first row measures in the launch at c2's size, which the product does not
lib = _lib.load()
lib.srk_pair_stamps.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_ulonglong * (256 * 8))()
with torch.no_grad():
    for label, fn in (("measured in the launch", lambda: ops.espcn_pair(x.detach(), net.layers[0], net.layers[1])),
                      ("declared", lambda: ops.espcn_pair(xd, net.layers[0], net.layers[1]))):
        rows = []
        for _ in range(12):
            fn()
            torch.cuda.synchronize()
            assert lib.srk_pair_stamps(buf) == 0
            rows.append([[buf[b * 8 + k] for k in range(6)] for b in range(256)])
        rows = rows[2:]   # warm
        print("max|x| %s (10 launches x 256 blocks)" % label)
        for p, name in enumerate(PHASES):
            d = [(r[b][p + 1] - r[b][p]) / 100.0 for r in rows for b in range(256)]
            print("  %-45s median %6.2f  max %6.2f" % (name, statistics.median(d), max(d)))
        tot = [(r[b][5] - r[b][0]) / 100.0 for r in rows for b in range(256)]
        start = [(max(r[b][0] for b in range(256)) - min(r[b][0] for b in range(256))) / 100.0 for r in rows]
        print("  %-45s median %6.2f  max %6.2f" % ("first instruction to tile loop", statistics.median(tot), max(tot)))
        print("  %-45s median %6.2f" % ("first block's start to last block's start", statistics.median(start)))
