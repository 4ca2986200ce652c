#!/usr/bin/env python3
"""k_espcn_pair alone at c2's shape (64 x 3 x 256 x 256, declared maximum) with the library SRK_LIB_PATH names: HIP events
around 30 calls, five such groups, us per call as min / median of the five, and the integer checksum of the output (the
wrapping sum of its words), which must not depend on the library.  One process per library and round; DESIGN 15.7.
   SRK_LIB_PATH=/path/to/libsrk_variant.so python tools/pair_l1_ab.py [label]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import pytorch_super_resolution_model_collection_amd as pkg
from pytorch_super_resolution_model_collection_amd import _lib, ops

label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("SRK_LIB_PATH", "libsrk.so"))
torch.manual_seed(0)
net = pkg.ESPCNNet(3, 64, 4).cuda()
net.weight_init()
net.eval()
x = ops.declare_absmax(torch.rand(64, 3, 256, 256, device="cuda"), 1.0)
lib = _lib.load()
with torch.no_grad():
    for _ in range(10):
        y = ops.espcn_pair(x, net.layers[0], net.layers[1])
    assert y is not None and lib.srk_last_kernel_name().decode() == "k_espcn_pair"
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(30):
            y = ops.espcn_pair(x, net.layers[0], net.layers[1])
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1000.0 / 30)
assert lib.srk_ring_timeouts(1) == 0 and lib.srk_espcn_pair_scans(1) == 0
ck = int(y.contiguous(memory_format=torch.channels_last).view(torch.int32).sum(dtype=torch.int64).item()) & 0xFFFFFFFFFFFFFFFF
print("%-14s kernel alone us min %.1f median %.1f  checksum %016x" % (label, min(us), statistics.median(us), ck))
