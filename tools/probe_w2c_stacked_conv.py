"""When2com, identity (c) of DESIGN.md section 8h: ``key_net.conv1`` on n maps plus ``query_net.conv1`` on the ego's map (two ``conv3x3_sp_s2`` launches) against one
stacked 256-row launch on the n maps.  Outputs are compared bit for bit first; then 9 interleaved rounds of 50 calls between device events; one JSON line.

    python tools/probe_w2c_stacked_conv.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coalign_amd import ops
from coalign_amd.backbone import Conv3x3Pack
dev = "cuda:0"
n, h, w = 5, 13, 44
g = torch.Generator().manual_seed(0)
m = ops.SplitMap.pack(torch.randn(n, 256, h, w, generator=g).abs().to(dev).contiguous(memory_format=torch.channels_last))
wk, wq = torch.randn(128, 256, 3, 3, generator=g) * 0.03, torch.randn(128, 256, 3, 3, generator=g) * 0.03
ik, iq, ikq = (Conv3x3Pack(t.to(dev)).emu(16, True) for t in (wk, wq, torch.cat([wk, wq])))
b128, b256 = torch.zeros(128, device=dev), torch.zeros(256, device=dev)
ego = ops.SplitMap(m.data[:1])
two = lambda: (ops.conv3x3_sp_s2(m, ik, b128, 128), ops.conv3x3_sp_s2(ego, iq, b128, 128))
one = lambda: ops.conv3x3_sp_s2(m, ikq, b256, 256)
a, b = two(), one()
assert torch.equal(a[0].data, b.data[:, :8]) and torch.equal(a[1].data, b.data[:1, 8:])
times = {"two launches": [], "one stacked launch": []}
for fn in (two, one):
    for _ in range(5): fn()
torch.cuda.synchronize()
for _ in range(9):
    for name, fn in (("two launches", two), ("one stacked launch", one)):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50): fn()
        t1.record(); t1.synchronize()
        times[name].append(t0.elapsed_time(t1) / 50 * 1e3)
print(json.dumps({k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v)} for k, v in times.items()}))
