"""One stream-K Winograd LIST launch alone (ops.conv2d_winograd_sk_active) on a fixed seeded tile list: device-event time per
launch, and the target of rocprofv3 passes (every pass profiles the same launches). SESSD_WINO_VAR selects the loop variant.

    python scripts/wino_list_probe.py [channels [HxW [tiles [workgroups [min_rounds [shape [launches]]]]]]]

defaults: 256 channels, the 100x88 map, 896 listed tiles (41 %), 128 workgroups (one CU set), whole-unit shares, shape 3."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import numpy as np
import torch
from sessd_hip import ops

a = sys.argv[1:]
cc = int(a[0]) if len(a) > 0 else 256
hh, ww = [int(v) for v in (a[1] if len(a) > 1 else "100x88").split("x")]
nt = (hh // 2) * (ww // 2)
n_act = int(a[2]) if len(a) > 2 else 896
wgs = int(a[3]) if len(a) > 3 else 128
mr = int(a[4]) if len(a) > 4 else -1
shape = int(a[5]) if len(a) > 5 else 3
launches = int(a[6]) if len(a) > 6 else 200
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
w = (torch.randn(cc, cc, 3, 3, generator=g) * 0.03).to(dev)
pc = ops.pack_conv2d(w, 1)
x = torch.randn(1, cc, hh, ww, generator=g).to(dev)
tiles = np.sort(np.random.default_rng(0).choice(nt, n_act, replace=False)).astype(np.int32)
tl, n = torch.from_numpy(tiles).to(dev), torch.tensor([n_act], dtype=torch.int32, device=dev)
ws = ops.winograd_sk_workspace(1, hh, ww, cc, dev, wgs, shape)
out = torch.zeros(1, cc, hh, ww, device=dev)
run = lambda: ops.conv2d_winograd_sk_active(x, pc.upk_sk(shape), cc, None, None, False, out, shape, ws, tl, n, workgroups=wgs, min_rounds=mr)
for _ in range(10):
    run()
torch.cuda.synchronize()
times = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches // 5):
        run()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) * 1000 / (launches // 5))
print("wino list probe: var %s shape %d, %d ch, %dx%d, %d of %d tiles, %d workgroups, min_rounds %d: %s us per launch (back to back, 5 windows)" % (
    os.environ.get("SESSD_WINO_VAR", "0"), shape, cc, hh, ww, n_act, nt, wgs, mr, " ".join("%.1f" % t for t in times)))
