"""Timing probe of the PointPillars front end at the config's size: 12 000 pillars of T = 100 slots (geometric point counts, mean
about 7) on the 432 x 496 grid, one frame. TIME PER CALL (device events around back-to-back calls, each window a few tenths of a
second; the host's share of a call is inside these figures) of
  * ops.pillar_features with the canvas output (checks + torch.empty + sessd_pillar_features; clear not included),
  * sessd_pillar_features called directly on preallocated outputs (the same launch without the wrapper),
  * the clear of the (1, 64, 496, 432) canvas (sessd_fill_u32, 55 MB),
  * ops.pillar_scatter (allocation + clear + scatter-alone launch),
  * the det3d-mirror modules' torch formulation (`_forward_torch` of reader and scatter) on the same device,
alternated over several rounds; prints one JSON line. KERNEL times come from a run of this script under
`rocprofv3 --kernel-trace --stats` (`--trace`: few calls, no timing). Usage: python scripts/pillar_probe.py [rounds | --trace]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from sessd_hip import ops  # noqa: E402
from sessd_hip._lib import lib, check  # noqa: E402
from sessd_hip.engine import fold_bn  # noqa: E402
from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter  # noqa: E402

N, T, NX, NY = 12000, 100, 432, 496
trace = "--trace" in sys.argv
rounds = int([a for a in sys.argv[1:] if a.isdigit()][0]) if any(a.isdigit() for a in sys.argv[1:]) else 5
dev = torch.device("cuda", 0)


def timeit(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds


rng = np.random.RandomState(0)
num = np.minimum(rng.geometric(1.0 / 7.0, N), T).astype(np.int32)
cells = rng.permutation(NX * NY)[:N]
coors = np.stack([np.zeros(N), np.zeros(N), cells // NX, cells % NX], 1).astype(np.int32)
vox = np.zeros((N, T, 4), np.float32)
for i in range(N):
    vox[i, :num[i]] = rng.rand(num[i], 4) * [69.12, 79.36, 4.0, 1.0] + [0.0, -39.68, -3.0, 0.0]
net = PillarFeatureNet(num_filters=[64]).eval()
with torch.no_grad():
    net.pfn_layers[0].norm.running_mean.normal_(0, 0.1)
    net.pfn_layers[0].norm.bias.normal_(0, 0.1)
net.to(dev)
scat = PointPillarsScatter(num_input_features=64)
vox_d, num_d, coors_d = (torch.from_numpy(a).to(dev) for a in (vox, num, coors))
w = net.pfn_layers[0].linear.weight.detach().contiguous()
scale, shift = fold_bn(net.pfn_layers[0].norm)
canvas = torch.empty((1, 64, NY, NX), dtype=torch.float32, device=dev)
err = torch.zeros(1, dtype=torch.int32, device=dev)


def kernel():
    return ops.pillar_features(vox_d, num_d, coors_d, w, scale, shift, net.vx, net.vy, net.x_offset, net.y_offset, canvas=canvas, err_flag=err)


def clear():
    ops.fill_zero(canvas)


feat = kernel()


def scatter():
    return ops.pillar_scatter(feat, coors_d, 1, NY, NX)


def raw_kernel():   # the launch alone: no checks, no allocation
    check(lib.sessd_pillar_features(vox_d.data_ptr(), num_d.data_ptr(), coors_d.data_ptr(), 0, N, T, 4, net.vx, net.vy, net.x_offset,
                                    net.y_offset, w.data_ptr(), scale.data_ptr(), shift.data_ptr(), 64, 0, 1, NY, NX, feat.data_ptr(),
                                    canvas.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream), "pillar_features")


def torch_modules():   # the mirror's torch formulation: what runs for several PFN layers, in training mode or on the CPU
    scat.nx, scat.ny = NX, NY
    with torch.no_grad():
        return scat._forward_torch(net._forward_torch(vox_d, num_d, coors_d), coors_d, 1)


# same results first (the fallback is a float32 torch evaluation: 1e-5 of the largest feature)
clear()
kernel()
ref = torch_modules()
assert int(err.item()) == 0
diff = float((canvas - ref).abs().max()) / float(ref.abs().max())
assert diff < 1e-5, diff
if trace:   # under rocprofv3 --kernel-trace --stats: a few launches of each kernel, their durations are in the trace
    for _ in range(20):
        clear()
        raw_kernel()
        scatter()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace=True, rel_diff_vs_torch=diff)))
    sys.exit(0)
legs = dict(pillar_features_with_canvas=(kernel, 20000), raw_launch_with_canvas=(raw_kernel, 20000), canvas_clear=(clear, 20000),
            pillar_scatter=(scatter, 10000), torch_modules=(torch_modules, 60))
times = {k: [] for k in legs}
for _ in range(rounds):
    for k, (fn, reps) in legs.items():
        times[k].append(timeit(fn, reps))
out = dict(pillars=N, T=T, grid=[NX, NY], mean_points=float(num.mean()), live_point_bytes=int(num.sum()) * 16, canvas_bytes=canvas.numel() * 4,
           rel_diff_vs_torch=diff, rounds=rounds, what="microseconds PER CALL, host enqueue included; reps per window: %s" % {k: v[1] for k, v in legs.items()})
for k, v in times.items():
    out[k + "_us_per_call"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
print(json.dumps(out))
