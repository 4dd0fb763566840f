"""Timing probe of the PointPillars reader + scatter in TRAIN mode at the config's size (the set-up of scripts/pillar_probe.py:
12 000 pillars of T = 100 slots, geometric point counts of mean about 7, the 432 x 496 grid, one frame). TIME PER CALL (device
events around back-to-back calls; the host's share of a call -- autograd, allocation, the wrappers -- is inside these figures) of
  * device:  PillarFeatureNet (fused_train: ops.pillar_features_train) + PointPillarsScatter (ops.pillar_scatter_train),
             forward alone and forward + backward with a random canvas gradient,
  * torch:   the same modules' torch formulation (`_forward_torch` of reader and scatter, what train mode ran before) on the
             same device, forward alone and forward + backward,
alternated over several rounds, medians reported; prints one JSON line. KERNEL times come from a run of this script under
`rocprofv3 --kernel-trace --stats` (`--trace`: twenty device steps, no timing).
Usage: python scripts/pillar_train_probe.py [rounds | --trace]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter  # noqa: E402

N, T, NX, NY = 12000, 100, 432, 496
trace = "--trace" in sys.argv
rounds = int([a for a in sys.argv[1:] if a.isdigit()][0]) if any(a.isdigit() for a in sys.argv[1:]) else 5
dev = torch.device("cuda", 0)


def timeit(fn, reps):
    for _ in range(3):
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
vox_d, num_d, coors_d = (torch.from_numpy(a).to(dev) for a in (vox, num, coors))
grad_canvas = torch.randn((1, 64, NY, NX), device=dev)

nets = {}
for name in ("device", "torch"):
    torch.manual_seed(0)
    net = PillarFeatureNet(num_filters=[64]).train()
    with torch.no_grad():
        net.pfn_layers[0].norm.bias.normal_(0, 0.1)
    net.fused_train = name == "device"
    nets[name] = (net.to(dev), PointPillarsScatter(num_input_features=64).train())
assert nets["device"][0].on_device_train_path(vox_d) and not nets["torch"][0].on_device_train_path(vox_d)


def forward(name):
    net, scat = nets[name]
    feat = net(vox_d, num_d, coors_d)
    if name == "device":
        return scat(feat, coors_d, 1, [NX, NY, 1])
    scat.nx, scat.ny = NX, NY
    return scat._forward_torch(feat, coors_d, 1)


def step(name):
    for p in nets[name][0].parameters():
        p.grad = None
    forward(name).backward(grad_canvas)


# the same results first (the torch formulation is a float32 evaluation)
outs = {k: forward(k).detach() for k in nets}
rel = float((outs["device"] - outs["torch"]).abs().max()) / float(outs["torch"].abs().max())
assert rel < 1e-5, rel
grad_rel = {}
for k in nets:
    step(k)
for (na, pa), (_, pb) in zip(nets["device"][0].named_parameters(), nets["torch"][0].named_parameters()):
    grad_rel[na] = float((pa.grad - pb.grad).abs().max()) / float(pb.grad.abs().max())
del outs
if trace:   # under rocprofv3 --kernel-trace --stats: the kernels' durations are in the trace
    for _ in range(20):
        step("device")
    torch.cuda.synchronize()
    print(json.dumps(dict(trace=True, rel_diff_canvas_vs_torch=rel)))
    sys.exit(0)

legs = dict(device_forward=(lambda: forward("device"), 2000), device_forward_backward=(lambda: step("device"), 1000),
            torch_forward=(lambda: forward("torch"), 100), torch_forward_backward=(lambda: step("torch"), 50))
times = {k: [] for k in legs}
for _ in range(rounds):
    for k, (fn, reps) in legs.items():
        times[k].append(timeit(fn, reps))
out = dict(pillars=N, T=T, grid=[NX, NY], mean_points=float(num.mean()), rel_diff_canvas_vs_torch=rel, rel_diff_grads_vs_torch=grad_rel,
           rounds=rounds, what="microseconds PER CALL (reader + scatter, train mode), host enqueue included; reps per window: %s"
           % {k: v[1] for k, v in legs.items()})
for k, v in times.items():
    out[k + "_us_per_call"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
out["speedup_forward_backward"] = out["torch_forward_backward_us_per_call"]["median"] / out["device_forward_backward_us_per_call"]["median"]
print(json.dumps(out))
