"""Timing probe of the train-mode RPN neck (RPN._forward_train). TIME PER CALL (device events around back-to-back calls; the
host's share of a call -- autograd, allocation, the wrappers -- is inside these figures), alternated over several rounds, medians
reported:
  (a) each up-sampler of the PointPillars neck, forward + backward with a random output gradient, batch 2:
      64 -> 128 s = 1 at 248 x 216, 128 -> 128 s = 2 at 124 x 108, 256 -> 128 s = 4 at 62 x 54;
      ops.DeconvKsFunction against F.conv_transpose2d autograd on the same device;
  (b) one forward + backward of the whole train-mode neck, batch 2, for the PointPillars neck (64 x 496 x 432 canvas) and the
      three-class config's neck (128 x 200 x 176): fused_train True against False (every layer its torch module); for the
      PointPillars neck a third arm, fused_train with train_any_width = True (the convs whose width is no multiple of 8 -- maps
      124 x 108 and 62 x 54 -- on the device too, weight gradient by sessd_conv2d_wgrad_any_width).
Writes profiles/rpn_train.json (or the path given) and prints the same JSON line.
Usage: python scripts/rpn_train_probe.py [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from det3d.models.necks.rpn_v1 import RPN  # noqa: E402
from sessd_hip import ops  # noqa: E402

rounds = int([a for a in sys.argv[1:] if a.isdigit()][0]) if any(a.isdigit() for a in sys.argv[1:]) else 5
paths = [a for a in sys.argv[1:] if a.endswith(".json")]
out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "rpn_train.json")
dev = torch.device("cuda", 0)
B = 2


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds


def measure(legs):
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            times[k].append(timeit(fn, reps))
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in times.items()}


out = dict(batch=B, rounds=rounds, what="microseconds PER CALL, forward + backward, host enqueue included; medians of alternated rounds")

# (a) the up-samplers alone
ups = {}
for cin, s, H, W in ((64, 1, 248, 216), (128, 2, 124, 108), (256, 4, 62, 54)):
    torch.manual_seed(s)
    x = torch.randn(B, cin, H, W, device=dev, requires_grad=True)
    w = ((torch.rand(cin, 128, s, s, device=dev) * 2 - 1) * (3.0 / cin) ** 0.5).requires_grad_(True)
    g = torch.randn(B, 128, s * H, s * W, device=dev)

    def step(fn, x=x, w=w, g=g):
        x.grad = w.grad = None
        fn(x, w).backward(g)
        return x.grad, w.grad

    dev_fn = lambda x, w, s=s: ops.DeconvKsFunction.apply(x, w, s)
    ref_fn = lambda x, w, s=s: F.conv_transpose2d(x, w, stride=s)
    (gx, gw), (rx, rw) = step(dev_fn), step(ref_fn)
    rel = dict(gx=float((gx - rx).abs().max() / rx.abs().max()), gw=float((gw - rw).abs().max() / rw.abs().max()))
    t = measure(dict(device=(lambda: step(dev_fn), 50), torch=(lambda: step(ref_fn), 50)))
    ups["%d->128 s=%d %dx%d" % (cin, s, H, W)] = dict(rel_diff_vs_torch=rel, device_us=t["device"], torch_us=t["torch"],
                                                      speedup=t["torch"]["median"] / t["device"]["median"])
    del x, w, g
out["up_samplers_forward_backward"] = ups

# (b) the whole neck
NECKS = {
    "pointpillars": (dict(layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[1, 2, 4],
                          us_num_filters=[128, 128, 128], num_input_features=64, norm_cfg=None), (B, 64, 496, 432)),
    "three_class": (dict(layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1], us_num_filters=[128],
                         num_input_features=128, norm_cfg=None), (B, 128, 200, 176)),
}
necks = {}
for name, (args, shape) in NECKS.items():
    torch.manual_seed(0)
    neck = RPN(**args).to(dev).train()
    x = torch.randn(*shape, device=dev, requires_grad=True)
    neck.fused_train = True
    with torch.no_grad():
        g = torch.randn_like(neck(x))

    def step(fused, any_width=False, neck=neck, x=x, g=g):
        neck.fused_train, neck.train_any_width = fused, any_width
        x.grad = None
        for p in neck.parameters():
            p.grad = None
        neck(x).backward(g)

    step(True)
    fused_grads = {k: p.grad.clone() for k, p in neck.named_parameters()}
    step(False)
    rel = max(float((fused_grads[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in neck.named_parameters())
    legs = dict(fused=(lambda: step(True), 10), torch=(lambda: step(False), 10))
    third = name == "pointpillars"   # the only neck here with maps whose width is no multiple of 8
    if third:
        torch_grads = {k: p.grad.clone() for k, p in neck.named_parameters()}
        step(True, True)
        rel_any = max(float((torch_grads[k] - p.grad).abs().max() / torch_grads[k].abs().max().clamp_min(1e-30))
                      for k, p in neck.named_parameters())
        legs["any_width"] = (lambda: step(True, True), 10)
    t = measure(legs)
    spread = max(v["max"] - v["min"] for v in t.values())
    necks[name] = dict(input=list(shape), worst_rel_diff_param_grads_vs_torch=rel, fused_us=t["fused"], torch_us=t["torch"],
                       speedup=t["torch"]["median"] / t["fused"]["median"], rounds_spread_us=spread,
                       fused_slower_beyond_spread=bool(t["fused"]["median"] - t["torch"]["median"] > spread))
    if third:
        best_other = min(t["fused"]["median"], t["torch"]["median"])
        necks[name].update(any_width_us=t["any_width"], any_width_worst_rel_diff_param_grads_vs_torch=rel_any,
                           any_width_speedup_vs_torch=t["torch"]["median"] / t["any_width"]["median"],
                           any_width_speedup_vs_fused=t["fused"]["median"] / t["any_width"]["median"],
                           any_width_faster_than_both_beyond_spread=bool(best_other - t["any_width"]["median"] > spread))
    del neck, x, g, fused_grads
    torch.cuda.empty_cache()
out["neck_forward_backward"] = necks

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
