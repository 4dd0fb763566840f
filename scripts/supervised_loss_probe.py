"""Timing probe of the supervised multi-task head loss: value + gradients with respect to every task's box / cls / dir outputs.
TIME PER CALL (device events around back-to-back calls; the host's share of a call -- autograd, the wrappers, for the torch
formulation its reads of the log terms -- is inside these figures), after warm-up, alternated over several rounds in one process,
medians and the rounds' spread reported. At the two sizes users run:
  pointpillars  B = 2, T = 1, A = 107 136      three_class  B = 2, T = 3, A = 70 400
Legs:
  device            MultiGroupHead.loss_supervised_device (sessd_supervised_loss, three launches) + backward
  device_with_log   the same + supervised_record_to_dict (one host read of the record), what a logging iteration costs
  device_launches   ops.SupervisedLoss.run alone (no autograd, no allocation): the three launches
  torch             MultiGroupHead.loss_supervised (the torch formulation, with the reference's host reads of its log terms) +
                    backward of the tasks' sum
Writes profiles/supervised_loss.json (or the path given) and prints the same JSON line.
Usage: python scripts/supervised_loss_probe.py [rounds] [out.json]"""
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from det3d.models.builder import build_head  # noqa: E402
from sessd_hip import configs  # noqa: E402

rounds = int([a for a in sys.argv[1:] if a.isdigit()][0]) if any(a.isdigit() for a in sys.argv[1:]) else 7
paths = [a for a in sys.argv[1:] if a.endswith(".json")]
out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "supervised_loss.json")
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


def measure(legs):
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            times[k].append(timeit(fn, reps))
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in times.items()}


def make_inputs(B, T, A, n_pos, seed):
    """Head outputs and targets on the device: n_pos positives and 2 % ignored labels per sample and task."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    example = dict(anchors=[], labels=[], reg_targets=[])
    leaves = []
    for t in range(T):
        labels = torch.zeros(B, A, dtype=torch.int32)
        for b in range(B):
            order = torch.randperm(A, generator=g)
            labels[b, order[n_pos:n_pos + A // 50]] = -1
            labels[b, order[:n_pos]] = 1
        anchors = torch.zeros(B, A, 7)
        anchors[..., 6] = torch.randint(0, 2, (B, A), generator=g).float() * 1.57
        tg = torch.randn(B, A, 7, generator=g) * 0.15 * (labels > 0).unsqueeze(-1)
        box = tg + torch.randn(B, A, 7, generator=g) * 0.08
        cls = torch.randn(B, A, generator=g) - 3.0 + 4.5 * (labels > 0)
        example["anchors"].append(anchors.to(dev)), example["labels"].append(labels.to(dev)), example["reg_targets"].append(tg.to(dev))
        leaves.append(dict(box_preds=box.to(dev).requires_grad_(True), cls_preds=cls.to(dev).requires_grad_(True),
                           dir_cls_preds=torch.randn(B, A, 2, generator=g).to(dev).requires_grad_(True)))
    return example, leaves


SIZES = dict(pointpillars=(2, 1, 107136, 60), three_class=(2, 3, 70400, 30))
out = dict(rounds=rounds, what="microseconds PER CALL of loss value + gradients, host enqueue included; medians of alternated rounds")
for name, (B, T, A, n_pos) in SIZES.items():
    head = build_head(copy.deepcopy(configs.kitti_car_model(tasks=configs.KITTI_3CLASS_TASKS[:T])["bbox_head"])).to(dev)
    example, preds = make_inputs(B, T, A, n_pos, 0)
    assert head.supervised_loss_covers(example, preds)
    params = [v for p in preds for v in p.values()]

    def clear():
        for v in params:
            v.grad = None

    def device_step(log=False):
        clear()
        total, rec = head.loss_supervised_device(example, preds)
        total.backward()
        return head.supervised_record_to_dict(rec) if log else total

    def torch_step():
        clear()
        ret = head.loss_supervised(example, preds)
        sum(ret["loss"]).backward()
        return ret

    d = device_step(True)
    got = [v.grad.clone() for v in params]
    r = torch_step()
    rel_grad = max(float((a - v.grad).abs().max() / v.grad.abs().max()) for a, v in zip(got, params))
    rel_loss = max(abs(float(d["loss"][t]) - float(r["loss"][t].detach())) / abs(float(r["loss"][t].detach())) for t in range(T))
    run = head._supervised_device_loss[1]
    tasks = [dict(box=p["box_preds"].detach(), cls=p["cls_preds"].detach(), dir=p["dir_cls_preds"].detach(), labels=example["labels"][t],
                  reg_targets=example["reg_targets"][t], anchors=example["anchors"][t]) for t, p in enumerate(preds)]
    t = measure(dict(device=(device_step, 50), device_with_log=(lambda: device_step(True), 50), device_launches=(lambda: run.run(tasks), 50),
                     torch=(torch_step, 20)))
    spread = max(v["max"] - v["min"] for k, v in t.items() if k in ("device", "torch"))
    out[name] = dict(batch=B, tasks=T, anchors=A, positives_per_sample=n_pos, worst_rel_diff_loss_vs_torch=rel_loss,
                     worst_rel_diff_grads_vs_torch=rel_grad, device_us=t["device"], device_with_log_us=t["device_with_log"],
                     device_launches_us=t["device_launches"], torch_us=t["torch"], speedup=t["torch"]["median"] / t["device"]["median"],
                     rounds_spread_us=spread, device_slower_beyond_spread=bool(t["device"]["median"] - t["torch"]["median"] > spread))
    del head, example, preds, params
    torch.cuda.empty_cache()
out["device_is_default"] = not any(out[k]["device_slower_beyond_spread"] for k in SIZES)

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
