"""Timing probe of the batched anchor target assignment (ops.AssignTargets -> sessd_assign_targets_batch: one clear and two launches
for all frames and tasks, written straight into the caller's tensors) against the loop that does the same work today: per frame
and task one ops.assign_targets call (a fill and two launches, four allocations) plus the copies of labels and targets into the
(B, A) / (B, A, 7) tensors of the example, as trainloop.DeviceBatcher.load does per view.
TIME PER BATCH (device events around back-to-back batches; the host's enqueue is inside these figures), after warm-up, the two
legs alternated over several rounds in one process, medians and the rounds' spread reported. 15 boxes per frame, of the task's
class, at the sizes users run:
  second_car    B = 4, T = 1, A = 70 400      three_class  B = 2, T = 3, A = 70 400      pointpillars  B = 2, T = 1, A = 107 136
Both legs must leave the same bits before anything is timed.
Writes profiles/assign_targets_batch.json (or the path given) and prints the same JSON line.
Usage: python scripts/assign_targets_probe.py [rounds] [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from sessd_hip import configs, ops  # noqa: E402
from sessd_hip.anchors import create_anchors_3d_range  # noqa: E402

rounds = max(7, int([a for a in sys.argv[1:] if a.isdigit()][0])) if any(a.isdigit() for a in sys.argv[1:]) else 7
paths = [a for a in sys.argv[1:] if a.endswith(".json")]
out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "assign_targets_batch.json")
dev = torch.device("cuda", 0)
BOXES = 15


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


def task_anchors(assigner):
    fmap = assigner.get("feature_map_size", [1, 200, 176])
    return [(create_anchors_3d_range(fmap, g["anchor_ranges"], g["sizes"], g["rotations"]).reshape(-1, 7), g)
            for g in assigner["target_assigner"]["anchor_generators"]]


def boxes(rng, B, gens):
    """(B, T * 15, 7) boxes and (B, T * 15) classes: 15 per frame and task, sized like the task's anchors"""
    T = len(gens)
    gt = np.zeros((B, T * BOXES, 7), np.float32)
    cls = np.zeros((B, T * BOXES), np.int32)
    for t, g in enumerate(gens):
        s = slice(t * BOXES, (t + 1) * BOXES)
        gt[:, s, 0], gt[:, s, 1], gt[:, s, 2] = rng.uniform(2, 66, (B, BOXES)), rng.uniform(-36, 36, (B, BOXES)), g["anchor_ranges"][2]
        gt[:, s, 3:6] = np.array(g["sizes"], np.float32) * rng.uniform(0.9, 1.1, (B, BOXES, 3))
        gt[:, s, 6] = rng.uniform(-np.pi, np.pi, (B, BOXES))
        cls[:, s] = t + 1
    return gt, cls


SIZES = dict(second_car=(4, dict(configs.ASSIGNER_POINTPILLARS, feature_map_size=[1, 200, 176])), three_class=(2, configs.ASSIGNER_3CLASS),
             pointpillars=(2, configs.ASSIGNER_POINTPILLARS))
out = dict(rounds=rounds, boxes_per_frame_and_task=BOXES,
           what="microseconds PER BATCH of labels + regression targets of all frames and tasks inside (B, A) / (B, A, 7) tensors, host "
                "enqueue included; medians of alternated rounds")
for name, (B, assigner) in SIZES.items():
    pairs = task_anchors(assigner)
    gens = [g for _, g in pairs]
    T, A = len(pairs), pairs[0][0].shape[0]
    anchors = [torch.from_numpy(a).to(dev) for a, _ in pairs]
    gt_np, cls_np = boxes(np.random.RandomState(0), B, gens)
    gt, cls = torch.from_numpy(gt_np).to(dev), torch.from_numpy(cls_np).to(dev)
    per_task = [[gt[b, t * BOXES:(t + 1) * BOXES].contiguous() for b in range(B)] for t in range(T)]
    mk = lambda: (dict(labels=[torch.zeros(B, A, dtype=torch.int32, device=dev) for _ in range(T)],
                       reg_targets=[torch.zeros(B, A, 7, device=dev) for _ in range(T)]))
    ex_loop, ex_batch = mk(), mk()
    op = ops.AssignTargets(B, A, [dict(anchors=anchors[t], class_id=t + 1, matched_threshold=g["matched_threshold"],
                                       unmatched_threshold=g["unmatched_threshold"]) for t, g in enumerate(gens)], dev, gt_capacity=T * BOXES)
    dest = dict(labels=ex_batch["labels"], reg_targets=ex_batch["reg_targets"], reg_weights=False, gt_id=False)

    def loop():
        for t, g in enumerate(gens):
            for b in range(B):
                tg = ops.assign_targets(anchors[t], per_task[t][b], None, g["matched_threshold"], g["unmatched_threshold"])
                ex_loop["labels"][t][b].copy_(tg["labels"])
                ex_loop["reg_targets"][t][b].copy_(tg["bbox_targets"])

    def batched():
        op.run(gt, cls, None, out=dest)

    loop(), batched()
    torch.cuda.synchronize()
    same = all(torch.equal(ex_loop[k][t], ex_batch[k][t]) for k in ex_loop for t in range(T))
    positives = int(sum(int((v > 0).sum()) for v in ex_batch["labels"]))
    t_us = measure(dict(loop=(loop, 20), batched=(batched, 50)))
    spread = max(v["max"] - v["min"] for v in t_us.values())
    out[name] = dict(batch=B, tasks=T, anchors=A, positives=positives, same_bits_as_loop=bool(same), loop_us=t_us["loop"],
                     batched_us=t_us["batched"], speedup=t_us["loop"]["median"] / t_us["batched"]["median"], rounds_spread_us=spread,
                     batched_faster_beyond_spread=bool(t_us["loop"]["median"] - t_us["batched"]["median"] > spread))
    assert same, name
out["batched_faster_beyond_spread_everywhere"] = all(out[k]["batched_faster_beyond_spread"] for k in SIZES)

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
