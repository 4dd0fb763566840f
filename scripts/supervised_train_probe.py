"""Timing probe of the supervised training path (train.SupervisedTrainStep, trainloop.SupervisedBatcher) on one MI355X, one process,
the legs of each comparison alternated over several rounds, medians and the rounds' spread reported.
  (a) microseconds per batch of the LOADER at full PointPillars size (107 136 anchors, 100 points per pillar, 12 000 pillars per
      frame, ~20 000-point clouds, B = 2 and B = 4): SupervisedBatcher.load (sessd_draw_batch, sessd_voxelize_frames into the
      example, sessd_assign_targets_batch into the example) against the same batch assembled the way trainloop.DeviceBatcher does
      it -- its torch formulation of the augmentation and the range filter per frame, ops.voxelize_frames and the masked copies,
      ops.assign_targets and two copies per frame. Device events around back-to-back batches, the host's enqueue inside the
      figure. Both must leave the same bits before anything is timed.
  (b) milliseconds per ITERATION on one fixed batch, eager (device schedule) against the replayed graph: the PointPillars config at
      full size (B = 2, neck.train_any_width = True) and the three-class SECOND config (B = 2). A leg that cannot run is recorded
      with its error instead of a figure.
Writes profiles/supervised_train.json (or the path given) and prints the same JSON line.
Usage: python scripts/supervised_train_probe.py [rounds] [out.json]"""
import copy
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from sessd_hip import configs, ops, synth, trainloop  # noqa: E402
from sessd_hip import train as strain  # noqa: E402
from sessd_hip.anchors import create_task_anchors  # noqa: E402

rounds = max(5, int([a for a in sys.argv[1:] if a.isdigit()][0])) if any(a.isdigit() for a in sys.argv[1:]) else 5
paths = [a for a in sys.argv[1:] if a.endswith(".json")]
out_path = paths[0] if paths else os.path.join(ROOT, "profiles", "supervised_train.json")
dev = torch.device("cuda", 0)


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


def compare(t, a, b):
    """a against b: medians, spread of the rounds, and whether a is faster beyond it"""
    spread = max(v["max"] - v["min"] for v in t.values())
    return dict(times=t, ratio=t[b]["median"] / t[a]["median"], rounds_spread=spread,
                faster_beyond_spread=bool(t[b]["median"] - t[a]["median"] > spread))


PPV = configs.VOXEL_GENERATOR_POINTPILLARS
PP_GRID = [432, 496, 1]
PP_HW = (248, 216)
pool = trainloop.ScenePool(range(700, 708), 20000)
out = dict(rounds=rounds, what="medians of alternated rounds in one process on one MI355X; loader legs in microseconds per batch, "
                               "iteration legs in milliseconds per iteration; host enqueue inside every figure")


# ------------------------------------------------------------------------------------------------------------------ (a) loader
def loader_legs(B, iterations=8):
    r = PPV["range"]
    anc = create_task_anchors(PP_HW, [configs.KITTI_3CLASS_ANCHORS[0]], (r[0], r[1], r[3], r[4]))[0]
    tasks = [dict(anchors=anc, class_id=1, matched_threshold=0.6, unmatched_threshold=0.45)]
    data = trainloop.SupervisedBatcher.from_scene_pool(pool, dev, B, iterations, PPV, PPV["max_points_in_voxel"], PPV["max_voxel_num"],
                                                      tasks, PP_GRID, seed=0)
    # the loader this replaces: DeviceBatcher's arithmetic (its constructor is tied to the SE-SSD config: the methods alone)
    old = object.__new__(trainloop.DeviceBatcher)
    old.lo = torch.tensor(r[:2], dtype=torch.float32, device=dev)
    old.hi = torch.tensor(r[3:5], dtype=torch.float32, device=dev)
    frames = [torch.from_numpy(f).to(dev) for f in pool.frames]
    boxes = [torch.from_numpy(pool.visible(i).astype(np.float32)).to(dev) for i in range(len(pool))]
    par, anchors = torch.from_numpy(data.par_host).to(dev), torch.from_numpy(anc).to(dev)
    cap, A = B * PPV["max_voxel_num"], anc.shape[0]
    rows = torch.arange(cap, device=dev, dtype=torch.int32)
    ex2 = dict(voxels=torch.zeros((cap, PPV["max_points_in_voxel"], 4), device=dev), coordinates=torch.full((cap, 4), -1, dtype=torch.int32, device=dev),
               num_points=torch.ones(cap, dtype=torch.int32, device=dev), num_voxels_dev=torch.zeros(1, dtype=torch.int32, device=dev),
               labels=[torch.zeros((B, A), dtype=torch.int32, device=dev)], reg_targets=[torch.zeros((B, A, 7), device=dev)],
               transformation_dev=torch.zeros((B, 5), device=dev))

    def torch_load(it):
        idx = data.choice_host[it]
        clouds = [old._student_cloud(frames[i], par[it, b]) for b, i in enumerate(idx)]
        v = ops.voxelize_frames(clouds, PPV["voxel_size"], r, PPV["max_points_in_voxel"], PPV["max_voxel_num"])
        n = v["prefix"][B:B + 1]
        live = rows < n
        ex2["voxels"].copy_(torch.where(live[:, None, None], v["voxels"], 0.0))
        ex2["coordinates"].copy_(torch.where(live[:, None], v["coors"], -1))
        ex2["num_points"].copy_(torch.where(live, v["num_points"], 1))
        ex2["num_voxels_dev"].copy_(n)
        for b, i in enumerate(idx):
            tg = ops.assign_targets(anchors, old._in_range(old._student_boxes(boxes[i], par[it, b])), None, 0.6, 0.45)
            ex2["labels"][0][b].copy_(tg["labels"])
            ex2["reg_targets"][0][b].copy_(tg["bbox_targets"])
        ex2["transformation_dev"].copy_(par[it])

    same, positives = True, 0
    for it in range(iterations):
        ex = data.load(it)
        torch_load(it)
        m = int(ex["num_voxels_dev"].item())
        same = same and m == int(ex2["num_voxels_dev"].item()) and all(
            torch.equal(a, b) for a, b in ((ex["voxels"][:m], ex2["voxels"][:m]), (ex["coordinates"][:m], ex2["coordinates"][:m]),
                                           (ex["num_points"][:m], ex2["num_points"][:m]), (ex["labels"][0], ex2["labels"][0]),
                                           (ex["reg_targets"][0], ex2["reg_targets"][0]), (ex["transformation_dev"], ex2["transformation_dev"])))
        positives += int((ex["labels"][0] > 0).sum())
    state = dict(it=0)

    def kernels():
        data.load(state["it"] % iterations)
        state["it"] += 1

    def torch_form():
        torch_load(state["it"] % iterations)
        state["it"] += 1

    res = compare(measure(dict(draw_batch=(kernels, 20), torch_formulation=(torch_form, 10))), "draw_batch", "torch_formulation")
    res.update(batch=B, anchors=A, points_per_scene=data.draw.P, boxes_per_scene=data.draw.G, same_bits=bool(same), positives=positives,
               pillars_last_batch=m, unit="us per batch")
    return res


for B in (2, 4):
    out["loader_pointpillars_b%d" % B] = loader_legs(B)


# ------------------------------------------------------------------------------------------------------------------ (b) iteration
def iteration_legs(model, data, reps=10):
    """eager against replay on batch 0, each on its own copy of the model"""
    ex = data.load(0)
    torch.cuda.synchronize()
    not_on_kernels = strain.check_trainable(model, ex)
    eager = strain.SupervisedTrainStep(copy.deepcopy(model), total_steps=100000)
    graph = strain.SupervisedTrainStep(copy.deepcopy(model), total_steps=100000)
    graph.capture(ex, warmup=2)
    res = compare(measure(dict(replay=(graph.replay, reps), eager=(lambda: eager(ex, device_schedule=True), reps))), "replay", "eager")
    rec = graph.record()
    res.update(batch=data.B, not_on_kernels=not_on_kernels, unit="ms per iteration", pillars_or_voxels=int(ex["num_voxels_dev"].item()),
               last_total=float(rec["total"]), finite=bool(torch.isfinite(graph.flat.data).all()))
    for v in res["times"].values():
        for k in v:
            v[k] /= 1e3
    res["rounds_spread"] /= 1e3
    return res


def pointpillars():
    from det3d.models import build_detector
    model = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    synth.init_synthetic_weights(model, 0)
    model = model.to(dev).train()
    model.supervised = True
    model.neck.train_any_width = True
    r = PPV["range"]
    anc = create_task_anchors(PP_HW, [configs.KITTI_3CLASS_ANCHORS[0]], (r[0], r[1], r[3], r[4]))[0]
    tasks = [dict(anchors=anc, class_id=1, matched_threshold=0.6, unmatched_threshold=0.45)]
    data = trainloop.SupervisedBatcher.from_scene_pool(pool, dev, 2, 4, PPV, PPV["max_points_in_voxel"], PPV["max_voxel_num"], tasks, PP_GRID)
    return iteration_legs(model, data)


def three_class():
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_rpn_model())
    anc = configs.kitti_3class_anchors((200, 176))
    gens = configs.ASSIGNER_3CLASS["target_assigner"]["anchor_generators"]
    tasks = [dict(anchors=anc[t], class_id=t + 1, matched_threshold=g["matched_threshold"], unmatched_threshold=g["unmatched_threshold"])
             for t, g in enumerate(gens)]
    data = trainloop.SupervisedBatcher.from_scene_pool(pool, dev, 2, 4, VG, VG["max_points_in_voxel"], 16000, tasks, [1408, 1600, 40])
    return iteration_legs(model, data)


for name, leg in (("iteration_pointpillars_b2", pointpillars), ("iteration_three_class_b2", three_class)):
    try:
        out[name] = leg()
    except Exception as e:   # recorded, not hidden: the file says which leg did not run and why
        if any(s in str(e).lower() for s in ("illegal memory access", "hip error", "hiperror", "launch failure")):
            raise            # a device fault ends the probe: nothing more is started on the device
        out[name] = dict(error="%s: %s" % (type(e).__name__, e), traceback=traceback.format_exc().splitlines()[-6:])

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
