"""Timing probe of sessd_hip.PillarEngine at the PointPillars config's full size: configs.kitti_pointpillars_model() with seeded,
calibrated weights, VOXEL_GENERATOR_POINTPILLARS (432 x 496 canvas, 248 x 216 head map), TEST_CFG_POINTPILLARS, batch 1, 20 000-point
synth.make_frame clouds. Device events around back-to-back calls, each window a few tenths of a second, the legs ALTERNATED over
several rounds, medians reported (min / max beside them). Writes one JSON file (default profiles/pillar_engine.json):
  (a) time per frame of the module path (ops.voxelize_frames + the det3d-mirror PointPillars, its one read-back of the counts
      included), of PillarEngine.enqueue() eager, and of replay() -- with the one-launch up-samplers and with the module path's
      lowering (`fused_upsamplers = False`);
  (b) PillarEngine.stage_times(): voxelize (with its hash and list clears), canvas_clear, pillar (the engine's default front end,
      "fused", reports canvas_clear and front_end instead: scripts/pillar_front_end_probe.py), blk<i>, up<i>, head, predict;
  (c) every up-sampler alone on the frame's own block outputs: sessd_deconv_ks_slice against the module path's lowering
      (s * s one-tap launches into a scratch map) + the copy into the slice, interleaved.
Before any timing the outputs are compared: the parent-lowering engine against the module path (bit for bit) and the fused head map
against it (relative to the largest head value). Usage: python scripts/pillar_engine_probe.py [rounds] [--out FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from sessd_hip import PillarEngine, configs, ops, synth  # noqa: E402
from det3d.models import build_detector  # noqa: E402

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "pillar_engine.json")
rounds = int([a for a in args if a.isdigit()][0]) if any(a.isdigit() for a in args) else 5
assert torch.cuda.is_available(), "this probe measures on the MI355X: no device, no figures"
dev = torch.device("cuda", 0)
VG, TC = configs.VOXEL_GENERATOR_POINTPILLARS, configs.TEST_CFG_POINTPILLARS
POINTS = 20000


def window(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # microseconds per call


def alternate(legs):
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            times[k].append(window(fn, reps))
    return {k: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2), reps_per_window=legs[k][1])
            for k, v in times.items()}


# ---- the seeded model, BatchNorm statistics and classification bias calibrated on frame 0 (torch modules, set-up only)
model = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=TC)
synth.init_synthetic_weights(model, 0)
model.to(dev)
cal = ops.voxelize_batch([torch.from_numpy(synth.make_frame(0, POINTS)).to(dev)], VG["voxel_size"], VG["range"], VG["max_points_in_voxel"],
                         VG["max_voxel_num"])
m = int(cal["prefix"][1].item())
grid = cal["grid"].tolist()
run = lambda _f, c, b, shape: model.backbone(model.reader(cal["voxels"][:m], cal["num_points"][:m], c), c, b, shape)
synth.calibrate_synthetic_model(model, None, cal["coors"][:m].contiguous(), 1, grid, sparse_runner=run)
model.eval()

frame = torch.from_numpy(synth.make_frame(1, POINTS)).to(dev)
eng = PillarEngine(model, VG, TC, batch_size=1, max_points=POINTS)
par = PillarEngine(model, VG, TC, batch_size=1, max_points=POINTS)
par.fused_upsamplers = False
anchors = eng.anchors[None] if eng.anchors.dim() == 2 else eng.anchors


def module_path():
    r = ops.voxelize_frames([frame], VG["voxel_size"], VG["range"], VG["max_points_in_voxel"], VG["max_voxel_num"])
    n = r["prefix"][1:].cpu()    # the module path needs the count on the host to slice its inputs
    k = int(n[0])
    example = dict(voxels=r["voxels"][:k], coordinates=r["coors"][:k], num_points=r["num_points"][:k], num_voxels=n, shape=[grid],
                   anchors=[anchors], metadata=[None])
    with torch.no_grad():
        return model(example, return_loss=False), example


# ---- same results first
for e in (eng, par):
    e.set_points([frame])
    e.enqueue()
want, example = module_path()
with torch.no_grad():
    data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"], batch_size=1, input_shape=grid)
    head_mod = model.bbox_head(model.extract_feat(data))[0]["_planar"]
torch.cuda.synchronize()
pillars = int(eng.prefix[1].item())
n_det = int(par.out["count"][0].item())
same = dict(parent_head_bit_equal=bool(torch.equal(par.head.view_as(head_mod), head_mod)),
            parent_boxes_bit_equal=bool(n_det == len(want[0]["scores"]) and torch.equal(par.out["box"][0, :n_det], want[0]["box3d_lidar"])
                                        and torch.equal(par.out["score"][0, :n_det], want[0]["scores"])),
            fused_head_max_abs_diff_over_max=float((eng.head.view_as(head_mod) - head_mod).abs().max() / head_mod.abs().max()),
            fused_detections=int(eng.out["count"][0].item()), parent_detections=n_det)
assert same["parent_head_bit_equal"] and same["parent_boxes_bit_equal"] and same["fused_head_max_abs_diff_over_max"] < 2e-4, same
assert int(eng.err.item()) == 0 and int(par.err.item()) == 0

# ---- (b) stages, eager
stages = {k: round(v * 1e3, 2) for k, v in eng.stage_times(reps=20).items()}
stages_parent = {k: round(v * 1e3, 2) for k, v in par.stage_times(reps=20).items()}

# ---- (a) whole frames
eng.capture(warmup=2)
par.capture(warmup=2)
frames = alternate(dict(module_path=(lambda: module_path(), 60), enqueue_eager=(eng.enqueue, 150), replay=(eng.replay, 300),
                        replay_parent_lowering=(par.replay, 300), replay_and_results=(lambda: (eng.replay(), eng.results()), 200)))

# ---- (c) the up-samplers alone, on the frame's block outputs
ups = {}
for i, u in enumerate(eng.ups):
    x = u["x"]

    def fused(u=u, x=x):
        ops.deconv_ks_slice(x, u["fused"], u["scale"], u["shift"], True, eng.neck, u["c_off"])

    def lowered(u=u, x=x):
        ops.conv2d(x, u["parent"], u["scale"], u["shift"], True, None, out=u["scratch"])

    def lowered_copy(u=u, x=x):
        lowered(u, x)
        eng.neck[:, u["c_off"]:u["c_off"] + u["cout"]].copy_(u["scratch"])

    t = alternate(dict(one_launch=(fused, 3000), lowered=(lowered, 1500), lowered_plus_copy=(lowered_copy, 1500)))
    flop = 2.0 * x.shape[1] * u["cout"] * u["s"] ** 2 * x.shape[2] * x.shape[3]
    ups["up%d" % i] = dict(stride=u["s"], cin=int(x.shape[1]), cout=u["cout"], in_hw=[int(x.shape[2]), int(x.shape[3])], gflop=round(flop / 1e9, 3),
                           launches_lowered=len(u["parent"].launches), us_per_call=t,
                           one_launch_tflops_enqueue_included=round(flop / t["one_launch"]["median"] / 1e6, 1))

out = dict(what="microseconds per call (device events around back-to-back calls, the host's enqueue inside the figure); stages: "
                "microseconds between HIP events of an eager frame", config="kitti_pointpillars_model, batch 1, %d points" % POINTS,
           canvas=[eng.ny, eng.nx], head_map=[eng.H, eng.W], pillars=pillars, rounds=rounds, same_results=same, frame_us=frames,
           stage_us=stages, stage_us_parent_lowering=stages_parent, upsamplers=ups)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
