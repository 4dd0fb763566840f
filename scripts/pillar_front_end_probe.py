"""The two front ends of sessd_hip.PillarEngine at the PointPillars config's full size, and the host-fed runner over PillarEngines:
configs.kitti_pointpillars_model() with seeded, calibrated weights, VOXEL_GENERATOR_POINTPILLARS (432 x 496 canvas),
TEST_CFG_POINTPILLARS, batch 1, 20 000-point synth.make_frame clouds -- the set-up and the method of scripts/pillar_engine_probe.py:
device events around back-to-back calls, the legs ALTERNATED over several rounds, medians with min / max beside them.
Writes one JSON file (default profiles/pillar_front_end_fused.json):
  (a) the front end alone (hash clear, canvas clear, clouds -> canvas), front_end="tensor" against "fused": as a captured graph of
      that part replayed back to back, and as eager calls; beside them the three clears alone (hash, canvas, the voxelizer's
      hash_capacity x T list fill), which both front ends share;
  (b) the whole frame, replay(), in both modes;
  (c) frames/s of four engines on two CU sets fed from the host (runner.pillar_engines_on_cu_sets + HostFedPipeline, wall clock from
      the first submit() to the return of finish()) against one engine's replay(), per mode;
  (d) `default`: "fused" if its median front-end time (graph) is below tensor mode's by more than the round-to-round spread
      (max - min) of either, else "tensor" -- the rule PillarEngine's DEFAULT_FRONT_END follows.
Before any timing the two modes' outputs are compared bit for bit. Usage: python scripts/pillar_front_end_probe.py [rounds] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
import torch  # noqa: E402
from sessd_hip import HostFedPipeline, PillarEngine, check, configs, lib, ops, pillar_engines_on_cu_sets, synth  # noqa: E402
from det3d.models import build_detector  # noqa: E402

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "pillar_front_end_fused.json")
rounds = int([a for a in args if a.isdigit()][0]) if any(a.isdigit() for a in args) else 5
assert torch.cuda.is_available(), "this probe measures on the MI355X: no device, no figures"
dev = torch.device("cuda", 0)
VG, TC = configs.VOXEL_GENERATOR_POINTPILLARS, configs.TEST_CFG_POINTPILLARS
POINTS = 20000
MODES = ("tensor", "fused")
JOB_FRAMES, FETCH_EVERY = 400, 16


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


def summary(v, **more):
    return dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2), **more)


def alternate(legs):
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            times[k].append(window(fn, reps))
    return {k: summary(v, reps_per_window=legs[k][1]) for k, v in times.items()}


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
del cal

host_frame = synth.make_frame(1, POINTS)
frame = torch.from_numpy(host_frame).to(dev)
engs = {mode: PillarEngine(model, VG, TC, batch_size=1, max_points=POINTS, front_end=mode) for mode in MODES}

# ---- same results first
for e in engs.values():
    e.set_points([frame])
    e.enqueue()
torch.cuda.synchronize()
t, f = engs["tensor"], engs["fused"]
n_det = int(t.out["count"][0].item())
same = dict(prefix=bool(torch.equal(t.prefix, f.prefix)), canvas=bool(torch.equal(t.canvas, f.canvas)), head=bool(torch.equal(t.head, f.head)),
            detections=bool(n_det == int(f.out["count"][0].item()) and torch.equal(t.out["box"][0, :n_det], f.out["box"][0, :n_det])
                            and torch.equal(t.out["score"][0, :n_det], f.out["score"][0, :n_det])), n_detections=n_det)
assert all(same.values()) and int(t.err.item()) == 0 and int(f.err.item()) == 0, same
pillars = int(f.prefix[1].item())
live = f.nump[:pillars].float()
stages = {mode: {k: round(v * 1e3, 2) for k, v in e.stage_times(reps=20).items()} for mode, e in engs.items()}


# ---- (a) the front end alone: a graph of that part per mode, and eager calls
def front_graph(e):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        e._enqueue_front(s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ops.new_capture_epoch()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e._enqueue_front(torch.cuda.current_stream().cuda_stream)
    return g


graphs = {mode: front_graph(e) for mode, e in engs.items()}
cur = lambda: torch.cuda.current_stream().cuda_stream
lists = torch.empty(f.hash.capacity * f.T, dtype=torch.int32, device=dev)
legs = {}
for mode in MODES:
    legs["front_graph_" + mode] = (graphs[mode].replay, 1000)
for mode in MODES:
    legs["front_eager_" + mode] = ((lambda e=engs[mode]: e._enqueue_front(cur())), 400)
legs["hash_clear_eager"] = (f.hash.clear, 1000)
legs["canvas_clear_eager"] = ((lambda: check(lib.sessd_fill_u32(f.canvas.data_ptr(), 0, f.canvas.numel(), cur()), "fill_u32")), 1000)
legs["list_fill_eager"] = ((lambda: check(lib.sessd_fill_u32(lists.data_ptr(), 0x7F7F7F7F, lists.numel(), cur()), "fill_u32")), 1000)
front = alternate(legs)

# ---- (b) whole frames
for e in engs.values():
    e.capture(warmup=2)
frames = alternate({"replay_" + mode: (engs[mode].replay, 300) for mode in MODES})

# ---- (c) four engines on two CU sets, fed from the host
pinned = torch.from_numpy(host_frame).pin_memory()
runner = {}
for mode in MODES:
    engines, streams = pillar_engines_on_cu_sets(model, VG, TC, n_engines=4, sets=2, records=2 * FETCH_EVERY, max_points=POINTS, front_end=mode)
    pipe = HostFedPipeline(engines, streams, fetch_every=FETCH_EVERY)
    rates = []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for _ in range(JOB_FRAMES):
            pipe.submit(pinned)
            got += len(pipe.poll())
        got += len(pipe.finish())
        dt = time.perf_counter() - t0
        assert got == JOB_FRAMES
        if r:   # the first job warms the pipeline up
            rates.append(JOB_FRAMES / dt)
    one = 1e6 / frames["replay_" + mode]["median"]
    runner[mode] = dict(frames_per_s_4_engines_2_cu_sets_host_fed=summary(rates, frames_per_job=JOB_FRAMES),
                        frames_per_s_one_engine_replay=round(one, 1), ratio=round(float(np.median(rates)) / one, 3),
                        nms_truncated=pipe.nms_truncated)
    del pipe, engines

tg, fg = front["front_graph_tensor"], front["front_graph_fused"]
spread = max(tg["max"] - tg["min"], fg["max"] - fg["min"])
default = "fused" if tg["median"] - fg["median"] > spread else "tensor"
out = dict(what="microseconds per call (device events around back-to-back calls; eager legs include the host's enqueue); runner: frames "
                "per second of wall clock", config="kitti_pointpillars_model, batch 1, %d points" % POINTS, canvas=[f.ny, f.nx],
           points_capacity=f.P_cap, hash_capacity=f.hash.capacity, max_points_per_pillar=f.T, list_fill_bytes=f.hash.capacity * f.T * 4,
           pillars=pillars, live_points_per_pillar=dict(mean=round(float(live.mean()), 2), max=int(live.max())), rounds=rounds,
           same_results=same, front_end_us=front, stage_us_eager=stages, frame_us=frames, runner=runner,
           rule=dict(front_graph_tensor_minus_fused_us=round(tg["median"] - fg["median"], 2), largest_round_to_round_spread_us=round(spread, 2)),
           default=default)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
