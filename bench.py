#!/usr/bin/env python
"""Benchmark of the SE-SSD inference hot path on MI355X: voxelize -> SpMiddleFHD -> SSFA -> heads -> rotated NMS.

    python bench.py --gpus N --steps K --warmup W
    N > 1: either under a launcher (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...
    bench.py --gpus N ...) or plainly `python bench.py --gpus N`: without WORLD_SIZE in the environment the script spawns its N
    ranks itself (127.0.0.1, a free port) and rank 0 prints the one line.

A "step" is ONE frame of BASELINE.json configs[1] ("Single MI355X inference, KITTI car voxel grid [1600,1408,40],
max 16000 voxels, batch=1") through the whole path, input points already resident in HBM, detections left on the
device (<= 100 boxes). Frames shard across ranks with no data-path collective (weak scaling: every rank runs K
frames); value = total frames / max-over-ranks wall time. By default FOUR frames are in flight per GPU: four independent
batch-1 engines, two on each HALF of the chip (CU-masked streams, hipExtStreamCreateWithCUMask: every engine owns a hardware
queue, its kernels are confined to its half, its persistent stream-K launches are sized for 128 CUs): 1925 - 1980 frames/s against
1557 - 1630 for rounds 1 - 4's two plain streams sharing the whole chip (`--streams 2 --cu-split none`; `--streams 1` = strictly
sequential frames on the whole chip). THE DETECTOR IS TRAINED FIRST (round 6): the `train_step` leg -- `--pretrain-iterations`
captured SE-SSD iterations on fresh synthetic batches -- runs before anything else and its student's weights go into the timed
engines (`--random-weights`: rounds 1 - 5's seeded random weights; `--weights FILE`: a saved state_dict). One JSON line on rank 0
(metric / value / unit / higher_is_better / dtype / ms_per_step / config, and train_step when the detector was trained in the
process). A plain run does only that: set up, warm up, time the K steps, print. `--dump-outputs DIR` writes the detections of the
last timed step as DIR/*.npy (same arguments, same input frames). Everything below except train_step needs `--full`:
  parity        THE TIMED CONFIGURATION held to the oracle before the clock starts: the frames of the cpu_baseline sample go
                through the very engines that are timed (autotuned tilings, stream-K workgroup counts, captured graphs) and
                every detection is compared with the oracle's under oracle/compare.py's STRICT rule (trained weights: 2 mm / 2 mrad
                absolute, scores 1e-3; identical, or identical under the oracle's own LISTED near-threshold NMS decisions; the
                synthetic rule only with --random-weights). A mismatch prints the line with parity.ok = false and exits 3.
                `config` carries the verdict as scalars: parity_ok / parity_matched / parity_frames / parity_rule.
  roofline      the dominant kernel (fused-Winograd f32-MFMA 3x3 conv: the seven 3x3 stride-1 SSFA layers, all over tile lists)
                against the WHOLE CHIP's dense f32 MFMA peak (157.3 TFLOP/s): EXECUTED matrix-core FLOPs / launch time measured
                live with HIP events on the launching stream; frac_of_cu_set_peak = against the launch's own 128 CUs;
                frac_chip_timed_region = executed GFLOP per step / ms_per_step / peak: what all frames in flight achieve together;
                `traffic` = rocprofv3 FETCH_SIZE / WRITE_SIZE of a fixed configuration (profiles/r6_wino_traffic.json)
  roofline_spmiddle / stages_ms_eager   SURVEY 8(d)'s HBM figure for the sparse stage and per-stage times (informational)
  value_sequential   one engine on the whole chip, strictly one frame at a time (informational)
  host_io       PCIe-inclusive rate: pinned host points in, host detections out, pipelined (sessd_hip/runner.py) and the
                strictly sequential latency mode (informational, never `value`)
  cpu_baseline  the CPU oracle pipeline (port of the reference path: the reference itself cannot run here) on a
                bounded sample of the same frames, on this box's host cores.
  train_step    BASELINE configs[2]: ms per replay of the captured SE-SSD training iteration (informational; measured by the
                training that precedes a plain run, or as a leg of its own under --full with --random-weights / --weights)
`--stress` = BASELINE configs[4] (200k points, 64k voxels, batch 8), `--batch B` = B frames per step.
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "se-ssd_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

F32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: dense f32-input MFMA peak
CONV_FLOPS = 2.0 * 200 * 176 * 128 * 128 * 9  # algorithmic FLOPs of one 3x3 128->128 launch at 200x176 (10.38 GFLOP)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--max-voxels", type=int, default=16000)
    ap.add_argument("--batch", type=int, default=1, help="frames per step (BASELINE configs[1] is batch 1)")
    ap.add_argument("--supersample", type=int, default=1, help="ray supersampling of the synthetic scanner (3 for 200k points)")
    ap.add_argument("--stress", action="store_true",
                    help="BASELINE configs[4]: 200k points/frame, max 64000 voxels, batch 8 (a parity/roofline case, not the metric line)")
    ap.add_argument("--pool", type=int, default=16, help="distinct synthetic frames cycled through")
    ap.add_argument("--eager", action="store_true", help="no hipGraph: launch every kernel from Python")
    ap.add_argument("--cpu-frames", type=int, default=40, help="frames of the CPU baseline / parity sample (0 = skip both)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="torch CPU threads of the baseline (capped by affinity)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="time budget of the CPU baseline sample")
    ap.add_argument("--streams", type=int, default=4,
                    help="frames in flight: independent batch-1 engines on separate HIP streams (1 = strictly one frame at a time). "
                         "Round 5 default: 4, on two CU sets (--cu-split / --cu-parts); rounds 1 - 4 ran `--streams 2 --cu-split none`")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-host-io", action="store_true", help="skip the informational host-buffer legs (kernel traces of the timed region)")
    ap.add_argument("--no-sequential", action="store_true", help="skip the informational one-frame-at-a-time leg")
    ap.add_argument("--no-active-tiles", action="store_true",
                    help="A/B: the first three SSFA layers over the whole BEV map (round 3) instead of only the tiles whose input is not "
                         "constant (csrc/dense_active.hip)")
    ap.add_argument("--dense-token", action="store_true",
                    help="EXPERIMENT: every engine's frame as two graphs (front: voxelizer + sparse stage + tile lists + fill; back: the dense "
                         "convs + heads + predict) and ONE dense stage at a time per CU set -- a frame's back waits for the event the set's "
                         "previous back recorded; the fronts run beside the other engines' backs")
    ap.add_argument("--no-active-conv", action="store_true",
                    help="A/B: conv_0 / conv_1 as the two-set full-map launch (rounds 3 - 5) instead of over their tile list (round 6)")
    ap.add_argument("--no-train-step", action="store_true",
                    help="skip the `train_step` leg (BASELINE configs[2]: the captured SE-SSD training iteration with the reference loss)")
    ap.add_argument("--train-replays", type=int, default=20, help="timed replays of the captured training iteration")
    ap.add_argument("--sk-workgroups", type=int, default=0,
                    help="persistent workgroups of the stream-K Winograd launches (multiple of 8; 0 = the kernel's default, all CUs). "
                         "224 with two frames in flight leaves 32 CUs to the other stream's small kernels: +2 %% frames/s, but the "
                         "kernel then runs 14 %% longer per launch -- the default keeps the timed kernel the one the roofline describes")
    ap.add_argument("--spinup-seconds", type=float, default=0.5,
                    help="untimed frames run for this long before the warm-up steps (the CPU oracle sample leaves the GPU idle at low clocks)")
    ap.add_argument("--fork-active", action="store_true", help="EXPERIMENT: the tile-list + fill launches as a side branch of the graph beside the sparse convs")
    ap.add_argument("--fork", action="store_true", help="engines with the parallel front branch (level-0 table + first two sparse convs beside the site chain; measured slower)")
    ap.add_argument("--no-autotune", action="store_true", help="keep the default conv tilings")
    ap.add_argument("--cu-parts", type=int, default=0,
                    help="with --cu-split: number of disjoint CU sets (default 2: the two halves of the chip); engine i runs on set i %% parts")
    ap.add_argument("--cu-budget", type=int, default=0,
                    help="size every engine's persistent launches for this many compute units (default: the CUs of its set)")
    ap.add_argument("--cu-split", default="contiguous", choices=["none", "contiguous", "interleaved"],
                    help="frames in flight on CU-masked streams (hipExtStreamCreateWithCUMask: a hardware queue of its own per engine, "
                         "confined to its CU set; persistent launches sized for the set). contiguous: set k = CU numbers [k n, (k+1) n); "
                         "none: plain torch streams sharing the whole chip (rounds 1 - 4)")
    ap.add_argument("--list-shares", default="auto", choices=["auto", "whole", "cut"],
                    help="A/B of the Winograd list launches: whole-unit shares for every layer / stream-K shares only / the autotune's "
                         "per-launch choice")
    ap.add_argument("--weights", default=None,
                    help="state_dict file (torch.save) loaded into the detector instead of the seeded random weights, e.g. the student "
                         "trained by tests/trained_parity.py --save; the parity gate then uses oracle/compare.py's STRICT rule")
    ap.add_argument("--random-weights", action="store_true",
                    help="rounds 1 - 5's line: the seeded random benchmark weights and oracle/compare.py's SYNTHETIC rule. Default (round 6, "
                         "batch 1): the detector is TRAINED first, in this process, by the `train_step` leg's captured SE-SSD iterations "
                         "on synthetic scans, and the timed engines are held to the oracle under the STRICT rule")
    ap.add_argument("--save-weights", default=None, help="torch.save the in-process trained student's state_dict here (for --weights on later runs)")
    ap.add_argument("--pretrain-iterations", type=int, default=300,
                    help="captured training iterations on fresh synthetic batches before the student's weights go into the timed detector")
    ap.add_argument("--sort-tiles", action="store_true",
                    help="EXPERIMENT: engines built with the offset-pattern tile sort (engine.sort_tiles); the autotune then times both tile "
                         "orders per sparse layer")
    ap.add_argument("--sparse-mt", action="store_true", help="EXPERIMENT: the multi-tile-per-wave sparse conv variants as autotune candidates at any level size")
    ap.add_argument("--no-offset-split", action="store_true", help="autotune without the offset-split sparse conv variants")
    ap.add_argument("--no-streamk", action="store_true", help="autotune without the stream-K Winograd variants")
    ap.add_argument("--wino-cfg", type=int, default=0, help="force this tile_cfg (20-25) on the seven 3x3 stride-1 SSFA layers after autotune")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: the cpu_baseline sample and the parity gate, value_sequential, the "
                         "roofline legs, host_io and the informational train_step leg (each still switched off by its own --no-* / "
                         "--cpu-frames 0). Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the detections of the last timed step (what a caller of the timed path "
                         "receives) as DIR/<name>.npy in float32")
    args = ap.parse_args(argv)
    if args.stress:
        args.points, args.max_voxels, args.batch, args.supersample, args.pool = 200000, 64000, 8, 3, 8
        args.streams = 1
    return args


def log(*a):
    if os.environ.get("SESSD_BENCH_VERBOSE"):
        print("[bench %.1fs]" % (time.perf_counter() - _T0), *a, file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def dump_outputs(path, results):
    """--dump-outputs: the per-frame results of one step (engine.results(): box3d_lidar (n, 7), scores (n,), label_preds (n,)),
    the frames of the batch concatenated in slot order, as float32 .npy files; detections_per_frame splits them again."""
    os.makedirs(path, exist_ok=True)
    arrays = {"box3d_lidar": np.concatenate([np.asarray(r["box3d_lidar"], np.float32).reshape(-1, 7) for r in results]),
              "scores": np.concatenate([np.asarray(r["scores"], np.float32).reshape(-1) for r in results]),
              "label_preds": np.concatenate([np.asarray(r["label_preds"], np.float32).reshape(-1) for r in results]),
              "detections_per_frame": np.array([len(r["scores"]) for r in results], np.float32)}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return arrays


def default_engine_factory(args, dev, model=None, count=None):
    """(model, [engines]) of the timed configuration: `--streams` independent batch-`--batch` engines on one detector."""
    from sessd_hip import configs
    from sessd_hip.engine import InferenceEngine
    VG = configs.VOXEL_GENERATOR
    if model is None:
        model = configs.build_synthetic_detector(dev, seed=0, max_voxels=args.max_voxels, num_points=args.points, supersample=args.supersample)
        if getattr(args, "weights", None):
            model.load_state_dict(torch.load(args.weights, map_location=dev))
            model.eval()
    engines = [InferenceEngine(model, VG["range"], VG["voxel_size"], VG["max_points_in_voxel"], args.max_voxels,
                               configs.TEST_CFG, batch_size=args.batch, max_points_per_frame=args.points, device=dev,
                               active_tiles=not getattr(args, "no_active_tiles", False), sort_tiles=bool(getattr(args, "sort_tiles", False)))
               for _ in range(max(1, args.streams if count is None else count))]
    # A/B hooks: SESSD_FORCE_SPARSE="6:0x10202:1,7::1" = layer:tuning:sorted (either may be empty) applied after the autotune
    force = {}
    for item in filter(None, os.environ.get("SESSD_FORCE_SPARSE", "").split(",")):
        f = item.split(":")
        force[int(f[0])] = (int(f[1], 0) if len(f) > 1 and f[1] else None, bool(int(f[2])) if len(f) > 2 and f[2] else None)
    for e in engines:
        e.fork_front = bool(args.fork)
        e.fork_active = bool(getattr(args, "fork_active", False))
        e.sparse_mt_candidates = bool(getattr(args, "sparse_mt", False))
        e.allow_active_conv = not getattr(args, "no_active_conv", False)
        e.force_sparse = force
    return model, engines


def oracle_sample(args, model, frames_np):
    """The CPU oracle (port of the reference path) on a bounded sample of the bench's frames: the cpu_baseline figure AND the
    expected detections of the parity gate. Returns (cpu_baseline dict, [(frame index, want, debug, bev)])."""
    from oracle import pipeline, postprocess as pp
    from sessd_hip import configs
    VG = configs.VOXEL_GENERATOR
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    anchors = pp.create_anchors_3d_range().reshape(-1, 7)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    ncores = max(1, min(avail, args.cpu_threads))
    torch.set_num_threads(ncores)
    budget = time.perf_counter() + args.cpu_seconds
    log("cpu baseline: %d threads of %d visible cores" % (ncores, avail))
    pipeline.run_frames([frames_np[0]], sd, VG["range"], VG["voxel_size"], 5, args.max_voxels, anchors)  # warm-up
    T, done, sample = {}, 0, []
    c0 = time.perf_counter()
    while done < args.cpu_frames and (done == 0 or time.perf_counter() < budget):
        fi = done % len(frames_np)
        want, inter = pipeline.run_frames([frames_np[fi]], sd, VG["range"], VG["voxel_size"], 5, args.max_voxels, anchors,
                                          timings=T, return_intermediate=True)
        sample.append((fi, want[0], inter["debug"][0], inter["bev"] if done == 0 else None))
        done += 1
        log("cpu frame", done, T)
    cdt = time.perf_counter() - c0
    base = {"value": done / cdt, "unit": "frames/s", "cores": ncores, "kind": "port",
            "sample": "%d of the same frames through oracle/pipeline.py (C voxelizer + rotated NMS single thread, torch-CPU "
                      "gather-mm-scatter sparse conv and oneDNN dense convs on %d threads; %d host cores visible)" % (done, ncores, avail),
            "stage_ms": {k: v / done * 1e3 for k, v in T.items()}}
    return base, sample


def parity_gate(args, engines, streams, frames, sample):
    """Every frame of the oracle sample through EVERY timed engine exactly as the timed region drives it (same tile_cfg, sparse
    tunings, stream-K workgroups and workspace, graph replay unless --eager, same batch size) and compared with the oracle's
    detections. At batch > 1 (--stress: BASELINE configs[4]) the distinct frames of the sample are packed into batches of
    `--batch` frames twice -- in pool order, as the timed region stages them, and rotated by three slots (where a stream-K
    unit is cut depends on the slot) -- and every frame of every batch is compared."""
    from oracle.compare import compare_detections
    B = args.batch
    rule = getattr(args, "parity_rule", None) or ("strict" if getattr(args, "weights", None) else "synthetic")
    rep = {"frames": 0, "identical": 0, "flipped_near_threshold": 0, "mismatch": [], "bev_rel_err": None, "engines": len(engines),
           "batch": B, "launch": "eager" if args.eager else "hipGraph replay",
           "rule_set": rule,
           "rule": "oracle/compare.py rule='%s' (strict = trained weights, the default line and --weights: same count / order, every box "
                   "component within 2e-3 ABSOLUTE, scores 1e-3 relative, <= 6 listed decisions; synthetic = the seeded random weights of "
                   "--random-weights: sizes relative beyond 1 m, centres 2e-3 + 5e-5 x the frame's largest |box code| x anchor size -- the decode "
                   "multiplies a code's float32 error by the 4.2 m anchor diagonal and random weights give codes of 18 --, <= 10 listed "
                   "decisions); a frame with oracle-LISTED NMS decisions within 1e-4 of the 0.01 IoU threshold may equal the oracle under "
                   "one assignment of those decisions (counted as flipped)" % rule}
    if B == 1:
        batches = [[s] for s in sample]
    else:
        seen, distinct = set(), []
        for s in sample:
            if s[0] not in seen:
                seen.add(s[0])
                distinct.append(s)
        batches = []
        for shift in (0, 3):
            order = distinct[shift % len(distinct):] + distinct[:shift % len(distinct)]
            for i in range(0, len(order), B):
                grp = order[i:i + B]
                batches.append(grp + [grp[j % len(grp)] for j in range(B - len(grp))])  # a short tail is padded by repeats
        rep["distinct_frames"] = len(distinct)
    for ei, (e, st) in enumerate(zip(engines, streams)):
        for grp in batches:
            with torch.cuda.stream(st):
                e.set_points([frames[s[0]] for s in grp])
                if args.eager:
                    e.enqueue()
                else:
                    e.replay()
            st.synchronize()
            res = e.results()
            for slot, ((fi, want, dbg, bev), got) in enumerate(zip(grp, res)):
                rep["frames"] += 1
                try:
                    r = compare_detections(got, want, dbg, rule=rule)
                    rep["identical" if not r["flipped"] else "flipped_near_threshold"] += 1
                    if not r["flipped"] and len(want["scores"]):
                        # how far inside the tolerance the identical frames are (boxes: metres / radians, absolute; scores: relative)
                        gb, wb = np.asarray(got["box3d_lidar"], np.float64).reshape(-1, 7), np.asarray(want["box3d_lidar"], np.float64).reshape(-1, 7)
                        dyaw = np.abs(gb[:, 6] - wb[:, 6]) % (2 * np.pi)
                        rep["max_centre_abs_diff_m"] = max(rep.get("max_centre_abs_diff_m", 0.0), float(np.abs(gb[:, :3] - wb[:, :3]).max()))
                        rep["max_size_abs_diff_m"] = max(rep.get("max_size_abs_diff_m", 0.0), float(np.abs(gb[:, 3:6] - wb[:, 3:6]).max()))
                        rep["max_yaw_abs_diff_rad"] = max(rep.get("max_yaw_abs_diff_rad", 0.0), float(np.minimum(dyaw, 2 * np.pi - dyaw).max()))
                        ws_ = np.asarray(want["scores"], np.float64)
                        rep["max_score_rel_diff"] = max(rep.get("max_score_rel_diff", 0.0),
                                                        float((np.abs(np.asarray(got["scores"], np.float64) - ws_) / np.maximum(ws_, 1e-6)).max()))
                except AssertionError as ex:
                    rep["mismatch"].append({"engine": ei, "frame": fi, "slot": slot, "why": str(ex)[:300]})
                if bev is not None and ei == 0 and rep["bev_rel_err"] is None:
                    rep["bev_rel_err"] = float((e.bev[slot].cpu() - bev[0]).abs().max()) / max(1.0, float(bev.abs().max()))
    rep["matched"] = rep["identical"] + rep["flipped_near_threshold"]
    rep["ok"] = rep["matched"] == rep["frames"] and (rep["bev_rel_err"] is None or rep["bev_rel_err"] < 2e-4)
    return rep


def trained_detector(args, dev):
    """THE WEIGHTS OF THE TIMED DETECTOR (round 6; review item "put the strict rule on the driver's line"): the `train_step` leg runs
    FIRST -- `--pretrain-iterations` captured SE-SSD iterations on fresh labelled synthetic batches (sessd_hip.trainbench.measure:
    teacher + student forward, reference loss, backward, clip / Adam / EMA; scenes 50 .. 73, the bench frames are scenes 0 .. 15) and
    its timed replays -- and the STUDENT's state_dict is loaded into a fresh eval-mode detector. Trained weights decode car-sized
    boxes, so the parity gate runs under oracle/compare.py's STRICT rule (tests/test_trained_gpu.py holds a 300-iteration model to
    it). Returns (model, the train_step record)."""
    from sessd_hip import configs, trainbench
    res, step = trainbench.measure(dev, batch=4, steps=args.train_replays, real_loss=True, pretrain=args.pretrain_iterations)
    step.check_overflow()   # sticky flags of the whole run: sparse level capacities of both networks, loss capacities
    state = {k: v.detach().clone() for k, v in step.student.state_dict().items()}
    step.graph = None
    del step
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    model = configs.build_synthetic_detector(dev, seed=0, max_voxels=args.max_voxels, num_points=args.points, supersample=args.supersample)
    model.load_state_dict(state)
    model.eval()
    if getattr(args, "save_weights", None):
        os.makedirs(os.path.dirname(os.path.abspath(args.save_weights)), exist_ok=True)
        torch.save({k: v.cpu() for k, v in state.items()}, args.save_weights)
    res["weights_go_to"] = "the timed inference engines (student after %d captured iterations + %d timed replays)" % (
        args.pretrain_iterations, args.train_replays)
    return model, res


def force_collectives():
    """SESSD_FORCE_COLLECTIVES=1: a process group of ONE rank runs every collective a larger group would (records all_gather,
    barriers, MAX all-reduce of the time) instead of short-circuiting -- how the RCCL path is executed on a one-GPU box
    (tests/test_rccl_gpu.py)."""
    return os.environ.get("SESSD_FORCE_COLLECTIVES") == "1"


def run_rank(args, rank=0, world=1, local_rank=0, backend="nccl", device=None, engine_factory=None):
    """One rank of the benchmark. Returns the result dict on rank 0 (None elsewhere). `engine_factory(args, dev)` ->
    (model, engines) lets the CPU tests drive the rank function with a stub engine over gloo."""
    on_gpu = device is None or torch.device(device).type == "cuda"
    if on_gpu:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    else:
        dev = torch.device(device)
    t_start = time.perf_counter()
    # ---- the detector's weights: trained in this process unless told otherwise (BEFORE the process group exists: the training
    # iteration of a one-rank job has no SyncBN and is captured as one graph; every rank trains the same bits from the same seed)
    pre_model, train_res, weights_kind = None, None, "random"
    if getattr(args, "weights", None):
        weights_kind = "file"
    elif (on_gpu and engine_factory is None and not getattr(args, "random_weights", False) and not args.stress and args.batch == 1
          and not args.no_train_step):
        try:
            pre_model, train_res = trained_detector(args, dev)
            weights_kind = "trained_in_process"
        except Exception as ex:   # the line must not die with the training leg: the round-5 line (random weights, synthetic rule), and say so
            train_res = {"error": repr(ex)[:300]}
            log("in-process training failed:", repr(ex)[:300])
    collective = world > 1 or (force_collectives() and on_gpu)
    if collective and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    ranks_seen = dist.get_world_size() if collective else 1

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    from sessd_hip import synth
    from sessd_hip import dist as sdist
    model, engines = (engine_factory(args, dev) if engine_factory else default_engine_factory(args, dev, model=pre_model))
    cu_split, cu_note = (getattr(args, "cu_split", "none") or "none"), None
    masked = on_gpu and cu_split != "none" and len(engines) > 1 and engine_factory is None
    if masked:
        # FRAMES IN FLIGHT ON CU SETS (round 5): engine i runs on a stream that is confined to CU set i % parts and owns a hardware
        # queue (a CU mask is a queue property; plain torch streams share a few queues), its persistent stream-K launches are
        # sized for the set. Measured on MI355X (profiles/r5_cu_sets_sweep.json): 4 frames on 2 halves 1925 frames/s against 1563
        # for round 4's two plain streams; 4 quarters 1885; 3 / 5 / 6 sets (uneven over the 8 XCDs) 1327 / 735 / 798; plain
        # streams with launches merely SIZED for a quarter 1387.
        from sessd_hip import ops as _ops
        parts = getattr(args, "cu_parts", 0) or min(2, len(engines))
        try:
            streams = []
            for k, e in enumerate(engines):
                st, ncu = _ops.cu_masked_stream(k % parts, parts, dev, layout=cu_split)
                streams.append(st)
                e.cu_budget = getattr(args, "cu_budget", 0) or ncu
        except Exception as ex:   # the line must not die with an optimisation: plain streams, and say so
            masked, cu_note = False, "CU-masked streams unavailable (%s): plain streams" % repr(ex)[:120]
            for e in engines:
                e.cu_budget = 0
    if not masked and on_gpu:
        streams = [torch.cuda.Stream() for _ in engines] if len(engines) > 1 else [torch.cuda.current_stream()]
        for e in engines:
            if getattr(args, "cu_budget", 0):
                e.cu_budget = args.cu_budget
    elif not on_gpu:
        streams = [None for _ in engines]

    class _on:  # `with torch.cuda.stream(st)` that is a no-op off the GPU
        def __init__(self, st):
            self.cm = torch.cuda.stream(st) if (on_gpu and st is not None) else None

        def __enter__(self):
            return self.cm.__enter__() if self.cm else None

        def __exit__(self, *a):
            return self.cm.__exit__(*a) if self.cm else False

    args.parity_rule = "synthetic" if weights_kind == "random" else "strict"
    eng = engines[0]
    # frames of this rank, resident in HBM before the clock starts (rank r takes seeds r*pool ...)
    frames_np = [synth.make_frame(rank * args.pool + i, args.points, supersample=args.supersample) for i in range(args.pool)]
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    log("model + engine built")

    def batch_of(i):
        return [frames[(i * args.batch + b) % args.pool] for b in range(args.batch)]

    eng.set_points(batch_of(0))
    eng.enqueue()
    sync()
    first = eng.results()[0]
    log("first frame done:", len(first["scores"]), "detections")
    if not args.no_autotune:
        eng.allow_offset_split = not args.no_offset_split
        eng.allow_streamk = not args.no_streamk
        if getattr(args, "list_shares", "auto") == "cut":
            eng.list_share_candidates = (1, 4, 8, 16)
        elif masked and getattr(args, "list_shares", "auto") in ("auto", "whole"):
            # engines that SHARE a CU set run their Winograd list layers on whole-unit shares (below): the autotune then chooses each
            # layer's SHAPE among whole-unit launches (round 5 chose the shape with stream-K shares in the race and forced the share rule
            # afterwards: b1.1 / b1.2 ended on 4-wave units, 132 / 164 of them on 128 CUs, 80 us each; 8-wave units need one round)
            eng.list_share_candidates = (-1,)
        with _on(streams[0] if masked else None):   # (a CU-masked engine is tuned on its own CU set)
            rep = eng.autotune()
            sync()
        if getattr(args, "list_shares", "auto") != "auto" and hasattr(eng, "set_list_shares"):
            eng.set_list_shares(args.list_shares)
        elif masked and hasattr(eng, "set_list_shares"):
            # engines that SHARE a CU set: whole-unit shares for every Winograd list layer (a list launch then occupies as many
            # workgroups as it has units and leaves the set's other CUs to the other frame). The per-launch autotune cannot see
            # that: measured 1953 / 1953 / 1948 frames/s against 1910 / 1910 with its own picks (profiles/r5_cu_sets_sweep.json)
            eng.set_list_shares("whole")
        # A/B hook: SESSD_LIST_SHAPE=0 / 1 forces the stream-K shape (0: 8 waves x 128 couts, 1: 4 waves x 64 couts) of every Winograd
        # list layer; SESSD_LIST_MIN_ROUNDS its share rule (-1 whole units, -2 two units per workgroup, > 0 stream-K rounds)
        if os.environ.get("SESSD_LIST_SHAPE") or os.environ.get("SESSD_LIST_MIN_ROUNDS"):
            only = [int(v) for v in filter(None, os.environ.get("SESSD_LIST_LAYERS", "").split(","))]
            for l, (shape, mr) in list(eng.active_cfg.items()):
                if l in eng.ACTIVE_SK or l == eng.ACTIVE_PAIR or (only and l not in only):
                    continue
                sh = int(os.environ.get("SESSD_LIST_SHAPE", shape))
                if eng.ACTIVE_SLOTS[l][1][0].upk_sk(sh) is None:
                    sh = shape
                eng.active_cfg[l] = (sh, int(os.environ.get("SESSD_LIST_MIN_ROUNDS", mr)))
        log("autotuned tile configs:", {k: (v[0], round(v[1], 4)) for k, v in rep.items()})
    if args.wino_cfg:
        for nm in ("b0.0", "b0.1", "b0.2", "conv_0", "conv_1", "b1.1", "b1.2"):
            eng.tile_cfg[nm] = args.wino_cfg
    for e in engines:
        e.sk_workgroups = args.sk_workgroups
    for e in engines[1:]:
        e.adopt_tuning(eng)
        e.set_points(batch_of(0))
        e.enqueue()
    sync()
    # every frame leaves a fixed-size detection record on the device; the end-of-job gather of those records (ONE all_gather
    # per tensor over RCCL when N > 1; tools/dist_test.py:150-186) is inside the timed region
    per_engine = (args.warmup + args.steps + len(engines) - 1) // len(engines) * args.batch + args.batch
    for e in engines:
        e.attach_records(per_engine)
    token = bool(getattr(args, "dense_token", False)) and on_gpu and not args.eager and len(engines) > 1
    if not args.eager:
        for e, st in zip(engines, streams):
            with _on(st):
                e.capture(split=True) if token else e.capture()
        sync()
        log("graph captured")
    n_sets = (parts if masked else 1)
    tokens = [None] * n_sets     # per CU set: the event the last dense stage (back graph) of the set recorded

    # ---- CPU oracle sample (cpu_baseline) and the parity gate on the configuration that is about to be timed (--full only)
    full = bool(getattr(args, "full", False))
    cpu_base, parity = None, None
    if full and args.cpu_frames > 0 and world == 1 and rank == 0 and on_gpu:
        cpu_base, sample = oracle_sample(args, model, frames_np)
        parity = parity_gate(args, engines, streams, frames, sample)  # at ANY batch size (round 3 skipped it at batch > 1)
        log("parity:", {k: v for k, v in parity.items() if k != "rule"})
        del sample
    elif full and args.cpu_frames > 0 and world > 1 and on_gpu:
        # N > 1 (round-4 review item: no multi-GPU result was ever held to the oracle; every rank autotunes on its own): EVERY rank
        # holds its own timed engines to the oracle on a SHORT sample of its own frames -- all ranks at the same time, so nobody
        # waits at the barrier for rank 0 --, the verdicts are summed over the ranks and rank 0 reports them. The cpu_baseline
        # figure stays on the N = 1 line.
        import copy
        sub = copy.copy(args)
        sub.cpu_frames = min(args.cpu_frames, 4 if args.batch == 1 else args.batch)
        sub.cpu_seconds = min(args.cpu_seconds, 8.0)
        sub.cpu_threads = max(1, args.cpu_threads // world)
        _, sample = oracle_sample(sub, model, frames_np)
        parity = parity_gate(args, engines, streams, frames, sample)
        del sample
        tot = torch.tensor([parity["frames"], parity["identical"], parity["flipped_near_threshold"], len(parity["mismatch"]),
                            0 if parity["ok"] else 1], dtype=torch.float64, device=dev)
        dist.all_reduce(tot)
        parity.update(frames=int(tot[0]), identical=int(tot[1]), flipped_near_threshold=int(tot[2]), matched=int(tot[1] + tot[2]),
                      mismatches_all_ranks=int(tot[3]), ok=bool(tot[4] == 0), ranks=world,
                      note="every rank checked its own engines on %d of its own frames; counts are sums over the ranks, `mismatch` "
                           "lists rank 0's" % sub.cpu_frames)
        log("parity (all ranks):", {k: v for k, v in parity.items() if k != "rule"})

    def step(i):
        k = i % len(engines)
        e, st = engines[k], streams[k]
        with _on(st):
            e.set_points(batch_of(i))  # device-to-device staging into the engine's static input buffer
            if args.eager:
                e.enqueue()
            elif token:
                # EXPERIMENT --dense-token: the front runs at once; the back waits until the set's previous back has finished
                e.graph_front.replay()
                cs = k % n_sets
                if tokens[cs] is not None:
                    st.wait_event(tokens[cs])
                e.graph_back.replay()
                ev = torch.cuda.Event()
                ev.record(st)
                tokens[cs] = ev
            else:
                e.replay()

    n_collectives = [0]

    def barrier():
        if collective:
            dist.barrier()
            n_collectives[0] += 1
        sync()

    # The oracle sample above (--full) leaves the GPU idle for tens of seconds: before the W warm-up steps the clocks are brought back up
    # by running frames for a fixed wall time (untimed, like the warm-up; the driver's W may be as small as 5 frames = 4 ms)
    if on_gpu:
        spin_until = time.perf_counter() + args.spinup_seconds
        i = 0
        while time.perf_counter() < spin_until:
            for _ in range(16):
                step(i)
                i += 1
            sync()
    for i in range(args.warmup):
        step(i)
    barrier()
    for e in engines:
        e.record_cursor.zero_()
    barrier()
    log("warmup done")
    t_timed_start = t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    # end-of-job gather of this rank's records (per engine: frames i, i + streams, ...), still inside the timed region
    gathered = []
    for e, st in zip(engines, streams):
        with _on(st):
            n_e = int(e.record_counts.shape[0])
            gathered.append(sdist.gather_records(e.records, e.record_counts, n_e * world))
            n_collectives[0] += 2 if collective else 0
    barrier()
    dt = time.perf_counter() - t0
    frames_gathered = sum(min(int(e.record_cursor.item()), int(g[0].shape[1])) * int(g[0].shape[0]) for g, e in zip(gathered, engines))
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if collective:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        n_collectives[0] += 1
    dt = float(tmax.item())
    log("timed region done: %.3f ms/step" % (dt / args.steps * 1e3))
    dets = int(eng.out["count"][0].item())
    if int(eng.err.item()) != 0:
        raise SystemExit("sparse capacity overflow during the benchmark: results invalid")
    if rank == 0 and getattr(args, "dump_outputs", None):
        # before any --full leg re-runs the engines: the detections of the LAST timed step, as its engine left them
        dump_outputs(args.dump_outputs, engines[(args.steps - 1) % len(engines)].results())

    out = None
    if rank == 0:
        wdesc = {"random": "seeded random weights, BatchNorm calibrated (--random-weights: rounds 1 - 5's line)",
                 "file": "TRAINED weights from %s (tests/trained_parity.py)" % os.path.basename(getattr(args, "weights", None) or "-"),
                 "trained_in_process": "weights TRAINED in this process: the student after %d captured SE-SSD iterations on fresh synthetic "
                                       "batches (the train_step leg, run first)" % getattr(args, "pretrain_iterations", 0)}[weights_kind]
        out = {
            "metric": "KITTI frames/sec (voxelize->backbone->head->NMS)",
            "value": world * args.steps * args.batch / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            # `config` holds SCALARS only (the driver's record keeps scalar config keys and drops nested objects: rounds 3 - 5 lost the
            # gate's verdict that way); the nested detail is in the top-level `tuning` / `cu_sets` / `parity` objects
            "config": {"workload": "SE-SSD KITTI-car inference, %d frame(s)/step: %d-point synthetic HDL-64E front-FOV scans, "
                                   "voxel grid [1408,1600,40], max_voxels %d, batch %d (BASELINE.json configs[%d]); "
                                   "%s"
                                   % (args.batch, args.points, args.max_voxels, args.batch, 4 if args.stress else 1, wdesc),
                       "weights": weights_kind,
                       "launch": "eager" if args.eager else "hipGraph replay", "frames_per_rank": args.steps * args.batch,
                       "frames_in_flight": len(engines), "streamk_workgroups": args.sk_workgroups, "dense_token": bool(token),
                       "cu_sets": (parts if masked else 0), "cus_per_set": (getattr(eng, "cu_budget", 0) if masked else 0),
                       "cu_layout": (cu_split if masked else "none"),
                       "cu_sets_note": cu_note,
                       "ms_latency_per_frame_in_flight": len(engines) * dt / args.steps * 1e3 / args.batch,
                       "parallelism": "frames sharded over %d rank(s), no data-path collective" % world,
                       "rccl_ranks_seen": ranks_seen,
                       "collective_backend": (dist.get_backend() if collective else "none"),
                       "collectives_in_timed_region": n_collectives[0],
                       "seconds_to_first_timed_step": round(t_timed_start - t_start, 2),
                       "detections_last_frame": dets, "detections_first_frame": int(len(first["scores"])),
                       "records_gathered": frames_gathered,
                       "gather": "one all_gather of fixed-size (frames, 100, 9) float32 records + counts per engine at the end "
                                 "of the job, inside the timed region (RCCL when n_gpus > 1; a device-side no-op at n_gpus = 1)"},
            "cu_sets": ({"layout": cu_split, "sets": parts, "cus_per_set": getattr(eng, "cu_budget", 0),
                         "what": "engine i on a CU-masked stream (hipExtStreamCreateWithCUMask) confined to CU set i % sets, "
                                 "persistent launches sized for the set"} if masked else None),
            "tuning": {"dense_tile_cfg": dict(getattr(eng, "tile_cfg", {})),
                       "sparse": {str(k): v for k, v in getattr(eng, "sparse_split", {}).items()},
                       "sparse_offset_pattern_tiles": {str(k): bool(v) for k, v in getattr(eng, "sparse_sorted", {}).items()},
                       # layers that run over tile lists: Winograd stream-K (shape, minimum share), the LDS-tiled
                       # stream-K kernel (tile_cfg 30, minimum share), or a direct kernel (its tile_cfg)
                       "active_tiles": {eng.ACTIVE_SLOTS[l][0]: ({"direct_tile_cfg": v[0]} if v[1] == 0 else
                                                                 {"lds_tiled_streamk": True, "min_rounds": v[1]} if v[0] == 30 else
                                                                 {"streamk_shape": v[0], "min_rounds": v[1]})
                                        for l, v in getattr(eng, "active_cfg", {}).items()}},
        }
        if train_res is not None:
            out["train_step"] = train_res
        if parity is not None:
            out["parity"] = parity
            # the gate's verdict as SCALAR config keys: what the driver's record keeps
            out["config"].update(parity_ok=bool(parity["ok"]), parity_matched=int(parity["matched"]), parity_frames=int(parity["frames"]),
                                 parity_identical=int(parity["identical"]), parity_rule=parity["rule_set"],
                                 parity_bev_rel_err=parity["bev_rel_err"], parity_max_centre_abs_diff_m=parity.get("max_centre_abs_diff_m"),
                                 parity_max_score_rel_diff=parity.get("max_score_rel_diff"))
    if rank == 0 and on_gpu and full:
        # ---- the same engines strictly one frame at a time (informational; the driver's record then holds both figures)
        seq_eng, seq_st = eng, streams[0]
        if masked and world == 1 and (not args.no_sequential or not args.no_roofline):
            # one frame at a time is a WHOLE-CHIP figure: an engine of its own on a plain stream, tuned and captured for all CUs
            seq_eng = default_engine_factory(args, dev, model=model, count=1)[1][0]
            seq_eng.set_points(batch_of(0))
            seq_eng.enqueue()
            sync()
            if not args.no_autotune:
                seq_eng.allow_offset_split, seq_eng.allow_streamk = not args.no_offset_split, not args.no_streamk
                seq_eng.autotune()
            seq_eng.attach_records(args.batch * 4)
            seq_st = torch.cuda.current_stream()
            if not args.eager:
                seq_eng.capture()
            sync()
        if not args.no_sequential and len(engines) > 1 and world == 1:
            nseq = max(20, min(args.steps, 200))
            for i in range(5):
                with _on(seq_st):
                    seq_eng.set_points(batch_of(i))
                    seq_eng.enqueue() if args.eager else seq_eng.replay()
            sync()
            s0 = time.perf_counter()
            for i in range(nseq):
                with _on(seq_st):
                    seq_eng.set_points(batch_of(i))
                    seq_eng.enqueue() if args.eager else seq_eng.replay()
            sync()
            out["value_sequential"] = {"frames_per_s": nseq * args.batch / (time.perf_counter() - s0), "frames": nseq,
                                       "what": "one engine on the whole chip, one stream, one frame in flight (--streams 1), inputs resident"}
            out["config"]["value_sequential_frames_per_s"] = out["value_sequential"]["frames_per_s"]
        if not args.no_roofline:
            # the dominant kernel's roofline in THE TIMED CONFIGURATION: on the stream (and CU set) the timed launches run on
            with _on(streams[0] if masked else None):
                roofline_legs(args, out, eng, batch_of, cus=(eng.cu_budget if masked else 0))
            if masked and seq_eng is not eng:
                # ... and on the whole chip, as rounds 1 - 4 reported it (one frame at a time)
                whole = {}
                roofline_legs(args, whole, seq_eng, batch_of)
                out["roofline_whole_chip_engine"] = {k: whole["roofline"][k] for k in ("achieved", "peak", "frac", "avg_launch_ms", "frac_full_map_launches",
                                                                                      "frac_list_launches", "dense_launch_ms", "active_tile_fraction")}
                out["stages_ms_eager_whole_chip_engine"] = whole["stages_ms_eager"]
                out["roofline_spmiddle_whole_chip_engine"] = {k: whole["roofline_spmiddle"][k] for k in ("achieved", "frac", "ms", "algorithmic_bytes")}
        if "roofline" in out and "roofline_spmiddle" in out:
            # what ALL frames in flight achieve together over the driver-timed region: executed matrix-core FLOPs per step (dense stage
            # + the sparse convolutions' executed tile steps) / ms_per_step / the whole chip's peak
            gf = out["roofline"]["dense_stage_executed_gflop"] + out["roofline_spmiddle"]["mfma"]["executed_gflop"]
            out["roofline"]["executed_gflop_per_step"] = gf
            out["roofline"]["frac_chip_timed_region"] = gf / out["ms_per_step"] / F32_MFMA_PEAK_TFLOPS
            cpath = os.path.join(ROOT, "profiles", "r6_mfma_flops_per_frame.json")
            if os.path.exists(cpath) and args.batch == 1 and not args.stress:
                # the same figure with the COUNTED instructions of one frame (SQ_INSTS_MFMA x FLOPs per instruction, committed)
                cg = json.load(open(cpath))["cu_half" if masked else "whole_chip"]["executed_gflop_per_frame"]
                out["roofline"]["executed_gflop_per_step_from_counters"] = cg
                out["roofline"]["frac_chip_timed_region_from_counters"] = cg / out["ms_per_step"] / F32_MFMA_PEAK_TFLOPS
            out["roofline"]["frac_chip_timed_region_note"] = (
                "executed MFMA GFLOP per step (analytic: listed layers with their computed shares, Winograd 16/36; `_from_counters`: "
                "SQ_INSTS_MFMA of one frame x FLOPs per instruction, profiles/r6_mfma_flops_per_frame.json) / ms_per_step / 157.3 "
                "TFLOP/s. The peak is quoted at 2.4 GHz; under this load the chip sustains about 2.0 GHz (profiles/r4_wino_sk_pmc.txt: "
                "SQ_BUSY_CU_CYCLES / CUs / launch time), so 0.83 is the ceiling of any `frac` here")
        if not args.eager and args.batch == 1 and not args.no_host_io and world == 1:
            host_io_legs(args, out, engines, streams, frames_np, dev, latency_engine=seq_eng)
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        if train_res is None and not args.no_train_step and world == 1 and not args.stress and args.batch == 1 and engine_factory is None:
            train_step_leg(args, out, engines, dev)   # (--random-weights / --weights: the leg is informational and runs last)
    if rank == 0:
        print(json.dumps(out), flush=True)
    # ---- ordered teardown (round-5 review item 8): graphs and engines first, the allocator's cached blocks, THEN the process
    # group, THEN the CU-masked streams -- nothing that was recorded on a masked stream (graph nodes, allocator events, the
    # communicator's work objects) outlives it. One deterministic path, with and without a profiler attached.
    if collective:
        dist.barrier()
    if on_gpu and engine_factory is None:
        import gc
        for e in engines:
            e.graph = None
        seq_eng = gathered = eng = e = st = None
        del engines[:]
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    if collective:
        dist.destroy_process_group()
    if masked:
        del streams[:]
        from sessd_hip import ops as _ops
        _ops.close_masked_streams()
    if out is not None and out.get("parity") and not out["parity"]["ok"]:
        raise SystemExit(3)
    return out


def roofline_legs(args, out, eng, batch_of, cus=0):
    """Roofline of the dominant kernel, measured IN THE FRAME: whole frames are enqueued eagerly with a HIP event before and
    after each dense conv launch on the launching stream (engine.dense_layer_times); avg_launch_ms = mean over the launches that
    carry the seven 3x3 stride-1 layers and 20 frames. A loop over ONE layer on a hot input (round 1) is a best case; this is
    what the frame pays, and it agrees with the rocprofv3 kernel trace of the timed region under profiles/."""
    from sessd_hip import ops
    # cus > 0: the engine's stream is confined to that many compute units (frames in flight on CU sets): the launch's roofline is
    # the f32 MFMA peak of ITS compute units; the whole-chip figure is carried beside it
    total_cus = torch.cuda.get_device_properties(eng.dev).multi_processor_count if cus else 0
    PEAK = F32_MFMA_PEAK_TFLOPS                                             # the guide's whole-chip figure: `peak` and `frac` (round 6)
    SET_PEAK = F32_MFMA_PEAK_TFLOPS * (float(cus) / total_cus if cus else 1.0)  # ... the launch's own compute units: frac_of_cu_set_peak
    names = ("b0.0", "b0.1", "b0.2", "conv_0", "conv_1", "b1.1", "b1.2")
    cfgs = [eng.tile_cfg.get(nm) for nm in names]
    wino = all(c in ops.WINOGRAD_CFGS or (c is None and ops.USE_WINOGRAD) for c in cfgs)
    streamk = sum(1 for c in cfgs if c in ops.WINOGRAD_SK_CFGS)
    log("dense tile_cfg:", {k: v for k, v in eng.tile_cfg.items()})
    eng.set_points(batch_of(0))
    lt = eng.dense_layer_times(reps=20)
    # conv_0 + conv_1 may run as ONE launch of twice the work (engine.merge_branch_convs): per-launch figures are averages
    # over the launches that carry the seven layers
    # layers in ACTIVE-TILE mode (block 0, csrc/dense_active.hip) compute only a share of the map's tiles: their FLOPs count with that
    # share (engine.active_tile_fractions(): device counts of the frame just timed). Per-launch figures are totals over the
    # launches that carry the seven layers divided by their number.
    act = eng.active_tile_fractions() if hasattr(eng, "active_tile_fractions") else {}
    per = [(nm, lt[nm], 1, act.get(nm, 1.0)) for nm in names if nm in lt]
    if "conv_0+conv_1" in lt:
        per.append(("conv_0+conv_1", lt["conv_0+conv_1"], 2, act.get("conv_0+conv_1", 1.0)))   # (round 6: may run over a tile list too)
    times = [p[1] for p in per]
    nlayers = sum(p[2] for p in per)
    assert nlayers == len(names)
    kms = sum(times) / len(times)
    flops = CONV_FLOPS * args.batch * sum(p[2] * p[3] for p in per) / len(times)
    ach = flops / (kms * 1e-3) / 1e12
    full = [p for p in per if p[3] == 1.0]
    ach_full = (CONV_FLOPS * args.batch * sum(p[2] for p in full) / (sum(p[1] for p in full) * 1e-3) / 1e12) if full else 0.0
    lst = [p for p in per if p[3] != 1.0]
    ach_list = (CONV_FLOPS * args.batch * sum(p[2] * p[3] for p in lst) / (sum(p[1] for p in lst) * 1e-3) / 1e12) if lst else 0.0
    log("roofline kernel: %.3f ms per launch in sequence" % kms)
    # executed matrix-core FLOPs per algorithmic FLOP: direct 1, Winograd F(2x2,3x3) 16/36, F(4x4,3x3) 36/144
    exe_ratio = sum(ops.winograd_mult_ratio(c if c is not None else (20 if ops.USE_WINOGRAD else 0)) for c in cfgs) / len(cfgs)
    kname = (("conv3x3s1_winograd_sk_kernel / conv3x3s1_winograd_kernel (fused Winograd on f32 MFMA; %d of the 7 "
              "layers are on the stream-K kernel, as the per-layer autotune chose)" % streamk) if wino
             else "conv2d_mfma_kernel<9 taps> (direct implicit GEMM on f32 MFMA)")
    exe = ach * exe_ratio
    out["roofline"] = {"bound": "mfma", "kernel": kname + ": Conv2d 3x3 128->128 @200x176 (5 layers per frame%s) and "
                       "256->256 @100x88 (2 launches, same FLOPs per layer); the seven layers are 72.6 of the frame's 90.8 "
                       "dense GFLOP" % ("; conv_0 and conv_1 as one launch of two weight sets: %d launches" % len(times)
                                        if "conv_0+conv_1" in lt else ""),
                       "achieved": exe, "peak": PEAK, "unit": "TFLOP/s", "frac": exe / PEAK,
                       "cu_set_peak": SET_PEAK, "frac_of_cu_set_peak": exe / SET_PEAK,
                       "compute_units_of_the_launch": cus or None,
                       "peak_note": (("`peak` = %.1f TFLOP/s, the whole chip's dense f32 MFMA peak (MI355X_MICROARCH.md), and `frac` is against it, "
                                      "as in rounds 1 - 4. The launch itself runs on a stream confined to %d of the chip's %d compute units "
                                      "(frames in flight on CU sets) while the other set runs other frames: `frac_of_cu_set_peak` prices it against "
                                      "ITS units' share (%.1f TFLOP/s; round 5 reported that figure as `frac`), `frac_chip_timed_region` is what "
                                      "all frames in flight achieve together over the driver-timed region, `roofline_whole_chip_engine` the same "
                                      "kernel tuned for and measured on the whole chip, one frame at a time")
                                     % (F32_MFMA_PEAK_TFLOPS, cus, total_cus, SET_PEAK)) if cus else None,
                       "frac_definition": "EXECUTED matrix-core FLOPs (what SQ_INSTS_MFMA counts: 16/36 of the direct-"
                                          "convolution count for Winograd F(2x2,3x3)) / launch time / dense f32 MFMA peak",
                       "avg_launch_ms": kms,
                       "active_tile_fraction": act,
                       "frac_full_map_launches": ach_full * exe_ratio / PEAK,
                       "frac_list_launches": (ach_list * exe_ratio / PEAK) if lst else None,
                       "frac_full_map_launches_of_cu_set_peak": ach_full * exe_ratio / SET_PEAK,
                       "frac_list_launches_of_cu_set_peak": (ach_list * exe_ratio / SET_PEAK) if lst else None,
                       "active_tile_note": ("layers listed in active_tile_fraction run over the listed 2x2-output tiles only (the BEV map is "
                                            "zero outside the sparse sites: the other tiles hold a per-channel constant, written by one fill "
                                            "launch); their FLOPs count with that share, the activity + fill launches are in "
                                            "dense_launch_ms['tile_activity+fill']; frac_full_map_launches = the same figure over the "
                                            "launches that cover the whole map (comparable with earlier rounds), frac_list_launches "
                                            "over the list launches alone (short stream-K shares: DESIGN.md section 3)") if act else None,
                       "avg_launch_source": "HIP events before / after each of the kernel's %d launches inside 20 whole frames " % len(times) +
                                            "(eager enqueue; same stream as the kernels; one frame in flight, the same "
                                            "launch configuration as the timed region unless --sk-workgroups says otherwise)",
                       "dense_launch_ms": {k: round(v, 5) for k, v in lt.items()},
                       "dense_tile_cfg": {k: eng.tile_cfg.get(k) for k in lt},
                       "flops_per_launch_executed": flops * exe_ratio,
                       "flops_per_launch_algorithmic": flops,
                       "achieved_algorithmic": ach, "frac_algorithmic": ach / PEAK,
                       "frac_algorithmic_note": "direct-convolution FLOPs 2*H*W*Cin*Cout*9 / time: a speed-up figure, not a "
                                                "utilisation -- it exceeds 1 at batch >= 4",
                       "traffic": None}
    # EXECUTED matrix-core FLOPs of the whole dense stage per batch (what SQ_INSTS_MFMA counts, up to the padding of the last tile block
    # of a list): Winograd layers 16/36 of the direct count, every listed layer with its computed share; direct kernels in full
    a_ = lambda nm: act.get(nm, 1.0)
    HW, HW2 = 200 * 176, 100 * 88
    dense_exec = (CONV_FLOPS * sum(p[2] * p[3] for p in per) * exe_ratio                       # the seven 3x3 stride-1 layers
                  + 2.0 * HW2 * 128 * 256 * 9 * a_("b1.0")                                    # 3x3 stride 2, 128 -> 256
                  + 2.0 * HW * 128 * 128 * a_("trans_0") + 2.0 * HW2 * 256 * 256 * a_("trans_1")  # the 1x1 layers
                  + 2 * 2.0 * HW2 * 256 * 128 * 9 * a_("deconv_0+deconv_1")                   # two ConvTranspose2d 3x3 stride 2, 256 -> 128
                  + 2.0 * HW * 128 * 22) * args.batch / 1e9                                    # the four 1x1 heads
    out["roofline"]["dense_stage_executed_gflop"] = dense_exec
    # HBM traffic of that kernel comes from separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE), committed
    # under profiles/; it cannot be collected inside this process
    cands = ["r4_wino_sk_traffic.json", "r3_wino_sk_traffic.json", "r2_wino_sk_traffic.json"] if streamk else ["r1_winograd_traffic.json"]
    if streamk and act:
        cands[:0] = ["r6_wino_traffic.json", "r5_wino_traffic.json", "r4s2_wino_traffic.json"]  # counter passes of the frame with the list launches (average over its six launches)
    cands = cands if wino else ["r1_conv_traffic.json"]
    for nm in cands:
        tpath = os.path.join(ROOT, "profiles", nm)
        if os.path.exists(tpath) and args.batch == 1:
            tj = json.load(open(tpath))
            out["roofline"]["traffic"] = tj["traffic_bytes"]
            out["roofline"]["traffic_source"] = tj["source"]
            if tj.get("algorithmic_bytes_per_launch"):
                out["roofline"]["traffic_algorithmic_bytes"] = tj["algorithmic_bytes_per_launch"]
                out["roofline"]["traffic_times_algorithmic"] = round(tj["traffic_bytes"] / float(tj["algorithmic_bytes_per_launch"]), 2)
                out["roofline"]["traffic_configuration"] = tj.get("traffic_configuration")
            break
    # ---- per-stage time (eager, events) and the HBM roofline of SpMiddleFHD (algorithmic bytes / time)
    eng.set_points(batch_of(0))
    st = eng.stage_times()
    sp_bytes, sites = eng.spmiddle_algorithmic_bytes()
    out["stages_ms_eager"] = {k: round(v, 4) for k, v in st.items()}
    gbs = sp_bytes / (st["spmiddle"] * 1e-3) / 1e9
    out["roofline_spmiddle"] = {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0,
                                "compute_units_of_the_stage": cus or None,
                                "algorithmic_bytes": sp_bytes, "sites_per_level": sites, "ms": st["spmiddle"],
                                "mfma": eng.spmiddle_mfma_report(),
                                "note": "all 14 sparse layers + the site / rulebook chain of one batch, eager launches; at "
                                        "batch 1 the stage is launch/latency-bound, see --stress for the meaningful case. "
                                        "`mfma`: per-layer HIP-event times of the sparse convs alone and their EXECUTED f32 "
                                        "MFMA rate (active 16-site tile x offset steps x 16 x Cin x Cout x 2 FLOP) against the "
                                        "157.3 TFLOP/s peak; counters and HBM traffic per kernel: profiles/r4_sparse_pmc.txt, r5_sparse_pmc_stress.txt"}


def train_step_leg(args, out, engines, dev):
    """BASELINE.json configs[2] next to the metric line (informational, never `value`): one SE-SSD training iteration -- teacher
    forward, student forward, MultiGroupHead.loss + consistency loss (the capacity-form device op sessd_head_loss), backward,
    fused clip / Adam / EMA -- captured as ONE hipGraph on a labelled synthetic batch of 4, ms per replay
    (sessd_hip.trainbench). The inference engines are released first."""
    from sessd_hip import trainbench
    for e in engines:
        e.graph = None
    torch.cuda.synchronize()
    try:
        res, _ = trainbench.measure(dev, batch=4, steps=args.train_replays, real_loss=True)
        out["train_step"] = res
    except Exception as ex:  # the inference line must not die with the informational leg
        out["train_step"] = {"error": repr(ex)[:300]}


def host_io_legs(args, out, engines, streams, frames_np, dev, latency_engine=None):
    """PCIe-inclusive rates (never `value`): (a) pipelined -- pinned host points in, host detections out, H2D one frame ahead on
    a copy stream, the timed engines and graphs, detections fetched from the device record rings every `fetch_every` frames
    (sessd_hip/runner.py); (b) latency mode -- one frame at a time with a host synchronisation per frame."""
    from sessd_hip.runner import HostFedPipeline
    eng = latency_engine if latency_engine is not None else engines[0]   # (latency mode: the whole-chip engine on the current stream)
    pinned = [torch.from_numpy(f).pin_memory() for f in frames_np[:8]]
    nio = 100
    stage = torch.empty((args.points, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    for i in range(nio):
        src = pinned[i % len(pinned)]
        dst = stage[:src.shape[0]]
        dst.copy_(src, non_blocking=True)
        eng.set_points([dst])
        eng.replay()
        last = eng.results()
    lat = nio / (time.perf_counter() - h0)
    # pipelined: needs rings of 2 * fetch_every records -> re-attach + re-capture (the ring address is part of the graph)
    fetch_every, ring = [int(v) for v in os.environ.get("SESSD_HOSTIO", "16,4").split(",")]   # (probe knob; the defaults ship)
    for e, st in zip(engines, streams):
        e.graph = None
        e.attach_records(2 * fetch_every)
        with torch.cuda.stream(st):
            e.capture()
    torch.cuda.synchronize()
    pipe = HostFedPipeline(engines, streams, ring=ring, fetch_every=fetch_every)
    npipe = 400
    for warm in (True, False):
        pipe.reset()
        n_out = 0
        p0 = time.perf_counter()
        t_sub = 0.0
        for i in range(64 if warm else npipe):
            ts = time.perf_counter()
            pipe.submit(pinned[i % len(pinned)])
            t_sub += time.perf_counter() - ts
            if (i & 15) == 15:
                n_out += len(pipe.poll())
        rest = pipe.finish()
        n_out += len(rest)
        pdt = time.perf_counter() - p0
    assert n_out == npipe, (n_out, npipe)
    # the pipelined path must return what the one-frame-at-a-time path returns for the same frame (same engines, same graphs)
    src = pinned[(npipe - 1) % len(pinned)]
    dst = stage[:src.shape[0]]
    dst.copy_(src)
    e_last = engines[(npipe - 1) % len(engines)]
    e_last.set_points([dst])
    e_last.replay()
    ref = e_last.results()[0]
    same = bool(np.array_equal(ref["box3d_lidar"], rest[-1]["box3d_lidar"]) and np.array_equal(ref["scores"], rest[-1]["scores"]))
    out["host_io"] = {"frames_per_s": npipe / pdt, "frames": npipe, "engines": len(engines), "staging_ring_depth": ring,
                      "fetch_every": fetch_every, "detections_returned": n_out, "last_frame_equals_latency_mode": same,
                      "host_ms_in_submit_per_frame": t_sub / npipe * 1e3,
                      "what": "pinned host points -> H2D on a copy stream (up to %d frames ahead per engine) -> stage + graph replay on "
                              "%d engine streams -> the frame appends its record on the device -> D2H of the record ring every %d "
                              "frames into pinned memory; host detections for every frame, no host sync per frame "
                              "(sessd_hip.runner.HostFedPipeline)" % (ring, len(engines), fetch_every),
                      "latency_mode_frames_per_s": lat,
                      "latency_mode": "H2D -> replay -> D2H with a host synchronisation per frame, one frame in flight"}


def _spawn_entry(local_rank, argv, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(local_rank), LOCAL_RANK=str(local_rank))
    args = parse(argv)
    os.environ["WORLD_SIZE"] = str(args.gpus)
    run_rank(args, local_rank, args.gpus, local_rank)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: one process per GPU spawned here (the torchrun path below stays as it was)
        import torch.multiprocessing as mp
        if torch.cuda.device_count() < args.gpus:
            raise SystemExit("--gpus %d but only %d GPU(s) visible" % (args.gpus, torch.cuda.device_count()))
        mp.spawn(_spawn_entry, args=(list(argv), free_port()), nprocs=args.gpus, join=True)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    run_rank(args, rank, world, local_rank)


if __name__ == "__main__":
    main()
