"""sessd_assign_targets_batch (ops.AssignTargets: every frame and every task of a batch in one clear and two launches, the
ground-truth counts read on the device) on the MI355X:
  * against tests/golden/assign_multi_ref.npz (the REFERENCE's create_target_np run from source per task) and the per-task CPU
    wrapper tests/assign_multi_ref.py: labels, positive sets and ids identical, targets within 1e-6 (float32 log / sqrt of the
    device library against numpy), exactly 0 off the positives -- the rule of tests/test_assign_target_gpu.py;
  * against the per-frame kernel that predates it (ops.assign_targets), bit for bit;
  * counts, classes, layouts, capture, and its users: the head loss, the AssignTarget stage, DeviceBatcher.batched_targets."""
import numpy as np
import pytest
import torch

import assign_multi_ref as amr
from sessd_hip import configs, ops

pytestmark = pytest.mark.gpu

KEYS = ("labels", "reg_targets", "reg_weights", "gt_id")
MIXES = {3: ("abc", "def", "gha"), 4: ("aceg", "bdfh")}   # every golden frame, as batches of three and of four


def _on(dev, tasks):
    return [dict(t, anchors=torch.from_numpy(np.ascontiguousarray(t["anchors"])).to(dev)) for t in tasks]


def _pack(frames, G, filler=np.nan):
    """frames: list of (gt (M, 7), classes (M,)) -> gt (B, G, 7) with `filler` beyond the count, classes (B, G), count (B,)"""
    B = len(frames)
    gt = np.full((B, G, 7), filler, np.float32)
    cls = np.full((B, G), 1, np.int32)
    cnt = np.zeros(B, np.int32)
    for b, (g, c) in enumerate(frames):
        gt[b, :len(g)], cls[b, :len(g)], cnt[b] = g, c, len(g)
    return gt, cls, cnt


def _run(dev, op, gt, cls=None, cnt=None, **kw):
    d = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    r = op.run(d(gt), d(cls), d(cnt), **kw)
    torch.cuda.synchronize()
    return {k: [None if v is None else v.cpu().numpy() for v in r[k]] for k in KEYS}


def _single(dev, anchors_dev, gt, matched, unmatched):
    """the per-frame kernel that predates the batched one"""
    r = ops.assign_targets(anchors_dev, torch.from_numpy(np.ascontiguousarray(gt, np.float32).reshape(-1, 7)).to(dev), None, matched, unmatched)
    return dict(labels=r["labels"].cpu().numpy(), reg_targets=r["bbox_targets"].cpu().numpy(),
                reg_weights=r["bbox_outside_weights"].cpu().numpy(), gt_id=r["gt_id"].cpu().numpy())


def _same_bits(got, b, t, want, where):
    for k in KEYS:
        if got[k][t] is not None:
            assert np.array_equal(got[k][t][b].view(np.int32), want[k].view(np.int32)), (k, where)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return {k: amr.Golden(golden_dir, k) for k in ("c3", "pp")}


@pytest.fixture(scope="module")
def wrapper(golden):
    """the CPU wrapper on every golden (config, frame): computed once, shared, never written"""
    return {(k, f): amr.assign_tasks(G.tasks, *G.frame(f)) for k, G in golden.items() for f in amr.FRAMES}


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("key", ["c3", "pp"])
def test_golden_wrapper_and_the_per_frame_kernel(dev, golden, wrapper, key, B):
    """cases 1 and 2 of the batched op: every golden frame in a batch mix, against the reference run, the wrapper and -- bit for
    bit, per (frame, task) -- ops.assign_targets on the rows of the task's class"""
    G = golden[key]
    tasks = _on(dev, G.tasks)
    op = ops.AssignTargets(B, G.A, tasks, dev, gt_capacity=32)
    for mix in MIXES[B]:
        got = _run(dev, op, *_pack([G.frame(f) for f in mix], 32))
        for b, f in enumerate(mix):
            gt, cls = G.frame(f)
            for t, task in enumerate(G.tasks):
                G.check(f, t, got["labels"][t][b], got["reg_targets"][t][b], got["reg_weights"][t][b], got["gt_id"][t][b])
                w = wrapper[key, f][t]
                assert np.array_equal(got["labels"][t][b], w["labels"]) and np.array_equal(got["gt_id"][t][b], w["gt_id"])
                assert np.abs(got["reg_targets"][t][b] - w["reg_targets"]).max() < 1e-6
                want = _single(dev, tasks[t]["anchors"], gt[cls == task["class_id"]], task["matched_threshold"], task["unmatched_threshold"])
                _same_bits(got, b, t, want, (key, f, t))


@pytest.mark.parametrize("A", [1, 70, 255, 256, 257, 2146])
def test_anchor_counts_around_the_block_size_equal_the_per_frame_kernel(dev, golden, A):
    G = golden["pp"]
    task = dict(G.tasks[0], anchors=G.tasks[0]["anchors"][500:500 + A] if A < 1000 else G.tasks[0]["anchors"])
    frames = [G.frame(f) for f in "hag"]
    tasks = _on(dev, [task])
    got = _run(dev, ops.AssignTargets(3, A, tasks, dev, gt_capacity=30), *_pack(frames, 30))
    for b, (gt, cls) in enumerate(frames):
        _same_bits(got, b, 0, _single(dev, tasks[0]["anchors"], gt[cls == 1], 0.6, 0.45), (A, b))
    assert A < 1000 or sum(int((got["labels"][0][b] > 0).sum()) for b in range(3)) > 50


def _cars(rng, n, extent):
    x0, y0, x1, y1 = extent
    b = np.zeros((n, 7), np.float32)
    b[:, 0] = rng.uniform(x0, x1, n); b[:, 1] = rng.uniform(y0, y1, n); b[:, 2] = -1.0
    b[:, 3:6] = np.array([1.6, 3.9, 1.56], np.float32) * rng.uniform(0.9, 1.1, (n, 3)).astype(np.float32)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


@pytest.mark.parametrize("G,counts", [(1, (0, 1, 1, 0)), (128, (0, 1, 128, 37))])
def test_counts_come_from_the_device_and_rows_beyond_them_are_never_read(dev, golden, G, counts):
    """case 3: gt_count holding 0, 1, G and a value in between in one batch; the rows beyond a count hold NaN, or copies of
    anchors (which would be forced positives with IoU 1): the outputs equal the run where those rows are harmless, and the
    per-frame kernel on the live rows; gt_count=None reads all G rows."""
    P = golden["pp"]
    tasks = _on(dev, P.tasks[:1])
    anchors = P.tasks[0]["anchors"]
    r = P.g["pp_range0"]
    rng = np.random.RandomState(7)
    live = [_cars(rng, G, (r[0], r[1], r[3], r[4])) for _ in counts]
    far = np.array([150.0, 150.0, -1.0, 1.6, 3.9, 1.56, 0.0], np.float32)
    bad, clean = np.stack(live), np.stack(live)
    for b, n in enumerate(counts):
        clean[b, n:] = far
        bad[b, n:] = np.nan
        bad[b, n::2] = anchors[(37 * np.arange(len(bad[b, n::2])) + 11) % len(anchors)]
    cnt = np.array(counts, np.int32)
    op = ops.AssignTargets(len(counts), P.A, tasks, dev, gt_capacity=G)
    got, ref = _run(dev, op, bad, None, cnt), _run(dev, op, clean, None, cnt)
    for k in KEYS:
        assert np.array_equal(got[k][0].view(np.int32), ref[k][0].view(np.int32)), k
    for b, n in enumerate(counts):
        _same_bits(got, b, 0, _single(dev, tasks[0]["anchors"], live[b][:n], 0.6, 0.45), (G, b))
        if n == 0:
            assert not got["labels"][0][b].any() and not got["reg_targets"][0][b].any() and np.all(got["gt_id"][0][b] == -1)
    full = _run(dev, op, np.stack(live), None, None)
    for b in range(len(counts)):
        _same_bits(full, b, 0, _single(dev, tasks[0]["anchors"], live[b], 0.6, 0.45), (G, b, "all rows"))
    assert int((full["labels"][0] > 0).sum()) > int((got["labels"][0] > 0).sum())


def test_classes(dev, golden):
    """case 4: a frame whose rows all belong to another task; class_id = 0; gt_classes = None"""
    G = golden["c3"]
    gt, cls = G.frame("h")
    cars = gt[cls == 1]
    tasks = _on(dev, G.tasks)
    op = ops.AssignTargets(2, G.A, tasks, dev, gt_capacity=30)
    got = _run(dev, op, *_pack([(cars, np.ones(len(cars), np.int32)), (gt, cls)], 30))
    for t in (1, 2):   # frame 0 has cars only
        assert not got["labels"][t][0].any() and not got["reg_targets"][t][0].any() and not got["reg_weights"][t][0].any()
        assert np.all(got["gt_id"][t][0] == -1) and (got["labels"][t][1] > 0).any()
    assert (got["labels"][0][0] > 0).any()
    every = [dict(t, class_id=0) for t in tasks]   # every live row, as enable_similar_type
    packed = _pack([(gt, cls), (cars, np.ones(len(cars), np.int32))], 30)
    for r in (_run(dev, ops.AssignTargets(2, G.A, every, dev, gt_capacity=30), *packed),
              _run(dev, op, packed[0], None, packed[2])):                                  # gt_classes = None
        for b, rows in enumerate((gt, cars)):
            for t, task in enumerate(G.tasks):
                _same_bits(r, b, t, _single(dev, tasks[t]["anchors"], rows, task["matched_threshold"], task["unmatched_threshold"]), (b, t))


def test_layouts(dev, golden):
    """case 5: per-frame anchors, int64 labels, optional outputs absent, and `out=` written in place with nothing else touched"""
    G = golden["c3"]
    frames = [G.frame("a"), G.frame("h")]
    packed = _pack(frames, 30)
    B, A, T = 2, G.A, 3
    shifted = []
    for t in G.tasks:
        a = np.stack([t["anchors"], t["anchors"]])
        a[1, :, 0] += np.float32(0.13)
        a[1, :, 1] -= np.float32(0.07)
        shifted.append(dict(t, anchors=a))
    per_frame = _on(dev, shifted)
    op = ops.AssignTargets(B, A, per_frame, dev, gt_capacity=30)
    got = _run(dev, op, *packed)
    assert all(tuple(a.shape) == (B, A, 7) and a.is_contiguous() for a in op.anchors)
    for b, (gt, cls) in enumerate(frames):
        for t, task in enumerate(G.tasks):
            want = _single(dev, per_frame[t]["anchors"][b].contiguous(), gt[cls == task["class_id"]], task["matched_threshold"],
                           task["unmatched_threshold"])
            _same_bits(got, b, t, want, ("per frame", b, t))
    assert any(not np.array_equal(got["labels"][t][0], got["labels"][t][1]) for t in range(T))
    # ---- shared anchors; int64 labels equal the int32 ones
    tasks = _on(dev, G.tasks)
    op32, op64 = ops.AssignTargets(B, A, tasks, dev, gt_capacity=30), ops.AssignTargets(B, A, tasks, dev, gt_capacity=30, labels_i64=True)
    r32, r64 = _run(dev, op32, *packed), _run(dev, op64, *packed)
    for t in range(T):
        assert r64["labels"][t].dtype == np.int64 and r32["labels"][t].dtype == np.int32
        assert np.array_equal(r64["labels"][t], r32["labels"][t].astype(np.int64))
        assert all(np.array_equal(r64[k][t].view(np.int32), r32[k][t].view(np.int32)) for k in KEYS[1:])
        assert torch.equal(op32.anchors[t][1], tasks[t]["anchors"]) and tuple(op32.anchors[t].shape) == (B, A, 7)
    # ---- out=: guard rows of a sentinel around every output, the object's own tensors untouched, weights and ids not computed
    pad = 3
    guarded = lambda tail, dt: [torch.full((B + 2 * pad, A) + tail, -77, dtype=dt, device=dev) for _ in range(T)]
    lab, reg = guarded((), torch.int64), guarded((7,), torch.float32)
    for k in KEYS:
        for v in op64.out[k]:
            v.fill_(-55)
    d = lambda a: torch.from_numpy(a).to(dev)
    res = op64.run(d(packed[0]), d(packed[1]), d(packed[2]),
                   out=dict(labels=[v[pad:pad + B] for v in lab], reg_targets=[v[pad:pad + B] for v in reg], reg_weights=False, gt_id=False))
    torch.cuda.synchronize()
    assert res["reg_weights"] == [None] * T and res["gt_id"] == [None] * T
    for t in range(T):
        assert res["labels"][t].data_ptr() == lab[t][pad].data_ptr()
        assert np.array_equal(lab[t][pad:pad + B].cpu().numpy(), r64["labels"][t])
        assert np.array_equal(reg[t][pad:pad + B].cpu().numpy().view(np.int32), r64["reg_targets"][t].view(np.int32))
        for v in (lab[t], reg[t]):
            assert bool((v[:pad] == -77).all()) and bool((v[pad + B:] == -77).all())
        assert all(bool((op64.out[k][t] == -55).all()) for k in KEYS)
    # ---- one of the optional outputs only, into the object's own tensors
    res = op64.run(d(packed[0]), d(packed[1]), d(packed[2]), out=dict(gt_id=False))
    torch.cuda.synchronize()
    for t in range(T):
        assert np.array_equal(res["reg_weights"][t].cpu().numpy(), r64["reg_weights"][t]) and bool((op64.out["gt_id"][t] == -55).all())
    with pytest.raises(ValueError):
        op64.run(d(packed[0]), d(packed[1]), d(packed[2]), out=dict(labels=[v[pad:pad + B].int() for v in lab]))
    with pytest.raises(ValueError):
        op64.run(d(packed[0]).cpu())
    with pytest.raises(ValueError):
        op64.run(d(packed[0]), d(packed[1]).long())


def test_capture_and_replay_with_boxes_and_counts_refilled(dev, golden):
    """case 6: run() captured once in a torch.cuda.graph; boxes, classes and counts refilled in place between two replays: the
    outputs equal the eager call on the same inputs bit for bit, and a repeated replay gives them again"""
    G = golden["c3"]
    B, T = 2, 3
    tasks = _on(dev, G.tasks)
    op, eager = ops.AssignTargets(B, G.A, tasks, dev, gt_capacity=32), ops.AssignTargets(B, G.A, tasks, dev, gt_capacity=32)
    fills = [_pack([G.frame(f) for f in mix], 32) for mix in ("ah", "cg", "hd")]
    d = lambda a: torch.from_numpy(a).to(dev)
    static = [d(a) for a in fills[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op.run(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op.run(*static)
    outs = lambda o: [v for k in KEYS for v in o.out[k]]
    for fill in fills[1:]:
        for dst, src in zip(static, fill):
            dst.copy_(d(src))
        for v in outs(op):
            v.fill_(-9)
        graph.replay()
        eager.run(*[d(a) for a in fill])
        torch.cuda.synchronize()
        first = [v.clone() for v in outs(op)]
        assert all(torch.equal(a, b) for a, b in zip(first, outs(eager)))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, outs(op)))
    assert sum(int((v > 0).sum()) for v in op.out["labels"]) > 20


def test_targets_feed_the_supervised_head_loss(dev, golden, wrapper):
    """case 7: a three-task head (B = 2, A = 3520) on the targets of AssignTargets against the same head on the wrapper's targets
    uploaded from the host: the same record and gradients bit for bit where labels and targets agree exactly, else within the
    bounds tests/test_supervised_loss_gpu.py holds the device op to against float64 (its VAL and GRAD)."""
    import supervised_loss_ref as SR
    from test_supervised_loss_gpu import GRAD, VAL, _head
    G = golden["c3"]
    B, T, A, mix = 2, 3, G.A, "ah"
    op = ops.AssignTargets(B, A, _on(dev, G.tasks), dev, gt_capacity=32, labels_i64=True)
    d = lambda a: torch.from_numpy(a).to(dev)
    res = op.run(*[d(a) for a in _pack([G.frame(f) for f in mix], 32)])
    c = SR.make_case(91, B, T, A)
    head = _head(T, dev)

    def loss(example):
        _, leaves, preds = SR.example_and_preds(c, dev, torch.int64)
        assert head.supervised_loss_covers(example, preds)
        total, rec = head.loss_supervised_device(example, preds)
        rec = rec.clone()
        total.backward()
        return rec, [l[k].grad.clone() for l in leaves for k in ("box", "cls", "dir")]

    rec_dev, grads_dev = loss(dict(anchors=res["anchors"], labels=res["labels"], reg_targets=res["reg_targets"]))
    host = dict(anchors=[d(np.stack([t["anchors"]] * B)) for t in G.tasks],
                labels=[d(np.stack([wrapper["c3", f][t]["labels"] for f in mix]).astype(np.int64)) for t in range(T)],
                reg_targets=[d(np.stack([wrapper["c3", f][t]["reg_targets"] for f in mix])) for t in range(T)])
    rec_host, grads_host = loss(host)
    assert all(torch.equal(a, b) for a, b in zip(res["labels"], host["labels"]))
    assert float(rec_dev[T, 0]) > 0 and rec_dev[:T, ops.SUPERVISED_LOSS_RECORD["positives"]].min() > 0
    if all(torch.equal(a, b) for a, b in zip(res["reg_targets"], host["reg_targets"])):
        assert torch.equal(rec_dev, rec_host) and all(torch.equal(a, b) for a, b in zip(grads_dev, grads_host))
    else:
        R = ops.SUPERVISED_LOSS_RECORD
        for t in range(T + 1):
            for k in (("loss",) if t == T else SR.VALUE_KEYS):
                assert SR.value_close(rec_dev[t, R[k]], float(rec_host[t, R[k]]), VAL), (t, k)
        for a, b in zip(grads_dev, grads_host):
            ok, msg = SR.grad_close(a.cpu().numpy(), b.cpu().numpy(), GRAD)
            assert ok, msg


def _annotated_frame(rng, names, extent):
    sizes = dict(Car=(1.6, 3.9, 1.56), Pedestrian=(0.6, 0.8, 1.73), Cyclist=(0.6, 1.76, 1.73), Van=(1.9, 5.0, 2.2))
    gt = _cars(rng, len(names), extent)
    for i, n in enumerate(names):
        gt[i, 3:6] = sizes[n]
    gt[:, 6] = rng.uniform(-6, 6, len(names))   # yaw outside [-pi, pi): folded by the stage
    order = ["Car", "Pedestrian", "Cyclist", "Van"]
    return gt, np.array(names), np.array([order.index(n) + 1 for n in names], np.int32)


@pytest.mark.parametrize("which", ["3class", "pointpillars"])
def test_pipeline_stage_on_the_full_maps(dev, which):
    """case 8: AssignTarget from ASSIGNER_3CLASS (three tasks on 200 x 176) and ASSIGNER_POINTPILLARS (one task on 248 x 216) on a
    synthetic annotated frame: per-task lists of the right shapes that equal the wrapper"""
    from det3d.datasets.pipelines import AssignTarget
    cfg, T, A = (configs.ASSIGNER_3CLASS, 3, 70400) if which == "3class" else (configs.ASSIGNER_POINTPILLARS, 1, 107136)
    stage = AssignTarget(cfg=cfg)
    names = ["Car", "Pedestrian", "Van", "Cyclist", "Car", "Pedestrian", "Cyclist", "Car"]
    gt, gt_names, gt_classes = _annotated_frame(np.random.RandomState(12), names, (5, -30, 60, 30))
    ann = lambda: dict(gt_boxes=gt.copy(), gt_classes=gt_classes.copy(), gt_names=gt_names.copy())
    res = dict(mode="train", labeled=True, lidar=dict(annotations=ann(), annotations_raw=ann()))
    res, _ = stage(res, None)
    tg = res["lidar"]["targets"]
    folded = gt.copy()
    folded[:, 6] = folded[:, 6] - np.floor(folded[:, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
    gens = cfg["target_assigner"]["anchor_generators"]
    for k in ("anchors", "labels", "reg_targets", "reg_weights", "positive_gt_id"):
        assert len(tg[k]) == T and len(res["lidar"]["targets_raw"][k]) == T, k
    for t, g in enumerate(gens):
        assert tg["anchors"][t].shape == (A, 7) and tg["labels"][t].shape == (A,) and tg["reg_targets"][t].shape == (A, 7)
        assert tg["reg_weights"][t].shape == (A,)
        rows = gt_names == g["class_name"]
        want = amr.assign_task(tg["anchors"][t], folded[rows], None, 0, g["matched_threshold"], g["unmatched_threshold"])
        assert np.array_equal(tg["labels"][t], want["labels"]) and np.abs(tg["reg_targets"][t] - want["reg_targets"]).max() < 1e-6
        assert np.array_equal(tg["positive_gt_id"][t][0], want["positive_gt_id"]) and np.array_equal(tg["reg_weights"][t], want["reg_weights"])
        assert int((want["labels"] > 0).sum()) >= int(rows.sum()) > 0
        assert np.array_equal(res["lidar"]["targets_raw"]["labels"][t], tg["labels"][t])
        assert np.array_equal(res["lidar"]["annotations"]["gt_boxes"][t], folded[rows])
    if which == "3class":
        assert np.array_equal(np.stack(tg["anchors"]), configs.kitti_3class_anchors())


def test_batcher_batched_targets_leaves_the_same_bits(dev):
    """case 9: DeviceBatcher.batched_targets = True (two AssignTargets.run calls into the example) against the default path (a
    call and two copies per frame and view), on a pool of 3 frames, B = 2, two iterations"""
    from sessd_hip import trainloop
    pool = trainloop.ScenePool(range(720, 723), 20000)
    a = trainloop.DeviceBatcher(pool, dev, 2, iterations=2, seed=3)
    b = trainloop.DeviceBatcher(pool, dev, 2, iterations=2, seed=3)
    assert a.batched_targets is False
    b.batched_targets = True
    for it in range(2):
        ea, eb = a.load(it), b.load(it)
        torch.cuda.synchronize()
        for k in ("labels", "reg_targets", "labels_raw", "reg_targets_raw"):
            assert torch.equal(ea[k][0], eb[k][0]), (it, k)
        assert int((eb["labels"][0] > 0).sum()) > 0 and int((eb["labels_raw"][0] > 0).sum()) > 0
    assert b._assigner is not None and a._assigner is None
