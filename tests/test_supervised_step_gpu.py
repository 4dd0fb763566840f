"""train.SupervisedTrainStep, the capacity form of the PointPillars pass, trainloop.SupervisedBatcher and fit_supervised on the
device, on the small models the other test files build: test_pointpillars_detector_gpu.build_model (48 x 32 pillar grid, 24 x 16
head map, B = 2) and the reduced three-class model of test_multitask_engine_gpu.

What is compared with what:
  capacity form   the live rows in a table of twice the capacity with finite junk behind the count against the exact example:
                  total, record and every parameter gradient torch.equal (dead rows add nothing to any total)
  one step        the flat parameters after one call against oracle/optim.py (clip_coef + adam_true_wd_ema_step, no teacher) on
                  the flat gradient the step produced: rtol 2e-6, atol 1e-7, the bound of tests/test_train_gpu.py; the device
                  schedule against the host schedule at the same bound
  it trains       twenty iterations on one batch: the record's total falls, everything finite, lr = one_cycle
  captured        capture(warmup=1) + two replays against three eager device-schedule iterations on the same three batches
                  (written INTO the static example between replays): flat.data, exp_avg, exp_avg_sq torch.equal
  fresh batches   fit_supervised, captured against eager: bit-identical final parameters; SupervisedBatcher.load's labels and
                  targets against ops.assign_targets per frame on the reference's kept boxes (tests/draw_batch_ref.py)"""
import copy

import numpy as np
import pytest
import torch

import draw_batch_ref as DR
import supervised_loss_ref as SR
import test_multitask_engine_gpu as MT
import test_pointpillars_detector_gpu as PP
from oracle import optim as ooptim
from sessd_hip import configs, ops, synth
from sessd_hip import train as strain
from sessd_hip import trainloop

pytestmark = pytest.mark.gpu
PP_VG = dict(range=PP.VRANGE, voxel_size=PP.VSIZE)


@pytest.fixture(scope="module")
def pp_model():
    """the seeded small PointPillars model, on the CPU: every test takes a deep copy to the device"""
    return PP.build_model()


def _pp(pp_model, dev, any_width=True):
    """A copy on the device, switched to supervised. train_any_width = True: the maps of the second and third neck block are 12
    and 6 cells wide, and without it their convs run as torch modules (strain.check_trainable names them) -- whose MIOpen
    convolutions are not reproducible from one call to the next on the same input (measured: equal canvas, unequal neck output),
    so nothing downstream could be held bit for bit."""
    m = copy.deepcopy(pp_model).to(dev).train()
    m.supervised = True
    if any_width:
        m.neck.train_any_width = True
    return m


def _targets(seed, B, T, anc, dev, labels_dtype=torch.int32):
    """synthetic labels / reg_targets on the model's own anchors: anc (A, 7) for every task or (T, A, 7)"""
    anc = np.asarray(anc, np.float32)
    A = anc.shape[-2]
    c = SR.make_case(seed, B, T, A, n_pos=20, n_ignore=40, anchors=anc if anc.ndim == 2 else None)
    if anc.ndim == 3:
        c["anchors"][:] = anc[:, None]
        c["reg_targets"][..., 6][(c["labels"] > 0) & (np.abs(c["reg_targets"][..., 6] + c["anchors"][..., 6]) < 4e-3)] += np.float32(0.05)
        SR.check_margin(c)
    return SR.example_and_preds(c, dev, labels_dtype)[0]


def _pp_batch(dev, frame_seeds, case_seed, capacity=None, junk=False):
    """An example of the small PointPillars geometry: exact (rows cut to the live count), or with `capacity` rows and the count in
    num_voxels_dev; junk=True fills the rows beyond the count with finite junk (features 1e3, T points, in-canvas cells)."""
    pts = [torch.from_numpy(synth.make_frame(s, 20000)).to(dev) for s in frame_seeds]
    B = len(pts)
    r = ops.voxelize_batch(pts, PP.VSIZE, PP.VRANGE, PP.T, PP.MAX_VOXELS)
    prefix = r["prefix"].cpu().numpy()
    m = int(prefix[B])
    ex = _targets(case_seed, B, 1, PP.anchors(), dev)
    ex.update(voxels=r["voxels"][:m].clone(), coordinates=r["coors"][:m].clone(), num_points=r["num_points"][:m].clone(),
              num_voxels=torch.from_numpy(np.diff(prefix)), shape=[PP.GRID])
    if capacity is None:
        return ex, m
    assert capacity >= m
    cap = strain.capacity_example(ex, capacity)
    if junk:
        cap["voxels"][m:] = 1.0e3
        cap["num_points"][m:] = PP.T
        cap["coordinates"][m:] = torch.tensor([0, 0, 3, 5], dtype=torch.int32, device=dev)
    return cap, m


def _grads(model, example):
    model.zero_grad(set_to_none=True)
    total, rec = model.forward_loss(example)
    total.backward()
    return total.detach().clone(), rec.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------------------------------------------------------ 1
def test_capacity_form_gives_the_exact_rows_bits(pp_model, dev):
    model = _pp(pp_model, dev)
    exact, m = _pp_batch(dev, PP.FRAME_SEEDS, 81)
    padded, _ = _pp_batch(dev, PP.FRAME_SEEDS, 81, capacity=2 * m, junk=True)
    assert padded["voxels"].shape[0] == 2 * m and int(padded["num_voxels_dev"].item()) == m
    assert model.reader.on_device_train_path(padded["voxels"])
    t0, r0, g0 = _grads(model, exact)
    t1, r1, g1 = _grads(model, padded)
    assert torch.isfinite(t0) and float(t0) > 0
    assert torch.equal(t0, t1), (float(t0), float(t1))
    assert torch.equal(r0, r1)
    assert set(g0) == set(g1) and len(g0) >= len(list(model.parameters())) - 2
    differ = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    for n in differ:
        print("%-40s max |difference| %.3e of %.3e" % (n, float((g0[n] - g1[n]).abs().max()), float(g0[n].abs().max())))
    assert not differ, differ
    # ... and the count is what is read, not the table: the same table with the count cut to half gives another loss
    padded["num_voxels_dev"].fill_(m // 2)
    t2, _, _ = _grads(model, padded)
    assert not torch.equal(t0, t2)
    # eval mode: the features and the canvas of the live rows
    model.eval()
    padded["num_voxels_dev"].fill_(m)
    with torch.no_grad():
        data = lambda e: dict(features=e["voxels"], num_voxels=e["num_points"], coors=e["coordinates"], batch_size=2, input_shape=PP.GRID,
                              num_voxels_dev=e.get("num_voxels_dev"))
        assert torch.equal(model.extract_feat(data(exact)), model.extract_feat(data(padded)))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_one_step_against_the_oracle_optimizer(pp_model, dev):
    ex, _ = _pp_batch(dev, PP.FRAME_SEEDS, 82)
    step = strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=10)
    assert step.opt.t is None and step.flat.numel == sum((p.numel() + 3) // 4 * 4 for p in step.model.parameters())
    p0 = step.flat.data.clone()
    loss, lr, mom = step(ex)
    assert np.isfinite(float(loss)) and abs(lr - 3e-4) < 1e-12 and abs(mom - 0.95) < 1e-12
    assert step.last_record.shape == (2, ops.SUPERVISED_LOSS_ROW)
    rec = step.record()
    assert abs(float(rec["total"]) - float(loss)) <= 1e-6 * abs(float(loss)) and int(rec["num_pos"][0]) == 20
    g = step.flat.grad.cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    p = p0.cpu().numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    ooptim.adam_true_wd_ema_step(p, g, m, v, None, lr, 0.01, mom, 0.99, 1e-8, 1, max_norm=35.0)
    assert np.allclose(step.flat.data.cpu().numpy(), p, rtol=2e-6, atol=1e-7)
    norm, coef = ooptim.clip_coef(g, 35.0)
    got = step.opt.norm_coef.cpu().numpy()
    assert abs(got[0] - norm) <= 1e-5 * norm and abs(got[1] - coef) <= 1e-5 * coef
    # the device schedule against the host schedule: a second trainer from the same start
    dev_step = strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=10)
    assert torch.equal(dev_step.flat.data, p0)
    _, lr_d, mom_d = dev_step(ex, device_schedule=True)
    assert lr_d is None and mom_d is None
    assert torch.equal(dev_step.flat.grad, step.flat.grad)
    assert np.allclose(dev_step.flat.data.cpu().numpy(), step.flat.data.cpu().numpy(), rtol=2e-6, atol=1e-7)
    assert np.allclose(dev_step.opt.lr_mom_dev.cpu().numpy(), [lr, mom], rtol=2e-6)
    # the model's tensors are still views of the flat buffer, and the step counters moved
    assert step.flat.params[0].data_ptr() == step.flat.data.data_ptr() + 4 * step.flat.offsets[0]
    assert step.global_step == 1 and int(step.opt.global_step_dev.item()) == 1 and int(dev_step.opt.global_step_dev.item()) == 1


# ------------------------------------------------------------------------------------------------------------------ 3
def test_twenty_iterations_on_one_batch_lower_the_loss(pp_model, dev):
    ex, _ = _pp_batch(dev, PP.FRAME_SEEDS, 83)
    step = strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=20)
    totals = []
    for i in range(20):
        loss, lr, mom = step(ex)
        want = strain.one_cycle(i, 20)
        assert lr == want[0] and mom == want[1]
        if i in (0, 19):
            totals.append(float(step.record()["total"]))
        assert bool(torch.isfinite(loss))
    print("record total: first %.5f, last %.5f" % tuple(totals))
    assert np.isfinite(totals).all() and totals[1] < totals[0]
    assert bool(torch.isfinite(step.flat.data).all()) and bool(torch.isfinite(step.opt.exp_avg_sq).all())


# ------------------------------------------------------------------------------------------------------------------ 4
def _captured_against_eager(make_step, batches, moving):
    """three eager device-schedule iterations on batches[0..2] against capture(warmup=1) on a static copy of batches[0] and two
    replays, batches[1] and [2] copied INTO the static example in between"""
    eager, graph = make_step(), make_step()
    assert torch.equal(eager.flat.data, graph.flat.data)
    for b in batches:
        eager(b, device_schedule=True)
    static = dict(batches[0])
    for k in moving:
        static[k] = [t.clone() for t in batches[0][k]] if isinstance(batches[0][k], list) else batches[0][k].clone()
    graph.capture(static, warmup=1)
    for b in batches[1:]:
        for k in moving:
            if isinstance(b[k], list):
                for dst, src in zip(static[k], b[k]):
                    dst.copy_(src)
            else:
                static[k].copy_(b[k])
        graph.replay()
    torch.cuda.synchronize()
    assert eager.global_step == graph.global_step == 3 and eager.opt.steps == graph.opt.steps == 3
    assert int(eager.opt.global_step_dev.item()) == int(graph.opt.global_step_dev.item()) == 3
    same = {n: torch.equal(getattr(eager.opt, n), getattr(graph.opt, n)) for n in ("exp_avg", "exp_avg_sq")}
    same["flat.data"] = torch.equal(eager.flat.data, graph.flat.data)
    same["record"] = torch.equal(eager.last_record, graph.last_record)
    assert all(same.values()), same
    return eager, graph


MOVING = ("voxels", "coordinates", "num_points", "num_voxels_dev", "labels", "reg_targets")


def test_captured_pointpillars_iterations_equal_the_eager_ones(pp_model, dev):
    cap = 2 * PP.MAX_VOXELS
    batches = [_pp_batch(dev, seeds, 90 + i, capacity=cap)[0] for i, seeds in enumerate(((5, 6), (7, 8), (9, 10)))]
    assert not torch.equal(batches[0]["num_voxels_dev"], batches[1]["num_voxels_dev"])
    eager, graph = _captured_against_eager(lambda: strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=20), batches, MOVING)
    # the result follows the contents: three iterations on batch 0 alone end elsewhere
    other = strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=20)
    for _ in range(3):
        other(batches[0], device_schedule=True)
    assert not torch.equal(other.flat.data, graph.flat.data)


@pytest.fixture(scope="module")
def three_class(dev):
    return configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_model(), voxel_range=MT.VRANGE)


def _three_class_batch(dev, frame_seed, case_seed, capacity):
    pts = [torch.from_numpy(synth.make_frame(frame_seed, 20000)).to(dev)]
    r = ops.voxelize_batch(pts, MT.VSIZE, MT.VRANGE, 5, MT.MAX_VOXELS)
    m = int(r["prefix"][1].item())
    ex = _targets(case_seed, 1, 3, configs.kitti_3class_anchors((MT.H, MT.W), MT.VRANGE), dev, torch.int64)
    ex.update(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m], num_voxels=torch.tensor([m]),
              shape=[MT.GRID])
    return strain.capacity_example(ex, capacity)


def test_captured_three_class_iterations_equal_the_eager_ones(three_class, dev):
    batches = [_three_class_batch(dev, 5 + i, 95 + i, MT.MAX_VOXELS) for i in range(3)]
    make = lambda: strain.SupervisedTrainStep(copy.deepcopy(three_class), total_steps=20)
    eager, graph = _captured_against_eager(make, batches, MOVING)
    assert eager.last_record.shape == (4, ops.SUPERVISED_LOSS_ROW)
    assert eager.sparse_overflow is not None and int(eager.sparse_overflow.item()) == 0 and int(graph.sparse_overflow.item()) == 0
    eager.check_overflow()
    rec = graph.record()
    assert len(rec["loss"]) == 3 and [int(v) for v in rec["num_pos"]] == [20, 20, 20]


# ------------------------------------------------------------------------------------------------------------------ 5
def _pool(n_scenes=4, n_boxes=6):
    """clouds of the small PointPillars range with car boxes in and around it (class 1). The seed is one at which, for the tables
    SupervisedBatcher draws from seed 0, every corner keeps DR.MARGIN from the range edges (asserted where it is used)."""
    rng = np.random.RandomState(9)
    lo_x, lo_y, _, hi_x, hi_y, _ = PP.VRANGE
    frames = [synth.make_frame(20 + i, 20000 - 1500 * i) for i in range(n_scenes)]
    boxes = []
    for i in range(n_scenes):
        b = np.zeros((n_boxes - (i == 1), 7), np.float32)      # (one scene with a box less: counts differ)
        b[:, 0], b[:, 1] = rng.uniform(lo_x - 3, hi_x + 3, len(b)), rng.uniform(lo_y - 3, hi_y + 3, len(b))
        b[:, 2], b[:, 3:6], b[:, 6] = -1.0, [1.6, 3.9, 1.56], rng.uniform(-np.pi, np.pi, len(b))
        boxes.append(b)
    return frames, boxes


def _batcher(dev, iterations, seed=0):
    frames, boxes = _pool()
    tasks = [dict(anchors=PP.anchors(), class_id=1, matched_threshold=0.6, unmatched_threshold=0.45)]
    return trainloop.SupervisedBatcher(frames, boxes, None, dev, 2, iterations, PP_VG, PP.T, PP.MAX_VOXELS, tasks, PP.GRID, seed=seed)


def test_batcher_targets_are_those_of_the_reference_boxes(dev):
    data = _batcher(dev, 6)
    t = [v.cpu() for v in data.draw.tables]
    case = dict(dims=(data.draw.S, data.draw.P, data.draw.G, data.draw.T, data.draw.B), range_xy=[PP.VRANGE[0], PP.VRANGE[1], PP.VRANGE[3], PP.VRANGE[4]],
                pool_points=t[0], pool_point_count=t[1], pool_boxes=t[2], pool_classes=t[3], pool_box_count=t[4], choice=t[5], par=t[6])
    assert DR.min_margin(case) > DR.MARGIN and torch.equal(t[6], torch.from_numpy(data.par_host))
    anc = torch.from_numpy(PP.anchors()).to(dev)
    ptrs = None
    kept_any = positives = 0
    for it in range(6):
        ex = data.load()
        assert ex is data.example and data.cursor == it + 1
        here = {k: (v if torch.is_tensor(v) else v[0]).data_ptr() for k, v in ex.items() if torch.is_tensor(v) or (isinstance(v, list) and torch.is_tensor(v[0]))}
        assert ptrs is None or here == ptrs        # one static example: the same tensors every time
        ptrs = here
        ref = DR.reference(case, it)
        assert torch.equal(ex["gt_count"].cpu(), ref["gt_count"]) and torch.equal(ex["gt_boxes"].cpu(), ref["gt_boxes"])
        assert torch.equal(ex["transformation_dev"].cpu(), ref["transformation"])
        want_vox = ops.voxelize_staged(data.draw.out["staged"], PP.VSIZE, PP.VRANGE, PP.T, PP.MAX_VOXELS)
        m = int(want_vox["prefix"][2].item())
        assert int(ex["num_voxels_dev"].item()) == m > 0
        assert torch.equal(ex["voxels"][:m], want_vox["voxels"][:m]) and torch.equal(ex["coordinates"][:m], want_vox["coors"][:m])
        for b in range(2):
            k = int(ref["gt_count"][b])
            kept_any += k
            tg = ops.assign_targets(anc, ref["gt_boxes"][b, :k].to(dev), None, 0.6, 0.45)
            assert torch.equal(ex["labels"][0][b], tg["labels"]) and torch.equal(ex["reg_targets"][0][b], tg["bbox_targets"])
        positives += int((ex["labels"][0] > 0).sum())
    assert kept_any > 0 and positives > 0
    with pytest.raises(IndexError):
        data.load()


def test_fit_supervised_captured_equals_eager_on_fresh_batches(pp_model, dev):
    runs = {}
    for capture in (True, False):
        step, rep = trainloop.fit_supervised(_pp(pp_model, dev), _batcher(dev, 6), 6, log_every=3, capture=capture)
        for k in ("iterations", "batch", "timed_iterations", "seconds", "ms_per_iteration", "samples_per_s", "log"):
            assert k in rep, k
        assert rep["iterations"] == 6 and rep["batch"] == 2 and rep["timed_iterations"] == (5 if capture else 6)
        assert [r["iteration"] for r in rep["log"]] == [3, 6] and all(np.isfinite(r["total"]) for r in rep["log"])
        assert step.global_step == 6
        runs[capture] = (step, rep)
    a, b = runs[True][0], runs[False][0]
    assert torch.equal(a.flat.data, b.flat.data) and torch.equal(a.opt.exp_avg, b.opt.exp_avg) and torch.equal(a.opt.exp_avg_sq, b.opt.exp_avg_sq)
    assert runs[True][1]["log"][-1]["total"] == runs[False][1]["log"][-1]["total"]


def test_scene_pool_feeds_the_batcher(dev):
    pool = trainloop.ScenePool(range(900, 903), 20000)
    tasks = [dict(anchors=PP.anchors(), class_id=1, matched_threshold=0.6, unmatched_threshold=0.45)]
    data = trainloop.SupervisedBatcher.from_scene_pool(pool, dev, 2, 3, PP_VG, PP.T, PP.MAX_VOXELS, tasks, PP.GRID, seed=1, augment=False)
    ex = data.load(0)
    assert bool((data.draw.tables[3][data.draw.tables[2][:, :, 3] > 0] == 1).all())   # the cars are class 1
    assert torch.equal(ex["transformation_dev"].cpu(), torch.tensor([[0.0, 1.0, 0.0, 0.0, 1.0]] * 2))
    assert int(ex["num_voxels_dev"].item()) > 0 and ex["labels"][0].shape == (2, PP.anchors().shape[0])


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals(pp_model, dev):
    model = copy.deepcopy(pp_model).to(dev).train()
    assert model.supervised is False
    with pytest.raises(ValueError, match="supervised = True"):
        strain.SupervisedTrainStep(model, total_steps=10)
    with pytest.raises(ValueError):
        strain.SupervisedTrainStep(torch.nn.Linear(2, 2), total_steps=10)
    exact, m = _pp_batch(dev, PP.FRAME_SEEDS, 84)
    padded, _ = _pp_batch(dev, PP.FRAME_SEEDS, 84, capacity=2 * m)
    step = strain.SupervisedTrainStep(_pp(pp_model, dev), total_steps=10)
    with pytest.raises(ValueError, match="num_voxels_dev"):
        step.capture(exact)
    head = step.model.bbox_head
    keep = head.loss_norm
    head.loss_norm = dict(keep, type="NormByNumExamples")      # a head the device loss does not cover
    try:
        with pytest.raises(ValueError, match="supervised_loss_covers"):
            step.capture(padded)
    finally:
        head.loss_norm = keep
    assert step.graph is None and step.global_step == 0
    step.model.reader.fused_train = False                      # the reader's torch formulation
    try:
        with pytest.raises(ValueError, match="device path"):
            step.model.forward_loss(padded)
    finally:
        del step.model.reader.fused_train
    cpu_reader = copy.deepcopy(pp_model).train().reader       # CPU tensors
    with pytest.raises(ValueError, match="device path"):
        cpu_reader(padded["voxels"].cpu(), padded["num_points"].cpu(), padded["coordinates"].cpu(), num_voxels_dev=padded["num_voxels_dev"].cpu())
    # defaults stay: forward(return_loss=True) of an unswitched model is refused by name, the neck does not take any width
    with pytest.raises(NotImplementedError, match="inference only"):
        model(exact, return_loss=True)
    assert type(model.neck).train_any_width is False


def test_check_trainable_reports_and_changes_nothing(pp_model, dev):
    model = _pp(pp_model, dev, any_width=False)
    ex, _ = _pp_batch(dev, PP.FRAME_SEEDS, 85)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    plain = strain.check_trainable(model, ex)
    model.neck.train_any_width = True
    wide = strain.check_trainable(model, ex)
    print("leave the kernels:", plain, "| with train_any_width:", wide)
    # maps 24, 12 and 6 cells wide: the convs of the second and third block are refused at wout % 8 != 0, and only they
    assert len(plain) == 12 and all(n.startswith("neck.blocks.1.") or n.startswith("neck.blocks.2.") for n in plain)
    assert wide == []
    model.reader.fused_train = False
    assert any(n.startswith("reader") for n in strain.check_trainable(model, ex))
    after = model.state_dict()
    assert model.training and all(torch.equal(before[k], after[k]) for k in before)
