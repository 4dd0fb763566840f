"""The supervised multi-task head loss as the device op sessd_supervised_loss (csrc/supervised_loss.hip, three launches for all
tasks) through MultiGroupHead.loss_supervised_device / ops.SupervisedLoss:
  * against tests/golden/supervised_loss_ref.npz (the REFERENCE's mg_head.py run from source) at the golden tolerances: values 5e-4
    relative with the 1e-3 floor, gradients 1e-2 of the largest entry, same support;
  * against the float64 restatement tests/supervised_loss_ref.py (itself held to that golden by tests/test_supervised_loss_cpu.py)
    at the project's standing tolerances for a device op against a restatement: values 2e-4 relative with the 1e-3 floor,
    gradients 2e-3 of the largest entry, identical support (an entry float32 cannot hold, |w| < 1e-30, may be zero).
Inputs keep |reg_target yaw + anchor yaw - offset| >= 1e-3 (supervised_loss_ref.DIR_MARGIN), so the direction target is not a
rounding decision; the deliberate exact cases of the constants test are differences of box and target, not yaw sums."""
import copy
import os

import numpy as np
import pytest
import torch

import supervised_loss_ref as SR
from sessd_hip import configs, ops

pytestmark = pytest.mark.gpu

VAL, GRAD = 2e-4, 2e-3
FOUR_TASKS = configs.KITTI_3CLASS_TASKS + [dict(num_class=1, class_names=["Van"])]


def _head(T, dev, cfg=SR.CFG, norm="NormByNumPositives"):
    """The mirror head with T one-class tasks and the loss constants of `cfg` (the keys of sessd_supervised_loss_cfg_t)."""
    from det3d.models.builder import build_head
    h = copy.deepcopy(configs.kitti_car_model(tasks=FOUR_TASKS[:T])["bbox_head"])
    h["loss_norm"] = dict(type=norm, pos_cls_weight=cfg["pos_cls_weight"], neg_cls_weight=cfg["neg_cls_weight"])
    h["loss_cls"].update(alpha=cfg["focal_alpha"], gamma=cfg["focal_gamma"], loss_weight=cfg["cls_loss_weight"])
    h["loss_bbox"].update(sigma=cfg["smooth_l1_sigma"], loss_weight=cfg["loc_loss_weight"])
    h["loss_aux"].update(loss_weight=cfg["dir_loss_weight"])
    h["direction_offset"] = cfg["direction_offset"]
    return build_head(h).to(dev)


def _device(head, c, dev, labels_dtype=torch.int64):
    """(ret dict, grads, record clone, total) of the device op on a case, gradients through autograd."""
    example, leaves, preds = SR.example_and_preds(c, dev, labels_dtype)
    assert head.supervised_loss_covers(example, preds)
    total, rec = head.loss_supervised_device(example, preds)
    rec = rec.clone()
    total.backward()
    grads = {k: [l[k].grad.cpu().numpy() for l in leaves] for k in ("box", "cls", "dir")}
    return head.supervised_record_to_dict(rec), grads, rec, total.detach()


def _hold_against_float64(label, head, c, dev, cfg=SR.CFG, labels_dtype=torch.int64):
    ret, grads, rec, total = _device(head, c, dev, labels_dtype)
    ref = SR.reference(c, cfg)
    SR.hold(label, ret, grads, ref, VAL, GRAD)
    T = c["labels"].shape[0]
    assert SR.value_close(float(total), ref["total"], VAL) and float(rec[T, 0]) == float(total)
    assert rec[:T, ops.SUPERVISED_LOSS_RECORD["positives"]].cpu().tolist() == ref["positives"].tolist()
    assert bool(torch.isfinite(rec).all())
    return ret, grads, ref


@pytest.mark.parametrize("name", ["a", "b"])
def test_device_op_matches_the_reference_run(dev, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "supervised_loss_ref.npz"))
    c, want = SR.golden_case(g, name)
    T = c["labels"].shape[0]
    ret, grads, rec, total = _device(_head(T, dev), c, dev)
    SR.hold("device/golden " + name, ret, grads, want, 5e-4, 1e-2)
    assert SR.value_close(float(total), float(np.sum(want["loss"])), 5e-4)


@pytest.mark.parametrize("A,B,T,labels_dtype", [(1, 1, 1, torch.int64), (63, 3, 3, torch.int32), (126, 1, 4, torch.int64),
                                                (256, 3, 1, torch.int32), (257, 1, 3, torch.int64), (600, 3, 4, torch.int32)])
def test_shapes_at_the_kernel_edges(dev, A, B, T, labels_dtype):
    """One anchor, less than a wave, less than a block, exactly one block, one anchor past it, several blocks with a ragged last
    one; 1 and 3 samples; 1, 3 and 4 tasks; int32 and int64 labels."""
    c = SR.make_case(100 + A, B, T, A)
    _hold_against_float64("A=%d B=%d T=%d" % (A, B, T), _head(T, dev), c, dev, labels_dtype=labels_dtype)


def test_degenerate_samples(dev):
    """Sample 0 without a positive (the normaliser clamps to 1: box and dir gradients exactly 0, cls gradient not), sample 1 with
    every label -1 (everything of it exactly 0), sample 2 all positives. Two blocks (A = 257)."""
    A = 257
    c = SR.make_case(7, 3, 1, A, n_pos=A, n_ignore=0)
    c["labels"][0, 0] = 0
    c["labels"][0, 0, ::9] = -1
    c["labels"][0, 1] = -1
    assert (c["labels"][0, 2] == 1).all()
    ret, grads, ref = _hold_against_float64("degenerate", _head(1, dev), c, dev)
    gb, gc, gd = grads["box"][0].reshape(3, A, 7), grads["cls"][0].reshape(3, A), grads["dir"][0].reshape(3, A, 2)
    assert not gb[0].any() and not gd[0].any() and (gc[0][c["labels"][0, 0] == 0] != 0).all() and not gc[0][c["labels"][0, 0] == -1].any()
    assert not gb[1].any() and not gd[1].any() and not gc[1].any()
    assert (gb[2] != 0).all() and (gd[2] != 0).all() and (gc[2] != 0).all()
    assert int(ret["num_pos"][0]) == 0 and int(ret["num_neg"][0]) == int((c["labels"][0, 0] == 0).sum())


CONSTANTS = {
    "sigma 2, exact +-0.25 and 0": dict(smooth_l1_sigma=2.0),
    "gamma 0": dict(focal_gamma=0.0),
    "gamma 1.5, alpha 0.4": dict(focal_gamma=1.5, focal_alpha=0.4),
    "class weights 2 / 0.5": dict(pos_cls_weight=2.0, neg_cls_weight=0.5),
    "direction offset 0.3": dict(direction_offset=0.3),
    "loss weights 1.5 / 0.7 / 0.4": dict(cls_loss_weight=1.5, loc_loss_weight=0.7, dir_loss_weight=0.4),
}


@pytest.mark.parametrize("what", list(CONSTANTS))
def test_constants_away_from_the_config(dev, what):
    cfg = dict(SR.CFG, **CONSTANTS[what])
    B, T, A = 2, 2, 300
    c = SR.make_case(21, B, T, A, direction_offset=cfg["direction_offset"])
    exact = None
    if "sigma" in what:
        # on the first positives of every sample: targets on a 1/64 grid, box - target exactly +0.25, -0.25 (the transition, 1 /
        # sigma^2: the `<=` side) and 0 (gradient exactly 0) in the six linear codes; yaw equal to the target's (sin difference 0)
        exact = []
        for t in range(T):
            for b in range(B):
                idx = np.flatnonzero(c["labels"][t, b] > 0)[:3]
                for i, delta in zip(idx, (0.25, -0.25, 0.0)):
                    c["reg_targets"][t, b, i, :6] = np.round(c["reg_targets"][t, b, i, :6] * 64) / 64
                    c["box"][t, b, i, :6] = c["reg_targets"][t, b, i, :6] + np.float32(delta)
                    assert (c["box"][t, b, i, :6] - c["reg_targets"][t, b, i, :6] == np.float32(delta)).all()
                    c["box"][t, b, i, 6] = c["reg_targets"][t, b, i, 6]
                    exact.append((t, b, i, delta))
        SR.check_margin(c, cfg["direction_offset"])
    ret, grads, ref = _hold_against_float64(what, _head(T, dev, cfg), c, dev, cfg)
    if exact:
        for t, b, i, delta in exact:
            g = grads["box"][t].reshape(B, A, 7)[b, i]
            w = ref["grad_box"][t, b, i]
            assert g[6] == 0 and (g[:6] == 0).all() == (delta == 0.0) and np.array_equal(np.sign(g[:6]), np.sign(w[:6]))


def test_saturated_logits_stay_finite(dev):
    """Logits of +-80 in cls (on positives, negatives and ignored anchors) and in dir (both orders, on positives): every output is
    finite and equal to float64 within the tolerance."""
    B, T, A = 2, 1, 300
    c = SR.make_case(31, B, T, A)
    for b in range(B):
        pos, neg, ign = (np.flatnonzero(c["labels"][0, b] == v) for v in (1, 0, -1))
        c["cls"][0, b, pos[:2]] = [80.0, -80.0]
        c["cls"][0, b, neg[:4]] = [80.0, -80.0, 80.0, -80.0]
        c["cls"][0, b, ign[:2]] = [80.0, -80.0]
        c["dir"][0, b, pos[1:4]] = [[80.0, -80.0], [-80.0, 80.0], [80.0, 80.0]]
        c["dir"][0, b, neg[:2]] = [[80.0, -80.0], [-80.0, 80.0]]
    ret, grads, ref = _hold_against_float64("+-80", _head(T, dev), c, dev)
    assert all(np.isfinite(grads[k][0]).all() for k in grads)
    assert float(ret["loss"][0]) > 5   # a confident wrong answer costs its logit


def _tasks_on(c, dev, labels_dtype=torch.int64):
    T = c["labels"].shape[0]
    F = lambda k, t: torch.from_numpy(np.ascontiguousarray(c[k][t])).to(dev)
    return [dict(box=F("box", t), cls=F("cls", t), dir=F("dir", t), labels=F("labels", t).to(labels_dtype),
                 reg_targets=F("reg_targets", t), anchors=F("anchors", t)) for t in range(T)]


def _runner(B, A, T, dev, i64=True):
    return ops.SupervisedLoss(B, A, T, dev, i64, SR.CFG)


def _outputs(run):
    return [run.record] + run.g_box + run.g_cls + run.g_dir


def test_every_output_element_is_written_and_two_calls_give_the_same_bits(dev):
    B, T, A = 3, 3, 600
    c = SR.make_case(41, B, T, A, empty=((2, 0),))
    run, tasks = _runner(B, A, T, dev), _tasks_on(c, dev)
    for o in _outputs(run):
        o.fill_(float("nan"))
    rec = run.run(tasks)
    assert rec.shape == (T + 1, ops.SUPERVISED_LOSS_ROW)
    assert not any(bool(torch.isnan(o).any()) for o in _outputs(run))
    first = [o.clone() for o in _outputs(run)]
    for o in _outputs(run):
        o.fill_(float("nan"))
    run.ws.fill_(255)
    run.run(tasks)
    assert all(torch.equal(a, b) for a, b in zip(first, _outputs(run)))
    other = _runner(B, A, T, dev)
    other.run(tasks)
    assert all(torch.equal(a, b) for a, b in zip(first, _outputs(other)))


def test_autograd_scales_by_the_incoming_gradient_and_unit_grad_hands_over_the_buffers(dev):
    B, T, A = 2, 3, 300
    c = SR.make_case(51, B, T, A)
    head = _head(T, dev)
    example, leaves, preds = SR.example_and_preds(c, dev)
    total, rec = head.loss_supervised_device(example, preds)
    assert total.requires_grad and not rec.requires_grad
    (3.0 * total).backward()
    run = head._supervised_device_loss[1]
    for t, l in enumerate(leaves):
        for k, buf in (("box", run.g_box[t]), ("cls", run.g_cls[t]), ("dir", run.g_dir[t])):
            assert l[k].grad.shape == l[k].shape and torch.equal(l[k].grad, buf.view_as(l[k]) * 3.0), (t, k)
    example, leaves, preds = SR.example_and_preds(c, dev)
    total, rec = head.loss_supervised_device(example, preds, unit_grad=True)
    (3.0 * total).backward()   # unit_grad: the incoming gradient is taken to be 1, the buffers go out as they are
    for t, l in enumerate(leaves):
        for k, buf in (("box", run.g_box[t]), ("cls", run.g_cls[t]), ("dir", run.g_dir[t])):
            assert torch.equal(l[k].grad, buf.view_as(l[k])), (t, k)
    assert "iou_preds" not in preds[0]   # the supervised loss has no IoU-prediction term: no gradient goes there


def test_capture_and_replay_with_inputs_overwritten_in_place(dev):
    """The op captured once in a torch.cuda.graph, replayed twice with every input overwritten in place between the replays:
    record and gradients after each replay equal an eager call on those inputs bit for bit."""
    B, T, A = 2, 3, 600
    cases = [SR.make_case(60 + i, B, T, A, empty=(((i, 1),) if i else ())) for i in range(3)]
    run, tasks = _runner(B, A, T, dev), _tasks_on(cases[0], dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.run(tasks)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.run(tasks)
    eager = _runner(B, A, T, dev)
    for c in cases[1:]:
        fresh = _tasks_on(c, dev)
        for dst, src in zip(tasks, fresh):
            for k in dst:
                dst[k].copy_(src[k])
        for o in _outputs(run):
            o.fill_(float("nan"))
        graph.replay()
        eager.run(fresh)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_outputs(run), _outputs(eager)))
        ref = SR.reference(c)
        assert SR.value_close(float(run.record[T, 0]), ref["total"], VAL)


def test_refusals(dev):
    B, T, A = 2, 2, 100
    c = SR.make_case(71, B, T, A)
    run = _runner(B, A, T, dev)
    good = _tasks_on(c, dev)
    with pytest.raises(ValueError):
        run.run(_tasks_on(c, "cpu"))
    with pytest.raises(ValueError):
        run.run([dict(good[0], cls=good[0]["cls"].double()), good[1]])
    with pytest.raises(ValueError):
        run.run([dict(good[0], box=good[0]["box"][:, :50].contiguous()), good[1]])
    with pytest.raises(ValueError):
        run.run([dict(good[0], labels=good[0]["labels"].int()), good[1]])
    with pytest.raises(ValueError):
        run.run(good[:1])
    # a head the op does not cover: another normaliser; another anchor count per task; CPU outputs
    example, _, preds = SR.example_and_preds(c, dev)
    assert _head(T, dev).supervised_loss_covers(example, preds)
    other = _head(T, dev, norm="NormByNumExamples")
    assert not other.supervised_loss_covers(example, preds)
    with pytest.raises(ValueError):
        other.loss_supervised_device(example, preds)
    short = dict(box_preds=preds[1]["box_preds"][:, :60], cls_preds=preds[1]["cls_preds"][:, :60], dir_cls_preds=preds[1]["dir_cls_preds"][:, :60])
    assert not _head(T, dev).supervised_loss_covers(example, [preds[0], short])
    ex_cpu, _, preds_cpu = SR.example_and_preds(c, "cpu")
    assert not _head(T, dev).supervised_loss_covers(ex_cpu, preds_cpu)


# ------------------------------------------------------------------------------------------------------------------ detectors
@pytest.fixture(scope="module")
def pillars(dev):
    """The small PointPillars model of tests/test_pointpillars_detector_gpu.py (48 x 32 pillar grid, 24 x 16 head map, two clouds)
    in train mode with supervised = True, and its example with synthetic targets on the model's own anchors."""
    import test_pointpillars_detector_gpu as PP
    model = PP.build_model().to(dev).train()
    model.supervised = True
    pts = [torch.from_numpy(f).to(dev) for f in PP.frames()]
    B = len(pts)
    r = ops.voxelize_batch(pts, PP.VSIZE, PP.VRANGE, PP.T, PP.MAX_VOXELS)
    prefix = r["prefix"].cpu().numpy()
    m = int(prefix[B])
    anc = PP.anchors()
    c = SR.make_case(81, B, 1, anc.shape[0], n_pos=20, n_ignore=40, anchors=anc)
    example, _, _ = SR.example_and_preds(c, dev, torch.int32)
    example.update(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.from_numpy(np.diff(prefix)), shape=[PP.GRID])
    return model, example


def _grads_of(model, example):
    model.zero_grad(set_to_none=True)
    total, rec = model.forward_loss(example)
    total.backward()
    return float(total), rec, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_pointpillars_trains_through_the_device_loss(pillars, dev):
    model, example = pillars
    assert model.device_loss is True
    total, rec, got = _grads_of(model, example)
    assert torch.is_tensor(rec) and rec.shape == (2, ops.SUPERVISED_LOSS_ROW)
    names = [n for n, _ in model.named_parameters() if "conv_iou" not in n]
    for n in names:
        assert n in got and bool(torch.isfinite(got[n]).all()) and float(got[n].abs().max()) > 0, n
    model.device_loss = False
    try:
        total_t, ret, want = _grads_of(model, example)
    finally:
        model.device_loss = True
    assert isinstance(ret, dict) and SR.value_close(total, total_t, VAL)
    d = model.bbox_head.supervised_record_to_dict(rec)
    for k in SR.VALUE_KEYS:
        assert SR.value_close(d[k][0], ret[k][0], VAL), k
    for n in names:
        err, top = float((got[n] - want[n]).abs().max()), float(want[n].abs().max())
        print("%-40s max err %.3e of %.3e" % (n, err, top))
        assert err <= GRAD * top, (n, err, top)
    # return_loss=True gives the dict of the torch formulation
    with torch.no_grad():
        ret2 = model(example, return_loss=True)
    assert SR.value_close(ret2["loss"][0], total_t, VAL) and len(ret2["num_pos"]) == 1


def test_forward_loss_of_an_uncovered_head_gives_the_torch_values(pillars, dev):
    model, example = pillars
    head = model.bbox_head
    keep = head.loss_norm
    head.loss_norm = dict(keep, type="NormByNumExamples")
    try:
        with torch.no_grad():
            total, ret = model.forward_loss(example)
            preds = head(model.extract_feat(dict(features=example["voxels"], num_voxels=example["num_points"],
                                                 coors=example["coordinates"], batch_size=2, input_shape=example["shape"][0])))
            assert not head.supervised_loss_covers(example, preds)
            want = head.loss_supervised(example, preds)
    finally:
        head.loss_norm = keep
    assert isinstance(ret, dict) and SR.value_close(total, want["loss"][0], 1e-6)


def test_voxelnet_three_class_without_teacher_predictions(dev):
    """VoxelNet.forward(example, is_ema=[False, None], return_loss=True) on the three-class model (reduced range of
    tests/test_multitask_engine_gpu.py): the supervised dict with three entries per key, equal to the device op's record."""
    import test_multitask_engine_gpu as MT
    from sessd_hip import synth
    model = configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_rpn_model(), voxel_range=MT.VRANGE)
    pts = [torch.from_numpy(synth.make_frame(5, 20000)).to(dev)]
    r = ops.voxelize_batch(pts, MT.VSIZE, MT.VRANGE, 5, MT.MAX_VOXELS)
    m = int(r["prefix"][1].item())
    anc = configs.kitti_3class_anchors((MT.H, MT.W), MT.VRANGE)
    A = anc.shape[1]
    c = SR.make_case(91, 1, 3, A, n_pos=20, n_ignore=40)
    c["anchors"][:, 0] = anc
    c["reg_targets"][..., 6][(c["labels"] > 0) & (np.abs(c["reg_targets"][..., 6] + c["anchors"][..., 6]) < 4e-3)] += np.float32(0.05)
    SR.check_margin(c)
    example, _, _ = SR.example_and_preds(c, dev)
    example.update(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.tensor([m]), shape=[MT.GRID])
    with torch.no_grad():
        ret = model(example, is_ema=[False, None], return_loss=True)
        preds = model.forward_preds(example)
        total, rec = model.bbox_head.loss_supervised_device(example, preds)
    assert all(len(ret[k]) == 3 for k in ret) and len(ret) == 9
    d = model.bbox_head.supervised_record_to_dict(rec)
    for t in range(3):
        for k in SR.VALUE_KEYS:
            assert SR.value_close(d[k][t], ret[k][t], VAL), (t, k, float(d[k][t]), float(ret[k][t]))
        assert int(d["num_pos"][t]) == int(ret["num_pos"][t]) == 20
