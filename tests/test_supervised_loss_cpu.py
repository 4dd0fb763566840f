"""The plain supervised multi-task head loss (mg_head.py:559-652) without a GPU: the mirror head's torch formulation
MultiGroupHead.loss_supervised on CPU tensors and the float64 restatement tests/supervised_loss_ref.py, both against
tests/golden/supervised_loss_ref.npz = the REFERENCE's own mg_head.py / losses.py run from source
(tests/golden/make_golden_supervised_loss.py). Values 5e-4 relative with the 1e-3 floor, gradients of sum(loss) 1e-2 of the largest
entry with the same support -- the tolerances tests/test_head_loss_gpu.py uses against its golden. And the detectors' loss entry:
PointPillars stays inference-only by default, VoxelNet without teacher predictions returns the supervised dict."""
import os

import numpy as np
import pytest
import torch

import supervised_loss_ref as SR
from sessd_hip import configs

KEYS = ("loss", "cls_pos_loss", "cls_neg_loss", "dir_loss_reduced", "cls_loss_reduced", "loc_loss_reduced", "loc_loss_elem", "num_pos",
        "num_neg")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "supervised_loss_ref.npz"))


def _head(tasks):
    from det3d.models import build_detector
    return build_detector(configs.kitti_car_model(tasks=tasks), train_cfg=None, test_cfg=configs.TEST_CFG).bbox_head


@pytest.mark.parametrize("name", ["a", "b"])
def test_mirror_loss_supervised_on_cpu_matches_the_reference_run(golden, name):
    c, want = SR.golden_case(golden, name)
    T = c["labels"].shape[0]
    if name == "a":   # the cases the golden was built for
        assert c["labels"].shape == (3, 2, 600) and int((c["labels"][1, 1] > 0).sum()) == 0 and int((c["labels"][0, 0] == -1).sum()) == 30
    else:
        assert c["labels"].shape == (1, 3, 257)
    head = _head(configs.KITTI_3CLASS_TASKS[:T])
    example, leaves, preds = SR.example_and_preds(c, "cpu")
    ret = head.loss_supervised(example, preds)
    assert sorted(ret) == sorted(KEYS) and all(len(ret[k]) == T for k in KEYS)
    sum(ret["loss"]).backward()
    SR.hold("mirror/cpu " + name, ret, {k: [l[k].grad for l in leaves] for k in ("box", "cls", "dir")}, want, 5e-4, 1e-2)
    assert not head.supervised_loss_covers(example, preds)   # CPU tensors: the device op does not cover them


@pytest.mark.parametrize("name", ["a", "b"])
def test_float64_restatement_matches_the_reference_run(golden, name):
    c, want = SR.golden_case(golden, name)
    ref = SR.reference(c)
    SR.hold("float64 " + name, ref, {k: ref["grad_" + k] for k in ("box", "cls", "dir")}, want, 5e-4, 1e-2)
    assert abs(ref["total"] - float(np.sum(want["loss"]))) <= 5e-4 * float(np.sum(want["loss"]))
    assert ref["positives"].tolist() == (c["labels"] > 0).reshape(len(want["loss"]), -1).sum(1).tolist()


def test_mirror_loss_supervised_other_norms_and_int32_labels(golden):
    """What the device op refuses still runs here: NormByNumExamples changes the classification term only, by the ratio of the
    normalisers when every sample has the same counts; int32 labels give the int64 result."""
    c, want = SR.golden_case(golden, "b")
    head = _head(configs.KITTI_3CLASS_TASKS[:1])
    example, _, preds = SR.example_and_preds(c, "cpu")
    base = head.loss_supervised(example, preds)
    ex32, _, preds32 = SR.example_and_preds(c, "cpu", torch.int32)
    r32 = head.loss_supervised(ex32, preds32)
    assert float(r32["loss"][0].detach()) == float(base["loss"][0].detach())
    head.loss_norm = dict(head.loss_norm, type="NormByNumExamples")
    other = head.loss_supervised(example, preds)
    npos, ncared = (c["labels"][0] > 0).sum(1), (c["labels"][0] >= 0).sum(1)
    assert len(set(npos.tolist())) == 1 and len(set(ncared.tolist())) == 1
    assert SR.value_close(other["cls_loss_reduced"][0], float(base["cls_loss_reduced"][0]) * npos[0] / ncared[0], 1e-5)
    assert SR.value_close(other["loc_loss_reduced"][0], base["loc_loss_reduced"][0], 1e-6)


def test_pointpillars_default_stays_inference_only_and_opt_in_returns_the_dict():
    from det3d.models import build_detector
    m = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    assert m.supervised is False
    example = dict(voxels=None, num_points=None, coordinates=None, num_voxels=[0], shape=[[12, 8, 1]])
    with pytest.raises(NotImplementedError, match="inference only"):
        m(example)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.forward_loss(example)
    # opt-in, on the CPU (the torch formulation of every stage): a 16 x 8 canvas, two samples
    m.supervised = True
    m.train()
    rng = np.random.RandomState(0)
    B, nx, ny, n = 2, 16, 8, 20
    cells = rng.permutation(B * nx * ny)[:n]
    coors = np.stack([cells // (nx * ny), np.zeros(n, np.int64), (cells % (nx * ny)) // nx, cells % nx], 1).astype(np.int32)
    coors = coors[np.argsort(coors[:, 0], kind="stable")]
    vox = rng.normal(0, 1, (n, 6, 4)).astype(np.float32)
    H, W = ny // 2, nx // 2
    A = H * W * 2
    c = SR.make_case(3, B, 1, A, n_pos=3, n_ignore=4)
    ex, _, _ = SR.example_and_preds(c, "cpu")
    ex.update(voxels=torch.from_numpy(vox), num_points=torch.full((n,), 6, dtype=torch.int32), coordinates=torch.from_numpy(coors),
              num_voxels=torch.tensor([int((coors[:, 0] == b).sum()) for b in range(B)]), shape=[[nx, ny, 1]])
    ret = m(ex, return_loss=True)
    assert sorted(ret) == sorted(KEYS) and all(len(ret[k]) == 1 for k in KEYS)
    total, d = m.forward_loss(ex)
    assert isinstance(d, dict) and torch.isfinite(total) and float(total.detach()) > 0
    total.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n_, p in m.named_parameters() if "conv_iou" not in n_)


def test_voxelnet_without_teacher_predictions_returns_the_supervised_dict():
    """VoxelNet.forward(example, is_ema=[False, None], return_loss=True), the reference's non-mean-teacher trainer call, on the
    three-class model. The voxel reader and the sparse middle have no CPU formulation (ops.vfe_mean refuses CPU tensors), so here
    the pass up to the neck is replaced by a fixed BEV map and the real three-task head and loss run on it; the whole detector on
    a tiny grid is in tests/test_supervised_loss_gpu.py."""
    from det3d.models import build_detector
    m = build_detector(configs.kitti_3class_rpn_model(), train_cfg=None, test_cfg=configs.TEST_CFG).train()
    B, H, W = 2, 4, 4
    torch.manual_seed(0)
    bev = torch.randn(B, 128, H, W)
    m.extract_feat = lambda data: bev
    c = SR.make_case(4, B, 3, H * W * 2, n_pos=3, n_ignore=4)
    ex, _, _ = SR.example_and_preds(c, "cpu")
    ex.update(voxels=None, coordinates=None, num_points=None, num_voxels=[0] * B, shape=[[32, 32, 40]])
    ret = m(ex, is_ema=[False, None], return_loss=True)
    assert sorted(ret) == sorted(KEYS) and all(len(ret[k]) == 3 for k in KEYS)
    assert all(torch.isfinite(v) for v in ret["loss"]) and [int(v) for v in ret["num_pos"]] == [3, 3, 3]
    sum(ret["loss"]).backward()
    assert all(float(t.conv_box.weight.grad.abs().max()) > 0 for t in m.bbox_head.tasks)
