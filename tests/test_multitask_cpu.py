"""Multi-task heads without a GPU: the three-class config builds, its parameters carry the reference's names, the (T * 22, C)
packing is task-major, and the limits of the inference path raise ValueError."""
import pytest
import torch
import torch.nn.functional as F

from det3d.models import build_detector
from sessd_hip import configs, ops
from sessd_hip.engine import pack_task_heads


@pytest.fixture(scope="module")
def model():
    m = build_detector(configs.kitti_3class_model(), train_cfg=None, test_cfg=configs.TEST_CFG)
    return m.eval()


def test_three_class_config_builds_with_the_reference_key_names(model):
    assert len(model.bbox_head.tasks) == 3 and model.bbox_head.num_classes == [1, 1, 1]
    assert model.bbox_head.class_names == [["Car"], ["Pedestrian"], ["Cyclist"]]
    keys = set(model.state_dict())
    for t in range(3):
        for conv, cout in (("conv_box", 14), ("conv_cls", 2), ("conv_dir", 4), ("conv_iou", 2)):
            for p in ("weight", "bias"):
                k = "bbox_head.tasks.%d.%s.%s" % (t, conv, p)
                assert k in keys and model.state_dict()[k].shape[0] == cout, k
    assert not any(k.startswith("bbox_head.tasks.3.") for k in keys)
    # the single-task config is what it was
    car = build_detector(configs.kitti_car_model(), train_cfg=None, test_cfg=configs.TEST_CFG)
    assert len(car.bbox_head.tasks) == 1


def test_anchor_sets_per_task():
    a = configs.kitti_3class_anchors((4, 6))
    assert a.shape == (3, 4 * 6 * 2, 7)
    for t, spec in enumerate(configs.KITTI_3CLASS_ANCHORS):
        assert torch.allclose(torch.from_numpy(a[t, :, 3:6]), torch.tensor(spec["sizes"]).expand(48, 3))
        assert (a[t, :, 2] == spec["z"]).all() and set(a[t, :, 6].tolist()) == {0.0, float(torch.tensor(1.57))}
    assert (a[0, :, :2] == a[1, :, :2]).all()   # the same grid of centres for every task
    from sessd_hip.anchors import create_anchors_3d_range
    assert (a[0] == create_anchors_3d_range((1, 4, 6)).reshape(-1, 7)).all()   # task 0 = the car anchors of the single-task engine


def test_packed_head_weights_are_task_major(model):
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in model.bbox_head.tasks.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    w, b = pack_task_heads(model.bbox_head.tasks)
    assert w.shape == (66, 128, 1, 1) and b.shape == (66,)
    x = torch.randn(2, 128, 3, 5, generator=g)
    got = F.conv2d(x, w, b).view(2, 3, 22, 3, 5)
    for t, h in enumerate(model.bbox_head.tasks):
        with torch.no_grad():
            ref = torch.cat([h.conv_box(x), h.conv_cls(x), h.conv_dir(x), h.conv_iou(x)], 1)
        assert torch.equal(got[:, t], ref), t
    w1, b1 = pack_task_heads(model.bbox_head.tasks[1])   # one Head module: the single-task packing
    assert torch.equal(w1, w[22:44]) and torch.equal(b1, b[22:44])


def _model_with_tasks(tasks):
    return build_detector(configs.kitti_car_model(tasks=tasks), train_cfg=None, test_cfg=configs.TEST_CFG).eval()


def test_limits_raise_value_errors_that_name_them():
    five = _model_with_tasks([dict(num_class=1, class_names=["c%d" % i]) for i in range(5)])
    with pytest.raises(ValueError, match="1 to 4 tasks"):
        pack_task_heads(five.bbox_head.tasks)
    two_class = _model_with_tasks([dict(num_class=1, class_names=["Car"]), dict(num_class=2, class_names=["Pedestrian", "Cyclist"])])
    with pytest.raises(ValueError, match="one class per task"):
        pack_task_heads(two_class.bbox_head.tasks)
    # the mirror's predict checks before it touches a device
    x = torch.zeros(1, 128, 2, 2)
    anchors = [torch.zeros(1, 8, 7)] * 5
    with torch.no_grad():
        with pytest.raises(ValueError, match="1 to 4 tasks"):
            five.bbox_head.predict(dict(anchors=anchors), [dict()] * 5, configs.TEST_CFG)
        with pytest.raises(ValueError, match="one class per task"):
            two_class.bbox_head.predict(dict(anchors=anchors[:2]), [dict()] * 2, configs.TEST_CFG)
    with pytest.raises(ValueError, match="1 to 4 tasks"):
        ops.check_num_tasks(0)


def test_c_entry_points_reject_task_counts_before_touching_the_device():
    from sessd_hip._lib import PredictArgs
    lib = ops.lib
    for nt in (0, 5):
        assert lib.sessd_ssfa_fuse_head_tasks(None, None, None, None, 1.0, 0.0, 1.0, 0.0, 1, 128, 64, None, None, None, nt, None, 0.0,
                                              None, 0, None, None) == -1
        args = PredictArgs(batch=1, num_tasks=nt, num_pixels=64, score_thresh=0.3, pre_max_size=100, post_max_size=10, nms_iou_thresh=0.01)
        assert lib.sessd_predict(args, None, 0, None) == -1
        assert lib.sessd_predict_workspace_bytes(1, nt, 128, 100, 10, 0) == 0
    # one task: the workspace of before (64000 bytes: what the single-task query returned for these arguments while it was a
    # function of its own); more tasks: per (frame, task) plus the rows the merge reads
    one = 64000
    assert lib.sessd_predict_workspace_bytes(2, 1, 128, 100, 10, 0) == one
    assert lib.sessd_predict_workspace_bytes(2, 3, 128, 100, 10, 0) > lib.sessd_predict_workspace_bytes(6, 1, 128, 100, 10, 0)
