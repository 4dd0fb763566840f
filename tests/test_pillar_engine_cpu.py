"""sessd_hip.check_pillar_model: the limits of PillarEngine, checked on CPU modules (no device is touched). The reference's
PointPillars config passes; each departure raises a ValueError whose text names the limit."""
import copy

import pytest

from sessd_hip import check_pillar_model, configs


def build(edit=None, train=False):
    from det3d.models import build_detector
    cfg = configs.kitti_pointpillars_model()
    if edit is not None:
        edit(cfg)
    model = build_detector(cfg, train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    return model.train() if train else model.eval()


def test_the_reference_config_passes():
    parts = check_pillar_model(build())
    assert [len(b) for b in parts["blocks"]] == [4, 6, 6]                    # 1 + layer_nums
    assert [(u[0].in_channels, u[0].out_channels, u[2]) for u in parts["ups"]] == [(64, 128, 1), (128, 128, 2), (256, 128, 4)]
    assert parts["head"].conv_box.in_channels == 384
    # the full-size canvas (496 x 432) and the small one of the GPU tests (32 x 48): one head-map size
    check_pillar_model(build(), (496, 432))
    check_pillar_model(build(), (32, 48))


def _two_pfn(c):
    c["reader"]["num_filters"] = [32, 64]


def _dist32(c):
    c["reader"].update(with_distance=True, num_filters=[32])


def _stride8(c):
    c["neck"]["us_layer_strides"] = [1, 2, 8]


def _short_us(c):
    c["neck"].update(us_layer_strides=[2, 4], us_num_filters=[128, 128])
    c["bbox_head"]["in_channels"] = 256


def _two_tasks(c):
    tasks = [dict(t) for t in configs.KITTI_3CLASS_TASKS[:2]]
    c["bbox_head"].update(tasks=tasks, weights=[1, 1])


@pytest.mark.parametrize("edit, names", [
    (_two_pfn, "ONE PFN layer"),
    (_dist32, "64 filters"),
    (_stride8, r"stride must be an integer in \(1, 2, 4\)"),
    (_short_us, "start at block 0"),
    (_two_tasks, "ONE task"),
], ids=["two_pfn_layers", "with_distance_32_filters", "upsampler_stride_8", "short_us_layer_strides", "two_task_head"])
def test_each_limit_is_named(edit, names):
    with pytest.raises(ValueError, match=names):
        check_pillar_model(build(edit))


def test_train_mode_is_refused():
    with pytest.raises(ValueError, match="eval mode"):
        check_pillar_model(build(train=True))


def test_upsampler_outputs_must_share_one_size():
    model = build()
    with pytest.raises(ValueError, match="share one spatial size"):
        check_pillar_model(copy.deepcopy(model), (30, 48))   # 30 -> 15 -> 8 -> 4: 15, 16, 16 rows
