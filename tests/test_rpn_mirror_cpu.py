"""The SECOND-style RPN neck of the reference's three-class config on the CPU: the det3d-mirror class, the test helper
tests/rpn_ref.py (the yardstick of the GPU tests) and the engine's plan, held to the REFERENCE's own RPN class run from source
(tests/golden/rpn_ref.npz, written by tests/golden/make_golden_rpn.py on the same seeded weights and input).

Bound: 1e-5 * max |golden| -- both sides run torch's CPU float32 kernels on the same values; what remains is the order of the
sums inside them."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import forward_cases as FC  # noqa: E402
import rpn_ref  # noqa: E402

REF_CFG = "/root/reference/examples/second/configs/kitti_all_vfev3_spmiddlefhd_rpn1_mghead_syncbn.py"
RPN_ARGS = dict(layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1], us_num_filters=[128],
                num_input_features=128, norm_cfg=None)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "rpn_ref.npz"))
    shapes = {k: ast.literal_eval(s) for k, s in zip(g["rpn_keys"].tolist(), g["rpn_shapes"].tolist())}
    wseed, iseed = [int(v) for v in g["rpn_seeds"]]
    sd = FC.seeded_state_dict(shapes, seed=wseed)
    x = FC.ssfa_input(iseed, B=2, H=16, W=12)
    # the generators have not drifted from what the reference ran on
    assert np.allclose([float(sd[k].double().sum()) for k in sorted(shapes)], g["rpn_weight_check"], rtol=1e-12, atol=1e-9)
    assert np.allclose([float(x.double().sum()), float(x.abs().max())], g["rpn_input_check"], rtol=1e-12)
    return dict(out=torch.from_numpy(g["rpn_eval"]), shapes=shapes, sd=sd, x=x)


def _mirror():
    from det3d.models.necks.rpn_v1 import RPN
    return RPN(**RPN_ARGS)


def test_mirror_state_dict_is_the_reference_layout(golden):
    shapes = {k: tuple(v.shape) for k, v in _mirror().state_dict().items()}
    assert shapes == golden["shapes"]
    assert shapes["deblocks.0.0.weight"] == (128, 128, 1, 1) and "blocks.0.16.weight" in shapes and "blocks.0.19.weight" not in shapes


def test_helper_forward_equals_the_reference(golden):
    sd = {"neck." + k: v for k, v in golden["sd"].items()}
    got = rpn_ref.rpn_forward(golden["x"], sd)
    ref = golden["out"]
    assert got.shape == ref.shape == (2, 128, 16, 12)
    err, bound = float((got - ref).abs().max()), 1e-5 * float(ref.abs().max())
    print("helper vs reference: max err %.3e (bound %.3e)" % (err, bound))
    assert err <= bound


def test_mirror_modules_equal_the_reference(golden):
    """The mirror's own modules applied by torch on the CPU (eval mode): the up-sampler must be the reference's transposed conv --
    same key, same shape as a 1x1 Conv2d weight, but y[o] = sum_i x[i] W[i][o]."""
    neck = _mirror()
    neck.load_state_dict(golden["sd"])
    neck.eval()
    with torch.no_grad():
        got = neck.deblocks[0](neck.blocks[0](golden["x"]))
    ref = golden["out"]
    err, bound = float((got - ref).abs().max()), 1e-5 * float(ref.abs().max())
    print("mirror modules vs reference: max err %.3e (bound %.3e)" % (err, bound))
    assert isinstance(neck.deblocks[0][0], torch.nn.ConvTranspose2d)
    assert err <= bound


def test_reference_three_class_config_loads_and_builds():
    if not os.path.exists(REF_CFG):
        pytest.skip("reference tree absent (GPU box)")
    from det3d.torchie import Config
    from det3d.models import build_detector
    from sessd_hip import configs
    cfg = Config.fromfile(REF_CFG)
    assert cfg.model.neck.type == "RPN" and [t["class_names"] for t in cfg.tasks] == [["Car"], ["Pedestrian"], ["Cyclist"]]
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert type(m.neck).__name__ == "RPN" and len(m.bbox_head.tasks) == 3
    # the in-repo dict config is the same model
    mine = build_detector(configs.kitti_3class_rpn_model(), train_cfg=None, test_cfg=configs.TEST_CFG)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    ref_model = dict(cfg.model)
    for part in ("reader", "backbone", "neck"):
        a, b = dict(ref_model[part]), dict(configs.kitti_3class_rpn_model()[part])
        a.pop("logger", None), b.pop("logger", None)
        assert a == b, part
    for k, v in configs.kitti_3class_rpn_model()["bbox_head"].items():
        if k != "box_coder":
            assert ref_model["bbox_head"][k] == v, k


def test_rpn_constants_chain_is_the_modules_on_constant_maps(golden):
    """sessd_hip.engine.rpn_tile_constants (float64 over the folded weights) against the neck's own conv / BatchNorm(eval) / ReLU
    modules applied to constant maps, read away from the border (in the manner of tests/test_active_rule_cpu.py; fold_bn folds
    BatchNorm in float32, hence 2e-6)."""
    from sessd_hip.engine import rpn_tile_constants
    neck = _mirror()
    neck.load_state_dict(golden["sd"])
    neck = neck.double().eval()
    chain = rpn_tile_constants(neck)
    assert len(chain) == 6 and chain[0].shape == (128,)
    blk = neck.blocks[0]
    S = 12
    c = torch.zeros(128, dtype=torch.float64)
    for k in range(6):
        x = c[None, :, None, None].expand(1, -1, S, S).contiguous()
        with torch.no_grad():
            if k == 0:
                x = blk[0](x)   # ZeroPad2d(1) in front of the unpadded first conv
            y = blk[3 + 3 * k](blk[2 + 3 * k](blk[1 + 3 * k](x)))
        c = y[0, :, S // 2, S // 2].clone()
        assert torch.allclose(chain[k], c, rtol=2e-6, atol=2e-6), k
        assert float((y[0, :, 1:-1, 1:-1] - c[:, None, None]).abs().max()) < 1e-12, k
    assert float(chain[5].abs().max()) > 0   # (not the trivial chain)


@pytest.mark.parametrize("args, limit", [
    (dict(layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[128, 128, 256], us_layer_strides=[1, 2, 4],
          us_num_filters=[256, 256, 256], num_input_features=128), "ONE block"),
    (dict(layer_nums=[5], ds_layer_strides=[2], ds_num_filters=[128], us_layer_strides=[2], us_num_filters=[128],
          num_input_features=128), "stride"),
    (dict(layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[64], us_layer_strides=[1], us_num_filters=[128],
          num_input_features=128), "128 filters"),
])
def test_plan_names_the_limit(args, limit):
    """What the engine does not lower raises a ValueError that names the limit, before anything touches the device (no GPU here)."""
    from det3d.models.necks.rpn_v1 import RPN
    from sessd_hip.engine import RpnPlan, check_rpn_neck
    neck = RPN(norm_cfg=None, **args)
    with pytest.raises(ValueError, match=limit):
        check_rpn_neck(neck)
    with pytest.raises(ValueError, match=limit):
        RpnPlan(neck, None, torch.device("cpu"))
    check_rpn_neck(_mirror())   # the three-class config's neck passes
