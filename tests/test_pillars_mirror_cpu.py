"""The PointPillars config on the CPU: the test helper tests/pillars_ref.py (the yardstick of the GPU tests) and the det3d-mirror
modules (PillarFeatureNet, PointPillarsScatter, the three-block RPN), run by torch, held to the REFERENCE's own classes run from
source (tests/golden/pillars_ref.npz, written by tests/golden/make_golden_pillars.py on the same seeded weights and inputs); the
config file itself; and the argument checks of sessd_pillar_features.

Bound: 1e-5 * max |golden| -- both sides run torch's CPU float32 kernels on the same values; what remains is the order of the
sums inside them (and, in the helper, BatchNorm folded to scale / shift)."""
import os

import numpy as np
import pytest
import torch

import pillars_ref as PR

REF_CFG = "/root/reference/examples/point_pillars/configs/original_pp_mghead_syncbn_kitti.py"
B, NY, NX = 2, 8, 12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return PR.load_golden(golden_dir)


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = float((got - ref).abs().max()), 1e-5 * float(ref.abs().max())
    print("%s vs reference: max err %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, what


@pytest.mark.parametrize("tag", ["plain", "dist"])
def test_helper_reader_equals_the_reference(golden, tag):
    g = golden[tag]
    assert g["shift_signs"].min() >= 8   # folded BatchNorm1d shifts of both signs (stored by the generator)
    sd = {"reader." + k: v for k, v in g["sd"].items()}
    got = PR.reader_forward(golden["voxels"], golden["num_points"], golden["coors"], sd, with_distance=tag == "dist")
    _close(got, g["out"], "helper reader (%s)" % tag)
    # the padding slots are not read: any value there gives the same bits
    vox = golden["voxels"].copy()
    for i, n in enumerate(golden["num_points"]):
        vox[i, n:] = np.nan
    again = PR.reader_forward(vox, golden["num_points"], golden["coors"], sd, with_distance=tag == "dist")
    assert torch.equal(again, got)


def test_helper_scatter_and_rpn_equal_the_reference(golden):
    got = PR.scatter(golden["plain"]["out"], golden["coors"], B, NY, NX)
    assert torch.equal(got, golden["scatter"])
    r = golden["rpn3"]
    sd = {"neck." + k: v for k, v in r["sd"].items()}
    out = PR.rpn_forward(r["x"], sd, PR.RPN3_ARGS["ds_layer_strides"], PR.RPN3_ARGS["us_layer_strides"])
    assert out.shape == (2, 384, 8, 12)
    _close(out, r["out"], "helper rpn_forward")


@pytest.mark.parametrize("tag", ["plain", "dist"])
def test_mirror_reader_equals_the_reference(golden, tag):
    from det3d.models.readers.pillar_encoder import PillarFeatureNet
    g = golden[tag]
    net = PillarFeatureNet(num_filters=[64], with_distance=tag == "dist", norm_cfg=None)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == g["shapes"]
    assert "pfn_layers.0.linear.weight" in g["shapes"] and "pfn_layers.0.norm.running_var" in g["shapes"]
    assert g["shapes"]["pfn_layers.0.linear.weight"] == (64, 10 if tag == "dist" else 9)
    assert (net.vx, net.vy, net.x_offset, net.y_offset) == (0.2, 0.2, 0.1, -39.9)   # the defaults, not the config's 0.16
    net.load_state_dict(g["sd"])
    net.eval()
    vox, num, coors = (torch.from_numpy(golden[k]) for k in ("voxels", "num_points", "coors"))
    with torch.no_grad():
        got = net(vox, num, coors)
        one = net(vox[:1], num[:1], coors[:1])
    _close(got, g["out"], "mirror reader (%s)" % tag)
    assert one.shape == (1, 64) and torch.equal(one, got[:1])   # (N, C) kept where the reference's squeeze() gives (C,)


def test_mirror_scatter_and_rpn_equal_the_reference(golden):
    from det3d.models.necks.rpn_v1 import RPN
    from det3d.models.readers.pillar_encoder import PointPillarsScatter
    sc = PointPillarsScatter(num_input_features=64, ds_factor=1, norm_cfg=None)
    assert not sc.state_dict()
    got = sc(golden["plain"]["out"], torch.from_numpy(golden["coors"]), B, [NX, NY, 1])
    assert torch.equal(got, golden["scatter"])
    r = golden["rpn3"]
    neck = RPN(**PR.RPN3_ARGS)
    assert {k: tuple(v.shape) for k, v in neck.state_dict().items()} == r["shapes"]
    assert r["shapes"]["deblocks.1.0.weight"] == (128, 128, 2, 2) and r["shapes"]["deblocks.2.0.weight"] == (256, 128, 4, 4)
    neck.load_state_dict(r["sd"])
    neck.eval()
    ups, x = [], r["x"]
    with torch.no_grad():
        for blk, de in zip(neck.blocks, neck.deblocks):
            x = blk(x)
            ups.append(de(x))
    _close(torch.cat(ups, 1), r["out"], "mirror RPN modules")


def test_reference_pointpillars_config_loads_and_builds():
    if not os.path.exists(REF_CFG):
        pytest.skip("reference tree absent (GPU box)")
    from det3d.torchie import Config
    from det3d.models import build_detector
    from sessd_hip import configs
    cfg = Config.fromfile(REF_CFG)
    assert cfg.model.type == "PointPillars" and cfg.model.reader.type == "PillarFeatureNet" and cfg.model.neck.type == "RPN"
    assert cfg.assigner.out_size_factor == 2
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert [type(x).__name__ for x in (m, m.reader, m.backbone, m.neck)] == ["PointPillars", "PillarFeatureNet", "PointPillarsScatter", "RPN"]
    assert len(m.bbox_head.tasks) == 1 and m.bbox_head.tasks[0].conv_box.in_channels == 384
    mine_cfg = configs.kitti_pointpillars_model()
    mine = build_detector(mine_cfg, train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    ref_model = dict(cfg.model)
    assert ref_model["type"] == mine_cfg["type"] and ref_model["pretrained"] == mine_cfg["pretrained"]
    for part in ("reader", "backbone", "neck"):
        a, b = dict(ref_model[part]), dict(mine_cfg[part])
        a.pop("logger", None), b.pop("logger", None)
        assert a == b, part
    for k, v in mine_cfg["bbox_head"].items():
        if k != "box_coder":
            assert ref_model["bbox_head"][k] == v, k
    assert set(ref_model["bbox_head"]) == set(mine_cfg["bbox_head"])
    assert dict(cfg.test_cfg) == configs.TEST_CFG_POINTPILLARS and dict(cfg.voxel_generator) == configs.VOXEL_GENERATOR_POINTPILLARS


def test_downsample_factor_of_the_pointpillars_model():
    from det3d.utils.config_tool import get_downsample_factor
    from sessd_hip import configs
    assert get_downsample_factor(configs.kitti_pointpillars_model()) == 2


def test_pillar_entry_point_rejects_bad_arguments_before_touching_the_device():
    """Null or dummy pointers, no GPU: every call must fail (SESSD_EINVAL = -1) before a launch."""
    import sessd_hip
    lib = sessd_hip.lib
    p = 16   # non-null, never dereferenced

    def call(voxels=p, num=p, coors=p, n=4, T=8, ndim=4, w=p, s=p, t=p, C=64, batch=2, ny=8, nx=12, feat=p, canvas=p):
        return lib.sessd_pillar_features(voxels, num, coors, None, n, T, ndim, 0.2, 0.2, 0.1, -39.9, w, s, t, C, 0, batch, ny, nx,
                                         feat, canvas, None, None)

    assert call(ndim=3) == -1 and call(ndim=5) == -1
    assert call(C=32) == -1 and call(C=128) == -1 and call(C=0) == -1      # the kernel covers 64 channels
    assert call(T=0) == -1 and call(n=-1) == -1
    assert call(feat=None, canvas=None) == -1
    assert call(batch=0) == -1 and call(ny=0) == -1 and call(nx=-3) == -1
    assert call(num=None) == -1 and call(coors=None) == -1 and call(w=None) == -1 and call(s=None) == -1 and call(t=None) == -1
    assert call(voxels=None, feat=None) == -1 and call(voxels=None, canvas=None) == -1   # scatter alone needs both
    assert call(n=0) == 0   # no pillars: nothing is launched


def test_pillar_ops_refuse_cpu_tensors():
    from sessd_hip import ops
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.pillar_features(z(2, 8, 4), z(2, dtype=torch.int32), z(2, 4, dtype=torch.int32), z(64, 9), z(64), z(64), 0.2, 0.2, 0.1, -39.9)
    with pytest.raises(ValueError):
        ops.pillar_scatter(z(2, 64), z(2, 4, dtype=torch.int32), 1, 8, 12)


def test_detector_is_inference_only_and_two_layer_reader_runs(golden):
    """return_loss=True is refused by name (training of this config is not supported); a reader with two PFN layers, which only
    the torch formulation covers, gives (N, C) with the first layer's half-width concatenation inside."""
    from det3d.models import build_detector
    from det3d.models.readers.pillar_encoder import PillarFeatureNet
    from sessd_hip import configs
    m = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(dict(voxels=None, num_points=None, coordinates=None, num_voxels=[0], shape=[[12, 8, 1]]))
    net = PillarFeatureNet(num_filters=[32, 64], norm_cfg=None).eval()
    assert [tuple(l.linear.weight.shape) for l in net.pfn_layers] == [(16, 9), (64, 32)]
    vox, num, coors = (torch.from_numpy(golden[k]) for k in ("voxels", "num_points", "coors"))
    with torch.no_grad():
        out = net(vox, num, coors)
    assert out.shape == (vox.shape[0], 64) and bool(torch.isfinite(out).all())
