"""sessd_pillar_frames / ops.pillar_frames / PillarEngine(front_end=): what can be checked without a device. Every argument check of
the entry point returns its code before any launch (null or dummy pointers, as tests/test_abi.py does for its neighbours)."""
import ctypes as C

import pytest
import torch

EINVAL, EWORKSPACE = -1, -2
B, P, T, MAXV = 2, 256, 5, 100
CAP = 1024          # >= 2 * B * P, a power of two


def call(lib, **kw):
    """The entry point with dummy non-null pointers everywhere (never dereferenced on the device: no launch happens) and host arrays
    for range / voxel size / grid, one argument changed at a time."""
    rng = (C.c_float * 6)(0, 0, 0, 8, 8, 4)
    vs = (C.c_float * 3)(1, 1, 4)
    grid = (C.c_int32 * 3)(8, 8, 1)
    a = dict(points=16, batch=B, P=P, ndim=4, rng=C.addressof(rng), vs=C.addressof(vs), grid=C.addressof(grid), T=T, maxv=MAXV, keys=16,
             vals=16, cap=CAP, weight=16, scale=16, shift=16, channels=64, dist=0, ny=8, nx=8, canvas=16, coors=16, prefix=16, nump=16,
             feat=16, err=16, ws=16, ws_bytes=0)
    a.update(kw)
    return lib.sessd_pillar_frames(a["points"], a["batch"], a["P"], a["ndim"], a["rng"], a["vs"], a["grid"], a["T"], a["maxv"], a["keys"],
                                   a["vals"], a["cap"], 0.2, 0.2, 0.1, -39.9, a["weight"], a["scale"], a["shift"], a["channels"], a["dist"],
                                   a["ny"], a["nx"], a["canvas"], a["coors"], a["prefix"], a["nump"], a["feat"], a["err"], a["ws"],
                                   a["ws_bytes"], None)


def test_every_argument_check_comes_before_any_launch():
    import sessd_hip
    lib = sessd_hip.lib
    need = lib.sessd_pillar_frames_workspace_bytes(CAP, B, P, T, MAXV)
    assert need == lib.sessd_voxelize_frames_workspace_bytes(CAP, B, P, T, MAXV) > CAP * T * 4
    assert lib.sessd_pillar_frames_workspace_bytes(CAP, 0, P, T, MAXV) == 0
    ok = dict(ws_bytes=need)
    assert call(lib, ndim=3, **ok) == EINVAL and call(lib, ndim=5, **ok) == EINVAL
    assert call(lib, channels=32, **ok) == EINVAL
    assert call(lib, batch=0, **ok) == EINVAL
    assert call(lib, cap=CAP - 24, **ok) == EINVAL                       # not a power of two
    assert call(lib, cap=CAP // 2, **ok) == EINVAL                       # a power of two below 2 * B * P
    assert call(lib, ny=0, **ok) == EINVAL and call(lib, nx=0, **ok) == EINVAL
    assert call(lib, T=0, **ok) == EINVAL and call(lib, maxv=0, **ok) == EINVAL and call(lib, P=0, cap=CAP, **ok) == EINVAL
    for required in ("points", "rng", "vs", "grid", "keys", "vals", "weight", "scale", "shift", "canvas", "coors", "prefix", "ws"):
        assert call(lib, **dict(ok, **{required: None})) == EINVAL, required
    # the workspace: one byte short, and none at all (the optional outputs may be null: the size check still comes first)
    assert call(lib, ws_bytes=need - 1) == EWORKSPACE
    assert call(lib, ws_bytes=0, nump=None, feat=None, err=None) == EWORKSPACE


def test_ops_pillar_frames_refuses_cpu_tensors():
    from sessd_hip import ops
    w, sc, sh = torch.zeros(64, 9), torch.zeros(64), torch.zeros(64)
    args = ([0.16, 0.16, 4.0], [0.0, -2.56, -3.0, 7.68, 2.56, 1.0], T, MAXV, w, sc, sh, 0.2, 0.2, 0.1, -39.9)
    with pytest.raises(ValueError, match="CUDA"):
        ops.pillar_frames([torch.zeros(10, 4)], *args)
    with pytest.raises(ValueError, match="CUDA"):
        ops.pillar_frames(torch.zeros(1, 10, 4), *args)


def test_engine_names_an_unknown_front_end():
    """check_pillar_model runs first and the device check comes later: a CPU model reaches the front_end check."""
    from det3d.models import build_detector
    from sessd_hip import PillarEngine, configs
    from sessd_hip.pillar_engine import DEFAULT_FRONT_END, FRONT_ENDS
    assert FRONT_ENDS == ("fused", "tensor") and DEFAULT_FRONT_END in FRONT_ENDS
    model = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS).eval()
    vg = dict(range=[4.0, -2.56, -3.0, 11.68, 2.56, 1.0], voxel_size=[0.16, 0.16, 4.0], max_points_in_voxel=100, max_voxel_num=2000)
    with pytest.raises(ValueError, match="front_end must be one of"):
        PillarEngine(model, vg, configs.TEST_CFG_POINTPILLARS, front_end="nonsense")
    # a known one passes that check and stops at the next: no CPU fallback
    with pytest.raises(ValueError, match="HIP device"):
        PillarEngine(model, vg, configs.TEST_CFG_POINTPILLARS, front_end="tensor")
