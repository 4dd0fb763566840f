"""sessd_assign_targets_batch without a GPU: the per-task CPU wrapper (tests/assign_multi_ref.py) against the reference's own
create_target_np run from source (tests/golden/assign_multi_ref.npz); the ctypes mirrors against the header's layout; the
argument checks, which come before any device call (dummy pointers; SESSD_EINVAL = -1, SESSD_EWORKSPACE = -2, the workspace
query returns 0 for what it refuses); and the AssignTarget stage's construction from the multi-task configs."""
import ctypes as C
import os

import numpy as np
import pytest

import sessd_hip
from sessd_hip._lib import AssignBatchCfg, AssignTask

import assign_multi_ref as amr

lib = sessd_hip.lib
REF = "/root/reference"
REF_3CLASS = os.path.join(REF, "examples/second/configs/kitti_all_vfev3_spmiddlefhd_rpn1_mghead_syncbn.py")
REF_PP = os.path.join(REF, "examples/point_pillars/configs/original_pp_mghead_syncbn_kitti.py")


@pytest.mark.parametrize("key", ["c3", "pp"])
def test_wrapper_equals_the_reference_run(golden_dir, key):
    G = amr.Golden(golden_dir, key)
    assert G.A == {"c3": 3520, "pp": 2146}[key] and len(G.tasks) == {"c3": 3, "pp": 1}[key]
    for f in amr.FRAMES:
        gt, cls = G.frame(f)
        for t, r in enumerate(amr.assign_tasks(G.tasks, gt, cls)):
            G.check(f, t, r["labels"], r["reg_targets"], r["reg_weights"], r["gt_id"])
            assert set(np.unique(r["labels"])) <= {-1, 0, 1}


def test_golden_frames_hold_the_cases_they_are_there_for(golden_dir):
    G = amr.Golden(golden_dir, "c3")
    names = [str(n) for n in G.g["names"]]
    cls = {f: G.frame(f)[1] for f in amr.FRAMES}
    assert set(cls["a"]) == {1, 2, 3} and 2 not in cls["b"] and len(cls["c"]) == 0 and names.index("Van") + 1 in cls["d"]
    assert len(cls["h"]) == 30 and np.all(G.frame("e")[0][3:, 0] == 150.0)
    yaw = G.frame("f")[0][:, 6]
    assert np.all(np.abs(yaw - np.pi / 4) < 1e-3) and (yaw < np.float32(np.pi / 4)).any() and (yaw > np.float32(np.pi / 4)).any()
    g = G.frame("g")[0]
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[2], g[3])
    for t in range(3):   # the far box forces nothing; of two identical boxes only the first is ever assigned
        assert set(G.want("e", t)["gt_id"]) == {0} and 1 not in set(G.want("g", t)["gt_id"])
        assert np.all(G.want("c", t)["labels"] == 0) and len(G.want("c", t)["pos"]) == 0
    assert np.all(G.want("b", 1)["labels"] == 0)


def _cfg(**kw):
    v = dict(batch=2, num_anchors=600, num_tasks=3, gt_capacity=128, labels_i64=0, anchors_per_frame=0)
    v.update(kw)
    return AssignBatchCfg(**v)


def _tasks(n, **null):
    arr = (AssignTask * 4)()
    for t in range(n):
        for name in ("anchors", "labels", "reg_targets", "reg_weights", "gt_id"):
            setattr(arr[t], name, 256)   # non-null, never dereferenced: the call must fail first
        arr[t].class_id, arr[t].matched, arr[t].unmatched = t + 1, 0.6, 0.45
    for name, t in null.items():
        setattr(arr[t], name, None)
    return arr


def test_struct_mirrors_have_the_header_layout():
    assert [n for n, _ in AssignBatchCfg._fields_] == ["batch", "num_anchors", "num_tasks", "gt_capacity", "labels_i64", "anchors_per_frame"]
    assert C.sizeof(AssignBatchCfg) == 6 * 4
    assert [n for n, _ in AssignTask._fields_] == ["anchors", "class_id", "matched", "unmatched", "labels", "reg_targets", "reg_weights",
                                                   "gt_id"]
    # LP64: pointer, three 4-byte fields padded to the next pointer, four pointers
    assert C.sizeof(AssignTask) == 8 + 16 + 4 * 8
    assert [getattr(AssignTask, n).offset for n, _ in AssignTask._fields_] == [0, 8, 12, 16, 24, 32, 40, 48]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sessd_hip_types.h")).read()
    body = hdr[hdr.index("const float* anchors;      /* (A, 7), or (B, A, 7)"):hdr.index("} sessd_assign_task_t;")]
    order = [body.index(k) for k in ("anchors;", "class_id;", "matched, unmatched;", "labels;", "reg_targets;", "reg_weights;", "gt_id;")]
    assert order == sorted(order)
    assert "int32_t batch, num_anchors, num_tasks, gt_capacity;" in hdr and hdr.index("labels_i64;        /* labels are int64") < hdr.index(
        "anchors_per_frame; /* 0: every task's anchors")


def test_workspace_query_refuses_what_the_kernels_do_not_cover():
    wb = lambda c: lib.sessd_assign_targets_batch_workspace_bytes(C.addressof(c) if c is not None else None)
    assert wb(None) == 0
    assert wb(_cfg(batch=0)) == 0 and wb(_cfg(num_anchors=0)) == 0
    assert wb(_cfg(num_tasks=0)) == 0 and wb(_cfg(num_tasks=5)) == 0
    assert wb(_cfg(gt_capacity=0)) == 0 and wb(_cfg(gt_capacity=129)) == 0
    assert wb(_cfg(batch=1 << 15, num_anchors=1 << 15)) == 0     # past 32-bit element offsets
    al = lambda n: (n + 255) // 256 * 256
    assert wb(_cfg()) == al(6 * 128 * 4) + 2 * al(6 * 600 * 4)   # maxima per ground truth, maximum and argmax per anchor
    for T in (1, 2, 3, 4):
        for G in (1, 15, 128):
            assert wb(_cfg(num_tasks=T, gt_capacity=G)) > 0
    assert 0 < wb(_cfg(batch=4, num_tasks=1, num_anchors=107136)) < 8 << 20


def test_entry_refuses_bad_arguments_before_any_device_call():
    ws, gt = 4096, 512   # dummy non-null addresses; ws is 256-byte aligned
    call = lambda c, tasks, boxes=gt, workspace=ws, nbytes=1 << 24: lib.sessd_assign_targets_batch(
        C.addressof(c) if c is not None else None, C.addressof(tasks) if tasks is not None else None, boxes, None, None, workspace,
        nbytes, None)
    good = _tasks(3)
    assert call(None, good) == -1 and call(_cfg(), None) == -1
    assert call(_cfg(batch=0), good) == -1 and call(_cfg(num_anchors=0), good) == -1
    assert call(_cfg(num_tasks=0), good) == -1 and call(_cfg(num_tasks=5), good) == -1
    assert call(_cfg(gt_capacity=0), good) == -1 and call(_cfg(gt_capacity=129), good) == -1
    assert call(_cfg(), good, boxes=None) == -1 and call(_cfg(), good, workspace=None) == -1
    for name in ("anchors", "labels", "reg_targets"):   # a null pointer in any task, also the last one
        assert call(_cfg(), _tasks(3, **{name: 2})) == -1, name
        assert call(_cfg(), _tasks(3, **{name: 0})) == -1, name
    c0 = _cfg()
    need = lib.sessd_assign_targets_batch_workspace_bytes(C.addressof(c0))
    assert need > 0 and call(_cfg(), good, nbytes=need - 1) == -2 and call(_cfg(), good, nbytes=0) == -2
    assert call(_cfg(), good, workspace=4100) == -1   # not 256-byte aligned
    # optional outputs may be null, and a task past num_tasks is not looked at: every check up to the workspace passes
    assert call(_cfg(), _tasks(3, reg_weights=1, gt_id=2), nbytes=0) == -2
    assert call(_cfg(num_tasks=2), _tasks(3, anchors=2), nbytes=0) == -2


def test_ops_wrapper_refuses_by_value_error_naming_the_limit():
    import torch
    from sessd_hip import ops
    a = torch.zeros(600, 7)
    task = lambda anchors=a: dict(anchors=anchors, class_id=1, matched_threshold=0.6, unmatched_threshold=0.45)
    cuda = torch.device("cuda:0")
    with pytest.raises(ValueError, match="1 to 4 tasks"):
        ops.AssignTargets(2, 600, [task()] * 5, cuda)
    with pytest.raises(ValueError, match="1 to 4 tasks"):
        ops.AssignTargets(2, 600, [], cuda)
    with pytest.raises(ValueError, match="1 to 128 ground-truth rows"):
        ops.AssignTargets(2, 600, [task()], cuda, gt_capacity=129)
    with pytest.raises(ValueError, match="1 to 128 ground-truth rows"):
        ops.AssignTargets(2, 600, [task()], cuda, gt_capacity=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.AssignTargets(2, 600, [task()], torch.device("cpu"))
    with pytest.raises(ValueError, match="anchors must be a float32 device tensor"):
        ops.AssignTargets(2, 600, [task()], cuda)   # CPU anchors
    assert ops.ASSIGN_MAX_TASKS == 4 and ops.ASSIGN_MAX_GT == 128


def _reference_assigner(path):
    from det3d.torchie import Config
    return Config.fromfile(path).train_cfg["assigner"]


def test_stage_constructs_from_the_multi_task_configs():
    from det3d.datasets.pipelines import AssignTarget
    from sessd_hip import configs
    cases = [(configs.ASSIGNER_3CLASS, 3, 70400), (configs.ASSIGNER_POINTPILLARS, 1, 248 * 216 * 2)]
    if os.path.isdir(REF):
        # the reference's PointPillars assigner has no feature_map_size: its stage's literal [1, 200, 176] applies
        cases += [(_reference_assigner(REF_3CLASS), 3, 70400), (_reference_assigner(REF_PP), 1, 70400)]
    for cfg, T, A in cases:
        stage = AssignTarget(cfg=cfg)
        anchors = stage.anchors_by_task if stage.multi else [stage.anchors]
        assert len(anchors) == T and all(a.shape == (A, 7) and a.dtype == np.float32 for a in anchors)
        val = stage(dict(mode="val", lidar=dict()), None)[0]   # no annotations: anchors only, no device call
        assert list(val["lidar"]["targets"].keys()) == ["anchors"] and len(val["lidar"]["targets"]["anchors"]) == T
    s3 = AssignTarget(cfg=configs.ASSIGNER_3CLASS)
    assert s3.target_class_names == ["Car", "Pedestrian", "Cyclist"] and s3.thresholds == [(0.6, 0.45), (0.4, 0.2), (0.4, 0.2)]
    assert np.array_equal(np.stack(s3.anchors_by_task), configs.kitti_3class_anchors())
    assert AssignTarget(cfg=configs.ASSIGNER_POINTPILLARS).feature_map_size == [1, 248, 216]


def test_config_dicts_equal_the_reference_config_files():
    from sessd_hip import configs
    assert configs.ASSIGNER_POINTPILLARS["feature_map_size"] == [1, 248, 216] and "feature_map_size" not in configs.ASSIGNER_3CLASS
    pairs = ((configs.ASSIGNER_3CLASS, REF_3CLASS), (configs.ASSIGNER_POINTPILLARS, REF_PP))
    for mine, path in pairs if os.path.isdir(REF) else ():   # the config files exist where the reference tree does
        ref = _reference_assigner(path)
        gm, gr = mine["target_assigner"]["anchor_generators"], ref["target_assigner"]["anchor_generators"]
        assert len(gm) == len(gr)
        for a, b in zip(gm, gr):
            for k in ("sizes", "anchor_ranges", "rotations", "matched_threshold", "unmatched_threshold", "class_name"):
                assert a[k] == b[k] or list(a[k]) == list(b[k]), k
        assert [list(t["class_names"]) for t in mine["target_assigner"]["tasks"]] == [list(t["class_names"]) for t in ref["target_assigner"]["tasks"]]
        assert mine["out_size_factor"] == ref["out_size_factor"]


def test_stage_refuses_two_generators_in_one_task():
    from det3d.datasets.pipelines import AssignTarget
    from sessd_hip import configs
    ta = dict(configs.ASSIGNER_3CLASS["target_assigner"])
    ta["anchor_generators"] = ta["anchor_generators"][:2]
    ta["tasks"] = [dict(num_class=2, class_names=["Car", "Pedestrian"])]
    with pytest.raises(ValueError, match="one anchor generator per task"):
        AssignTarget(cfg=dict(configs.ASSIGNER_3CLASS, target_assigner=ta))
