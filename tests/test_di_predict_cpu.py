"""DI-NMS inside predict, the parts that need no GPU: tests/di_predict_ref.py (the CPU reference of the GPU tests) against the
reference's own wrappers (tests/golden/di_predict_ref.npz, make_golden_di_predict.py), the argument checks of ops.predict /
InferenceEngine / the C entry points (before any device call), and the configuration."""
import ctypes
import os

import numpy as np
import pytest
import torch

import di_predict_ref as R


def test_di_predict_ref_reproduces_reference_wrappers(golden_dir):
    """rotate_weighted_nms with the literal arguments of get_task_detections on seeded candidate sets: keep lists equal, boxes
    2e-4, scores 1e-5, directions equal (the tolerances of tests/test_di_nms_gpu.py)."""
    import sys
    sys.path.insert(0, golden_dir)
    from make_golden_di_predict import CASES
    g = np.load(os.path.join(golden_dir, "di_predict_ref.npz"))
    kept, unkept = [], []
    for ci, case in enumerate(CASES):
        box, anchors, scores, ioup, dirs = [g["c%d_in_%s" % (ci, k)] for k in ("box", "anchors", "scores", "iou_preds", "dirs")]
        assert len(scores) == case["n"] and len(np.unique(scores)) == len(scores)
        order = np.argsort(-scores.astype(np.float64), kind="stable")[:case["pre"]]   # the reference's topk (distinct scores)
        c = dict(box=box[order], score=scores[order], iou_pred=ioup[order], dir=dirs[order], anchor_xy=anchors[order, :2])
        r = R.select(c, post_max=case["post"])
        want = g["c%d_selected" % ci].tolist()
        assert order[r["keep"]].tolist() == want and r["full_keep"] == r["keep"] and r["truncated"] == 0, ci
        kept.append(len(want))
        unkept.append(r["unkept_passes"])
        if not want:
            continue
        assert np.allclose(r["core"]["box"], g["c%d_boxes" % ci].reshape(-1, 7), atol=2e-4, equal_nan=True), ci   # NaN: a pick beyond the last distance bound (weight 0 / 0), as in the reference
        assert np.allclose(r["core"]["score"], g["c%d_scores" % ci], atol=1e-5), ci
        assert r["core"]["dir"].tolist() == g["c%d_dirs" % ci].tolist() and not g["c%d_labels" % ci].any()
    print(kept, unkept)
    assert max(unkept[:-1]) > 0 and unkept[-1] == 1          # both branches of the core ran
    assert kept[0] >= 10 and kept[1] >= 5 and kept[-1] == 0   # the single candidate of the last case: score 0, cnt <= 1
    assert CASES[1]["pre"] < CASES[1]["n"]                     # the top-k cut binds


def test_di_predict_ref_cut_and_truncation_flag(golden_dir):
    g = np.load(os.path.join(golden_dir, "di_predict_ref.npz"))
    box, anchors, scores, ioup, dirs = [g["c0_in_%s" % k] for k in ("box", "anchors", "scores", "iou_preds", "dirs")]
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    c = dict(box=box[order], score=scores[order], iou_pred=ioup[order], dir=dirs[order], anchor_xy=anchors[order, :2])
    full = R.select(c, post_max=100)
    cut = R.select(c, post_max=5)
    assert len(full["keep"]) > 5 and cut["keep"] == full["keep"][:5] and cut["truncated"] == 1 and full["truncated"] == 0
    assert np.array_equal(cut["core"]["box"], full["core"]["box"][:5], equal_nan=True)
    exact = R.select(c, post_max=len(full["keep"]))   # stops exactly at the last keep: flag = were candidates left
    assert exact["keep"] == full["keep"] and exact["truncated"] in (0, 1)


def test_unknown_nms_type_and_too_many_candidates_raise_before_any_device_call():
    from sessd_hip import configs, ops
    from sessd_hip.engine import InferenceEngine
    head, anchors = torch.zeros((1, 22, 8)), torch.zeros((16, 7))   # CPU tensors: the checks come first
    with pytest.raises(ValueError, match="nms_type"):
        ops.predict(head, anchors, nms_type="soft_nms")
    with pytest.raises(ValueError, match="1024"):
        ops.predict(head, anchors, pre_max=1025, nms_type="rotate_weighted_nms")
    with pytest.raises(ValueError, match="unknown DI-NMS"):
        ops.predict(head, anchors, nms_type="rotate_weighted_nms", di=dict(cnt_thresh=1.0))
    with pytest.raises(ValueError, match="CUDA"):   # valid settings reach the tensor checks (no CPU fallback)
        ops.predict(head, anchors, pre_max=1024, nms_type="rotate_weighted_nms")
    VG = configs.VOXEL_GENERATOR
    bad = dict(configs.TEST_CFG, nms=dict(configs.TEST_CFG["nms"], nms_type="soft_nms"))
    big = dict(configs.TEST_CFG, nms=dict(configs.TEST_CFG_DI_NMS["nms"], nms_pre_max_size=1025))
    for cfg, msg in ((bad, "nms_type"), (big, "1024")):
        with pytest.raises(ValueError, match=msg):   # model None: nothing else of the constructor may have run
            InferenceEngine(None, VG["range"], VG["voxel_size"], 5, 16000, cfg, 1, 20480, torch.device("cpu"))
    assert ops.nms_settings(configs.TEST_CFG["nms"]) == ("rotate_nms", None)
    assert ops.nms_settings(dict(nms_type="rotate_nms")) == ("rotate_nms", None)
    t, di = ops.nms_settings(dict(configs.TEST_CFG_DI_NMS["nms"], nms_cnt_thresh=0.8))
    assert t == "rotate_weighted_nms" and di == dict(ops.DI_DEFAULTS, nms_cnt_thresh=0.8)
    c = ops.check_di(di)
    assert abs(c.cnt_thresh - 0.8) < 1e-7 and c.n_interval == 4 and list(c.interval)[:4] == [0, 20, 40, 60] and c.centerness_pow == 2
    assert ops.DI_DEFAULTS == R.DI_DEFAULTS   # the literals of mg_head_sessd.py:1012-1017, stated twice


def test_c_entry_points_check_their_arguments():
    import sessd_hip
    from sessd_hip._lib import DiCfg, PredictArgs
    lib = sessd_hip.lib
    wb = lambda *v: lib.sessd_predict_workspace_bytes(*v, 1)
    assert wb(1, 1, 128, 1025, 10) == 0 and wb(1, 5, 128, 100, 10) == 0 and wb(0, 1, 128, 100, 10) == 0
    # the dense overlap matrices are counted: (pre_max, pre_max) float32 per virtual frame
    assert wb(2, 3, 5120, 1000, 100) >= 6 * 1000 * 1000 * 4 and wb(1, 1, 5120, 1000, 100) - wb(1, 1, 5120, 500, 100) >= 3 * 10 ** 6
    c = DiCfg()
    c.n_interval = 4

    def call(pre, nt=1):
        args = PredictArgs(batch=1, num_tasks=nt, num_pixels=64, score_thresh=0.3, pre_max_size=pre, post_max_size=10, nms_iou_thresh=0.01,
                           di=ctypes.pointer(c))
        return lib.sessd_predict(args, None, 0, None)

    assert call(1025) == -1 and call(100, nt=5) == -1
    assert call(100) == -2   # valid settings pass every argument check and stop at the workspace (none given)
    # DI requested without a usable config: n_interval out of range (a NULL `di` selects the greedy NMS)
    for bad in (9, -1):
        c.n_interval = bad
        assert call(100) == -1


def test_configs():
    from sessd_hip import configs
    assert configs.TEST_CFG == dict(nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000,
                                             nms_post_max_size=100, nms_iou_threshold=0.01),
                                    score_threshold=0.3, post_center_limit_range=[0, -40.0, -5.0, 70.4, 40.0, 5.0], max_per_img=100)
    want = dict(configs.TEST_CFG, nms=dict(configs.TEST_CFG["nms"], nms_type="rotate_weighted_nms"))
    assert configs.TEST_CFG_DI_NMS == want and configs.TEST_CFG_DI_NMS["nms"] is not configs.TEST_CFG["nms"]
