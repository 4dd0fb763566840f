"""DI-NMS (test_cfg nms_type "rotate_weighted_nms", sessd_hip.configs.TEST_CFG_DI_NMS) through InferenceEngine on the reduced
range and the three-task synthetic detector of tests/test_multitask_engine_gpu.py (40 x 48 map): eager pass, graph replays and
results() bit for bit, the records ring, MultiGroupHead.predict of the mirror model, the CPU helper tests/di_predict_ref.py fed
with the engine's own head tensor, and a greedy-NMS engine built before and after that still gives its own result.

The seeded detector's IoU head keeps cnt = sum(overlap * iou_pred) of a candidate's neighbourhood well below the reference's
2.6, so the configuration passes nms_cnt_thresh = ENGINE_CNT through the new key; the preconditions (at least two kept boxes, at
least one pass that was not kept, no near-tie deciding a pick) are asserted on the CPU side of the test."""
import numpy as np
import pytest
import torch

import di_predict_ref as R
from sessd_hip import configs, ops, synth
from sessd_hip.engine import InferenceEngine
from test_multitask_engine_gpu import GRID, H, MAX_VOXELS, T, VRANGE, VSIZE, W

pytestmark = pytest.mark.gpu
ENGINE_CNT = 1.0
DI_CFG = dict(configs.TEST_CFG_DI_NMS, nms=dict(configs.TEST_CFG_DI_NMS["nms"], nms_cnt_thresh=ENGINE_CNT))


def _split(head, P):
    box = head[:14].reshape(2, 7, P).transpose(2, 0, 1).reshape(-1, 7)
    return box, head[14:16].T.reshape(-1), head[16:20].reshape(2, 2, P).transpose(2, 0, 1).reshape(-1, 2), head[20:22].T.reshape(-1)


def _same(a, b):
    for k in ("box3d_lidar", "scores", "label_preds"):
        assert np.array_equal(a[k], b[k]), k


def test_di_engine(dev):
    model = configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_model(), voxel_range=VRANGE)
    anchors = configs.kitti_3class_anchors((H, W), VRANGE)
    frame = synth.make_frame(5, 20000)
    pts = [torch.from_numpy(frame).to(dev)]

    def run(cfg):
        e = InferenceEngine(model, VRANGE, VSIZE, 5, MAX_VOXELS, cfg, 1, 20480, dev, anchors=anchors)
        e.set_points(pts)
        e.enqueue()
        return e, e.results()[0]

    _, greedy_before = run(configs.TEST_CFG)
    eng, got = run(DI_CFG)
    assert eng.nms_type == "rotate_weighted_nms" and eng.num_tasks == T and (eng.H, eng.W) == (H, W)
    tc = eng.out["task_count"].cpu().numpy()[0]
    assert len(got["scores"]) == int(tc.sum()) and (tc > 0).any() and int(eng.nms_truncated.item()) == 0
    assert not eng.out["di_truncated"].any()
    bounds = np.concatenate([[0], np.cumsum(tc)])
    for t in range(T):
        assert (got["label_preds"][bounds[t]:bounds[t + 1]] == t).all()
    # ---- the CPU helper on the engine's own head tensor (read back)
    hv = eng.head.view(1, T, 22, H * W).cpu().numpy()
    kept, unkept = 0, 0
    for t in range(T):
        args = _split(hv[0, t], H * W) + (np.asarray(anchors[t], np.float32), None, eng.score_thresh, eng.pre_max, eng.post_max,
                                         dict(nms_cnt_thresh=ENGINE_CNT))
        w = R.predict_task(*args)
        assert R.predict_task(*args, score_dtype=np.float64, with_replay=False)["full_keep"] == w["full_keep"], t   # no near-tie
        kept, unkept = kept + len(w["keep"]), unkept + w["unkept_passes"]
        sl = slice(bounds[t], bounds[t + 1])
        assert int(tc[t]) == len(w["scores"]) and w["truncated"] == 0, t
        if tc[t]:
            eb, es = np.abs(got["box3d_lidar"][sl] - w["box3d_lidar"]).max(), np.abs(got["scores"][sl] - w["scores"]).max()
            print("task %d: %d candidates, %d kept, %d passes not kept, max |box - ref| %.3g, max |score - ref| %.3g"
                  % (t, w["n_top"], len(w["keep"]), w["unkept_passes"], eb, es))
            assert eb <= 2e-4 and es <= 1e-5, (t, eb, es)
    assert kept >= 2 and unkept >= 1   # both branches of the core ran
    # ---- records ring, two graph replays
    rec, cnt = eng.attach_records(2)
    eng.capture()
    eng.record_cursor.zero_()   # the capture's own warm-up passes took slots
    for _ in range(2):
        eng.replay()
        _same(eng.results()[0], got)
    n = len(got["scores"])
    assert int(eng.record_cursor.item()) == 2 and rec.shape == (2, T * eng.post_max, 9) and int(eng.nms_truncated.item()) == 0
    for slot in range(2):
        assert int(cnt[slot].item()) == n
        r = rec[slot].cpu().numpy()
        assert np.array_equal(r[:n, :7], got["box3d_lidar"]) and np.array_equal(r[:n, 7], got["scores"])
        assert np.array_equal(r[:n, 8].astype(np.int64), got["label_preds"]) and not r[n:].any()
    # ---- MultiGroupHead.predict of the mirror model on the same frame
    r = ops.voxelize_batch(pts, VSIZE, VRANGE, 5, MAX_VOXELS)
    m = int(r["prefix"][1].item())
    anc = [torch.from_numpy(anchors[t][None]).to(dev) for t in range(T)]
    example = dict(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.tensor([m]), shape=[GRID], anchors=anc, metadata=[dict(token="0")])
    with torch.no_grad():
        mirror = model.bbox_head.predict(example, model.forward_preds(example), DI_CFG)[0]
    assert mirror["box3d_lidar"].shape[0] == n and np.array_equal(mirror["label_preds"].cpu().numpy(), got["label_preds"])
    assert np.allclose(mirror["scores"].cpu().numpy(), got["scores"], rtol=2e-3, atol=1e-6)   # tests/test_multitask_engine_gpu.py's
    assert np.allclose(mirror["box3d_lidar"].cpu().numpy(), got["box3d_lidar"], rtol=1e-3, atol=1e-3)
    # ---- a greedy-NMS engine built in the same process, after all of that: its pre-existing result
    e2, greedy_after = run(configs.TEST_CFG)
    assert e2.nms_type == "rotate_nms" and "di_truncated" not in e2.out and len(greedy_after["scores"]) > 0
    _same(greedy_before, greedy_after)
    assert len(greedy_after["scores"]) != n or not np.array_equal(greedy_after["box3d_lidar"], got["box3d_lidar"])
