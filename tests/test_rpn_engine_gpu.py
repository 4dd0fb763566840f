"""The model of the reference's three-class config (Car / Pedestrian / Cyclist on the SECOND-style RPN neck,
sessd_hip.configs.kitti_3class_rpn_model) through InferenceEngine: eager pass, graph replays and results() bit for bit with the
records ring; every task against the CPU pipeline of tests/rpn_ref.py (the synthetic rule tests/test_multitask_engine_gpu.py uses
for seeded weights); the det3d-mirror model's eager forward; the two-launch tail against the fused launch; DI-NMS; and the runner's
engines on CU sets.

Geometry of tests/test_multitask_engine_gpu.py: x 0..19.2 m, y -8..8 m -> a 40 x 48 BEV map, synth.make_frame(5, 20000)."""
import numpy as np
import pytest
import torch

import rpn_ref
from oracle.compare import compare_detections
from sessd_hip import configs, ops, synth
from sessd_hip.engine import InferenceEngine
from test_multitask_engine_gpu import GRID, H, MAX_VOXELS, T, VRANGE, VSIZE, W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(dev):
    return configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_rpn_model(), voxel_range=VRANGE)


@pytest.fixture(scope="module")
def anchors():
    return configs.kitti_3class_anchors((H, W), VRANGE)


@pytest.fixture(scope="module")
def frame():
    return synth.make_frame(5, 20000)


def _engine(model, anchors, dev, cfg=configs.TEST_CFG, **kw):
    return InferenceEngine(model, VRANGE, VSIZE, 5, MAX_VOXELS, cfg, 1, 20480, dev, anchors=anchors, **kw)


def _same(a, b):
    for k in ("box3d_lidar", "scores", "label_preds"):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def eager(model, anchors, frame, dev):
    eng = _engine(model, anchors, dev)
    assert eng.form == "rpn" and eng.num_tasks == T and (eng.H, eng.W) == (H, W)
    assert sorted(eng.t) == ["l%d" % i for i in range(6)] + ["out"] and not eng.h   # no branches, no half-resolution maps
    assert eng.fuse_head is False   # the measured default of an RPN engine: the two-launch tail
    eng.fuse_head = True            # this engine: the fused tail + heads launch
    eng.set_points([torch.from_numpy(frame).to(dev)])
    eng.enqueue()
    return eng, eng.results()[0]


def test_rpn_engine_eager_replay_results(eager, frame, dev):
    eng, got = eager
    tc = eng.out["task_count"].cpu().numpy()[0]
    assert len(got["scores"]) == int(tc.sum()) and (tc > 0).all(), tc   # calibrated biases: detections in every task
    bounds = np.concatenate([[0], np.cumsum(tc)])
    for t in range(T):
        assert (got["label_preds"][bounds[t]:bounds[t + 1]] == t).all()
    rec, cnt = eng.attach_records(2)
    eng.capture()
    eng.record_cursor.zero_()   # the capture's own warm-up passes took slots
    for _ in range(2):
        eng.replay()
        _same(eng.results()[0], got)
    assert int(eng.record_cursor.item()) == 2 and rec.shape == (2, T * eng.post_max, 9)
    n = len(got["scores"])
    for slot in range(2):
        assert int(cnt[slot].item()) == n
        r = rec[slot].cpu().numpy()
        assert np.array_equal(r[:n, :7], got["box3d_lidar"]) and np.array_equal(r[:n, 7], got["scores"])
        assert np.array_equal(r[:n, 8].astype(np.int64), got["label_preds"]) and not r[n:].any()
    eng.graph, eng.records = None, None
    # the launches of the frame, by name: six 3x3 layers and the fused tail
    names = sorted(eng.dense_layer_times(reps=1))
    assert names == ["blk0.%d" % i for i in range(6)] + ["rpn_tail+head"], names


def test_rpn_engine_vs_oracle_per_task(eager, model, anchors, frame):
    eng, got = eager
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tc = eng.out["task_count"].cpu().numpy()[0]
    start, shared = 0, {}
    for t in range(T):
        want, inter = rpn_ref.run_frame_task(frame, sd, t, VRANGE, VSIZE, 5, MAX_VOXELS, anchors[t], shared=shared)
        if t == 0:
            bev_err = float((eng.bev.cpu() - inter["bev"]).abs().max()) / max(1.0, float(inter["bev"].abs().max()))
            assert bev_err < 2e-4, bev_err
        sl = slice(start, start + int(tc[t]))
        assert (got["label_preds"][sl] == t).all()
        mine = dict(box3d_lidar=got["box3d_lidar"][sl], scores=got["scores"][sl])
        w = dict(box3d_lidar=want["box3d_lidar"], scores=want["scores"])
        r = compare_detections(mine, w, inter["debug"], rule="synthetic")
        assert r["matched"] == r["n"] == int(tc[t]) > 0, (t, r)
        start += int(tc[t])
    assert start == len(got["scores"])


def test_rpn_mirror_model_matches_engine(eager, model, anchors, frame, dev):
    eng, ref = eager
    pts = torch.from_numpy(frame).to(dev)
    r = ops.voxelize_batch([pts], VSIZE, VRANGE, 5, MAX_VOXELS)
    m = int(r["prefix"][1].item())
    anc = [torch.from_numpy(anchors[t][None]).to(dev) for t in range(T)]
    example = dict(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.tensor([m]), shape=[GRID], anchors=anc, metadata=[dict(token="0")])
    with torch.no_grad():
        got = model(example, return_loss=False)[0]
    assert got["box3d_lidar"].shape[0] == ref["box3d_lidar"].shape[0] > 0
    assert np.array_equal(got["label_preds"].cpu().numpy(), ref["label_preds"])
    assert np.allclose(got["scores"].cpu().numpy(), ref["scores"], rtol=2e-3, atol=1e-6)
    assert np.allclose(got["box3d_lidar"].cpu().numpy(), ref["box3d_lidar"], rtol=1e-3, atol=1e-3)


def test_two_launch_tail_against_the_fused_launch(eager, model, anchors, frame, dev):
    """engine.fuse_head = False (an RPN engine's default): the up-sampler through ops.conv2d, the heads through ops.conv2d,
    predict's own score filter."""
    e1, fused = eager
    e2 = _engine(model, anchors, dev)
    assert e1.fuse_head is True and e2.fuse_head is False
    e2.set_points([torch.from_numpy(frame).to(dev)])
    e2.enqueue()
    two = e2.results()[0]
    ref = e1.head.double()
    err, bound = float((e2.head.double() - ref).abs().max()), 2e-4 * float(ref.abs().max())
    print("two-launch head vs fused: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert np.array_equal(two["label_preds"], fused["label_preds"])
    assert torch.equal(e2.out["task_count"], e1.out["task_count"]) and torch.equal(e2.out["count"], e1.out["count"])
    # ... and the neck's output on request (keep_ssfa) is what the two-launch form leaves in t["out"]
    e3 = _engine(model, anchors, dev)
    e3.fuse_head, e3.keep_ssfa = True, True
    e3.set_points([torch.from_numpy(frame).to(dev)])
    e3.enqueue()
    torch.cuda.synchronize()
    assert torch.equal(e3.head, e1.head)
    u = e2.t["out"].double()
    assert float((e3.t["out"].double() - u).abs().max()) <= 2e-4 * float(u.abs().max())


def test_rpn_engine_di_nms(model, anchors, frame, dev):
    eng = _engine(model, anchors, dev, cfg=configs.TEST_CFG_DI_NMS)
    assert eng.nms_type == "rotate_weighted_nms"
    eng.set_points([torch.from_numpy(frame).to(dev)])
    eng.enqueue()
    got = eng.results()[0]
    want = ops.predict(eng.head, eng.anchors, None, eng.score_thresh, eng.pre_max, eng.post_max, eng.nms_thresh,
                       post_center_range=[float(v) for v in eng.post_range], direction_offset=eng.dir_offset, num_tasks=T,
                       nms_type="rotate_weighted_nms", di=eng.di)
    n = int(want["count"][0].item())
    assert n == len(got["scores"]) > 0 and torch.equal(want["task_count"], eng.out["task_count"])
    assert np.array_equal(want["box"][0, :n].cpu().numpy(), got["box3d_lidar"])
    assert np.array_equal(want["score"][0, :n].cpu().numpy(), got["scores"])
    assert np.array_equal(want["label"][0, :n].cpu().numpy().astype(np.int64), got["label_preds"])


def test_rpn_engines_on_cu_sets(eager, model, anchors, frame, dev):
    """runner.engines_on_cu_sets without a tune cloud: force_active_tiles() + whole-unit shares leave an RPN engine in a valid list
    configuration, the engines capture, and each engine's replay equals, bit for bit, a single engine in the same launch
    configuration (same kernels, same workgroup counts => same summation order). Against the default-launch engine of the other
    tests the kernels differ (Winograd over lists against the direct convolution): the tolerances of the mirror check."""
    from sessd_hip.runner import engines_on_cu_sets
    _, ref = eager
    engines, streams = engines_on_cu_sets(model, VRANGE, VSIZE, 5, MAX_VOXELS, configs.TEST_CFG, n_engines=2, sets=2, device=dev,
                                          anchors=anchors, max_points_per_frame=20480)
    pts = torch.from_numpy(frame).to(dev)
    single = _engine(model, anchors, dev)
    single.cu_budget = engines[0].cu_budget
    assert sorted(single.force_active_tiles()) == list(range(6))
    single.set_list_shares("whole")   # what the runner does without a tune cloud
    assert all(single.tile_cfg["blk0.%d" % i] == 22 for i in range(6))
    single.set_points([pts])
    single.enqueue()
    want = single.results()[0]
    assert len(want["scores"]) == len(ref["scores"]) > 0 and np.array_equal(want["label_preds"], ref["label_preds"])
    assert np.allclose(want["scores"], ref["scores"], rtol=2e-3, atol=1e-6)
    assert np.allclose(want["box3d_lidar"], ref["box3d_lidar"], rtol=1e-3, atol=1e-3)
    for e, st in zip(engines, streams):
        assert e.graph is not None and e.active_cfg == single.active_cfg and e.tile_cfg == single.tile_cfg and e.cu_budget == single.cu_budget
        with torch.cuda.stream(st):
            e.set_points([pts])
            e.replay()
    for e, st in zip(engines, streams):
        st.synchronize()
        _same(e.results()[0], want)
