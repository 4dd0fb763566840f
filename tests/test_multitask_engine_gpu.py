"""A three-task model (Car / Pedestrian / Cyclist, sessd_hip.configs.kitti_3class_model) through InferenceEngine: eager pass,
graph replay and results() bit for bit; the det3d-mirror model's eager forward (tolerance of tests/test_pipeline_gpu.py::
test_module_path_matches_engine); the CPU oracle pipeline run once per task on that task's weights and anchors (the synthetic
rule tests/test_pipeline_gpu.py uses for seeded weights); and the single-task engine untouched by all of it.

Reduced voxel range x 0..19.2 m, y -8..8 m: a 40 x 48 BEV map (48 % 8 == 0 and 40 % 4 == 0 keep the engine's tile-activity
set-up on), so that three oracle runs take seconds."""
import numpy as np
import pytest
import torch

from oracle import pipeline
from oracle.compare import compare_detections
from sessd_hip import configs, ops, synth
from sessd_hip.engine import InferenceEngine

pytestmark = pytest.mark.gpu
VRANGE = [0, -8.0, -3.0, 19.2, 8.0, 1.0]
VSIZE = configs.VOXEL_GENERATOR["voxel_size"]
GRID = [384, 320, 40]
H, W = 40, 48
MAX_VOXELS = 16000
T = 3


@pytest.fixture(scope="module")
def model(dev):
    return configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_model(), voxel_range=VRANGE)


@pytest.fixture(scope="module")
def anchors():
    return configs.kitti_3class_anchors((H, W), VRANGE)


@pytest.fixture(scope="module")
def frame():
    return synth.make_frame(5, 20000)


def _engine(model, anchors, dev, **kw):
    return InferenceEngine(model, VRANGE, VSIZE, 5, MAX_VOXELS, configs.TEST_CFG, 1, 20480, dev, anchors=anchors, **kw)


def _same(a, b):
    for k in ("box3d_lidar", "scores", "label_preds"):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def eager(model, anchors, frame, dev):
    eng = _engine(model, anchors, dev)
    assert eng.num_tasks == T and (eng.H, eng.W) == (H, W)
    eng.set_points([torch.from_numpy(frame).to(dev)])
    eng.enqueue()
    return eng, eng.results()[0]


def test_three_task_engine_eager_replay_results(eager, frame, dev):
    eng, got = eager
    tc = eng.out["task_count"].cpu().numpy()[0]
    assert len(got["scores"]) == int(tc.sum()) and (tc > 0).all(), tc   # calibrated biases: candidates in every task
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


def test_three_task_mirror_model_matches_engine(eager, model, anchors, frame, dev):
    eng, ref = eager
    pts = torch.from_numpy(frame).to(dev)
    r = ops.voxelize_batch([pts], VSIZE, VRANGE, 5, MAX_VOXELS)
    m = int(r["prefix"][1].item())
    anc = [torch.from_numpy(anchors[t][None]).to(dev) for t in range(T)]
    example = dict(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.tensor([m]), shape=[GRID], anchors=anc, metadata=[dict(token="0")])
    with torch.no_grad():
        got = model(example, return_loss=False)[0]
    assert got["metadata"] == dict(token="0")
    assert got["box3d_lidar"].shape[0] == ref["box3d_lidar"].shape[0] > 0
    assert np.array_equal(got["label_preds"].cpu().numpy(), ref["label_preds"])
    assert np.allclose(got["scores"].cpu().numpy(), ref["scores"], rtol=2e-3, atol=1e-6)
    assert np.allclose(got["box3d_lidar"].cpu().numpy(), ref["box3d_lidar"], rtol=1e-3, atol=1e-3)


def test_three_task_engine_vs_oracle_per_task(eager, model, anchors, frame):
    eng, got = eager
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tc = eng.out["task_count"].cpu().numpy()[0]
    start = 0
    for t in range(T):
        sd_t = dict(sd)
        for k in sd:
            if k.startswith("bbox_head.tasks.%d." % t):
                sd_t["bbox_head.tasks.0." + k[len("bbox_head.tasks.%d." % t):]] = sd[k]
        want, inter = pipeline.run_frames([frame], sd_t, VRANGE, VSIZE, 5, MAX_VOXELS, anchors[t], None, return_intermediate=True)
        sl = slice(start, start + int(tc[t]))
        assert (got["label_preds"][sl] == t).all()
        mine = dict(box3d_lidar=got["box3d_lidar"][sl], scores=got["scores"][sl])
        w = dict(box3d_lidar=want[0]["box3d_lidar"], scores=want[0]["scores"])
        r = compare_detections(mine, w, inter["debug"][0], rule="synthetic")
        assert r["matched"] == r["n"] == int(tc[t]) > 0, (t, r)
        start += int(tc[t])
    assert start == len(got["scores"])


@pytest.mark.parametrize("fuse_head", [True, False])
def test_single_task_engine_is_task0_of_the_three_task_engine(model, anchors, frame, dev, fuse_head):
    """A single-task engine (the launch sequence of before) built from tasks[0] alone == task 0's rows of the three-task
    engine, bit for bit, with the fused head launch and with the two-launch head (fuse_head=False)."""
    from det3d.models import build_detector
    car = build_detector(configs.kitti_car_model(), train_cfg=None, test_cfg=configs.TEST_CFG)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith(("bbox_head.tasks.1.", "bbox_head.tasks.2."))}
    car.load_state_dict(sd)
    car.to(dev).eval()
    pts = [torch.from_numpy(frame).to(dev)]
    res = []
    for mdl, anc in ((car, anchors[0]), (model, anchors)):
        eng = _engine(mdl, anc, dev)
        eng.fuse_head = fuse_head
        eng.set_points(pts)
        eng.enqueue()
        res.append((eng, eng.results()[0]))
    (e1, one), (e3, three) = res
    assert e1.num_tasks == 1 and "task_count" not in e1.out and e1.head.shape == (1, 22, H * W)
    assert torch.equal(e3.head.view(1, T, 22, H * W)[:, 0], e1.head)
    n = int(e3.out["task_count"][0, 0].item())
    assert n == len(one["scores"]) > 0
    for k in ("box3d_lidar", "scores", "label_preds"):
        assert np.array_equal(three[k][:n], one[k]), k
