"""PillarEngine's two front ends, its record ring, and the host-fed runner over PillarEngines on CU sets.

Geometry, frames, model and anchors of tests/test_pointpillars_detector_gpu.py (48 x 32 canvas, frames of seeds 5 and 6).
front_end="tensor" is the frame the engine had before (sessd_voxelize_frames + sessd_pillar_features); "fused" runs
sessd_pillar_frames. They must agree bit for bit; the ring and the pipeline must hand out what a plain batch-1 engine computes."""
import numpy as np
import pytest
import torch

import test_pointpillars_detector_gpu as D
from sessd_hip import HostFedPipeline, PillarEngine, configs, pillar_engines_on_cu_sets

pytestmark = pytest.mark.gpu

B = len(D.FRAME_SEEDS)
CUT = 200            # below both frames' pillar counts (tests/test_pillar_engine_gpu.py)
MAX_POINTS = 20000
TEST_CFG_DI = dict(configs.TEST_CFG_POINTPILLARS, nms=dict(configs.TEST_CFG_POINTPILLARS["nms"], nms_type=configs.TEST_CFG_DI_NMS["nms"]["nms_type"]))


def vg_cfg(max_voxels=D.MAX_VOXELS):
    return dict(range=D.VRANGE, voxel_size=D.VSIZE, max_points_in_voxel=D.T, max_voxel_num=max_voxels)


@pytest.fixture(scope="module")
def model(dev):
    return D.build_model().to(dev)


@pytest.fixture(scope="module")
def clouds(dev):
    return [torch.from_numpy(f).to(dev) for f in D.frames()]


def snapshot(eng):
    torch.cuda.synchronize()
    return dict(head=eng.head.clone(), box=eng.out["box"].clone(), score=eng.out["score"].clone(), label=eng.out["label"].clone(),
                count=eng.out["count"].clone(), prefix=eng.prefix.clone())


def same_frame(a, ia, b, ib):
    n = int(a["count"][ia])
    return (n == int(b["count"][ib]) and torch.equal(a["head"][ia], b["head"][ib]) and torch.equal(a["box"][ia, :n], b["box"][ib, :n])
            and torch.equal(a["score"][ia, :n], b["score"][ib, :n]) and torch.equal(a["label"][ia, :n], b["label"][ib, :n]))


def engine(model, mode, max_voxels=D.MAX_VOXELS, batch=B, test_cfg=configs.TEST_CFG_POINTPILLARS):
    return PillarEngine(model, vg_cfg(max_voxels), test_cfg, batch_size=batch, max_points=MAX_POINTS, anchors=D.anchors(), front_end=mode)


def test_front_end_modes_agree(model, clouds):
    snaps = {}
    for mode in ("fused", "tensor"):
        eng = engine(model, mode)
        assert eng.front_end == mode and (eng.voxels is None) == (eng.mean is None) == (mode == "fused")
        eng.set_points(clouds)
        eng.enqueue()
        eager = snapshot(eng)
        eng.capture(warmup=1)
        eng.replay()
        replayed = snapshot(eng)
        eng.set_points(clouds[::-1])
        eng.replay()
        swapped = snapshot(eng)
        assert int(eng.err.item()) == 0
        snaps[mode] = (eager, replayed, swapped)
        # within a mode: replay == eager, restaged in the other order the frames' results swap
        assert all(same_frame(eager, b, replayed, b) for b in range(B)) and torch.equal(eager["prefix"], replayed["prefix"])
        assert same_frame(swapped, 0, eager, 1) and same_frame(swapped, 1, eager, 0)
        n = np.diff(eager["prefix"].cpu().numpy())
        assert n[0] != n[1] and np.diff(swapped["prefix"].cpu().numpy()).tolist() == n[::-1].tolist()
    assert min(int(c) for c in snaps["tensor"][0]["count"]) >= 5     # there is something to compare
    for f, t in zip(snaps["fused"], snaps["tensor"]):
        assert torch.equal(f["prefix"], t["prefix"]) and all(same_frame(f, b, t, b) for b in range(B))


def test_front_end_modes_agree_at_the_max_voxel_cut(model, clouds):
    snaps = []
    for mode in ("fused", "tensor"):
        eng = engine(model, mode, max_voxels=CUT)
        eng.set_points(clouds)
        eng.enqueue()
        snaps.append(snapshot(eng))
        assert eng.prefix.cpu().tolist() == [0, CUT, 2 * CUT] and int(eng.err.item()) == 0
    assert all(same_frame(snaps[0], b, snaps[1], b) for b in range(B))


def test_stage_times_name_the_front_end(model, clouds):
    keys = {}
    for mode in ("fused", "tensor"):
        eng = engine(model, mode, batch=1)
        eng.set_points(clouds[:1])
        keys[mode] = set(eng.stage_times(reps=1))
    common = {"blk0", "blk1", "blk2", "up0", "up1", "up2", "head", "predict"}
    assert keys["tensor"] == common | {"voxelize", "canvas_clear", "pillar"}
    assert keys["fused"] == common | {"canvas_clear", "front_end"}


def test_record_ring_wraps(model, clouds):
    eng = engine(model, "fused", batch=1)
    rec, cnt = eng.attach_records(4)
    assert tuple(rec.shape) == (4, eng.post_max, 9) and tuple(cnt.shape) == (4,) and eng.num_tasks == 1
    outs = []
    for i in range(6):
        eng.set_points([clouds[i % 2]])
        eng.enqueue()
        torch.cuda.synchronize()
        outs.append({k: eng.out[k].clone() for k in ("box", "score", "label", "count")})
    assert int(eng.record_cursor.item()) == 6
    assert not torch.equal(outs[0]["box"], outs[1]["box"])           # the two clouds' records can be told apart
    for i in range(2, 6):     # frames 4 and 5 overwrote slots 0 and 1
        slot, o = i % 4, outs[i]
        n = int(o["count"][0])
        assert n >= 5 and int(eng.record_counts[slot]) == n
        assert torch.equal(eng.records[slot, :n, :7], o["box"][0, :n]) and torch.equal(eng.records[slot, :n, 7], o["score"][0, :n])
        assert torch.equal(eng.records[slot, :n, 8], o["label"][0, :n].float())
    eng.capture(warmup=1)
    with pytest.raises(RuntimeError, match="precede capture"):
        eng.attach_records(4)


def host_clouds():
    fr = D.frames()
    lengths = (20000, 18000, 15000, 20000, 9000, 12000, 17000)
    return [np.ascontiguousarray(fr[i % 2][:n]) for i, n in enumerate(lengths)]


def plain_results(model, dev, test_cfg):
    eng = engine(model, None, batch=1, test_cfg=test_cfg)
    out = []
    for c in host_clouds():
        eng.set_points([torch.from_numpy(c).to(dev)])
        eng.enqueue()
        out.append(eng.results()[0])
    return out


def assert_results_equal(got, want):
    assert len(got) == len(want) == 7
    for g, w in zip(got, want):
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), k


def run_job(pipe):
    got = []
    for c in host_clouds():
        pipe.submit(c)
        got += pipe.poll()
    return got + pipe.finish()


def test_host_fed_pipeline_over_pillar_engines(model, dev):
    want = plain_results(model, dev, configs.TEST_CFG_POINTPILLARS)
    assert min(len(w["scores"]) for w in want[:2]) >= 5 and not np.array_equal(want[0]["scores"], want[1]["scores"])   # order shows
    engines, streams = pillar_engines_on_cu_sets(model, vg_cfg(), configs.TEST_CFG_POINTPILLARS, n_engines=2, sets=2, records=4,
                                                 max_points=MAX_POINTS, anchors=D.anchors())
    assert all(e.graph is not None and e.cu_budget > 0 and e.records.shape[0] == 4 for e in engines)
    pipe = HostFedPipeline(engines, streams, fetch_every=2)
    assert_results_equal(run_job(pipe), want)       # seven frames on two engines: finish() flushes partial fetches
    assert pipe.nms_truncated is False
    eager = HostFedPipeline(engines, streams, fetch_every=2, eager=True)
    assert_results_equal(run_job(eager), want)
    assert eager.nms_truncated is False


def test_host_fed_pipeline_with_di_nms(model, dev):
    want = plain_results(model, dev, TEST_CFG_DI)
    engines, streams = pillar_engines_on_cu_sets(model, vg_cfg(), TEST_CFG_DI, n_engines=2, sets=2, records=4, max_points=MAX_POINTS,
                                                 anchors=D.anchors())
    assert all(e.nms_type == "rotate_weighted_nms" for e in engines)
    pipe = HostFedPipeline(engines, streams, fetch_every=2)
    assert_results_equal(run_job(pipe), want)
    # the sticky flag says what the frames' own di_truncated said (post_max = 300 leaves room on these clouds)
    assert pipe.nms_truncated == any(int(e.nms_truncated.item()) for e in engines)
