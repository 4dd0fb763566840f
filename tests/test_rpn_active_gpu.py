"""Tile lists for the RPN neck of the three-class config: the six stride-1 3x3 layers over the 2x2-output tiles that can differ
from the layer's constant (activity program {0, 0, 0, 0, 0, 0}, constants = sessd_hip.engine.rpn_tile_constants, the first five
outputs filled where their one reader can reach, the sixth everywhere), against an engine without tile lists on the same frame.

Geometry of tests/test_rpn_engine_gpu.py (40 x 48 BEV map = 480 tiles). Bounds: head tensors 2e-4 * max |ref| (DESIGN.md section 3,
Numerics: the list launches are Winograd, the reference engine runs the direct kernels), detections under
oracle.compare.same_detections' strict defaults (2 mm, 1e-3 relative scores)."""
import numpy as np
import pytest
import torch

from oracle.compare import same_detections
from sessd_hip import configs, synth
from sessd_hip.engine import InferenceEngine
from test_multitask_engine_gpu import H, MAX_VOXELS, T, VRANGE, VSIZE, W

pytestmark = pytest.mark.gpu


def test_list_engine_against_the_dense_engine(dev):
    model = configs.build_synthetic_detector(dev, seed=0, model_cfg=configs.kitti_3class_rpn_model(), voxel_range=VRANGE)
    anchors = configs.kitti_3class_anchors((H, W), VRANGE)
    pts = [torch.from_numpy(synth.make_frame(5, 20000)).to(dev)]

    def engine(**kw):
        return InferenceEngine(model, VRANGE, VSIZE, 5, MAX_VOXELS, configs.TEST_CFG, 1, 20480, dev, anchors=anchors, **kw)

    dense = engine(active_tiles=False)
    assert dense.ta is None and sorted(dense.t) == ["l0", "l1", "out"]   # ping-pong buffers: nothing the form does not need
    dense.set_points(pts)
    dense.enqueue()
    want = dense.results()[0]
    lists = engine()
    lists.fuse_head = True   # the fused tail reads the sixth map, which is filled everywhere
    assert sorted(lists.t) == ["l%d" % i for i in range(6)] + ["out"] and not lists.h
    cfg = lists.force_active_tiles()
    assert sorted(cfg) == list(range(6)) and lists.ta.steps == [0] * 6
    lists.set_points(pts)
    lists.enqueue()
    got = lists.results()[0]
    assert lists._active_layers() == list(range(6))
    ref = dense.head.double()
    err, bound = float((lists.head.double() - ref).abs().max()), 2e-4 * float(ref.abs().max())
    print("list engine head vs dense engine: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert len(want["scores"]) > 0 and same_detections(got, want) is None, same_detections(got, want)
    assert np.array_equal(got["label_preds"], want["label_preds"])
    n = lists.ta.n_list.cpu().numpy()
    tiles = (H // 2) * (W // 2)
    print("tiles per slot:", n.tolist(), "of", tiles, lists.active_tile_fractions())
    assert len(n) == 6 and (n > 0).all() and (np.diff(n) >= 0).all() and n[0] < tiles, n
    # every layer's map: computed tiles + constants == the dense engine's map (the fill covers what a reader can reach; the last
    # map is filled everywhere)
    last = lists.t["l5"].double()
    dl = dense.t["l1"].double()   # six layers ping-pong: the sixth output is in "l1"
    assert float((last - dl).abs().max()) <= 2e-4 * float(dl.abs().max())
    # the capture replays the eager pass bit for bit
    lists.capture()
    for _ in range(2):
        lists.replay()
        r = lists.results()[0]
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert np.array_equal(r[k], got[k]), k
    # runner's share rule leaves a valid configuration, too
    lists.graph = None
    lists.set_list_shares("whole")
    assert all(mr == -1 for _, mr in lists.active_cfg.values())
    lists.enqueue()
    assert same_detections(lists.results()[0], want) is None
