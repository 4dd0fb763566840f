"""sessd_hip.PillarEngine: the PointPillars config as a pre-allocated, sync-free frame of launches (voxelize -> pillar kernel with
the canvas -> RPN blocks -> one-launch up-samplers into the neck map -> head -> predict), eager, captured and replayed.

Geometry, seeds and helpers of tests/test_pointpillars_detector_gpu.py: a 48 x 32 pillar grid, a 24 x 16 head map, T = 100, two
frames (seeds 5, 6), model seed 0, 2000 pillars per frame at the most. Against (1) the module path, bit for bit, with the module
path's up-sampler lowering; (2) the CPU chain of that file with the fused up-samplers, head map within 2e-4 * max |ref| (the
project's figure for float32 dense layers) and detections under the synthetic rule; (3) itself: replay == eager, swapped frames
give swapped outputs; (4) the CPU chain on pillars cut at max_voxel_num = 200.

The cut is 200, not 300: frame 5 has 247 pillars in this geometry (frame 6: 1025), so 300 would not cut it. 200 is below BOTH
frames' counts, which is what the case is for; the CPU voxelizer is asserted to return exactly 200 pillars for each frame."""
import numpy as np
import pytest
import torch

import pillars_ref as PR
import test_pointpillars_detector_gpu as D
from oracle import capi, dense_head
from oracle.compare import compare_detections
from sessd_hip import PillarEngine, configs, ops

pytestmark = pytest.mark.gpu

B = len(D.FRAME_SEEDS)
CUT = 200   # below each frame's pillar count (247, 1025)


def vg_cfg(max_voxels=D.MAX_VOXELS):
    return dict(range=D.VRANGE, voxel_size=D.VSIZE, max_points_in_voxel=D.T, max_voxel_num=max_voxels)


def make_engine(model, dev, max_voxels=D.MAX_VOXELS, order=(0, 1)):
    eng = PillarEngine(model, vg_cfg(max_voxels), configs.TEST_CFG_POINTPILLARS, batch_size=B, max_points=20000, anchors=D.anchors())
    stage(eng, dev, order)
    return eng


def stage(eng, dev, order=(0, 1)):
    fr = D.frames()
    eng.set_points([torch.from_numpy(fr[i]).to(dev) for i in order])


def snapshot(eng):
    torch.cuda.synchronize()
    return dict(head=eng.head.clone(), box=eng.out["box"].clone(), score=eng.out["score"].clone(), label=eng.out["label"].clone(),
                count=eng.out["count"].clone(), prefix=eng.prefix.clone())


def same_frame(a, ia, b, ib):
    """frame ia of snapshot a == frame ib of snapshot b, bit for bit (head map, count, the live detections)"""
    n = int(a["count"][ia])
    return (n == int(b["count"][ib]) and torch.equal(a["head"][ia], b["head"][ib]) and torch.equal(a["box"][ia, :n], b["box"][ib, :n])
            and torch.equal(a["score"][ia, :n], b["score"][ib, :n]) and torch.equal(a["label"][ia, :n], b["label"][ib, :n]))


def err_clear(eng):
    return int(eng.err.item()) == 0


@pytest.fixture(scope="module")
def setup():
    model = D.build_model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    head, dets = D.cpu_chain(sd)
    counts = [len(r["scores"]) for r, _ in dets]
    assert min(counts) >= 5, counts    # the condition the seeds were chosen for, on the oracle alone
    return model, sd, head, dets


@pytest.fixture(scope="module")
def shared(setup, dev):
    """One engine with the default (fused) up-samplers on frames (5, 6), run once eagerly."""
    eng = make_engine(setup[0].to(dev), dev)
    eng.enqueue()
    return eng, snapshot(eng)


def captured(eng):
    if eng.graph is None:
        eng.capture(warmup=2)
    return eng


def test_parent_lowering_equals_the_module_path_bit_for_bit(setup, dev):
    model = setup[0].to(dev)
    pts = [torch.from_numpy(f).to(dev) for f in D.frames()]
    r = ops.voxelize_batch(pts, D.VSIZE, D.VRANGE, D.T, D.MAX_VOXELS)
    prefix = r["prefix"].cpu().numpy()
    m = int(prefix[B])
    anc = torch.from_numpy(D.anchors()[None]).to(dev).repeat(B, 1, 1)
    example = dict(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.from_numpy(np.diff(prefix)), shape=[D.GRID], anchors=[anc],
                   metadata=[dict(token=str(b)) for b in range(B)])
    with torch.no_grad():
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"], batch_size=B,
                    input_shape=D.GRID)
        head = model.bbox_head(model.extract_feat(data))[0]["_planar"]
        want = model(example, return_loss=False)
    eng = make_engine(model, dev)
    eng.fused_upsamplers = False
    eng.enqueue()
    torch.cuda.synchronize()
    assert (eng.H, eng.W) == (D.H, D.W) and eng.prefix.cpu().tolist() == prefix.tolist()
    assert torch.equal(eng.head.view(B, 22, D.H, D.W), head)
    cnt = eng.out["count"].cpu().tolist()
    for b in range(B):
        n = len(want[b]["scores"])
        assert cnt[b] == n >= 5
        assert torch.equal(eng.out["box"][b, :n], want[b]["box3d_lidar"]) and torch.equal(eng.out["score"][b, :n], want[b]["scores"])
        assert torch.equal(eng.out["label"][b, :n].long(), want[b]["label_preds"])
    # ... and the same through a captured graph
    eager = snapshot(eng)
    eng.capture(warmup=1)
    eng.replay()
    again = snapshot(eng)
    assert all(same_frame(eager, b, again, b) for b in range(B))
    assert err_clear(eng)


def test_fused_upsamplers_against_the_cpu_chain(setup, shared):
    _, _, head_ref, want = setup
    eng, snap = shared
    assert eng.fused_upsamplers is True
    head = snap["head"].view(B, 22, D.H, D.W).cpu()
    err, bound = float((head.double() - head_ref.double()).abs().max()), 2e-4 * float(head_ref.abs().max())
    print("engine head map (fused up-samplers) vs CPU chain: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    got = eng.results()
    assert len(got) == B
    for b in range(B):
        w, dbg = want[b]
        res = compare_detections(dict(box3d_lidar=got[b]["box3d_lidar"], scores=got[b]["scores"]),
                                 dict(box3d_lidar=w["box3d_lidar"], scores=w["scores"]), dbg, rule="synthetic")
        print("frame %d: %d detections, %d near-threshold NMS decisions" % (b, res["n"], len(res["near_pairs"])))
        assert res["matched"] == res["n"] == len(w["scores"]), (b, res)
        assert (got[b]["label_preds"] == 0).all()
    assert err_clear(eng)


def test_replay_reproduces_the_eager_frame(shared):
    eng, eager = shared
    captured(eng).replay()
    again = snapshot(eng)
    assert all(same_frame(eager, b, again, b) for b in range(B))
    assert torch.equal(eager["prefix"], again["prefix"])
    assert err_clear(eng)


def test_no_state_is_left_over_from_the_previous_frame(shared, dev):
    eng, first = shared
    captured(eng).replay()
    try:
        stage(eng, dev, (1, 0))
        eng.replay()
        swapped = snapshot(eng)
    finally:
        stage(eng, dev, (0, 1))
    n = np.diff(first["prefix"].cpu().numpy())
    assert n[0] != n[1] and np.diff(swapped["prefix"].cpu().numpy()).tolist() == n[::-1].tolist()
    assert same_frame(swapped, 0, first, 1) and same_frame(swapped, 1, first, 0)
    assert err_clear(eng)


def test_truncation_at_max_voxel_num(setup, dev):
    model, sd, _, _ = setup
    vs, ns, cs = [], [], []
    for b, pts in enumerate(D.frames()):
        v, c, n = capi.points_to_voxel(pts, D.VSIZE, D.VRANGE, D.T, CUT)
        assert len(c) == CUT     # below the frame's pillar count: the reference's break rule cuts
        vs.append(v), ns.append(n), cs.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
    vox, num, coors = np.concatenate(vs), np.concatenate(ns), np.concatenate(cs)
    feat = PR.reader_forward(vox, num, coors, sd)
    canvas = PR.scatter(feat, coors, B, D.GRID[1], D.GRID[0])
    neck = PR.rpn_forward(canvas, {k: v.float() for k, v in sd.items() if k.startswith("neck.")}, PR.RPN3_ARGS["ds_layer_strides"],
                          PR.RPN3_ARGS["us_layer_strides"])
    preds = dense_head.head_forward(neck, sd)
    head_ref = torch.cat([preds[k].permute(0, 3, 1, 2) for k in ("box_preds", "cls_preds", "dir_cls_preds", "iou_preds")], 1)
    eng = make_engine(model.to(dev), dev, max_voxels=CUT)
    eng.enqueue()
    torch.cuda.synchronize()
    assert eng.prefix.cpu().tolist() == [0, CUT, 2 * CUT]
    head = eng.head.view(B, 22, D.H, D.W).cpu()
    err, bound = float((head.double() - head_ref.double()).abs().max()), 2e-4 * float(head_ref.abs().max())
    print("engine head map at max_voxel_num = %d vs CPU chain: max err %.3e, bound %.3e" % (CUT, err, bound))
    assert err <= bound
    assert err_clear(eng)


def test_error_flag_is_clean(shared):
    eng, _ = shared
    eng.enqueue()
    eng.results()    # raises if the sticky flag is set
    assert err_clear(eng)
