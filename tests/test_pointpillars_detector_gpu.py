"""The reference's PointPillars config end to end on the device: sessd_hip.configs.kitti_pointpillars_model() with seeded weights,
ops.voxelize_batch chained into the det3d-mirror PointPillars (pillar kernel -> scatter -> three-block RPN with the lowered
up-samplers -> head -> predict), against the CPU chain oracle.capi.points_to_voxel -> tests/pillars_ref.py (reader, scatter,
rpn_forward) -> oracle.dense_head.head_forward -> oracle.postprocess.predict_frame under oracle.compare.compare_detections (the
synthetic rule, as tests/test_rpn_engine_gpu.py uses for seeded weights).

Geometry: 0.16 m pillars (the config's voxel generator) over x 4 .. 11.68 m, y -2.56 .. 2.56 m -> a 48 x 32 pillar grid, a
24 x 16 head map; T = 100 points per pillar; two frames of synth.make_frame(.., 20000), cropped by the voxelizer to a few thousand
points each. The reader keeps its own 0.2 m defaults, as in the reference.

Condition on the seed (chosen on the CPU, with the oracle alone): the oracle yields at least five detections in each frame --
asserted below before anything is compared."""
import numpy as np
import pytest
import torch

import pillars_ref as PR
from oracle import capi, dense_head, postprocess
from oracle.compare import compare_detections
from sessd_hip import configs, ops, synth
from sessd_hip.anchors import create_task_anchors

pytestmark = pytest.mark.gpu

VSIZE = [0.16, 0.16, 4.0]
VRANGE = [4.0, -2.56, -3.0, 11.68, 2.56, 1.0]
GRID = [48, 32, 1]
H, W = 16, 24
T, MAX_VOXELS = 100, 2000
SEED, FRAME_SEEDS = 0, (5, 6)
PASS_FRACTION = 0.04   # of the anchors clear the score threshold before NMS (synth.calibrate_synthetic_model)


def build_model(seed=SEED):
    """The mirror model on the CPU (its torch composition), seeded and calibrated on the two frames' oracle pillars."""
    from det3d.models import build_detector
    model = build_detector(configs.kitti_pointpillars_model(), train_cfg=None, test_cfg=configs.TEST_CFG_POINTPILLARS)
    synth.init_synthetic_weights(model, seed)
    vox, num, coors = cpu_pillars()
    run = lambda _f, c, b, shape: model.backbone(model.reader(torch.from_numpy(vox), torch.from_numpy(num), c), c, b, shape)
    synth.calibrate_synthetic_model(model, None, torch.from_numpy(coors), len(FRAME_SEEDS), GRID, pass_fraction=PASS_FRACTION,
                                    sparse_runner=run)
    return model.eval()


def frames():
    return [synth.make_frame(s, 20000) for s in FRAME_SEEDS]


def cpu_pillars():
    vs, cs, ns = [], [], []
    for b, pts in enumerate(frames()):
        v, c, n = capi.points_to_voxel(pts, VSIZE, VRANGE, T, MAX_VOXELS)
        vs.append(v), ns.append(n), cs.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
    return np.concatenate(vs), np.concatenate(ns), np.concatenate(cs)


def anchors():
    return create_task_anchors((H, W), [configs.KITTI_3CLASS_ANCHORS[0]], (VRANGE[0], VRANGE[1], VRANGE[3], VRANGE[4]))[0]


def cpu_chain(sd):
    """(head (B, 22, H, W) planar [box | cls | dir | iou], [(detections, debug) per frame]) of the oracle chain."""
    vox, num, coors = cpu_pillars()
    B = len(FRAME_SEEDS)
    feat = PR.reader_forward(vox, num, coors, sd)
    canvas = PR.scatter(feat, coors, B, GRID[1], GRID[0])
    neck = PR.rpn_forward(canvas, {k: v.float() for k, v in sd.items() if k.startswith("neck.")},
                          PR.RPN3_ARGS["ds_layer_strides"], PR.RPN3_ARGS["us_layer_strides"])
    preds = dense_head.head_forward(neck, sd)
    head = torch.cat([preds[k].permute(0, 3, 1, 2) for k in ("box_preds", "cls_preds", "dir_cls_preds", "iou_preds")], 1)
    nms = configs.TEST_CFG_POINTPILLARS["nms"]
    anc, out = anchors(), []
    for b in range(B):
        args = (preds["box_preds"][b].reshape(-1, 7).numpy(), preds["cls_preds"][b].reshape(-1).numpy(),
                preds["dir_cls_preds"][b].reshape(-1, 2).numpy(), preds["iou_preds"][b].reshape(-1).numpy(), anc, None,
                0.3, nms["nms_pre_max_size"], nms["nms_post_max_size"], nms["nms_iou_threshold"])   # 0.3: the head's own threshold
        r, d = postprocess.predict_frame(*args, return_debug=True)
        d["rerun"] = (lambda a: (lambda forced: postprocess.predict_frame(*a, forced=forced)))(args)
        out.append((r, d))
    return head, out


@pytest.fixture(scope="module")
def setup():
    model = build_model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    head, dets = cpu_chain(sd)
    return model, head, dets


def test_pointpillars_detections_against_the_cpu_chain(setup, dev):
    model, head_ref, want = setup
    counts = [len(r["scores"]) for r, _ in want]
    assert min(counts) >= 5, counts    # the condition the seed was chosen for, on the oracle alone
    model = model.to(dev)
    pts = [torch.from_numpy(f).to(dev) for f in frames()]
    B = len(pts)
    r = ops.voxelize_batch(pts, VSIZE, VRANGE, T, MAX_VOXELS)
    prefix = r["prefix"].cpu().numpy()
    m = int(prefix[B])
    assert 1000 < m <= B * MAX_VOXELS and r["grid"].tolist() == GRID
    anc = torch.from_numpy(anchors()[None]).to(dev).repeat(B, 1, 1)
    example = dict(voxels=r["voxels"][:m], coordinates=r["coors"][:m], num_points=r["num_points"][:m],
                   num_voxels=torch.from_numpy(np.diff(prefix)), shape=[GRID], anchors=[anc],
                   metadata=[dict(token=str(b)) for b in range(B)])
    assert model.reader.on_device_path(example["voxels"])
    with torch.no_grad():
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"], batch_size=B,
                    input_shape=GRID)
        head = model.bbox_head(model.extract_feat(data))[0]["_planar"]
        got = model(example, return_loss=False)
    assert head.shape == head_ref.shape == (B, 22, H, W)
    err, bound = float((head.cpu().double() - head_ref.double()).abs().max()), 2e-4 * float(head_ref.abs().max())
    print("head map vs CPU chain: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert len(got) == B
    for b in range(B):
        mine = dict(box3d_lidar=got[b]["box3d_lidar"].cpu().numpy(), scores=got[b]["scores"].cpu().numpy())
        w, dbg = want[b]
        res = compare_detections(mine, dict(box3d_lidar=w["box3d_lidar"], scores=w["scores"]), dbg, rule="synthetic")
        print("frame %d: %d detections, %d near-threshold NMS decisions" % (b, res["n"], len(res["near_pairs"])))
        assert res["matched"] == res["n"] == counts[b], (b, res)
        assert (got[b]["label_preds"] == 0).all() and got[b]["metadata"]["token"] == str(b)
