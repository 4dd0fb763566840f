"""TEST INFRASTRUCTURE ONLY -- the SECOND-style RPN neck of the three-class config (det3d/models/necks/rpn_v1.py:23-116 with
layer_nums=[n], strides 1) in plain torch CPU ops on a state dict with the reference's key names, and the CPU pipeline of one
frame and ONE task around it, composed from the oracle's existing pieces.

  rpn_forward     blocks.0.{1,2} (ZeroPad2d(1) + unpadded 3x3 == F.conv2d pad 1), blocks.0.{4,5} ... (F.conv2d pad 1), each +
                  F.batch_norm (running statistics, eps 1e-3) + ReLU; deblocks.0.{0,1}: F.conv_transpose2d stride 1 + BN + ReLU
                  -- the torch ops the reference's modules call. tests/test_rpn_mirror_cpu.py holds it to the golden output of the
                  reference's own class (tests/golden/rpn_ref.npz).
  run_frame_task  oracle.capi.points_to_voxel / vfe_mean -> oracle.sparse_conv.spmiddle_fhd -> rpn_forward ->
                  oracle.dense_head.head_forward(prefix = task t) -> oracle.postprocess.predict_frame(return_debug=True) with the
                  `rerun` closure oracle/pipeline.py builds (what oracle.compare.compare_detections needs)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import capi, dense_head, postprocess, sparse_conv
from oracle.pipeline import split_state_dict

EPS = 1e-3  # rpn_v1.py:36 norm_cfg = dict(type="BN", eps=1e-3, momentum=0.01)


def _bn_relu(x, sd, p):
    return torch.relu(F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS))


def rpn_forward(x, sd, prefix="neck."):
    """x (B, C, H, W) -> the neck's output; sd: reference-keyed state dict (any float dtype, the same as x)."""
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    assert not any(k.startswith(("blocks.1.", "deblocks.1.")) for k in sd), "one block, one up-sampler"
    ci = 1
    while "blocks.0.%d.weight" % ci in sd:
        x = _bn_relu(F.conv2d(x, sd["blocks.0.%d.weight" % ci], None, stride=1, padding=1), sd, "blocks.0.%d" % (ci + 1))
        ci += 3
    assert ci > 1
    w = sd["deblocks.0.0.weight"]   # ConvTranspose2d weight (cin, cout, 1, 1)
    return _bn_relu(F.conv_transpose2d(x, w, None, stride=1), sd, "deblocks.0.1")


def run_frame_task(points, sd, task, voxel_range, voxel_size, max_points, max_voxels, anchors, test_cfg=None, shared=None):
    """One frame, one task: (detections, dict(bev, neck, preds, debug)). `shared`: a dict that keeps the task-independent part
    (voxels -> BEV map -> neck output) between calls on the same frame and weights."""
    tc = dict(score_thresh=0.3, pre_max=1000, post_max=100, nms_thresh=0.01)
    if test_cfg:
        tc.update(test_cfg)
    if shared is None or "neck" not in shared:
        grid = np.round((np.array(voxel_range[3:], np.float32) - np.array(voxel_range[:3], np.float32)) / np.array(voxel_size, np.float32)).astype(np.int64)
        v, c, n = capi.points_to_voxel(points, voxel_size, voxel_range, max_points, max_voxels)
        feats = torch.from_numpy(capi.vfe_mean(v, n, 4))
        coors = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
        convs, bns = split_state_dict(sd)
        bev = sparse_conv.spmiddle_fhd(feats, coors, 1, [int(g) for g in grid], convs, bns)
        neck = rpn_forward(bev, {k: v.float() for k, v in sd.items() if k.startswith("neck.")})
        if shared is not None:
            shared.update(bev=bev, neck=neck)
    else:
        bev, neck = shared["bev"], shared["neck"]
    preds = dense_head.head_forward(neck, sd, prefix="bbox_head.tasks.%d." % task)
    box = preds["box_preds"][0].reshape(-1, 7).numpy()
    cls = preds["cls_preds"][0].reshape(-1).numpy()
    dirl = preds["dir_cls_preds"][0].reshape(-1, 2).numpy()
    iou = preds["iou_preds"][0].reshape(-1).numpy()
    args = (box, cls, dirl, iou, anchors, None, tc["score_thresh"], tc["pre_max"], tc["post_max"], tc["nms_thresh"])
    r, d = postprocess.predict_frame(*args, return_debug=True)
    d["rerun"] = (lambda a: (lambda forced: postprocess.predict_frame(*a, forced=forced)))(args)
    return r, dict(bev=bev, neck=neck, preds=preds, debug=d)
