"""Generates tests/golden/di_predict_ref.npz: the REFERENCE's DI-NMS wrappers run from source on CPU with the literal arguments
of get_task_detections (det3d/models/bbox_heads/mg_head_sessd.py:1002-1018):

  rotate_weighted_nms(box_preds, box_preds[:, [0, 1, 3, 4, -1]], dir_labels, top_labels, top_scores, iou_preds, anchors,
                      pre_max_size=, post_max_size=, iou_threshold=, enable_centerness=True, centerness_pow=2, nms_cnt_thresh=2.6,
                      nms_sigma_dist_interval=(0, 20, 40, 60), nms_sigma_square=(0.0009, 0.009, 0.1, 1), suppressed_thresh=0.3)

  det3d/core/bbox/box_torch_ops.py:552-621  rotate_weighted_nms   (topk, softmax centerness damping, assembly of the outputs)
  det3d/ops/nms/nms_cpu.py:52-93            rotate_weighted_nms_cc (footprint corners, stand-up boxes, iou_jit)

on a few seeded candidate sets (one label: a task has one class). As in make_golden_di_nms.py the pybind core (boost::geometry)
is substituted by oracle.capi.di_nms_core and `.cuda()` is neutralised by the stubs of make_golden_head_loss.install. The
fixture holds data only: the candidate sets as fed and the five returned arrays.

    python tests/golden/make_golden_di_predict.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
sys.path.insert(0, HERE)

# n candidates in `clusters` groups; pre = nms_pre_max_size (binding for case 1: top-k cut), post = nms_post_max_size (ignored by
# the reference wrapper)
CASES = [dict(seed=21, n=260, clusters=14, pre=1000, post=100), dict(seed=22, n=300, clusters=10, pre=120, post=100),
         dict(seed=23, n=90, clusters=3, pre=1000, post=100), dict(seed=24, n=1, clusters=1, pre=1000, post=100)]


def make_case(seed, n, clusters):
    """make_golden_di_nms.make_case with ONE label: boxes around `clusters` objects, anchors near them, distinct scores."""
    from make_golden_di_nms import make_case as base
    box, anchors, scores, iou_preds, labels, dirs = base(seed, n=n, clusters=clusters)
    return box, anchors, scores, iou_preds, np.zeros_like(labels), dirs


def main():
    warnings.filterwarnings("ignore")
    from oracle import capi
    import make_golden_head_loss as HL
    assert os.path.isdir(HL.REF), "the reference tree is needed to regenerate this fixture"
    HL.install(capi)
    mod, load_as = HL.mod, HL.load_as
    mod("det3d.ops"); mod("det3d.ops.nms")
    mod("det3d.ops.nms.nms", non_max_suppression_cpu=None, rotate_non_max_suppression_cpu=None,
        IOU_weighted_rotate_non_max_suppression_cpu=capi.di_nms_core)
    nms_cpu = load_as("det3d/ops/nms/nms_cpu.py", "det3d.ops.nms.nms_cpu")
    nms_cpu.IOU_weighted_rotate_non_max_suppression_cpu = capi.di_nms_core
    bto = sys.modules["det3d.core.bbox.box_torch_ops"]
    bto.rotate_weighted_nms_cc = nms_cpu.rotate_weighted_nms_cc
    out = {}
    for ci, c in enumerate(CASES):
        box, anchors, scores, iou_preds, labels, dirs = make_case(c["seed"], c["n"], c["clusters"])
        for nm, v in zip(("box", "anchors", "scores", "iou_preds", "dirs"), (box, anchors, scores, iou_preds, dirs)):
            out["c%d_in_%s" % (ci, nm)] = v
        T = lambda a: torch.from_numpy(a.copy())
        box_preds = T(box)
        res = bto.rotate_weighted_nms(box_preds, box_preds[:, [0, 1, 3, 4, -1]], T(dirs), T(labels), T(scores), T(iou_preds), T(anchors),
                                      pre_max_size=c["pre"], post_max_size=c["post"], iou_threshold=0.01, enable_centerness=True,
                                      centerness_pow=2, nms_cnt_thresh=2.6, nms_sigma_dist_interval=(0, 20, 40, 60),
                                      nms_sigma_square=(0.0009, 0.009, 0.1, 1), suppressed_thresh=0.3)
        for nm, v in zip(("boxes", "dirs", "labels", "scores", "selected"), res):
            v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            out["c%d_%s" % (ci, nm)] = v
        print("case", ci, c, "kept", len(out["c%d_selected" % ci]))
    path = os.path.join(HERE, "di_predict_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
