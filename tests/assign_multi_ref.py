"""TEST INFRASTRUCTURE ONLY -- the per-task CPU reference of the batched multi-task target assignment: oracle.assign_target.assign
on the rows of a frame that belong to a task, with that task's thresholds, as det3d/core/anchor/target_assigner.py:89-119
(assign_v2) runs create_target_np per class. Plus the loader of tests/golden/assign_multi_ref.npz (the reference's own
create_target_np run from source, tests/golden/make_golden_assign_multi.py)."""
import os

import numpy as np

from oracle import assign_target as oat, postprocess as pp

FRAMES = "abcdefgh"


def assign_task(anchors, gt_boxes, gt_classes, class_id, matched, unmatched):
    """One (frame, task): rows with gt_classes == class_id (every row when class_id <= 0 or gt_classes is None), labels 1.
    Returns dict(labels (A,) int32, reg_targets (A, 7), reg_weights (A,), gt_id (A,) int32 dense, positive_gt_id (P,))."""
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 7)
    rows = np.ones(len(gt_boxes), bool) if gt_classes is None or class_id <= 0 else np.asarray(gt_classes) == class_id
    r = oat.assign(anchors, gt_boxes[rows], None, matched, unmatched)
    gid = np.full(anchors.shape[0], -1, np.int32)
    # the foreground set of the reference (taken before the background pass) is labels > 0 whenever matched >= unmatched
    assert int((r["labels"] > 0).sum()) == len(r["positive_gt_id"])
    gid[r["labels"] > 0] = r["positive_gt_id"]
    return dict(labels=r["labels"], reg_targets=r["bbox_targets"], reg_weights=r["bbox_outside_weights"], gt_id=gid,
                positive_gt_id=r["positive_gt_id"])


def assign_tasks(tasks, gt_boxes, gt_classes=None):
    """tasks: list of dict(anchors (A, 7) numpy, class_id, matched_threshold, unmatched_threshold) -> list of assign_task results"""
    return [assign_task(t["anchors"], gt_boxes, gt_classes, t["class_id"], t["matched_threshold"], t["unmatched_threshold"])
            for t in tasks]


class Golden:
    """One config of the golden file: `tasks` (anchors rebuilt from the stored ranges, class_id = 1 + index of the task's name
    in the file's `names`, thresholds) and per frame gt / classes / the reference's results."""

    def __init__(self, golden_dir, key):
        g = np.load(os.path.join(golden_dir, "assign_multi_ref.npz"))
        self.g, self.key = g, key
        names = [str(n) for n in g["names"]]
        self.fmap = tuple(int(v) for v in g[key + "_feature_map"])
        self.tasks = []
        for t, n in enumerate(g[key + "_task_names"]):
            a = pp.create_anchors_3d_range(self.fmap, g["%s_range%d" % (key, t)], g["%s_sizes%d" % (key, t)],
                                           g["%s_rotations%d" % (key, t)]).reshape(-1, 7).astype(np.float32)
            assert np.allclose(a.astype(np.float64).sum(0), g["%s_anchors_checksum%d" % (key, t)], rtol=0, atol=1e-3)
            m, u = g[key + "_thresholds"][t]
            self.tasks.append(dict(anchors=a, class_id=names.index(str(n)) + 1, matched_threshold=float(m), unmatched_threshold=float(u)))
        self.A = self.tasks[0]["anchors"].shape[0]

    def frame(self, f):
        """(gt (M, 7), classes (M,) int32 = 1 + name index)"""
        return self.g["%s_%s_gt" % (self.key, f)], self.g["%s_%s_codes" % (self.key, f)].astype(np.int32) + 1

    def want(self, f, t):
        p = "%s_%s_t%d_" % (self.key, f, t)
        return {k: self.g[p + k] for k in ("labels", "pos", "targets_pos", "gt_id")}

    def check(self, f, t, labels, reg_targets, reg_weights, gt_id):
        """a (frame, task) result against the reference run: labels, positive set and ids identical, targets within 1e-6 at the
        positives and exactly 0 elsewhere, weights = labels > 0 (the rule of tests/test_assign_target_gpu.py)"""
        w = self.want(f, t)
        labels = np.asarray(labels)
        assert np.array_equal(labels, w["labels"].astype(labels.dtype)), (self.key, f, t)
        pos = np.nonzero(labels > 0)[0]
        assert np.array_equal(pos, w["pos"]), (self.key, f, t)
        if len(pos):
            assert np.abs(reg_targets[pos] - w["targets_pos"]).max() < 1e-6, (self.key, f, t)
        assert np.all(reg_targets[labels <= 0] == 0), (self.key, f, t)
        if gt_id is not None:
            assert np.array_equal(gt_id[gt_id >= 0], w["gt_id"]) and np.array_equal(np.nonzero(gt_id >= 0)[0], pos), (self.key, f, t)
        if reg_weights is not None:
            assert np.array_equal(reg_weights, (labels > 0).astype(np.float32)), (self.key, f, t)
