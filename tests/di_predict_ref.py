"""TEST INFRASTRUCTURE ONLY -- numpy restatement of get_task_detections with nms_type = 'rotate_weighted_nms' (DI-NMS) for ONE
(frame, task), the CPU reference of sessd_predict with args->di / ops.predict(nms_type="rotate_weighted_nms").

Follows, line by line:
  det3d/models/bbox_heads/mg_head_sessd.py:955-982    sigmoid, >= thresh, iou_preds = (iou + 1) / 2, score *= iou_preds^4
  det3d/models/bbox_heads/mg_head_sessd.py:999-1018   rotate_weighted_nms(box, box[:, [0,1,3,4,6]], dirs, labels, scores,
                                                      iou_preds[keep], anchors[keep], enable_centerness=True, centerness_pow=2, ...)
  det3d/core/bbox/box_torch_ops.py:571-586            topk(pre_max), score *= (1 - softmax(|xy - anchor xy|))^pow
  det3d/ops/nms/nms_cpu.py:52-93                      corners, stand-up boxes, iou_jit(eps=0), centerness_c = 0
  det3d/ops/nms/nms_cpu.h:173-384                     the core = oracle.capi.di_nms_core (oracle/di_nms.c)
  det3d/models/bbox_heads/mg_head_sessd.py:1024-1045  frustum, direction fix, centre-range mask -- on the AVERAGED boxes
built from oracle.postprocess (sigmoid32, second_box_decode, points_in_frustum), the numpy helpers of the det3d mirror the DI-NMS
tests use (center_to_corner_box2d, corner_to_standup_nd, iou_jit) and oracle.capi.di_nms_core.

Two stated deviations of the device path, restated here: the anchors are the task's own, and the keep list is cut at post_max
before the filters (the reference wrapper ignores post_max_size). `truncated` = the selection loop, stopped at post_max kept
boxes, would have had an unsuppressed candidate left. The loop's pass accounting (which passes were kept, what was left) comes
from `replay`, a plain numpy walk of the same loop over the pairwise overlaps; it must reproduce the core's keep list."""
import numpy as np

from oracle import capi
from oracle import postprocess as pp

DI_DEFAULTS = dict(nms_cnt_thresh=2.6, nms_sigma_dist_interval=(0, 20, 40, 60), nms_sigma_square=(0.0009, 0.009, 0.1, 1),
                   suppressed_thresh=0.3, centerness_pow=2)   # mg_head_sessd.py:1012-1017


def candidates(box_codes, cls_logits, dir_logits, iou_preds, anchors, score_thresh, pre_max):
    """mg_head_sessd.py:955-982 + the topk of box_torch_ops.py:571-580 (ties by ascending anchor index, the project's rule):
    dict(box (k,7), score, iou_pred, dir, anchor_xy, anchor_id), k <= pre_max, in descending (undamped) score order."""
    boxes = pp.second_box_decode(box_codes, anchors)
    dir_labels = (dir_logits[:, 1] > dir_logits[:, 0]).astype(np.int64)
    scores = pp.sigmoid32(cls_logits)
    idx = np.nonzero(scores >= np.float32(score_thresh))[0]
    ioup = ((np.asarray(iou_preds, np.float32)[idx] + np.float32(1)) * np.float32(0.5)).astype(np.float32)
    s = (scores[idx] * (ioup * ioup * ioup * ioup)).astype(np.float32)
    order = np.lexsort((idx, -s.astype(np.float64)))[:min(len(idx), pre_max)]
    sel = idx[order]
    return dict(box=boxes[sel], score=s[order], iou_pred=ioup[order], dir=dir_labels[sel],
                anchor_xy=np.asarray(anchors, np.float32)[sel, :2], anchor_id=sel)


def damped_scores(c, centerness_pow=2, dtype=np.float32):
    """box_torch_ops.py:582-586 in `dtype` (float32 = the reference; float64 for the near-tie precondition of the tests)."""
    if len(c["score"]) == 0:
        return np.zeros((0,), np.float32)
    d = np.abs(c["box"][:, :2].astype(dtype) - c["anchor_xy"].astype(dtype))
    dist = np.sqrt((d * d).sum(-1, dtype=dtype)).astype(dtype)
    e = np.exp(dist - dist.max()).astype(dtype)
    m = (e / e.sum(dtype=dtype)).astype(dtype)
    one = dtype(1) - m
    w = one * one if centerness_pow == 2 else np.power(one, dtype(centerness_pow))
    return (c["score"].astype(dtype) * w).astype(np.float32)


def footprints(box):
    from det3d.core.bbox import box_np_ops
    dets = np.ascontiguousarray(box[:, [0, 1, 3, 4, 6]], np.float32)
    corners = box_np_ops.center_to_corner_box2d(dets[:, :2], dets[:, 2:4], dets[:, 4]).astype(np.float32)
    standup = box_np_ops.corner_to_standup_nd(corners)
    return corners, box_np_ops.iou_jit(standup, standup, eps=0.0).astype(np.float32)


def replay(scores, iou_pred, corners, sio, cnt_thresh, suppressed_thresh, post_max=None):
    """The loop of nms_cpu.h:264-384 for one label, pass accounting only: (keep, number of passes that were not kept, left) --
    left = an unsuppressed candidate remained when the loop stopped at post_max kept boxes (False when it ran out). Overlaps
    only where the stand-up IoU is > 0 (elsewhere the footprints cannot intersect)."""
    n = len(scores)
    ov = np.zeros((n, n), np.float32)
    for i, j in zip(*np.nonzero(sio > 0)):
        ov[i, j] = np.float32(capi.quad_iou(corners[i], corners[j]))
    sup = np.zeros(n, bool)
    keep, unkept = [], 0
    while True:
        if post_max is not None and len(keep) >= post_max:
            return keep, unkept, bool((~sup & (scores > -1)).any())
        live = np.nonzero(~sup & (scores > -1))[0]
        if len(live) == 0:
            return keep, unkept, False
        a = live[np.argmax(scores[live])]   # first maximum = lowest index on ties
        sup[a] = True
        cnt = np.float32(0)
        for j in np.nonzero(ov[a] > 0)[0]:   # box order, float32 (nms_cpu.h: cnt += overlap * iou_pred[j])
            cnt = np.float32(cnt + np.float32(ov[a, j] * iou_pred[j]))
        new = ~sup & (sio[a] > 0) & (ov[a] >= np.float32(suppressed_thresh)) & (ov[a] > 0)
        if cnt > np.float32(cnt_thresh):
            sup |= new
            keep.append(int(a))
        else:
            unkept += 1


def select(c, post_max=100, di=None, score_dtype=np.float32, with_replay=True):
    """box_torch_ops.py:582-621 on the candidates `c` (candidates()' layout, already the top-k in descending score order): damped
    scores, footprints, the core, the keep list cut at post_max. Returns dict(keep (candidate ranks), truncated, full_keep,
    unkept_passes, damped, core = dict(box, score, dir) of the kept boxes) -- before the filters of :1024-1045."""
    d = dict(DI_DEFAULTS)
    d.update(di or {})
    n = len(c["score"])
    if n == 0:   # box_torch_ops.py:600-601
        z = np.zeros((0,), np.float32)
        return dict(keep=[], truncated=0, full_keep=[], unkept_passes=0, damped=z,
                    core=dict(box=np.zeros((0, 7), np.float32), score=z, dir=np.zeros((0,), np.int64)))
    s = damped_scores(c, d["centerness_pow"], score_dtype)
    corners, sio = footprints(c["box"])
    with np.errstate(all="ignore"):
        core = capi.di_nms_core(c["box"], corners, sio, 0.5, s, c["iou_pred"], np.zeros(n, np.int32), c["dir"].astype(np.int32),
                                np.zeros((1, 1)), d["nms_cnt_thresh"], d["nms_sigma_dist_interval"], d["nms_sigma_square"],
                                d["suppressed_thresh"], 0)
    full_keep = [int(k) for k in core[4]]
    unkept, left = 0, len(full_keep) > post_max
    if with_replay:
        rk, unkept, left = replay(s, c["iou_pred"], corners, sio, d["nms_cnt_thresh"], d["suppressed_thresh"], post_max)
        assert rk == full_keep[:post_max], "the numpy walk of the loop and the core disagree"
    nk = min(len(full_keep), post_max)
    return dict(keep=full_keep[:nk], truncated=int(left), full_keep=full_keep, unkept_passes=unkept, damped=s,
                core=dict(box=np.asarray(core[0], np.float32).reshape(-1, 7)[:nk], score=np.asarray(core[1], np.float32)[:nk],
                          dir=np.asarray(core[3], np.int64)[:nk]))


def predict_task(box_codes, cls_logits, dir_logits, iou_preds, anchors, frustum=None, score_thresh=0.3, pre_max=1000, post_max=100,
                 di=None, post_center_range=(0, -40.0, -5.0, 70.4, 40.0, 5.0), direction_offset=0.0, score_dtype=np.float32,
                 with_replay=True):
    """One (frame, task). Returns select()'s dict + box3d_lidar, scores, label_preds (after the filters), n_top, cand."""
    c = candidates(box_codes, cls_logits, dir_logits, iou_preds, anchors, score_thresh, pre_max)
    out = select(c, post_max, di, score_dtype, with_replay)
    out.update(n_top=len(c["score"]), cand=c, box3d_lidar=np.zeros((0, 7), np.float32), scores=np.zeros((0,), np.float32),
               label_preds=np.zeros((0,), np.int64))
    b, sc, dl = out["core"]["box"], out["core"]["score"], out["core"]["dir"]
    if frustum is not None and len(b):
        m = pp.points_in_frustum(b[:, :3], frustum)
        b, sc, dl = b[m], sc[m], dl[m]
    if len(b) == 0:
        return out
    opp = ((b[:, 6] - np.float32(direction_offset)) > 0) ^ (dl == 1)
    b = b.copy()
    b[:, 6] = b[:, 6] + np.where(opp, np.float32(np.pi), np.float32(0.0)).astype(np.float32)
    pr = np.array(post_center_range, np.float32)
    m = (b[:, :3] >= pr[:3]).all(1) & (b[:, :3] <= pr[3:]).all(1)
    out.update(box3d_lidar=b[m], scores=sc[m], label_preds=np.zeros((int(m.sum()),), np.int64))
    return out
