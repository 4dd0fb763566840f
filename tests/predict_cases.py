"""One table of predict() edge cases, shared by tests/test_predict_cases_cpu.py (the table's own validity, from the CPU oracle
alone) and tests/test_predict_edges_gpu.py (sessd_hip.ops.predict against the oracle under oracle/compare.py's strict rule).
Imports numpy and the oracle only.

Map: 48 x 44 locations, P = 2112, A = 4224 anchors -- the smallest map whose candidates still need three passes of the 2048-key
sort window of csrc/postprocess.hip (A > 2 * 2048).

Frame construction (make_frame):
  * the candidates are N anchors drawn without order; every other class logit is -30 (sigmoid 1e-13);
  * the candidate of score rank k gets the rectified score 0.70 * (1 - 1.5e-4)**k, through an IoU prediction drawn from
    [0.92, 1] and the class logit that gives this product: neighbouring scores differ by 1.5e-4 relative, a thousand times
    the few ulp a device expf may differ by, so the score order is not in doubt; all sigmoids are >= 0.37, far from the 0.3
    score threshold;
  * ties are the exception: the ranks of a tie group share ONE class logit and ONE IoU prediction bit for bit, so their scores are
    bit-identical on any implementation; the order inside a group must be ascending anchor index (DESIGN.md's tie rule);
  * box codes: "normal" ~ N(0, 0.25) in all seven; "zero" (the decode is then exact: a box sits on its anchor); "big": normal with
    the two plan size codes shifted by +1.5 (boxes 4.5 times the anchor: tens of thousands of stand-up overlaps).
"""
import numpy as np

from oracle import capi, postprocess as pp

FEATURE = (1, 48, 44)
P = FEATURE[1] * FEATURE[2]
A = 2 * P
SCORE_THRESH = 0.3
TOP_SCORE, SCORE_RATIO = 0.70, 1.0 - 1.5e-4
WIDE = (-1e4, -1e4, -1e4, 1e4, 1e4, 1e4)
KITTI_RANGE = (0, -40.0, -5.0, 70.4, 40.0, 5.0)
MAX_NEAR = 6          # the strict rule's cap (oracle/compare.py); never wider


def anchors():
    return pp.create_anchors_3d_range(feature_size=FEATURE).reshape(-1, 7).astype(np.float32)


def _case(name, kind, seed, n, pre_max, post_max, nms_thresh, codes="normal", rng=KITTI_RANGE, ties=None, exact=False,
          short_walk=False, direction_offset=0.0, frustum=False, equal_dir=False, dropped=None):
    """exact: the oracle must report 0 near-threshold decisions (identity is then demanded outright); short_walk: the oracle's walk
    ends with fewer kept boxes than post_max (the whole mask is walked); dropped: for a range case `past` a bound, the anchor
    column / row (axis, value) that the `on` twin keeps and this one drops."""
    return dict(name=name, kind=kind, seed=seed, n=n, pre_max=pre_max, post_max=post_max, nms_thresh=nms_thresh, codes=codes,
                range=tuple(float(v) for v in rng), ties=ties, exact=exact, short_walk=short_walk,
                direction_offset=float(direction_offset), frustum=frustum, equal_dir=equal_dir, dropped=dropped)


# ---- top-k edges: nms_thresh 0.99 on scattered boxes suppresses nothing, the range is wide open, no frustum -- the output is the
# top-k itself, in order. pre_max 256: fused walk, passes after the first take 2048 - 256 = 1792 keys (pass ends at 2048, 3840).
# pre_max 1984 = the limit (2048 - 64): 64 keys per pass after the first (pass ends at 2048, 2112, ...), unfused walk.
TOPK_256_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3840, 3841, 4224)
TOPK_1984_N = (1983, 1984, 1985, 2048, 2049, 2112, 2113, 4224)
TOPK = [_case("topk256_n%d" % n, "topk", 100, n, 256, 256, 0.99, rng=WIDE, exact=True) for n in TOPK_256_N] + \
       [_case("topk1984_n%d" % n, "topk", 101, n, 1984, 1984, 0.99, rng=WIDE, exact=True) for n in TOPK_1984_N]

# ---- ties: 600 bit-identical scores across the pre_max cut (ranks 100 .. 699 against the cut at 256), and across the cut at 1984
# (ranks 1700 .. 2299) where the members also come from different sort passes: with all 4224 anchors as candidates a group of
# 600 has members on both sides of key 2048 of the filter's append order whatever that order is.
TIES = [_case("ties_cut256", "ties", 100, A, 256, 256, 0.99, rng=WIDE, ties=(100, 600), exact=True),
        _case("ties_cut1984", "ties", 101, A, 1984, 1984, 0.99, rng=WIDE, ties=(1700, 600), exact=True)]

# ---- the whole walk: 4224 candidates, (pre_max, post_max, nms_thresh). The walk kernel is chosen by predict_impl's
#   lds = pre_max * ceil(pre_max / 64) * 8 + post_max * 4 + post_max * 36  <=  160 * 1024 - 1024 = 162816   -> fused (mask in LDS)
# (1102, 100): 1102 * 18 * 8 + 4000 = 162688 fused; (1103, 100): 1103 * 18 * 8 + 4000 = 162832 unfused -- the two sides of the switch.
# (1000, 500): 128000 + 20000 fused; (1000, 1000): 168000 unfused; (1024, 1024): 172032 unfused; (1025, 200): 147400 fused;
# 1984: 492032 + ... unfused. 191 * 3 words is odd (the 16-byte staging copy takes one 8-byte word more).
WALK_CFG = [(63, 63, 0.01), (64, 7, 0.1), (65, 65, 0.5), (128, 1, 0.01), (191, 191, 0.1), (1000, 500, 0.01), (1000, 1000, 0.1),
            (1024, 1024, 0.3), (1025, 200, 0.3), (1102, 100, 0.01), (1103, 100, 0.01), (1984, 1984, 0.5), (1984, 100, 0.01)]
# the oracle's walk ends below post_max in these (57, 64, 154, 324, 475, 838 and 1893 kept): the mask is walked to its last block
WALK_SHORT = {(63, 63, 0.01), (65, 65, 0.5), (191, 191, 0.1), (1000, 500, 0.01), (1000, 1000, 0.1), (1024, 1024, 0.3),
              (1984, 1984, 0.5)}
WALK = [_case("walk_%d_%d_%g" % c, "walk", 100, A, c[0], c[1], c[2], short_walk=c in WALK_SHORT) for c in WALK_CFG]

# ---- pair-list overflow: beyond 1024 candidates the pair list of rnms_pairs_kernel holds 64 * pre_max pairs; the rest are
# clipped on the spot. Precondition (test_predict_cases_cpu.py): more stand-up overlaps than that.
OVERFLOW = [_case("overflow_1500", "overflow", 100, A, 1500, 1500, 0.3, codes="big")]


def _f32(v):
    return float(np.float32(v))


def _post_cases():
    """Zero box codes: a box sits exactly on its anchor, so a post_center_range bound set to an anchor column's x (row's y, the
    plane's z) lies ON the centres of that column: kept (the bounds are inclusive); one float32 step past it: dropped."""
    an = pp.create_anchors_3d_range(feature_size=FEATURE)
    xs, ys, z = an[0, 0, :, 0, 0, 0], an[0, :, 0, 0, 0, 1], an[0, 0, 0, 0, 0, 2]
    inf = np.float32(np.inf)
    sides = [(0, xs[10], inf), (1, ys[12], inf), (2, z, inf), (3, xs[30], -inf), (4, ys[40], -inf), (5, z, -inf)]
    out = []
    for side, v, step in sides:
        for past in (False, True):
            r = list(WIDE)
            r[side] = _f32(np.nextafter(np.float32(v), step)) if past else _f32(v)
            out.append(_case("post_range_side%d_%s" % (side, "past" if past else "on"), "post", 100, 600, 512, 512, 0.5, codes="zero",
                             rng=r, exact=True, equal_dir=True, dropped=(side % 3, _f32(v)) if past else None))
    # direction: yaw = anchor rotation (0 or 1.57); at offset 1.57 the second rotation's yaw EQUALS the offset ((yaw - offset) > 0 is
    # false there); a third of the dir logit pairs are equal (label 0: torch.max returns the first maximum)
    for off in (0.0, 1.57, 0.78):
        out.append(_case("post_dir_offset_%g" % off, "post", 100, 600, 512, 512, 0.5, codes="zero", rng=WIDE, exact=True,
                         equal_dir=True, direction_offset=_f32(off)))
    out.append(_case("post_frustum", "post", 100, 600, 512, 512, 0.5, codes="zero", exact=True, equal_dir=True, frustum=True))
    return out


POST = _post_cases()
CASES = TOPK + TIES + WALK + OVERFLOW + POST
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# frames of the batch / workspace-reuse / odd-stride / records / task tests (tests/test_predict_edges_gpu.py): walk-style frames
BATCH = [_case("batch_full", "walk", 102, A, 1000, 100, 0.1), _case("batch_empty", "walk", 103, 0, 1000, 100, 0.1),
         _case("batch_120", "walk", 104, 120, 1000, 100, 0.1)]
BATCH_SHIFT = ((0.0, 0.0), (3.25, -1.5), (-2.0, 4.75))      # per-frame xy shift of the anchors (B, A, 7)
REUSE = [_case("reuse_first_1000", "walk", 105, A, 1000, 100, 0.1), _case("reuse_then_65", "walk", 106, A, 65, 65, 0.5)]
# two frames at pre_max 191: a frame's mask is 191 * 3 = 573 words, so the second frame's mask starts on an odd word (8-byte, not
# 16-byte aligned) under the walk kernel's 16-byte staging copy
ODD = [_case("odd_191_frame0", "walk", 110, A, 191, 191, 0.1, short_walk=True),
       _case("odd_191_frame1", "walk", 111, A, 191, 191, 0.1, short_walk=True)]
TASKS = [_case("task0_capped", "walk", 107, A, 1000, 20, 0.1), _case("task1_empty", "walk", 108, 0, 1000, 20, 0.1),
         _case("task2_some", "walk", 109, 300, 1000, 20, 0.1)]
TASK_SIZES = ((1.6, 3.9, 1.56), (0.6, 0.8, 1.73), (0.6, 1.76, 1.73))


def target_scores(n, ties=None):
    """float64 rectified score of rank k = 0 .. n-1 (descending); a tie group (start, length) repeats its first value."""
    k = np.arange(n, dtype=np.float64)
    if ties is not None:
        s, m = ties
        k = np.where((k >= s) & (k < s + m), float(s), k)
    return TOP_SCORE * SCORE_RATIO ** k


_FRAMES = {}


def make_frame(case):
    """(box_codes (A,7), cls (A,), dir (A,2), iou (A,)) float32, read-only (shared between the tests that use the frame)."""
    key = (case["seed"], case["n"], case["codes"], case["ties"], case["equal_dir"])
    if key in _FRAMES:
        return _FRAMES[key]
    rng = np.random.RandomState(case["seed"])
    n = case["n"]
    cand = rng.permutation(A)[:n]                       # cand[k] = the anchor of score rank k, in no order
    box = rng.normal(0, 0.25, (A, 7)).astype(np.float32)
    if case["codes"] == "zero":
        box[:] = 0
    elif case["codes"] == "big":
        box[:, 3:5] += np.float32(1.5)
    dirl = rng.normal(0, 1.0, (A, 2)).astype(np.float32)
    if case["equal_dir"]:
        dirl[::3, 1] = dirl[::3, 0]
    iou = rng.uniform(-0.2, 1.0, A).astype(np.float32)
    cls = np.full(A, -30.0, np.float32)
    if n:
        ci = rng.uniform(0.92, 1.0, n).astype(np.float32)
        if case["ties"] is not None:
            s, m = case["ties"]
            ci[s:s + m] = ci[s]
        r = ((ci + np.float32(1)) * np.float32(0.5)).astype(np.float32)
        r4 = (r * r * r * r).astype(np.float64)
        sig = target_scores(n, case["ties"]) / r4
        assert sig.max() < 0.95 and sig.min() > 0.35
        cls[cand] = np.log(sig / (1.0 - sig)).astype(np.float32)
        iou[cand] = ci
    frame = (box, cls, dirl, iou)
    for a in frame:
        a.flags.writeable = False
    _FRAMES[key] = frame
    return frame


def pack_head(frame):
    """(box (A,7), cls (A,), dir (A,2), iou (A,)) -> the planar (22, P) head tensor predict() reads: channel a * 7 + q = code q of
    rotation a, 14 + a = class logit, 16 + 2 a + k = dir logit k, 20 + a = IoU prediction; anchor = 2 * location + a."""
    box, cls, dirl, iou = frame
    head = np.empty((22, P), np.float32)
    head[:14] = box.reshape(P, 2, 7).transpose(1, 2, 0).reshape(14, P)
    head[14:16] = cls.reshape(P, 2).T
    head[16:20] = dirl.reshape(P, 2, 2).transpose(1, 2, 0).reshape(4, P)
    head[20:22] = iou.reshape(P, 2).T
    return head


def split_head(head):
    """The inverse of pack_head (what the oracle takes)."""
    box = head[:14].reshape(2, 7, P).transpose(2, 0, 1).reshape(-1, 7)
    cls = head[14:16].T.reshape(-1)
    dirl = head[16:20].reshape(2, 2, P).transpose(2, 0, 1).reshape(-1, 2)
    iou = head[20:22].T.reshape(-1)
    return box, cls, dirl, iou


def kitti_frustum(calib):
    """calib: dict(rect, Trv2c, P2, image_shape) (sessd_hip.synth.kitti_calib()) -> (1,6,4,3) float64 surfaces."""
    return pp.get_valid_frustum(calib["rect"], calib["Trv2c"], calib["P2"], calib["image_shape"])


_ORACLE = {}


def run_oracle(case, frustum=None, anchors_=None, cache=True):
    """(want, dbg) of pp.predict_frame for the case, dbg['rerun'] set the way oracle/pipeline.py does. Computed once per case."""
    key = case["name"] if (cache and anchors_ is None) else None
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    box, cls, dirl, iou = make_frame(case)
    an = anchors() if anchors_ is None else anchors_
    args = (box, cls, dirl, iou, an, frustum if case["frustum"] else None, SCORE_THRESH, case["pre_max"], case["post_max"],
            case["nms_thresh"], case["range"], case["direction_offset"])
    want, dbg = pp.predict_frame(*args, return_debug=True)
    dbg["rerun"] = (lambda a: (lambda forced: pp.predict_frame(*a, forced=forced)))(args)
    if key is not None:
        _ORACLE[key] = (want, dbg)
    return want, dbg


def rectified_scores(frame):
    """The oracle's float32 rectified score of every anchor and the candidate mask (score filter of predict_frame)."""
    _, cls, _, iou = frame
    sg = pp.sigmoid32(cls)
    r = ((iou + np.float32(1)) * np.float32(0.5)).astype(np.float32)
    return (sg * (r * r * r * r)).astype(np.float32), sg >= np.float32(SCORE_THRESH), sg


def standup_overlap_pairs(cand_dets):
    """Number of pairs i < j of the oracle's NMS candidates (K,6) whose stand-up boxes overlap with positive area, in float32 like
    the prefilter (box_np_ops.py:1007-1045 iou_jit, eps = 0)."""
    c = capi.box2d_corners(cand_dets)
    x0, x1, y0, y1 = c[:, :, 0].min(1), c[:, :, 0].max(1), c[:, :, 1].min(1), c[:, :, 1].max(1)
    total = 0
    for i0 in range(0, len(c), 256):
        s = slice(i0, i0 + 256)
        iw = np.minimum(x1[s, None], x1[None]) - np.maximum(x0[s, None], x0[None])
        ih = np.minimum(y1[s, None], y1[None]) - np.maximum(y0[s, None], y0[None])
        upper = np.arange(len(c))[None] > np.arange(i0, min(i0 + 256, len(c)))[:, None]
        total += int(((iw > 0) & (ih > 0) & upper).sum())
    return total
