"""The detection parity rule itself (oracle/compare.py) on the oracle's own NMS problems: identical selections pass; a missing /
moved / re-scored box fails when there is no near-threshold decision; a difference is accepted only if it is exactly what the
oracle produces with its LISTED near-threshold decisions taken the other way; too many marginal decisions are rejected.
Also pins the `forced` / `pairs` entry points of oracle/rotate_nms.c to the plain one."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import forward_cases as FC  # noqa: E402
from oracle import capi, postprocess as pp  # noqa: E402
from oracle.compare import compare_detections, same_detections  # noqa: E402


@pytest.fixture(scope="module")
def frame():
    pc = FC.predict_case(21)
    anchors = pp.create_anchors_3d_range().reshape(-1, 7).astype(np.float32)
    args = (pc["box_preds"][0].reshape(-1, 7), pc["cls_preds"][0].reshape(-1), pc["dir_cls_preds"][0].reshape(-1, 2),
            pc["iou_preds"][0].reshape(-1), anchors, None)
    out, dbg = pp.predict_frame(*args, return_debug=True)
    dbg["rerun"] = lambda forced: pp.predict_frame(*args, forced=forced)
    return out, dbg


def _drop(d, i):
    return {k: np.delete(v, i, axis=0) for k, v in d.items()}


def test_identical_passes_and_any_change_fails_without_near_pairs(frame):
    out, dbg = frame
    d0 = dict(dbg, near_threshold_pairs=0, near_pairs=np.zeros((0, 2), np.int64))
    r = compare_detections(out, out, d0)
    assert r["matched"] == r["n"] == len(out["scores"]) > 20 and r["flipped"] == []
    with pytest.raises(AssertionError):
        compare_detections(_drop(out, 5), out, d0)
    moved = copy.deepcopy(out)
    moved["box3d_lidar"][3, 0] += 0.05
    with pytest.raises(AssertionError):
        compare_detections(moved, out, d0)
    rescored = copy.deepcopy(out)
    rescored["scores"][2] *= 1.01
    with pytest.raises(AssertionError):
        compare_detections(rescored, out, d0)
    swapped = copy.deepcopy(out)
    for k in swapped:
        swapped[k][[0, 1]] = swapped[k][[1, 0]]
    assert same_detections(swapped, out) is not None  # order matters


def test_only_the_outcome_of_a_flipped_listed_decision_is_accepted(frame):
    out, dbg = frame
    kept = np.asarray(dbg["nms_kept_rows"])
    dets = dbg["cand_dets"]
    # a pair the oracle really evaluated: kept row i and a lower-scored candidate j it suppresses
    # (most flips change nothing: in a cluster the candidate is suppressed by the next kept box anyway -- take one that matters)
    corners = capi.box2d_corners(dets)
    i = j = alt = None
    for i in kept[:10].tolist():
        for c in range(i + 1, len(dets)):
            if c in set(kept.tolist()) or capi.quad_iou(corners[i], corners[c]) < 0.01:
                continue
            cand = dbg["rerun"](np.array([[i, c, 0]], np.int32))  # the decision taken the other way: c survives row i
            if same_detections(cand, out) is not None:
                j, alt = c, cand
                break
        if alt is not None:
            break
    assert alt is not None
    d1 = dict(dbg, near_threshold_pairs=1, near_pairs=np.array([[i, j]]))
    r = compare_detections(alt, out, d1)   # exactly the flipped outcome: accepted, and the flip is reported
    assert r["flipped"] == [(i, j, 0)]
    assert compare_detections(out, out, d1)["flipped"] == []
    # anything else is not
    with pytest.raises(AssertionError):
        compare_detections(_drop(out, 7), out, d1)
    with pytest.raises(AssertionError):
        compare_detections(_drop(alt, 2), out, d1)
    # without the rerun hook a difference cannot be excused
    with pytest.raises(AssertionError):
        compare_detections(alt, out, {k: v for k, v in d1.items() if k != "rerun"})


def test_too_many_marginal_decisions_are_rejected(frame):
    out, dbg = frame
    K = dbg["cand_dets"].shape[0]
    pairs = np.stack([np.arange(0, 9), np.arange(1, 10)], 1)
    d2 = dict(dbg, near_threshold_pairs=len(pairs), near_pairs=pairs)
    with pytest.raises(AssertionError):
        compare_detections(_drop(out, 1), out, d2)


def test_pairs_and_forced_entry_points_equal_the_plain_one():
    from sessd_hip import synth
    d = synth.clustered_boxes7(300, seed=9)[:, [0, 1, 3, 4, 6]].astype(np.float32)
    d = np.concatenate([d, np.linspace(0.95, 0.3, 300, dtype=np.float32)[:, None]], 1)
    k0, n0 = capi.rotate_nms_cc(d, 0.01, margin=5e-3)
    k1, n1, pairs = capi.rotate_nms_cc(d, 0.01, margin=5e-3, return_pairs=True)
    k2, n2, _ = capi.rotate_nms_cc(d, 0.01, margin=5e-3, forced=np.zeros((0, 3), np.int32))
    assert np.array_equal(k0, k1) and np.array_equal(k0, k2) and n0 == n1 == n2 == len(pairs)
    for i, j in pairs:
        iou = capi.quad_iou(capi.box2d_corners(d[i:i + 1])[0], capi.box2d_corners(d[j:j + 1])[0])
        assert abs(iou - 0.01) < 5e-3 and i in set(k1.tolist())
    # forcing a decision to what it already is changes nothing; forcing it the other way changes the kept list
    i, j = int(k0[0]), None
    for c in range(i + 1, 300):
        if c not in set(k0.tolist()) and capi.quad_iou(capi.box2d_corners(d[i:i + 1])[0], capi.box2d_corners(d[c:c + 1])[0]) >= 0.01:
            j = c
            break
    assert j is not None
    same, _, _ = capi.rotate_nms_cc(d, 0.01, forced=np.array([[i, j, 1]], np.int32))
    flip, _, _ = capi.rotate_nms_cc(d, 0.01, forced=np.array([[i, j, 0]], np.int32))
    assert np.array_equal(same, k0) and not np.array_equal(flip, k0)


def test_box_tolerance_is_absolute_for_the_pose_and_relative_for_large_sizes():
    """Centres and yaw: 2e-3 absolute. Sizes under rule "synthetic": 2e-3 * max(1, size) -- a size is exp(code) * anchor size, so
    the float32 error of the network output is a RELATIVE error of the size (the random benchmark weights decode boxes of
    kilometres); under the DEFAULT rule "strict" (real KITTI weights) sizes are absolute like the pose."""
    want = dict(box3d_lidar=np.array([[10.0, -3.0, -1.0, 1.6, 3.9, 1.5, 0.3], [19.2, -14.8, -1.2, 5946.9, 0.236, 26.578, 3.97]], np.float32),
                scores=np.array([0.9, 0.5], np.float32))
    ok = copy.deepcopy(want)
    ok["box3d_lidar"][1, 3] = 5950.8   # 6.6e-4 relative: the case bench.py's parity gate found
    ok["box3d_lidar"][0, 4] += 1.5e-3  # within 2e-3 * max(1, 3.9)
    assert same_detections(ok, want, relative_sizes=True) is None
    assert same_detections(ok, want) is not None                 # the strict default does not excuse the kilometre box
    dbg = dict(near_pairs=np.zeros((0, 2), np.int64))
    assert compare_detections(ok, want, dbg, rule="synthetic")["rule"] == "synthetic"
    with pytest.raises(AssertionError):
        compare_detections(ok, want, dbg)                        # rule="strict"
    for row, col, delta in ((0, 0, 3e-3), (1, 1, 3e-3), (0, 3, 5e-3), (1, 3, 20.0), (1, 4, 3e-3), (0, 6, 3e-3)):
        bad = copy.deepcopy(want)
        bad["box3d_lidar"][row, col] += delta
        assert same_detections(bad, want, relative_sizes=True) is not None, (row, col)
        assert same_detections(bad, want) is not None, (row, col)
    # centres under the synthetic rule (round 6): box_tol + code_rtol * code_scale * anchor size PER FRAME, code_scale = the largest
    # |x / y / z code| of the frame's head output as the ORACLE computed it -- a box code's float32 error reaches the centre times
    # the 4.2 m anchor diagonal (z: the 1.56 m anchor height) and is proportional to the scale of the head output. A frame with
    # tame codes keeps ~2 mm; the strict rule never takes the code term.
    from oracle.compare import RULES, ANCHOR_CENTRE_SCALE
    rt = RULES["synthetic"]["code_rtol"]
    assert rt == 5e-5 and RULES["strict"]["code_rtol"] == 0.0
    wild, tame = 18.5, 0.8    # code scale of a frame of the random benchmark weights / of a trained model
    for col in (0, 1, 2):
        big = 2e-3 + rt * 18.5 * ANCHOR_CENTRE_SCALE[col]    # 5.9 mm (x, y) / 3.4 mm (z)
        off = copy.deepcopy(want)
        off["box3d_lidar"][0, col] += 0.9 * big
        assert same_detections(off, want, relative_sizes=True, code_rtol=rt, code_scale=wild) is None, col
        assert same_detections(off, want) is not None                      # strict: flat 2 mm
        assert same_detections(off, want, relative_sizes=True, code_rtol=rt) is not None   # no code scale at hand: flat 2 mm as well
        assert same_detections(off, want, relative_sizes=True, code_rtol=rt, code_scale=tame) is not None   # a tame frame: 2.2 mm
        off["box3d_lidar"][0, col] += 0.3 * big
        assert same_detections(off, want, relative_sizes=True, code_rtol=rt, code_scale=wild) is not None, col
    small = copy.deepcopy(want)
    small["box3d_lidar"][1, 0] += 2.1e-3
    assert same_detections(small, want, relative_sizes=True, code_rtol=rt, code_scale=tame) is None and same_detections(small, want) is not None
    far = copy.deepcopy(want)
    far["box3d_lidar"][0, 0] += 4e-3
    assert compare_detections(far, want, dict(dbg, code_scale=wild), rule="synthetic")["matched"] == 2
    with pytest.raises(AssertionError):
        compare_detections(far, want, dict(dbg, code_scale=tame), rule="synthetic")
    with pytest.raises(AssertionError):
        compare_detections(far, want, dict(dbg, code_scale=wild), rule="strict")
    yaw = copy.deepcopy(want)
    yaw["box3d_lidar"][0, 6] += 3e-3
    assert same_detections(yaw, want, relative_sizes=True, code_rtol=rt) is not None
    with pytest.raises(AssertionError):
        compare_detections(yaw, want, dbg, rule="synthetic")
    car = copy.deepcopy(want)
    car["box3d_lidar"][0, 4] += 1.5e-3     # a car-sized box 1.5 mm off: fine under both rule sets
    car["box3d_lidar"] = car["box3d_lidar"][:1]
    car["scores"] = car["scores"][:1]
    one = dict(box3d_lidar=want["box3d_lidar"][:1], scores=want["scores"][:1])
    assert same_detections(car, one) is None and same_detections(car, one, relative_sizes=True) is None
    nan = copy.deepcopy(want)
    nan["box3d_lidar"][0, 3] = np.nan
    assert same_detections(nan, want) is not None


def test_strict_rule_allows_fewer_listed_decisions():
    from oracle.compare import RULES
    assert RULES["strict"] == dict(relative_sizes=False, max_pairs=6, code_rtol=0.0) and RULES["synthetic"]["max_pairs"] == 10
    want = dict(box3d_lidar=np.zeros((1, 7), np.float32), scores=np.array([0.5], np.float32))
    got = dict(box3d_lidar=np.zeros((0, 7), np.float32), scores=np.zeros((0,), np.float32))
    dbg = dict(near_pairs=np.stack([np.arange(8), np.arange(8) + 1], 1), rerun=lambda forced: want)
    with pytest.raises(AssertionError, match="too many"):
        compare_detections(got, want, dbg)                       # 8 listed decisions > 6
    with pytest.raises(AssertionError, match="NO assignment"):
        compare_detections(got, want, dbg, rule="synthetic")     # 8 <= 10: explored, and none matches


# ---- compare_keep: the same rule for a bare keep list of the rotated NMS
def _marginal_triples(m, thresh=0.3):
    """m groups far apart, each three 2 x 2 axis-aligned boxes A > B > C in score: IoU(A, B) sits ON the threshold (one listed
    decision per group), C overlaps B (IoU 1/3) and not A -- so C is kept exactly when the marginal decision suppresses B."""
    dx = 2.0 - thresh * 8.0 / (1.0 + thresh) / 2.0
    rows = []
    for g in range(m):
        x0 = 20.0 * g
        for k, x in enumerate((x0, x0 + dx, x0 + dx + 1.0)):
            rows.append([x, 0.0, 2.0, 2.0, 0.0, 0.9 - 0.01 * (3 * g + k)])
    return np.asarray(rows, np.float32)


def test_compare_keep_identical_passes_and_a_dropped_index_fails_without_near_pairs():
    from oracle.compare import compare_keep
    from sessd_hip import synth
    d = synth.clustered_boxes7(300, seed=9)[:, [0, 1, 3, 4, 6]].astype(np.float32)
    d = np.concatenate([d, np.linspace(0.95, 0.3, 300, dtype=np.float32)[:, None]], 1)
    want, near, pairs = capi.rotate_nms_cc(d, 0.1, return_pairs=True)
    assert near == 0 and len(pairs) == 0 and len(want) > 20
    assert compare_keep(want, d, 0.1) == dict(n=len(want), near_pairs=[], flipped=[])
    assert compare_keep(want[:10], d, 0.1, post_max=10)["n"] == 10
    with pytest.raises(AssertionError, match="no near-threshold"):
        compare_keep(np.delete(want, 5), d, 0.1)
    with pytest.raises(AssertionError, match="no near-threshold"):
        compare_keep(want[:9], d, 0.1, post_max=10)     # the whole list is compared, not a prefix
    with pytest.raises(AssertionError, match="no near-threshold"):
        compare_keep(want, d, 0.1, post_max=10)
    # an explicit order is passed through: the reversed score order keeps other boxes
    rev = np.arange(300, dtype=np.int32)[::-1].copy()
    w2 = capi.rotate_nms_cc(d, 0.1, order=rev)[0]
    assert not np.array_equal(w2, want) and compare_keep(w2, d, 0.1, order=rev)["flipped"] == []
    with pytest.raises(AssertionError):
        compare_keep(want, d, 0.1, order=rev)


def test_compare_keep_accepts_only_an_assignment_of_the_listed_decisions():
    from oracle.compare import compare_keep
    d = _marginal_triples(2)
    base, near, pairs = capi.rotate_nms_cc(d, 0.3, return_pairs=True)
    assert near == 2 and pairs.tolist() == [[0, 1], [3, 4]]
    assert compare_keep(base, d, 0.3)["flipped"] == []
    for f0 in (0, 1):
        for f1 in (0, 1):
            forced = [(0, 1, f0), (3, 4, f1)]
            alt = capi.rotate_nms_cc(d, 0.3, forced=np.asarray(forced, np.int32))[0]
            assert alt.tolist() == [0, 2 if f0 else 1, 3, 5 if f1 else 4]
            r = compare_keep(alt, d, 0.3)
            assert r["flipped"] == ([] if np.array_equal(alt, base) else forced) and r["near_pairs"] == [[0, 1], [3, 4]]
    for bad in ([0, 1, 2, 3, 4], [0, 3], [0, 1, 3], [1, 2, 3, 4], [0, 1, 4, 3]):   # no assignment gives these
        with pytest.raises(AssertionError, match="NO assignment"):
            compare_keep(np.asarray(bad), d, 0.3)
    assert compare_keep([0], d, 0.3, post_max=1)["n"] == 1
    with pytest.raises(AssertionError, match="NO assignment"):
        compare_keep([1], d, 0.3, post_max=1)


def test_compare_keep_rejects_too_many_listed_decisions():
    from oracle.compare import compare_keep
    d = _marginal_triples(7)
    base, near, _ = capi.rotate_nms_cc(d, 0.3, return_pairs=True)
    assert near == 7
    assert compare_keep(base, d, 0.3)["flipped"] == []           # identical needs no excuse
    flip = capi.rotate_nms_cc(d, 0.3, forced=np.array([[0, 1, 0]], np.int32))[0]
    other = flip if not np.array_equal(flip, base) else capi.rotate_nms_cc(d, 0.3, forced=np.array([[0, 1, 1]], np.int32))[0]
    with pytest.raises(AssertionError, match="too many"):
        compare_keep(other, d, 0.3)                              # 7 listed decisions > 6
    assert len(compare_keep(other, d, 0.3, max_pairs=7)["flipped"]) == 7


def test_score_atol_is_a_parameter_of_the_rule():
    want = dict(box3d_lidar=np.zeros((1, 7), np.float32), scores=np.array([1e-3], np.float32))
    got = dict(box3d_lidar=np.zeros((1, 7), np.float32), scores=np.array([1e-3 + 5e-7], np.float32))
    dbg = dict(near_pairs=np.zeros((0, 2), np.int64))
    assert same_detections(got, want, score_rtol=1e-5) is None                    # default absolute term 1e-6
    assert same_detections(got, want, score_rtol=1e-5, score_atol=1e-7) is not None
    assert compare_detections(got, want, dbg, score_rtol=1e-5)["matched"] == 1
    with pytest.raises(AssertionError):
        compare_detections(got, want, dbg, score_rtol=1e-5, score_atol=1e-7)
