"""The validity of tests/predict_cases.py, from the CPU oracle alone: what tests/test_predict_edges_gpu.py relies on when it holds
ops.predict to the oracle -- few (or no) near-threshold NMS decisions, scores that a 1-ulp expf cannot reorder, no score on the
score threshold, the overflow / frustum / range preconditions, walks that end below post_max, and the oracle's tie order."""
import numpy as np
import pytest

import predict_cases as pc
from oracle import postprocess as pp


@pytest.fixture(scope="module")
def frustum():
    from sessd_hip import synth
    return pc.kitti_frustum(synth.kitti_calib())


def _ids(cases):
    return [c["name"] for c in cases]


EVERY = pc.CASES + pc.BATCH + pc.REUSE + pc.ODD + pc.TASKS


def test_table_covers_what_it_claims():
    assert pc.P == 2112 and pc.A == 4224 and pc.anchors().shape == (4224, 7)
    assert [c["n"] for c in pc.TOPK if c["pre_max"] == 256] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3840, 3841, 4224]
    assert [c["n"] for c in pc.TOPK if c["pre_max"] == 1984] == [1983, 1984, 1985, 2048, 2049, 2112, 2113, 4224]
    assert all(c["pre_max"] == c["post_max"] and c["nms_thresh"] == 0.99 and c["range"] == pc.WIDE and c["exact"] for c in pc.TOPK + pc.TIES)
    assert [(c["pre_max"], c["post_max"], c["nms_thresh"]) for c in pc.WALK] == [
        (63, 63, 0.01), (64, 7, 0.1), (65, 65, 0.5), (128, 1, 0.01), (191, 191, 0.1), (1000, 500, 0.01), (1000, 1000, 0.1),
        (1024, 1024, 0.3), (1025, 200, 0.3), (1102, 100, 0.01), (1103, 100, 0.01), (1984, 1984, 0.5), (1984, 100, 0.01)]
    assert all(c["n"] == pc.A for c in pc.WALK + pc.TIES + pc.OVERFLOW)
    assert sum(c["short_walk"] for c in pc.WALK) >= 4
    assert all(c["exact"] for c in pc.POST) and len(pc.POST) == 16
    # the two sides of the LDS switch of predict_impl, recomputed
    lds = lambda pre, post: pre * ((pre + 63) // 64) * 8 + post * 40
    assert lds(1102, 100) <= 160 * 1024 - 1024 < lds(1103, 100)
    assert lds(1000, 500) <= 160 * 1024 - 1024 < lds(1000, 1000) and lds(1025, 200) <= 160 * 1024 - 1024 < lds(1024, 1024)
    assert lds(256, 256) <= 160 * 1024 - 1024 < lds(1984, 100) and (191 * 3) % 2 == 1


def test_pack_head_is_the_inverse_of_split():
    frame = pc.make_frame(pc.BY_NAME["walk_191_191_0.1"])
    head = pc.pack_head(frame)
    assert head.shape == (22, pc.P) and head.dtype == np.float32
    for a, b in zip(pc.split_head(head), frame):
        assert np.array_equal(a, b)
    # anchor 2 * p + a: code q at channel a * 7 + q, class logit at 14 + a, dir logit k at 16 + 2 a + k, IoU at 20 + a
    box, cls, dirl, iou = frame
    for aid in (0, 1, 2 * 777 + 1, pc.A - 1):
        p, a = aid // 2, aid % 2
        assert head[a * 7 + 3, p] == box[aid, 3] and head[14 + a, p] == cls[aid] and head[17 + 2 * a, p] == dirl[aid, 1]
        assert head[20 + a, p] == iou[aid]


@pytest.mark.parametrize("case", EVERY, ids=_ids(EVERY))
def test_scores_are_separated_and_off_the_threshold(case):
    frame = pc.make_frame(case)
    sc, cand, sg = pc.rectified_scores(frame)
    assert int(cand.sum()) == case["n"]
    assert int((np.abs(sg.astype(np.float64) - 0.3) < 1e-6).sum()) == 0      # nothing on the score threshold ...
    assert sg[cand].min() > 0.35 if case["n"] else True                        # ... nor anywhere near it
    assert sg[~cand].max() < 1e-12 if case["n"] < pc.A else True
    s = np.sort(sc[cand].astype(np.float64))[::-1]
    ratio = s[:-1] / s[1:]
    if case["ties"] is None:
        assert (ratio >= 1 + 1e-4).all()
    else:
        t0, m = case["ties"]
        eq = np.nonzero(s[:-1] == s[1:])[0]
        assert np.array_equal(eq, np.arange(t0, t0 + m - 1))                   # ONE group of m bit-identical scores
        assert (np.delete(ratio, eq) >= 1 + 1e-4).all()
        box, cls, dirl, iou = frame
        grp = np.nonzero(sc == np.float32(s[t0]))[0]
        assert len(grp) == m and len(np.unique(cls[grp])) == 1 and len(np.unique(iou[grp])) == 1
        assert t0 < case["pre_max"] < t0 + m                                   # the group straddles the pre_max cut


@pytest.mark.parametrize("case", EVERY, ids=_ids(EVERY))
def test_near_decisions_within_the_strict_cap(case, frustum):
    want, dbg = pc.run_oracle(case, frustum)
    near = dbg.get("near_threshold_pairs", 0)
    assert near == len(dbg.get("near_pairs", ())) <= pc.MAX_NEAR
    if case["exact"]:
        assert near == 0
    assert dbg["num_candidates"] == case["n"]
    if case["n"]:
        assert dbg["topk"] == min(case["n"], case["pre_max"])
    if case["short_walk"]:
        assert dbg["nms_kept"] < case["post_max"] and dbg["nms_kept"] < dbg["topk"]
    if case["kind"] in ("topk", "ties") and case["n"]:
        # the output is the top-k itself, in order: nothing suppressed, nothing filtered
        k = min(case["n"], case["pre_max"])
        assert dbg["nms_kept"] == k == len(want["scores"])
        assert np.array_equal(dbg["selected_anchor"], dbg["cand_anchor"])
        assert (np.diff(want["scores"].astype(np.float64)) <= 0).all()


def test_walk_cases_cover_the_range_of_kept_counts():
    kept = [pc.run_oracle(c)[1]["nms_kept"] for c in pc.WALK]
    assert min(kept) == 1 and max(kept) > 1800
    assert any(pc.run_oracle(c)[1]["near_threshold_pairs"] > 0 for c in pc.WALK)   # the rerun hook is exercised as well


@pytest.mark.parametrize("case", pc.TIES, ids=_ids(pc.TIES))
def test_oracle_orders_ties_by_ascending_anchor(case):
    want, dbg = pc.run_oracle(case)
    sc = want["scores"]
    t0, m = case["ties"]
    sel = dbg["selected_anchor"]
    inside = np.arange(t0, case["pre_max"])
    assert len(sel) == case["pre_max"] and (sc[inside] == sc[t0]).all() and sc[t0 - 1] > sc[t0]
    assert (np.diff(sel[inside]) > 0).all()
    # the members that made the cut are the group's lowest anchor indices
    score_all, _, _ = pc.rectified_scores(pc.make_frame(case))
    grp = np.nonzero(score_all == sc[t0])[0]
    assert np.array_equal(sel[inside], grp[:len(inside)]) and len(grp) == m


@pytest.mark.parametrize("case", pc.OVERFLOW, ids=_ids(pc.OVERFLOW))
def test_overflow_case_overflows_the_pair_list(case):
    _, dbg = pc.run_oracle(case)
    assert 1024 < case["pre_max"] <= 1984 and dbg["topk"] == case["pre_max"]
    pairs = pc.standup_overlap_pairs(dbg["cand_dets"])
    print("stand-up overlaps", pairs, "pair list", 64 * case["pre_max"])
    assert pairs > 64 * case["pre_max"]


def test_range_cases_sit_on_and_one_step_past_an_anchor_value(frustum):
    an = pc.anchors()
    for on, past in zip(pc.POST[0:12:2], pc.POST[1:12:2]):
        axis, v = past["dropped"]
        side = int(on["name"][len("post_range_side")])
        assert on["range"][side] == v and (an[:, axis] == np.float32(v)).any()
        assert past["range"][side] == float(np.nextafter(np.float32(v), np.float32(np.inf if side < 3 else -np.inf))) != v
        (w_on, d_on), (w_past, d_past) = pc.run_oracle(on), pc.run_oracle(past)
        a_on, a_past = set(d_on["selected_anchor"].tolist()), set(d_past.get("selected_anchor", np.zeros(0, np.int64)).tolist())
        lost = np.array(sorted(a_on - a_past))
        assert a_past < a_on and len(lost) > 0 and (an[lost, axis] == np.float32(v)).all()   # exactly the boxes ON the bound go
        assert not (an[np.array(sorted(a_past), np.int64), axis] == np.float32(v)).any()
    # boxes sit exactly on their anchors (zero codes)
    want, dbg = pc.run_oracle(pc.BY_NAME["post_dir_offset_0"])
    assert np.array_equal(want["box3d_lidar"][:, :6], an[dbg["selected_anchor"], :6])


def test_direction_cases_meet_the_offset_and_equal_logits():
    an = pc.anchors()
    for name in ("post_dir_offset_0", "post_dir_offset_1.57", "post_dir_offset_0.78"):
        case = pc.BY_NAME[name]
        want, dbg = pc.run_oracle(case)
        sel = dbg["selected_anchor"]
        dirl = pc.make_frame(case)[2][sel]
        yaw0 = an[sel, 6]
        if name != "post_dir_offset_0.78":   # offsets 0 and 1.57 are anchor rotations: a yaw EQUAL to the offset, '> 0' is false
            assert ((yaw0 - np.float32(case["direction_offset"])) == 0).sum() > 20
        assert (dirl[:, 0] == dirl[:, 1]).sum() > 20 and (dirl[:, 0] != dirl[:, 1]).sum() > 20
        flipped = want["box3d_lidar"][:, 6] != yaw0
        assert flipped.any() and (~flipped).any()
        opp = ((yaw0 - np.float32(case["direction_offset"])) > 0) ^ (dirl[:, 1] > dirl[:, 0])
        assert np.array_equal(flipped, opp)
    a, b = (pc.run_oracle(pc.BY_NAME[n])[0]["box3d_lidar"][:, 6] for n in ("post_dir_offset_0", "post_dir_offset_1.57"))
    assert not np.array_equal(a, b)


def test_frustum_case_has_no_centre_on_a_plane(frustum):
    case = pc.BY_NAME["post_frustum"]
    want, dbg = pc.run_oracle(case, frustum)
    kept = dbg["cand_boxes"][dbg["nms_kept_rows"]][:, :3].astype(np.float64)     # every box the walk kept, before the filters
    n, d = pp.frustum_planes(frustum)
    dist = kept @ n.T + d[None]
    assert (np.abs(dist) > 1e-6 * np.linalg.norm(n, axis=1)[None]).all()
    inside = ~(dist >= 0).any(1)
    assert 0 < inside.sum() < len(kept) and len(want["scores"]) <= inside.sum()
