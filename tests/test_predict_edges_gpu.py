"""ops.predict (csrc/postprocess.hip: score filter, running top-k, decode, suppression mask, greedy walk, post filters, records,
task merge) held to the CPU oracle on the edge cases of tests/predict_cases.py -- away from the one operating point
(200 x 176, pre_max 1000, post_max 100, nms_thresh 0.01) the other files run it at.

Rule (oracle/compare.py, "strict"): count and every row identical to the oracle -- boxes to 1e-4 (m / rad), scores to 1e-5
relative + 1e-7 -- or identical to the oracle re-run under one assignment of its listed near-threshold NMS decisions (at most
6). Where the table demands 0 listed decisions (top-k, ties, post filters) nothing can be excused, and in addition:
  * the anchor behind every output row, recovered from the row's box, is the oracle's selected anchor, in the oracle's order;
  * scores within 8 float32 ulp of the oracle's. The rectified score is sigmoid(x) * r^4 with r^4 the same IEEE products on both
    sides; the two expf (each within 1 ulp of the exact value) differ by at most 2 ulp, which 1 / (1 + e) scales by
    e / (1 + e) < 0.63 for the sigmoids >= 0.37 of the table, and the add, the divide and the last product round once more on
    each side: under 5 ulp in all. 8 ulp = 1e-6 relative, 150 times below the table's score spacing."""
import numpy as np
import pytest
import torch

import predict_cases as pc
from oracle.compare import compare_detections
from sessd_hip import ops, synth
from sessd_hip._lib import SessdError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frustum():
    return pc.kitti_frustum(synth.kitti_calib())


@pytest.fixture(scope="module")
def anchors_dev(dev):
    return torch.from_numpy(pc.anchors()).to(dev)


def _ids(cases):
    return [c["name"] for c in cases]


def _head(case, dev):
    return torch.from_numpy(pc.pack_head(pc.make_frame(case))).to(dev)


def _predict(dev, case, anchors_dev, frustum=None, **kw):
    fr = torch.from_numpy(frustum[None].copy()).to(dev) if case["frustum"] else None
    return ops.predict(_head(case, dev)[None], anchors_dev, fr, pc.SCORE_THRESH, case["pre_max"], case["post_max"], case["nms_thresh"],
                       case["range"], case["direction_offset"], **kw)


def _rows(out, b, lo=0, hi=None):
    hi = int(out["count"][b].item()) if hi is None else hi
    return dict(box3d_lidar=out["box"][b, lo:hi].cpu().numpy(), scores=out["score"][b, lo:hi].cpu().numpy(),
                label_preds=out["label"][b, lo:hi].cpu().numpy().astype(np.int64))


def _recover_anchors(got_box, dbg):
    """The anchor behind every output row: the ONE top-k candidate of the oracle whose box is the row's box (centre and size to
    1e-4, yaw to 1e-4 modulo pi -- the direction fix adds pi)."""
    cb = dbg["cand_boxes"].astype(np.float64)
    g = got_box.astype(np.float64)
    rec = np.empty(len(g), np.int64)
    for i0 in range(0, len(g), 128):
        d = np.abs(g[i0:i0 + 128, None, :6] - cb[None, :, :6]).max(2)
        da = np.abs((g[i0:i0 + 128, None, 6] - cb[None, :, 6] + np.pi / 2) % np.pi - np.pi / 2)
        hit = np.maximum(d, da) < 1e-4
        assert (hit.sum(1) == 1).all(), "an output row matches %s candidates" % sorted(set(hit.sum(1).tolist()))
        rec[i0:i0 + 128] = dbg["cand_anchor"][hit.argmax(1)]
    return rec


def _check(got, case, want, dbg, label=0):
    """One frame against the oracle; every row is compared. Returns compare_detections' report."""
    if "label_preds" in got:
        assert (got["label_preds"] == label).all()
        got = dict(got, label_preds=np.zeros_like(got["label_preds"]))   # the oracle frame is one task: label 0
    n = len(got["scores"])
    print(case["name"], "candidates", dbg["num_candidates"], "walk kept", dbg.get("nms_kept", 0), "oracle", len(want["scores"]), "device", n,
          "listed", dbg.get("near_threshold_pairs", 0))
    r = compare_detections(got, want, dbg, box_tol=1e-4, score_rtol=1e-5, score_atol=1e-7, rule="strict")
    assert r["matched"] == n
    if case["exact"]:
        assert dbg.get("near_threshold_pairs", 0) == 0 and r["flipped"] == [] and n == len(want["scores"])
        if n:
            assert np.array_equal(_recover_anchors(got["box3d_lidar"], dbg), dbg["selected_anchor"])
            ulp = np.abs(got["scores"].astype(np.float64) - want["scores"]) / np.spacing(want["scores"]).astype(np.float64)
            print("    score difference, float32 ulp: max %.1f, rows that differ %d of %d" % (ulp.max(), int((ulp > 0).sum()), n))
            assert ulp.max() <= 8
    return r


@pytest.mark.parametrize("pre_max", [256, 1984])
def test_topk_edges(dev, anchors_dev, pre_max):
    """Candidate counts at the edges of the 2048-key sort passes; nothing suppressed or filtered: the output is the top-k in order.
    pre_max 256: passes end at keys 2048 and 3840; pre_max 1984 (the limit): 64 keys per pass after the first."""
    for case in [c for c in pc.TOPK if c["pre_max"] == pre_max]:
        want, dbg = pc.run_oracle(case)
        out = _predict(dev, case, anchors_dev)
        n = int(out["count"][0].item())
        assert n == min(case["n"], pre_max), case["name"]
        _check(_rows(out, 0), case, want, dbg)
        if n > 1:
            assert (np.diff(out["score"][0, :n].cpu().numpy().astype(np.float64)) < 0).all()


def test_pre_max_over_the_limit_is_an_error(dev, anchors_dev):
    case = dict(pc.BY_NAME["topk1984_n1985"], pre_max=1985, post_max=100)
    with pytest.raises(SessdError, match="invalid argument"):
        _predict(dev, case, anchors_dev)


@pytest.mark.parametrize("case", pc.TIES, ids=_ids(pc.TIES))
def test_ties_are_ordered_by_ascending_anchor(dev, anchors_dev, case):
    """600 bit-identical scores across the pre_max cut, arriving in the filter's (unordered) append order and, with 4224
    candidates, from different sort passes: the members that make the cut are the lowest anchor indices, in ascending order."""
    want, dbg = pc.run_oracle(case)
    out = _predict(dev, case, anchors_dev)
    got = _rows(out, 0)
    _check(got, case, want, dbg)
    t0, _ = case["ties"]
    sc = got["scores"]
    assert len(sc) == case["pre_max"] and (sc[t0:] == sc[t0]).all() and sc[t0 - 1] > sc[t0]
    rec = _recover_anchors(got["box3d_lidar"], dbg)
    assert (np.diff(rec[t0:]) > 0).all()


@pytest.mark.parametrize("case", pc.WALK, ids=_ids(pc.WALK))
def test_whole_walk(dev, anchors_dev, case):
    """The greedy walk compared to its end, on both walk kernels (mask in LDS / mask in global memory), at pre_max below 64, off
    the multiples of 64, at the LDS switch and at the limit, post_max 1 and post_max = pre_max, four NMS thresholds."""
    want, dbg = pc.run_oracle(case)
    out = _predict(dev, case, anchors_dev)
    _check(_rows(out, 0), case, want, dbg)


@pytest.mark.parametrize("case", pc.OVERFLOW, ids=_ids(pc.OVERFLOW))
def test_pair_list_overflow(dev, anchors_dev, case):
    """More stand-up overlaps than the pair list holds (tests/test_predict_cases_cpu.py asserts it): the pairs past the list's
    capacity are clipped on the spot and must reach the mask like the listed ones."""
    want, dbg = pc.run_oracle(case)
    out = _predict(dev, case, anchors_dev)
    _check(_rows(out, 0), case, want, dbg)


@pytest.mark.parametrize("case", pc.POST, ids=_ids(pc.POST))
def test_post_filters(dev, anchors_dev, frustum, case):
    """Centres exactly on a post_center_range bound (kept) and one float32 step outside it (dropped), direction offsets that equal
    a yaw, equal dir logits, the KITTI frustum. Zero box codes: the decode is exact."""
    want, dbg = pc.run_oracle(case, frustum)
    out = _predict(dev, case, anchors_dev, frustum)
    got = _rows(out, 0)
    _check(got, case, want, dbg)
    if len(want["scores"]):
        assert np.array_equal(got["box3d_lidar"][:, :6], want["box3d_lidar"][:, :6])     # exact decode, exact bounds
    if case["dropped"] is not None:
        axis, v = case["dropped"]
        assert not (got["box3d_lidar"][:, axis] == np.float32(v)).any()


def _stack(cases, dev):
    return torch.stack([_head(c, dev) for c in cases])


def test_batch_with_per_frame_anchors(dev):
    """B = 3, anchors (B, A, 7) shifted differently per frame, the middle frame without a candidate."""
    an = np.stack([pc.anchors() + np.array([dx, dy, 0, 0, 0, 0, 0], np.float32) for dx, dy in pc.BATCH_SHIFT])
    c0 = pc.BATCH[0]
    out = ops.predict(_stack(pc.BATCH, dev), torch.from_numpy(an).to(dev), None, pc.SCORE_THRESH, c0["pre_max"], c0["post_max"],
                      c0["nms_thresh"], c0["range"], c0["direction_offset"])
    kept = []
    for b, case in enumerate(pc.BATCH):
        want, dbg = pc.run_oracle(case, anchors_=an[b])
        _check(_rows(out, b), case, want, dbg)
        kept.append(len(want["scores"]))
    assert kept[0] > 50 and kept[1] == 0 and 0 < kept[2] < c0["post_max"] and int(out["count"][1].item()) == 0
    # the shift matters: frame 2 under frame 0's anchors is another result
    other = pc.run_oracle(pc.BATCH[2], anchors_=an[0])[0]
    assert len(other["scores"]) != kept[2] or not np.allclose(other["box3d_lidar"], _rows(out, 2)["box3d_lidar"], atol=1e-2)


def test_batch_of_two_with_an_odd_mask_stride(dev, anchors_dev):
    """pre_max 191: 573 mask words per frame, so frame 1's mask starts on an odd 8-byte word under the 16-byte staging copy."""
    c0 = pc.ODD[0]
    assert (c0["pre_max"] * ((c0["pre_max"] + 63) // 64)) % 2 == 1
    out = ops.predict(_stack(pc.ODD, dev), anchors_dev, None, pc.SCORE_THRESH, c0["pre_max"], c0["post_max"], c0["nms_thresh"],
                      c0["range"], c0["direction_offset"])
    for b, case in enumerate(pc.ODD):
        _check(_rows(out, b), case, *pc.run_oracle(case))


def test_workspace_reuse_after_another_pre_max(dev, anchors_dev):
    """The cached "predict" workspace holds another layout's bytes (here: all ones, then a pre_max 1000 call's mask) when the
    pre_max 65 call runs: every word a call reads it must have written itself."""
    first, then = pc.REUSE
    need = ops.lib.sessd_predict_workspace_bytes(1, 1, pc.A, first["pre_max"], first["post_max"], 0)
    ws = ops.workspace(need, dev, "predict")
    ws.fill_(0xFF)
    out1 = _predict(dev, first, anchors_dev)
    assert ops.workspace(1, dev, "predict") is ws
    out2 = _predict(dev, then, anchors_dev)
    assert ops.workspace(1, dev, "predict") is ws
    _check(_rows(out1, 0), first, *pc.run_oracle(first))
    _check(_rows(out2, 0), then, *pc.run_oracle(then))


@pytest.mark.parametrize("pre_max,post_max,path", [(1000, 100, "fused"), (1200, 100, "unfused")])
def test_records_ring_over_two_calls(dev, anchors_dev, pre_max, post_max, path):
    """A records ring of 4 slots over two B = 3 calls -- sessd_pack_detections' rule: slot = (cursor + b) % capacity, cursor +=
    batch -- written by the walk kernel itself (fused) and by pack_detections_kernel from the stored base (unfused)."""
    lds = pre_max * ((pre_max + 63) // 64) * 8 + post_max * 40
    assert (lds <= 160 * 1024 - 1024) == (path == "fused")
    cap = 4
    rec = torch.full((cap, post_max, 9), -7.0, device=dev)
    rcnt = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    cur = torch.zeros((1,), dtype=torch.int32, device=dev)
    calls = [pc.BATCH, pc.BATCH[::-1]]
    want_slot = {}
    for k, cases in enumerate(calls):
        c0 = pc.BATCH[0]
        out = ops.predict(_stack(cases, dev), anchors_dev, None, pc.SCORE_THRESH, pre_max, post_max, c0["nms_thresh"], c0["range"],
                          c0["direction_offset"], records=(rec, rcnt, cur))
        assert int(cur.item()) == 3 * (k + 1)
        for b, case in enumerate(cases):
            cc = dict(case, pre_max=pre_max, post_max=post_max)
            got = _rows(out, b)
            _check(got, cc, *pc.run_oracle(cc, cache=False))
            want_slot[(3 * k + b) % cap] = got
    assert sorted(want_slot) == [0, 1, 2, 3]      # slots 0, 1, 2 then 3, 0, 1: slot 2 still holds the first call's frame 2
    for slot, got in want_slot.items():
        n = len(got["scores"])
        r = rec[slot].cpu().numpy()
        assert int(rcnt[slot].item()) == n
        assert np.array_equal(r[:n, :7], got["box3d_lidar"]) and np.array_equal(r[:n, 7], got["scores"])
        assert (r[:n, 8] == 0).all() and (r[n:] == 0).all()
    assert len(want_slot[2]["scores"]) > 0 and len(want_slot[3]["scores"]) > 0


def test_three_tasks_one_empty_one_capped(dev):
    """T = 3 through the multi-task entry point: task 0 bound by post_max, task 1 without a candidate, task 2 in between; every
    task against the oracle on its own anchors; labels = task index, task_count, and the merge order."""
    T, post = 3, pc.TASKS[0]["post_max"]
    from oracle import postprocess as pp
    an = np.stack([pp.create_anchors_3d_range(pc.FEATURE, sizes=s).reshape(-1, 7).astype(np.float32) for s in pc.TASK_SIZES])
    head = torch.cat([_head(c, dev) for c in pc.TASKS])[None]
    c0 = pc.TASKS[0]
    out = ops.predict(head, torch.from_numpy(an).to(dev), None, pc.SCORE_THRESH, c0["pre_max"], post, c0["nms_thresh"], c0["range"],
                      c0["direction_offset"], num_tasks=T)
    tc = out["task_count"][0].cpu().numpy()
    lo = 0
    for t, case in enumerate(pc.TASKS):
        want, dbg = pc.run_oracle(case, anchors_=an[t])
        _check(_rows(out, 0, lo, lo + int(tc[t])), case, want, dbg, label=t)
        lo += int(tc[t])
    assert int(out["count"][0].item()) == lo and tc[1] == 0 and tc[0] > 0 and tc[2] > 0
    assert pc.run_oracle(pc.TASKS[0], anchors_=an[0])[1]["nms_kept"] == post        # task 0 is bound by post_max
