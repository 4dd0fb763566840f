"""HIP predict / rotated NMS vs the CPU oracle (oracle/postprocess.py + oracle/rotate_nms.c).

Selection (which anchors survive, in which order) must be IDENTICAL to the oracle, or to the oracle re-run under one assignment
of the near-threshold NMS decisions it lists (pairs within 1e-4 of the NMS threshold; at most 6: oracle/compare.py, rule
"strict"); no score may lie within 1e-6 of the score threshold; kept boxes must agree to 1e-4 (m / rad) and scores to 1e-5
relative + 1e-7."""
import numpy as np
import pytest
import torch

from oracle import postprocess as pp
from oracle.compare import compare_detections, compare_keep
from sessd_hip import ops, synth

pytestmark = pytest.mark.gpu

H, W = 200, 176


def _make_head(seed, n_hot, H=H, W=W, cls_bias=-4.0):
    rng = np.random.RandomState(seed)
    P = H * W
    head = np.zeros((22, P), np.float32)
    head[:14] = rng.normal(0, 0.25, (14, P))
    head[14:16] = cls_bias + rng.normal(0, 0.5, (2, P))
    head[16:20] = rng.normal(0, 1.0, (4, P))
    head[20:22] = rng.uniform(-0.2, 1.0, (2, P))
    # hot blobs: clusters of neighbouring locations with high class logits (real NMS work)
    for _ in range(n_hot):
        cy, cx = rng.randint(5, H - 5), rng.randint(5, W - 5)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                p = (cy + dy) * W + cx + dx
                head[14 + rng.randint(2), p] = rng.uniform(-0.5, 3.0)
    return head


def _split(head):
    P = head.shape[1]
    box = head[:14].reshape(2, 7, P).transpose(2, 0, 1).reshape(-1, 7)
    cls = head[14:16].T.reshape(-1)
    dirl = head[16:20].reshape(2, 2, P).transpose(2, 0, 1).reshape(-1, 2)
    iou = head[20:22].T.reshape(-1)
    return box, cls, dirl, iou


def _frame_vs_oracle(out, b, head, anchors, fr):
    """Frame b of a predict call against the oracle under the strict rule: identical, or identical to the oracle re-run under one
    assignment of its listed near-threshold NMS decisions (oracle/compare.py). Every row is compared; returns the oracle's dbg."""
    box, cls, dirl, iou = _split(head)
    args = (box, cls, dirl, iou, anchors, fr)
    want, dbg = pp.predict_frame(*args, return_debug=True)
    dbg["rerun"] = lambda forced: pp.predict_frame(*args, forced=forced)
    # no score sits on the score threshold (from the oracle alone): the candidate set is not in doubt
    assert int((np.abs(pp.sigmoid32(cls).astype(np.float64) - 0.3) < 1e-6).sum()) == 0
    n = int(out["count"][b].item())
    got = dict(box3d_lidar=out["box"][b, :n].cpu().numpy(), scores=out["score"][b, :n].cpu().numpy(),
               label_preds=out["label"][b, :n].cpu().numpy().astype(np.int64))
    r = compare_detections(got, want, dbg, box_tol=1e-4, score_rtol=1e-5, score_atol=1e-7, rule="strict")
    assert r["matched"] == n
    assert (got["label_preds"] == 0).all()
    print("candidates", dbg["num_candidates"], "kept", n, "flipped", r["flipped"])
    return dbg


@pytest.mark.parametrize("seed,n_hot,use_frustum", [(0, 40, True), (1, 150, False), (2, 0, True), (3, 400, True)])
def test_predict_vs_oracle(dev, seed, n_hot, use_frustum):
    head = _make_head(seed, n_hot)
    anchors = pp.create_anchors_3d_range().reshape(-1, 7)
    cal = synth.kitti_calib()
    fr = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], cal["image_shape"]) if use_frustum else None
    out = ops.predict(torch.from_numpy(head[None]).to(dev), torch.from_numpy(anchors).to(dev),
                      None if fr is None else torch.from_numpy(fr[None].copy()).to(dev))
    _frame_vs_oracle(out, 0, head, anchors, fr)


def test_predict_batch_and_many_candidates(dev):
    """B=3 with one frame above the 2048-key sort window (running top-k) and one empty frame."""
    heads = [_make_head(5, 60), _make_head(6, 0, cls_bias=-0.2), _make_head(7, 0, cls_bias=-30.0)]
    anchors = pp.create_anchors_3d_range().reshape(-1, 7)
    out = ops.predict(torch.from_numpy(np.stack(heads)).to(dev), torch.from_numpy(anchors).to(dev), None)
    counts = out["count"].cpu().numpy()
    for b, head in enumerate(heads):
        dbg = _frame_vs_oracle(out, b, head, anchors, None)
        if b == 1:
            assert dbg["num_candidates"] > 2048
    assert counts[2] == 0


@pytest.mark.parametrize("n,thresh", [(1, 0.01), (100, 0.01), (700, 0.1), (1000, 0.5), (2500, 0.3)])
def test_rotate_nms_sorted_vs_oracle(dev, n, thresh):
    b = synth.clustered_boxes7(n, seed=n)
    rng = np.random.RandomState(n)
    score = np.sort(rng.uniform(0.3, 1, n).astype(np.float32))[::-1]
    dets = np.concatenate([b[:, [0, 1, 3, 4, 6]], score[:, None]], 1).astype(np.float32)
    keep, num = ops.rotate_nms_sorted(torch.from_numpy(np.ascontiguousarray(dets[:, :5])).to(dev), thresh, 100)
    k = int(num.item())
    compare_keep(keep[:k].cpu().numpy(), dets, thresh, post_max=100, order=np.arange(n, dtype=np.int32))


def test_fused_forms_equal_the_plain_call(dev):
    """sessd_predict's two optional fusions give what the separate launches give, bit for bit:
    * the score-filter keys produced INSIDE the head launch (sessd_ssfa_fuse_head_keys) -- same detections as the call that
      filters the stored head tensor itself, and the same KEY SET as score_filter_kernel would append;
    * the frame's detection record written by the call's last launch == sessd_pack_detections of the outputs (ring rule:
      slot = (cursor + b) % capacity, cursor += batch), also across a wrap of the ring."""
    torch.manual_seed(0)
    B, C = 2, 128
    x0 = torch.randn(B, C, H, W, device=dev)
    x1 = torch.randn(B, C, H, W, device=dev)
    w0, w1 = torch.randn(C, device=dev) * 0.05, torch.randn(C, device=dev) * 0.05
    hw = torch.randn(22, C, device=dev) * 0.08
    hb = torch.randn(22, device=dev) * 0.1
    hb[14:16] = -2.2  # a few hundred to a few thousand candidates above the score threshold
    anchors = torch.from_numpy(pp.create_anchors_3d_range().reshape(-1, 7)).to(dev)
    keys = torch.zeros((B, 2 * H * W), dtype=torch.int64, device=dev)
    kcnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    head = ops.ssfa_fuse_head(x0, x1, w0, w1, 1.1, 0.05, 0.9, -0.03, hw, hb, score_thresh=0.3, keys=keys, key_count=kcnt)
    head_plain = ops.ssfa_fuse_head(x0, x1, w0, w1, 1.1, 0.05, 0.9, -0.03, hw, hb)
    assert torch.equal(head, head_plain)
    # the key set of the stand-alone filter, recomputed on the host from the stored tensor in float32
    hc = head.cpu().numpy()
    for b in range(B):
        s = pp.sigmoid32(hc[b, 14:16].T.reshape(-1))
        n_want = int((s >= np.float32(0.3)).sum())
        n_got = int(kcnt[b].item())
        assert abs(n_got - n_want) <= int((np.abs(s - 0.3) < 1e-6).sum()) and n_got > 100
        aid = (keys[b, :n_got].cpu().numpy() & 0xFFFFFFFF).astype(np.int64)
        assert len(np.unique(aid)) == n_got and (s[aid] >= 0.3 - 1e-6).all()
    plain = ops.predict(head, anchors, None)
    cap = 3
    rec = torch.full((cap, 100, 9), -7.0, device=dev)
    rcnt = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    cur = torch.zeros((1,), dtype=torch.int32, device=dev)
    for rep in range(2):  # second call wraps: slots 2, 0
        fused = ops.predict(head, anchors, None, keys=keys, key_count=kcnt, records=(rec, rcnt, cur))
        for k in ("box", "score", "label", "count"):
            assert torch.equal(fused[k][:, :int(plain["count"].max())] if k != "count" else fused[k],
                               plain[k][:, :int(plain["count"].max())] if k != "count" else plain[k]), k
        assert int(cur.item()) == 2 * (rep + 1)
        for b in range(B):
            slot = (2 * rep + b) % cap
            n = int(plain["count"][b].item())
            assert int(rcnt[slot].item()) == n and n > 5
            r = rec[slot].cpu()
            assert torch.equal(r[:n, :7], plain["box"][b, :n].cpu()) and torch.equal(r[:n, 7], plain["score"][b, :n].cpu())
            assert float(r[:n, 8].abs().max()) == 0 and float(r[n:].abs().max()) == 0


def _valid_rows_equal(got, want, B, T):
    """two predict results, bit for bit in every row a caller may read (rows past a count are never written)"""
    assert set(got) == set(want)
    for k in set(got) - {"box", "score", "label", "di_keep"}:        # count, task_count, di_truncated, di_keep_count
        assert torch.equal(got[k], want[k]), k
    for b in range(B):
        n = int(want["count"][b].item())
        for k in ("box", "score", "label"):
            assert torch.equal(got[k][b, :n], want[k][b, :n]), (b, k)
        for t in range(T if "di_keep" in want else 0):
            n = int(want["di_keep_count"][b, t].item())
            assert torch.equal(got["di_keep"][b, t, :n], want["di_keep"][b, t, :n]), (b, t)


@pytest.mark.parametrize("T,nms_type,pre_max", [(1, "rotate_nms", 64), (3, "rotate_nms", 64), (1, "rotate_weighted_nms", 64),
                                                (3, "rotate_weighted_nms", 64), (1, "rotate_nms", 1300)])
def test_one_predict_object_launched_three_times(dev, T, nms_type, pre_max):
    """One ops.Predict on one head, launched with keys and records bound, then with neither, then with records only: every launch
    == a fresh ops.predict call with the same bindings, bit for bit -- a binding of an earlier launch never reaches a later one
    (the key counts are zeroed after launch 1: a stale key binding would find no candidate; the ring is compared around launch 2).
    Shapes: 10 x 14 pixels (280 anchors per task), B = 2, the seeded head of tests/test_rpn_head_gpu.py whose bias lets a few per
    cent of the anchors pass; post_max 8; pre_max 1300: the suppression mask does not fit the LDS, the record is written by
    pack_detections_kernel. A ring of 3 slots: launch 1 takes slots 0, 1, launch 3 wraps into 2, 0."""
    from sessd_hip import configs
    from test_rpn_head_gpu import B, _inputs, _ref
    Hs, Ws, post = 10, 14, 8
    P = Hs * Ws
    x, up_w, scale, shift, hw, hb = _inputs(T, Hs, Ws, seed=7)
    _, _, head0 = _ref(x, up_w, scale, shift, hw, None)
    hb = hb.clone()
    for t in range(T):   # per task: the 0.95 quantile of its cls logits lands on the 0.3 score threshold
        q = float(torch.quantile(head0[:, t * 22 + 14:t * 22 + 16].reshape(-1), 0.95))
        hb[t * 22 + 14:t * 22 + 16] = float(np.log(0.3 / 0.7)) - q
        hb[t * 22 + 20:t * 22 + 22] = 0.5
    d = lambda v: v.to(dev)
    keys = torch.zeros((B, T, 2 * P), dtype=torch.int64, device=dev)
    kcnt = torch.zeros((B * T,), dtype=torch.int32, device=dev)
    head = ops.rpn_up_head(d(x), d(up_w), d(scale), d(shift), d(hw), d(hb), score_thresh=0.3, keys=keys, key_count=kcnt, num_tasks=T)
    assert int(kcnt.min().item()) > 0
    anchors = torch.from_numpy(np.ascontiguousarray(configs.kitti_3class_anchors((Hs, Ws), [0, -4.0, -3.0, 5.6, 4.0, 1.0]))).float()[:T]
    anc = d(anchors if T > 1 else anchors[0])
    di = dict(nms_cnt_thresh=0.8) if nms_type == "rotate_weighted_nms" else None   # the seeded heads cannot reach the default 2.6
    cap = 3
    ring = lambda: (torch.full((cap, T * post, 9), -7.0, device=dev), torch.full((cap,), -1, dtype=torch.int32, device=dev),
                    torch.zeros((1,), dtype=torch.int32, device=dev))
    mine, theirs = ring(), ring()   # the object's ring and the fresh calls'
    stage = ops.Predict(B, T, P, anc, None, 0.3, pre_max, post, 0.01, nms_type=nms_type, di=di, device=dev)
    cursor = 0
    for launch, (with_keys, with_rec) in enumerate([(True, True), (False, False), (False, True)]):
        ring_before = [v.clone() for v in mine]
        out = stage.launch(head, keys=(keys, kcnt) if with_keys else None, records=mine if with_rec else None)
        fresh = ops.predict(head, anc, None, 0.3, pre_max, post, 0.01, keys=keys if with_keys else None,
                            key_count=kcnt if with_keys else None, records=theirs if with_rec else None, num_tasks=T, nms_type=nms_type,
                            di=di)
        assert out is stage.out
        _valid_rows_equal(out, fresh, B, T)
        count = out["count"].cpu()
        print("launch", launch, "count", count.tolist(), "keys", kcnt.tolist())
        if nms_type == "rotate_nms":
            assert int(count.min()) > 0
        if not with_rec:     # the ring of launch 1 is not touched
            assert all(torch.equal(a, b) for a, b in zip(mine, ring_before))
        else:
            for b in range(B):
                slot = (cursor + b) % cap
                n = int(count[b])
                r = mine[0][slot]
                assert int(mine[1][slot].item()) == n and torch.equal(r, theirs[0][slot])
                assert torch.equal(r[:n, :7], out["box"][b, :n]) and torch.equal(r[:n, 7], out["score"][b, :n])
                assert torch.equal(r[:n, 8], out["label"][b, :n].float()) and bool((r[n:] == 0).all())
            cursor += B
        assert int(mine[2].item()) == cursor == int(theirs[2].item())
        kcnt.zero_()         # from here on a launch that still read the keys of launch 1 would find no candidate


def test_fill_multi(dev):
    a = torch.full((1000003,), 5, dtype=torch.int32, device=dev)[:1000000]   # not a multiple of 4096 words
    b = torch.full((4096 * 3,), 5, dtype=torch.int32, device=dev)
    c = torch.full((7,), 5.0, dtype=torch.float32, device=dev)
    guard = a.clone()
    ops.fill_multi([(a[:999996], 0x7F7F7F7F), (b, 0), (c[:4], 0x3F800000)])
    assert int((a[:999996] != 0x7F7F7F7F).sum()) == 0 and torch.equal(a[999996:], guard[999996:])
    assert int(b.abs().sum()) == 0
    assert torch.equal(c.cpu(), torch.tensor([1.0, 1, 1, 1, 5, 5, 5]))
