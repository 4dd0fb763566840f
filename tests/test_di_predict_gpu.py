"""DI-NMS as the post-processor of the fused predict call (sessd_predict with args->di, ops.predict(nms_type="rotate_weighted_nms")) at
kernel level, per (frame, task), against the CPU helper tests/di_predict_ref.py, on the 40 x 32 map, the `_task_head` recipe and
the TASK_ANCHORS of tests/test_multitask_head_gpu.py (2560 anchors per task), B = 2, T in {1, 3}.

Tolerances are the project's own for this core (tests/test_di_nms_gpu.py): keep lists EQUAL, boxes atol 2e-4, scores atol 1e-5,
labels equal. The seeded heads cannot reach cnt > 2.6 (a candidate's neighbours overlap it by 0.1 - 0.4), so the calls pass
nms_cnt_thresh = 0.8 (both branches of the core on the 'few' heads) or 1.2 (both branches on the 'all' heads) through the new
setting. Preconditions on the inputs are asserted on the CPU side: see _ref()."""
import numpy as np
import pytest
import torch

import di_predict_ref as R
from oracle import postprocess as pp
from sessd_hip import ops, synth
from test_multitask_head_gpu import H, P, TASK_ANCHORS, W, _split, _task_head

pytestmark = pytest.mark.gpu
B, T = 2, 3
DI = "rotate_weighted_nms"


def _counted_head(seed, k):
    """Exactly k candidates, clustered: the 'none' head with k anchors of a block of neighbouring pixels above the threshold."""
    rng = np.random.RandomState(seed)
    head = _task_head(seed, "none")
    y0, x0 = rng.randint(4, H - 12), rng.randint(4, W - 12)
    for i in range(k):
        pix, a = i // 2, i % 2
        head[14 + a, (y0 + pix // 8) * W + x0 + pix % 8] = rng.uniform(0.0, 3.0)
    return head


def _scene(kinds):
    """kinds[b][t]: 'all' / 'none' / 'few' or a candidate count."""
    heads = np.stack([np.stack([_counted_head(100 + 10 * b + t, k) if isinstance(k, int) else _task_head(10 * b + t, k)
                                for t, k in enumerate(row)]) for b, row in enumerate(kinds)])
    anchors = np.stack([pp.create_anchors_3d_range((1, H, W), (0, -40.0, z, 70.4, 40.0, z), sizes).reshape(-1, 7)
                        for sizes, z in TASK_ANCHORS]).astype(np.float32)
    cal = synth.kitti_calib()
    fr0 = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], cal["image_shape"])
    fr1 = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], (cal["image_shape"][0], cal["image_shape"][1] // 2))
    return dict(kinds=kinds, heads=heads, anchors=anchors, frusta=[fr0, fr1])


SCENES = dict(main=_scene([("all", "none", "few"), ("all", "none", "few")]),
              edge=_scene([(63, 64, 65), (1, "few", 65)]))
_REF = {}


def _ref(name, cnt, pre_max, post_max, use_frustum):
    """The CPU helper per (frame, task), computed once per configuration and shared. Preconditions (CPU side, so that a bad seed
    fails loudly instead of hiding a flip): the damped scores recomputed in float64 and rounded leave the keep list unchanged;
    at cnt 0.8 every 'few' case keeps at least two boxes and has at least one pass that was not kept."""
    key = (name, cnt, pre_max, post_max, use_frustum)
    if key not in _REF:
        sc, res = SCENES[name], {}
        for b in range(B):
            for t in range(T):
                args = _split(sc["heads"][b, t]) + (sc["anchors"][t], sc["frusta"][b] if use_frustum else None, 0.3, pre_max, post_max,
                                                    dict(nms_cnt_thresh=cnt))
                r = R.predict_task(*args)
                r64 = R.predict_task(*args, score_dtype=np.float64, with_replay=False)
                assert r64["full_keep"] == r["full_keep"], ("a near-tie decides a pick", name, b, t)
                kind = sc["kinds"][b][t]
                if isinstance(kind, int):
                    assert r["n_top"] == kind
                if kind == "few" and cnt == 0.8 and post_max == 100:
                    assert 12 <= r["n_top"] <= 100 and len(r["keep"]) >= 2 and r["unkept_passes"] >= 1, (name, b, t)
                if kind == "all":
                    assert r["n_top"] == min(pre_max, 2 * P) and len(r["full_keep"]) > 8
                res[b, t] = r
        _REF[key] = res
    return _REF[key]


def _call(dev, name, cnt, pre_max, post_max, use_frustum, records=None, sticky=None, **kw):
    sc = SCENES[name]
    head = torch.from_numpy(sc["heads"].reshape(B, T * 22, P)).to(dev)
    anchors = torch.from_numpy(sc["anchors"]).to(dev)
    fr = torch.from_numpy(np.stack(sc["frusta"])).to(dev) if use_frustum else None
    out = dict(box=torch.full((B, T * post_max, 7), float("nan"), device=dev), score=torch.full((B, T * post_max), float("nan"), device=dev),
               label=torch.full((B, T * post_max), -9, dtype=torch.int32, device=dev),
               count=torch.full((B,), -1, dtype=torch.int32, device=dev), task_count=torch.full((B, T), -1, dtype=torch.int32, device=dev),
               di_truncated=torch.full((B, T), -1, dtype=torch.int32, device=dev))
    ops.predict(head, anchors, fr, 0.3, pre_max, post_max, 0.01, out=out, records=records, num_tasks=T, nms_type=DI,
                di=dict(nms_cnt_thresh=cnt), sticky=sticky, **kw)
    return head, anchors, fr, out


def _check_against_ref(out, want, post_max):
    """count, concatenation order, label == task, keep lists, boxes / scores per (frame, task); prints the measured maxima."""
    count, tcount = out["count"].cpu().numpy(), out["task_count"].cpu().numpy()
    kc, keep = out["di_keep_count"].cpu().numpy(), out["di_keep"].cpu().numpy()
    trunc = out["di_truncated"].cpu().numpy()
    box, score, label = out["box"].cpu().numpy(), out["score"].cpu().numpy(), out["label"].cpu().numpy()
    emax = [0.0, 0.0]
    for b in range(B):
        assert int(count[b]) == int(tcount[b].sum())
        n = int(count[b])
        # rows past the count are never written: no NaN of a lone candidate's normalised score can reach a row
        assert np.isnan(box[b, n:]).all() and np.isnan(score[b, n:]).all() and (label[b, n:] == -9).all()
        assert not np.isnan(box[b, :n]).any() and not np.isnan(score[b, :n]).any()
        start = 0
        for t in range(T):
            w = want[b, t]
            assert keep[b, t, :kc[b, t]].tolist() == w["keep"], (b, t)            # keep lists equal
            assert int(trunc[b, t]) == w["truncated"], (b, t)
            nt = int(tcount[b, t])
            assert nt == len(w["scores"]), (b, t)
            sl = slice(start, start + nt)
            assert (label[b, sl] == t).all()
            if nt:
                eb, es = float(np.abs(box[b, sl] - w["box3d_lidar"]).max()), float(np.abs(score[b, sl] - w["scores"]).max())
                emax = [max(emax[0], eb), max(emax[1], es)]
                assert eb <= 2e-4 and es <= 1e-5, (b, t, eb, es)
            start += nt
    print("max |box - ref| %.3g, max |score - ref| %.3g" % tuple(emax))
    return tcount


@pytest.mark.parametrize("cnt", [0.8, 1.2])
@pytest.mark.parametrize("use_frustum", [False, True])
def test_predict_di_vs_cpu_helper(dev, cnt, use_frustum):
    """'all' (2560 keys: the top-k cut at pre_max = 1000, a full 1000-candidate workgroup), 'none' (count 0), 'few' (clustered)."""
    want = _ref("main", cnt, 1000, 100, use_frustum)
    _, _, _, out = _call(dev, "main", cnt, 1000, 100, use_frustum)
    tc = _check_against_ref(out, want, 100)
    assert (tc[:, 1] == 0).all() and (tc[:, 0] > 8).all()
    if cnt == 0.8 and not use_frustum:
        assert (tc[:, 2] >= 2).all()
        assert (out["di_truncated"].cpu().numpy()[:, 2] == 0).all()               # capacity: 'few' with post_max = 100


def test_predict_di_edge_counts(dev):
    """63, 64 and 65 candidates in one (frame, task) (partial wave, exact wave, crossing a wave) and a head with exactly ONE
    candidate: softmax 1, score 0, NaN normalised score, cnt <= 1 -> no detection and no NaN in any output or record row."""
    want = _ref("edge", 0.8, 1000, 100, False)
    assert want[1, 0]["n_top"] == 1 and want[1, 0]["keep"] == [] and sum(len(want[0, t]["keep"]) for t in range(T)) >= 3
    cap = 2
    rec = torch.full((cap, T * 100, 9), float("nan"), device=dev)
    rcnt = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    cur = torch.zeros((1,), dtype=torch.int32, device=dev)
    _, _, _, out = _call(dev, "edge", 0.8, 1000, 100, False, records=(rec, rcnt, cur))
    tc = _check_against_ref(out, want, 100)
    assert tc[1, 0] == 0 and int(out["di_keep_count"][1, 0].item()) == 0
    assert int(cur.item()) == B and not bool(torch.isnan(rec).any())
    for b in range(B):
        n = int(out["count"][b].item())
        assert int(rcnt[b].item()) == n
        assert torch.equal(rec[b, :n, :7], out["box"][b, :n]) and torch.equal(rec[b, :n, 7], out["score"][b, :n])
        assert torch.equal(rec[b, :n, 8], out["label"][b, :n].float()) and float(rec[b, n:].abs().max()) == 0


def test_predict_di_capacity(dev):
    """post_max = 8 on the 'all' heads: the rows are the helper's keep list cut at 8, then filtered, and di_truncated == 1."""
    want = _ref("main", 0.8, 1000, 8, True)
    assert all(len(want[b, 0]["full_keep"]) > 8 and want[b, 0]["truncated"] == 1 for b in range(B))
    sticky = torch.zeros((1,), dtype=torch.int32, device=dev)
    _, _, _, quiet = _call(dev, "edge", 0.8, 1000, 100, True, sticky=sticky)   # nothing truncated ...
    assert int(sticky.item()) == 0 and not bool(quiet["di_truncated"].any())
    _, _, _, out = _call(dev, "main", 0.8, 1000, 8, True, sticky=sticky)
    assert int(sticky.item()) == 1
    _check_against_ref(out, want, 8)
    tr = out["di_truncated"].cpu().numpy()
    assert (tr[:, 0] == 1).all() and (tr[:, 1] == 0).all()
    assert (out["di_keep_count"].cpu().numpy()[:, 0] == 8).all()
    _call(dev, "edge", 0.8, 1000, 100, True, sticky=sticky)   # ... and the flag is sticky: only ever ORed into
    assert int(sticky.item()) == 1


@pytest.mark.parametrize("name", ["main", "edge"])
def test_predict_di_virtual_frames(dev, name):
    """Task t's rows of a T = 3 call == a T = 1 call on task t's head planes and anchors, bit for bit."""
    head, anchors, fr, out = _call(dev, name, 0.8, 1000, 100, True)
    hv = head.view(B, T, 22, P)
    tc = out["task_count"].cpu().numpy()
    for t in range(T):
        one = ops.predict(hv[:, t].contiguous(), anchors[t], fr, 0.3, 1000, 100, 0.01, nms_type=DI, di=dict(nms_cnt_thresh=0.8))
        assert one["box"].shape == (B, 100, 7) and one["task_count"].shape == (B, 1)
        for b in range(B):
            nt, st = int(tc[b, t]), int(tc[b, :t].sum())
            assert int(one["count"][b].item()) == nt == int(one["task_count"][b, 0].item()), (b, t)
            assert torch.equal(one["box"][b, :nt], out["box"][b, st:st + nt]) and torch.equal(one["score"][b, :nt], out["score"][b, st:st + nt])
            assert bool((one["label"][b, :nt] == 0).all())
            assert torch.equal(one["di_keep_count"][b, 0], out["di_keep_count"][b, t]) and torch.equal(one["di_truncated"][b, 0], out["di_truncated"][b, t])


def test_predict_di_agrees_with_the_operator_path(dev):
    """The same candidates through the mirror's host-wrapped box_torch_ops.rotate_weighted_nms (-> sessd_di_nms): the same keep
    list, boxes / scores within the tolerances."""
    from det3d.core.bbox import box_torch_ops as bto
    want = _ref("main", 0.8, 1000, 100, False)
    _, _, _, out = _call(dev, "main", 0.8, 1000, 100, False)
    tc = out["task_count"].cpu().numpy()
    for b in range(B):
        for t in (0, 2):
            c = want[b, t]["cand"]
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            anc = np.zeros((len(c["score"]), 7), np.float32)
            anc[:, :2] = c["anchor_xy"]
            box = d(c["box"])
            res = bto.rotate_weighted_nms(box, box[:, [0, 1, 3, 4, 6]].contiguous(), d(c["dir"]), d(np.zeros(len(anc), np.int64)),
                                          d(c["score"].copy()), d(c["iou_pred"]), d(anc), enable_centerness=True, centerness_pow=2,
                                          nms_cnt_thresh=0.8)
            kc = int(out["di_keep_count"][b, t].item())
            # the operator has no capacity: its keep list is cut at post_max here, like the helper's
            assert res[4].cpu().tolist() == want[b, t]["full_keep"] and (t != 0 or len(want[b, t]["full_keep"]) > 100)
            assert res[4].cpu().tolist()[:100] == out["di_keep"][b, t, :kc].cpu().tolist() == want[b, t]["keep"], (b, t)
            # no frustum and every averaged box inside the range: the fused rows are the operator's boxes after the direction fix
            nt, st = int(tc[b, t]), int(tc[b, :t].sum())
            ob, od, osc = res[0].cpu().numpy()[:100], res[1].cpu().numpy()[:100], res[3].cpu().numpy()[:100]
            ob[:, 6] += np.where((ob[:, 6] > 0) ^ (od == 1), np.float32(np.pi), np.float32(0)).astype(np.float32)
            pr = np.array([0, -40.0, -5.0, 70.4, 40.0, 5.0], np.float32)
            m = (ob[:, :3] >= pr[:3]).all(1) & (ob[:, :3] <= pr[3:]).all(1)
            assert nt == int(m.sum())
            assert np.allclose(out["box"][b, st:st + nt].cpu().numpy(), ob[m], atol=2e-4)
            assert np.allclose(out["score"][b, st:st + nt].cpu().numpy(), osc[m], atol=1e-5)


@pytest.mark.parametrize("name", ["main", "edge"])
def test_default_path_untouched(dev, name):
    """nms_type="rotate_nms" and no nms_type: bit-identical outputs and records, T = 3 and T = 1."""
    sc = SCENES[name]
    head = torch.from_numpy(sc["heads"].reshape(B, T * 22, P)).to(dev)
    anchors = torch.from_numpy(sc["anchors"]).to(dev)
    res = []
    for kw in (dict(), dict(nms_type="rotate_nms")):
        rec = (torch.full((2, T * 8, 9), -7.0, device=dev), torch.full((2,), -1, dtype=torch.int32, device=dev),
               torch.zeros((1,), dtype=torch.int32, device=dev))
        o = ops.predict(head, anchors, None, 0.3, 1000, 8, 0.01, records=rec, num_tasks=T, **kw)
        o1 = ops.predict(head.view(B, T, 22, P)[:, 0].contiguous(), anchors[0], None, 0.3, 1000, 8, 0.01, **kw)
        res.append((o, rec, o1))
    (a, ra, a1), (b_, rb, b1) = res
    assert "di_truncated" not in a and "task_count" not in a1
    assert torch.equal(a["count"], b_["count"]) and torch.equal(a["task_count"], b_["task_count"]) and torch.equal(a1["count"], b1["count"])
    for b in range(B):
        n, n1 = int(a["count"][b].item()), int(a1["count"][b].item())
        for k in ("box", "score", "label"):
            assert torch.equal(a[k][b, :n], b_[k][b, :n]) and torch.equal(a1[k][b, :n1], b1[k][b, :n1])
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    if name == "main":
        assert int(a["count"].min().item()) > 8


def test_too_many_candidates_for_di(dev):
    head, anchors = torch.zeros((1, 22, P), device=dev), torch.zeros((2 * P, 7), device=dev)
    with pytest.raises(ValueError, match="1024"):
        ops.predict(head, anchors, pre_max=1500, nms_type=DI)
    with pytest.raises(ValueError, match="nms_type"):
        ops.predict(head, anchors, nms_type="nms")
