"""Multi-task heads at kernel level: sessd_ssfa_fuse_head_tasks and sessd_predict (ops.ssfa_fuse_head / ops.predict with
num_tasks > 1) against the single-task entry points (bit for bit), a float64 restatement and the CPU oracle.

Tolerances are the existing tests' own: head planes within 2e-5 * max(1, |ref|max) of float64 (tests/test_dense_conv_gpu.py::
test_ssfa_fuse_with_heads); detections against oracle.postprocess.predict_frame with the figures of tests/test_postprocess_gpu.py
(boxes 1e-4 m / rad, scores 1e-5 relative) under oracle.compare.compare_detections' strict rule, which accepts a difference only
when the oracle lists a near-threshold NMS decision that explains it."""
import numpy as np
import pytest
import torch

from oracle import postprocess as pp
from oracle.compare import compare_detections
from sessd_hip import ops, synth

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ fused SSFA tail + heads
def _fuse_inputs(C, T, B=2, H=7, W=10):
    g = torch.Generator().manual_seed(100 * C + T)
    x0, x1 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    w0, w1 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    hw, hb = torch.randn(T * 22, C, generator=g) * 0.05, torch.randn(T * 22, generator=g) * 0.1
    hb.view(T, 22)[:, 14:16] = -0.6  # sigmoid(-0.6 +- 0.6) around the 0.3 threshold: every (frame, task) has keys and non-keys
    return x0, x1, w0, w1, hw, hb


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("T", [2, 3])
def test_fused_head_tasks(dev, C, T):
    """B = 2, 70 pixels (one full 64-pixel block + a 6-pixel tail): task t's 22 planes and key set == the single-task launch
    with task t's weights, bit for bit; planes within the fused-head test's tolerance of float64."""
    B, H, W = 2, 7, 10
    P = H * W
    x0, x1, w0, w1, hw, hb = _fuse_inputs(C, T, B, H, W)
    s0, t0, s1, t1 = 1.3, -0.2, 0.7, 0.1
    d = lambda t: t.to(dev)
    X0, X1, W0, W1, HW, HB = d(x0), d(x1), d(w0), d(w1), d(hw), d(hb)
    keys = torch.zeros((B, T, 2 * P), dtype=torch.int64, device=dev)
    kcnt = torch.zeros((B * T,), dtype=torch.int32, device=dev)
    out = torch.full((B, C, H, W), float("nan"), device=dev)
    got = ops.ssfa_fuse_head(X0, X1, W0, W1, s0, t0, s1, t1, HW, HB, out=out, score_thresh=0.3, keys=keys, key_count=kcnt,
                             num_tasks=T)
    assert got.shape == (B, T * 22, P)
    nokeys = ops.ssfa_fuse_head(X0, X1, W0, W1, s0, t0, s1, t1, HW, HB, num_tasks=T)
    assert torch.equal(got, nokeys)
    kc = kcnt.view(B, T).cpu().numpy()
    for t in range(T):
        k1 = torch.zeros((B, 2 * P), dtype=torch.int64, device=dev)
        c1 = torch.zeros((B,), dtype=torch.int32, device=dev)
        o1 = torch.full((B, C, H, W), float("nan"), device=dev)
        one = ops.ssfa_fuse_head(X0, X1, W0, W1, s0, t0, s1, t1, HW[t * 22:(t + 1) * 22].contiguous(),
                                 HB[t * 22:(t + 1) * 22].contiguous(), out=o1, score_thresh=0.3, keys=k1, key_count=c1)
        assert torch.equal(got.view(B, T, 22, P)[:, t], one), t
        assert torch.equal(out, o1)
        for b in range(B):
            n = int(c1[b].item())
            assert int(kc[b, t]) == n and 0 < n < 2 * P
            assert torch.equal(torch.sort(keys[b, t, :n])[0], torch.sort(k1[b, :n])[0]), (b, t)
    # float64 restatement (tests/test_dense_conv_gpu.py::test_ssfa_fuse_with_heads)
    a = (x0.double() * w0.double().view(1, -1, 1, 1)).sum(1) * s0 + t0
    b_ = (x1.double() * w1.double().view(1, -1, 1, 1)).sum(1) * s1 + t1
    p = torch.softmax(torch.stack([a, b_], 1), 1)
    ssfa = x0.double() * p[:, 0:1] + x1.double() * p[:, 1:2]
    head = torch.einsum("oc,bchw->bohw", hw.double(), ssfa) + hb.double().view(1, -1, 1, 1)
    assert float((got.cpu().double().view(B, T * 22, H, W) - head).abs().max()) < 2e-5 * max(1.0, float(head.abs().max()))
    assert float((out.cpu().double() - ssfa).abs().max()) < 1e-5 * max(1.0, float(ssfa.abs().max()))


@pytest.mark.parametrize("C", [128, 64])
def test_one_task_through_the_tasks_entry_point(dev, C):
    """num_tasks = 1 through sessd_ssfa_fuse_head_tasks itself == sessd_ssfa_fuse_head_keys, planes and keys."""
    B, H, W = 2, 7, 10
    P = H * W
    x0, x1, w0, w1, hw, hb = [t.to(dev) for t in _fuse_inputs(C, 1, B, H, W)]
    k_old = torch.zeros((B, 2 * P), dtype=torch.int64, device=dev)
    c_old = torch.zeros((B,), dtype=torch.int32, device=dev)
    old = ops.ssfa_fuse_head(x0, x1, w0, w1, 1.3, -0.2, 0.7, 0.1, hw, hb, score_thresh=0.3, keys=k_old, key_count=c_old)
    k_new, c_new = torch.zeros_like(k_old), torch.zeros_like(c_old)
    new = torch.empty_like(old)
    ops.check(ops.lib.sessd_ssfa_fuse_head_tasks(x0.data_ptr(), x1.data_ptr(), w0.data_ptr(), w1.data_ptr(), 1.3, -0.2, 0.7, 0.1, B, C,
                                                 P, 0, hw.data_ptr(), hb.data_ptr(), 1, new.data_ptr(), 0.3, k_new.data_ptr(), 2 * P,
                                                 c_new.data_ptr(), torch.cuda.current_stream().cuda_stream), "ssfa_fuse_head_tasks")
    assert torch.equal(old, new) and torch.equal(c_old, c_new)
    for b in range(B):
        n = int(c_old[b].item())
        assert n > 0 and torch.equal(torch.sort(k_old[b, :n])[0], torch.sort(k_new[b, :n])[0])


# ------------------------------------------------------------------ predict
B, T, H, W = 2, 3, 40, 32          # 2560 anchors per task
P = H * W
TASK_ANCHORS = [((1.6, 3.9, 1.56), -1.0), ((0.6, 0.8, 1.73), -0.6), ((0.6, 1.76, 1.73), -0.6)]
NMS_THRESH, POST_MAX = 0.01, 8


def _task_head(seed, kind):
    """The recipe of tests/test_postprocess_gpu.py::_make_head on the 40 x 32 map. kind 'all': every anchor above the score
    threshold (2560 keys: more than one 2048-key sort pass); 'none': cls logits forced to -20; 'few': a few dozen candidates."""
    rng = np.random.RandomState(seed)
    head = np.zeros((22, P), np.float32)
    head[:14] = rng.normal(0, 0.25, (14, P))
    head[14:16] = -4.0 + rng.normal(0, 0.5, (2, P))
    head[16:20] = rng.normal(0, 1.0, (4, P))
    head[20:22] = rng.uniform(-0.2, 1.0, (2, P))
    if kind == "all":
        head[14:16] = rng.uniform(0.0, 3.0, (2, P))
    elif kind == "none":
        head[14:16] = -20.0
    else:
        for _ in range(2):
            cy, cx = rng.randint(5, H - 5), rng.randint(5, W - 5)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    head[14 + rng.randint(2), (cy + dy) * W + cx + dx] = rng.uniform(-0.5, 3.0)
    return head


def _split(head):
    box = head[:14].reshape(2, 7, P).transpose(2, 0, 1).reshape(-1, 7)
    cls = head[14:16].T.reshape(-1)
    dirl = head[16:20].reshape(2, 2, P).transpose(2, 0, 1).reshape(-1, 2)
    iou = head[20:22].T.reshape(-1)
    return box, cls, dirl, iou


@pytest.fixture(scope="module")
def scene():
    heads = np.stack([np.stack([_task_head(10 * b + t, kind) for t, kind in enumerate(("all", "none", "few"))]) for b in range(B)])
    anchors = np.stack([pp.create_anchors_3d_range((1, H, W), (0, -40.0, z, 70.4, 40.0, z), sizes).reshape(-1, 7)
                        for sizes, z in TASK_ANCHORS]).astype(np.float32)
    cal = synth.kitti_calib()
    fr0 = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], cal["image_shape"])
    shape1 = (cal["image_shape"][0], cal["image_shape"][1] // 2)  # frame 1: the left half of the image only
    fr1 = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], shape1)
    assert not np.array_equal(fr0, fr1)
    return dict(heads=heads, anchors=anchors, frusta=[fr0, fr1])


def _oracle(scene, cache, pre_max, use_frustum):
    key = (pre_max, use_frustum)
    if key not in cache:
        res = {}
        for b in range(B):
            for t in range(T):
                args = _split(scene["heads"][b, t]) + (scene["anchors"][t], scene["frusta"][b] if use_frustum else None, 0.3, pre_max,
                                                     POST_MAX, NMS_THRESH)
                want, dbg = pp.predict_frame(*args, return_debug=True)
                dbg["rerun"] = (lambda a: (lambda forced: pp.predict_frame(*a, forced=forced)))(args)
                res[b, t] = (want, dbg)
        cache[key] = res
    return cache[key]


_ORACLE_CACHE = {}


@pytest.mark.parametrize("pre_max", [64, 1500])   # LDS-resident walk with the cap binding for task 0 / the pre_max > ~1280 fallback
@pytest.mark.parametrize("use_frustum", [False, True])
def test_predict_tasks(dev, scene, pre_max, use_frustum):
    head = torch.from_numpy(scene["heads"].reshape(B, T * 22, P)).to(dev)
    anchors = torch.from_numpy(scene["anchors"]).to(dev)
    fr = torch.from_numpy(np.stack(scene["frusta"])).to(dev) if use_frustum else None
    box = torch.full((B, T * POST_MAX, 7), float("nan"), device=dev)
    score = torch.full((B, T * POST_MAX), float("nan"), device=dev)
    label = torch.full((B, T * POST_MAX), -9, dtype=torch.int32, device=dev)
    out = dict(box=box, score=score, label=label, count=torch.full((B,), -1, dtype=torch.int32, device=dev),
               task_count=torch.full((B, T), -1, dtype=torch.int32, device=dev))
    ops.predict(head, anchors, fr, 0.3, pre_max, POST_MAX, NMS_THRESH, out=out, num_tasks=T)
    count, tcount = out["count"].cpu().numpy(), out["task_count"].cpu().numpy()
    # per-frame anchors (B, T, A, 7): the same detections
    out_pf = ops.predict(head, anchors[None].expand(B, T, 2 * P, 7).contiguous(), fr, 0.3, pre_max, POST_MAX, NMS_THRESH, num_tasks=T)
    want = _oracle(scene, _ORACLE_CACHE, pre_max, use_frustum)
    hv = head.view(B, T, 22, P)
    for b in range(B):
        assert int(count[b]) == int(tcount[b].sum())                       # (b) merged count
        n = int(count[b])
        assert torch.equal(out_pf["box"][b, :n], box[b, :n]) and torch.equal(out_pf["count"], out["count"])
        # rows past the count are never written (the caller never reads them)
        assert bool(torch.isnan(box[b, n:]).all()) and bool(torch.isnan(score[b, n:]).all()) and bool((label[b, n:] == -9).all())
        assert tcount[b, 1] == 0 and tcount[b, 0] > 0
        start = 0
        for t in range(T):
            nt = int(tcount[b, t])
            sl = slice(start, start + nt)
            # (a) == the single-task call on this task's planes and anchors, bit for bit
            one = ops.predict(hv[:, t].contiguous(), anchors[t], fr, 0.3, pre_max, POST_MAX, NMS_THRESH)
            assert int(one["count"][b].item()) == nt, (b, t)
            assert torch.equal(one["box"][b, :nt], box[b, sl]) and torch.equal(one["score"][b, :nt], score[b, sl]), (b, t)
            assert bool((label[b, sl] == t).all())                            # (b) order and labels
            # (c) the CPU oracle on this task's slice
            w, dbg = want[b, t]
            if t == 0:
                assert dbg["num_candidates"] == 2 * P > 2048 and dbg["topk"] == pre_max
            if t == 2:
                assert 12 <= dbg["num_candidates"] <= 100
            got = dict(box3d_lidar=box[b, sl].cpu().numpy(), scores=score[b, sl].cpu().numpy())
            r = compare_detections(got, dict(box3d_lidar=w["box3d_lidar"], scores=w["scores"]), dbg, box_tol=1e-4, score_rtol=1e-5)
            assert r["matched"] == r["n"] == nt
            start += nt
    if not use_frustum:
        assert (tcount[:, 0] == POST_MAX).all()                            # the post_max cap binds for task 0


@pytest.mark.parametrize("pre_max", [64, 1500])
def test_predict_tasks_records(dev, scene, pre_max):
    """Two consecutive calls with a ring of 3 frames: slots 0, 1 then 2, 0; each record = the frame's merged rows [box | score |
    label], zero past the count; the cursor advances by the batch, not by batch * tasks."""
    head = torch.from_numpy(scene["heads"].reshape(B, T * 22, P)).to(dev)
    anchors = torch.from_numpy(scene["anchors"]).to(dev)
    plain = ops.predict(head, anchors, None, 0.3, pre_max, POST_MAX, NMS_THRESH, num_tasks=T)
    cap = 3
    rec = torch.full((cap, T * POST_MAX, 9), -7.0, device=dev)
    rcnt = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    cur = torch.zeros((1,), dtype=torch.int32, device=dev)
    for rep in range(2):
        got = ops.predict(head, anchors, None, 0.3, pre_max, POST_MAX, NMS_THRESH, records=(rec, rcnt, cur), num_tasks=T)
        assert torch.equal(got["count"], plain["count"]) and torch.equal(got["task_count"], plain["task_count"])
        assert int(cur.item()) == B * (rep + 1)
        for b in range(B):
            slot = (B * rep + b) % cap
            n = int(plain["count"][b].item())
            assert int(rcnt[slot].item()) == n and n > POST_MAX
            r = rec[slot]
            assert torch.equal(r[:n, :7], plain["box"][b, :n]) and torch.equal(r[:n, 7], plain["score"][b, :n])
            assert torch.equal(r[:n, 8], plain["label"][b, :n].float()) and float(r[n:].abs().max()) == 0
            assert int(r[:n, 8].max().item()) == 2
    assert int(rcnt[1].item()) == int(plain["count"][1].item())             # slot 1 was written once, by the first call
