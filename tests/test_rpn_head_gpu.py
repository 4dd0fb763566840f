"""sessd_rpn_up_head_tasks (ops.rpn_up_head) alone: the stride-1 up-sampler of the RPN neck (ConvTranspose2d(128, 128, 1) +
folded BatchNorm + ReLU on the f32 matrix cores) fused with the 22-channel heads of T tasks and predict's score filter, against
torch float64 on the same float32 inputs.

Bound: 2e-4 * max |ref| per output tensor, the project's feature tolerance (Numerics). The keys are held bit
for bit: predict fed the launch's keys must return what it returns when it runs its own score filter on the same head tensor.
Shapes: B = 2, 128 channels; 10 x 14 = 140 pixels (two full 64-pixel blocks + a 12-pixel tail, and a partial last 32-pixel MFMA
tile) and 2 x 6 = 12 pixels (less than one block)."""
import numpy as np
import pytest
import torch

from sessd_hip import configs, ops

C = 128
B = 2


def _inputs(T, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * H + W + seed)
    x = torch.randn(B, C, H, W, generator=g)                       # both signs
    up_w = torch.randn(C, C, generator=g) * 0.1                    # [cin][cout], the ConvTranspose2d weight as stored
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    scale[3], scale[64], scale[127] = -0.8, -1.2, -0.6             # negative BatchNorm scales (gamma < 0)
    shift[5], shift[77], shift[96] = -50.0, -60.0, -45.0            # pre-activation negative everywhere: ReLU gives 0
    hw = torch.randn(T * 22, C, generator=g) * 0.05
    hb = torch.randn(T * 22, generator=g) * 0.1
    return x, up_w, scale, shift, hw, hb


def _ref(x, up_w, scale, shift, hw, hb):
    pre = torch.einsum("io,bihw->bohw", up_w.double(), x.double()) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    u = torch.relu(pre)
    head = torch.einsum("oc,bchw->bohw", hw.double(), u)
    if hb is not None:
        head = head + hb.double().view(1, -1, 1, 1)
    return pre, u, head


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H, W", [(10, 14), (2, 6)])
@pytest.mark.parametrize("with_bias, with_out", [(True, True), (False, False), (True, False), (False, True)])
def test_rpn_up_head_against_float64(dev, T, H, W, with_bias, with_out):
    x, up_w, scale, shift, hw, hb = _inputs(T, H, W)
    pre, u, head = _ref(x, up_w, scale, shift, hw, hb if with_bias else None)
    assert bool((pre[:, [5, 77, 96]] < 0).all()) and float(u.max()) > 0 and bool((pre[:, 3] > 0).any()) and bool((pre[:, 3] < 0).any())
    d = lambda t: t.to(dev)
    out = torch.full((B, C, H, W), float("nan"), device=dev) if with_out else None
    got = ops.rpn_up_head(d(x), d(up_w), d(scale), d(shift), d(hw), d(hb) if with_bias else None, out=out, num_tasks=T)
    assert got.shape == (B, T * 22, H * W)
    err = float((got.cpu().double().view(B, T * 22, H, W) - head).abs().max())
    print("head: max err %.3e, bound %.3e" % (err, 2e-4 * float(head.abs().max())))
    assert err <= 2e-4 * float(head.abs().max())
    if with_out:
        eo = float((out.cpu().double() - u).abs().max())
        print("neck output: max err %.3e, bound %.3e" % (eo, 2e-4 * float(u.abs().max())))
        assert eo <= 2e-4 * float(u.abs().max())
        assert float(out[:, [5, 77, 96]].abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
def test_launch_keys_equal_predicts_own_score_filter(dev, T):
    """A cls bias that lets a few per cent of the anchors pass: sessd_predict (T = 3 and T = 1) fed the
    launch's keys == the same call with keys = NULL (its own score filter over the same head tensor), bit for bit."""
    H, W = 10, 14
    P = H * W
    x, up_w, scale, shift, hw, hb = _inputs(T, H, W, seed=7)
    _, _, head0 = _ref(x, up_w, scale, shift, hw, None)
    hb = hb.clone()
    for t in range(T):   # per task: the 0.95 quantile of its cls logits lands on the 0.3 score threshold
        q = float(torch.quantile(head0[:, t * 22 + 14:t * 22 + 16].reshape(-1), 0.95))
        hb[t * 22 + 14:t * 22 + 16] = float(np.log(0.3 / 0.7)) - q
        hb[t * 22 + 20:t * 22 + 22] = 0.5
    d = lambda t: t.to(dev)
    keys = torch.zeros((B, T, 2 * P), dtype=torch.int64, device=dev)
    kcnt = torch.zeros((B * T,), dtype=torch.int32, device=dev)
    head = ops.rpn_up_head(d(x), d(up_w), d(scale), d(shift), d(hw), d(hb), score_thresh=0.3, keys=keys, key_count=kcnt, num_tasks=T)
    plain = ops.rpn_up_head(d(x), d(up_w), d(scale), d(shift), d(hw), d(hb), num_tasks=T)
    assert torch.equal(head, plain)   # the filter does not disturb the head tensor
    kc = kcnt.cpu().numpy()
    assert ((kc > 0) & (kc < 2 * P // 4)).all(), kc   # a few per cent of the 280 anchors of every (frame, task)
    hv = head.view(B, T, 22, P)
    for b in range(B):
        for t in range(T):   # the key set itself: anchors whose sigmoid(cls) >= 0.3, each once
            n = int(kc[b * T + t])
            aid = (keys[b, t, :n] & 0xFFFFFFFF).sort()[0].cpu().tolist()
            sg = torch.sigmoid(hv[b, t, 14:16].T.reshape(-1).cpu().double())   # anchor id = 2 * pixel + a
            assert len(set(aid)) == n and set(torch.nonzero(sg >= 0.3 + 1e-6).reshape(-1).tolist()) <= set(aid), (b, t)
            assert set(aid) <= set(torch.nonzero(sg >= 0.3 - 1e-6).reshape(-1).tolist()), (b, t)
    anchors = torch.from_numpy(np.ascontiguousarray(configs.kitti_3class_anchors((H, W), [0, -4.0, -3.0, 5.6, 4.0, 1.0]))).float()[:T]
    anc = d(anchors if T > 1 else anchors[0])
    kw = dict(score_thresh=0.3, pre_max=1000, post_max=100, nms_thresh=0.01, num_tasks=T)
    with_keys = ops.predict(head, anc, keys=keys, key_count=kcnt, **kw)
    own = ops.predict(head, anc, **kw)
    assert torch.equal(with_keys["count"], own["count"]) and int(own["count"].sum().item()) > 0
    if T > 1:
        assert torch.equal(with_keys["task_count"], own["task_count"])
    for b in range(B):
        n = int(own["count"][b].item())
        for k in ("box", "score", "label"):
            assert torch.equal(with_keys[k][b, :n], own[k][b, :n]), (b, k)


def test_entry_point_checks_its_arguments():
    """Before any device call (fake non-null pointers, never dereferenced; no GPU needed): channels == 128 only, 1 <= T <= 4,
    null tensors, keys without their counts. SESSD_EINVAL = -1."""
    import sessd_hip
    lib = sessd_hip.lib
    p = 16
    call = lambda x=p, w=p, sc=p, sh=p, ch=128, hw=p, T=3, ho=p, keys=None, cap=0, kc=None, batch=1, npix=64: \
        lib.sessd_rpn_up_head_tasks(x, w, sc, sh, batch, ch, npix, None, hw, None, T, ho, 0.3, keys, cap, kc, None)
    assert call(ch=64) == -1 and call(ch=256) == -1
    assert call(T=5) == -1 and call(T=0) == -1 and ops.MAX_TASKS == 4
    assert call(x=None) == -1 and call(w=None) == -1 and call(sc=None) == -1 and call(sh=None) == -1
    assert call(hw=None) == -1 and call(ho=None) == -1
    assert call(keys=p, cap=128) == -1 and call(kc=p) == -1 and call(keys=p, cap=0, kc=p) == -1
    assert call(batch=0) == -1 and call(npix=0) == -1 and call(npix=1 << 23) == -1   # 32-bit buffer offsets per batch element
    with pytest.raises(ValueError):
        ops.check_num_tasks(5)
