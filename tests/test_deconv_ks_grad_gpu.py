"""sessd_deconv_ks_dgrad / sessd_deconv_ks_wgrad (csrc/deconv_ks_grad.hip) and ops.DeconvKsFunction: the data and weight gradient of
ConvTranspose2d(cin, cout, s, stride=s), s in {1, 2, 4}, against torch float64 on the CPU (torch.autograd.grad of
F.conv_transpose2d(x64, w64, stride=s) against a random gout).

Bound, per element, derived and not measured: (K + 2) * 2^-24 * sum |a| |b|, the sum of absolute products formed in float64 (the
same convolution on |.| inputs); K = cout * s * s for gin, K = B * H * W for gW. A float32 fma chain of K terms in ANY order --
and so any split into partial sums that are added afterwards -- stays inside (K - 1 roundings of the running sum + what the
inputs' own conversion costs: none here, the inputs are float32 numbers).

Channels (cin, cout): (6, 32) less than one cin block, (34, 96) one block and a part, three cout blocks (no multiple of the
forward's four-block group), (64, 32) two cin blocks. Maps: (5, 7) = 35 pixels, odd width, a 32-pixel tile that straddles rows with a
three-pixel tail (wgrad: five stages of 8 pixels, the last with 3); (1, 1) with B = 3. Depth: B = 2, 41 x 37, cin 64, cout 32, s = 2 --
by the kernel's own chunk rule (the header: tiles = 1 * 1 * 2, clamp(2048 / 2, 8, 128) = 128, stages = 2 * ceil(1517 / 8) = 380)
128 chunk partials of two or three stages each are added, and the last stage of each image holds 5 of 8 pixels; the test reads the
chunk count back from the workspace size. Every case takes milliseconds."""
import pytest
import torch
import torch.nn.functional as F

from sessd_hip import lib, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _case(B, cin, cout, s, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * s + 10 * cin + cout + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w = (torch.rand(cin, cout, s, s, generator=g) * 2 - 1) * (3.0 / cin) ** 0.5
    gout = torch.randn(B, cout, s * H, s * W, generator=g)
    return x, w, gout


def _reference(x, w, gout, s):
    """(gin, gW, bound_gin, bound_gW) in float64"""
    def grads(x64, w64, g64):
        x64, w64 = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
        return torch.autograd.grad(F.conv_transpose2d(x64, w64, stride=s), (x64, w64), g64)
    gin, gw = grads(x.double(), w.double(), gout.double())
    ain, aw = grads(x.double().abs(), w.double().abs(), gout.double().abs())
    B, cin, H, W = x.shape
    cout = w.shape[1]
    return gin, gw, (cout * s * s + 2) * U * ain, (B * H * W + 2) * U * aw


def _ratio(got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    assert bool(torch.isfinite(err).all())
    if float(bound.min()) > 0:
        return float((err / bound).max())
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


def _check(dev, B, cin, cout, s, H, W):
    x, w, gout = _case(B, cin, cout, s, H, W)
    gin64, gw64, bin_, bw_ = _reference(x, w, gout, s)
    xd, wd, gd = x.to(dev), w.to(dev), gout.to(dev)
    gin = ops.deconv_ks_dgrad(gd, wd, s)
    gw = ops.deconv_ks_wgrad(xd, gd, s)
    assert gin.shape == x.shape and gw.shape == w.shape and gin.is_contiguous() and gw.is_contiguous()
    r_in, r_w = _ratio(gin, gin64, bin_), _ratio(gw, gw64, bw_)
    print("B %d, %d -> %d, s = %d, %d x %d: worst error / bound  gin %.3f  gW %.3f" % (B, cin, cout, s, H, W, r_in, r_w))
    assert r_in <= 1.0 and r_w <= 1.0
    # repeatability: the same bits on a second call
    assert torch.equal(ops.deconv_ks_dgrad(gd, wd, s), gin) and torch.equal(ops.deconv_ks_wgrad(xd, gd, s), gw)
    return gin, gw


@pytest.mark.parametrize("B, H, W", [(2, 5, 7), (3, 1, 1)])
@pytest.mark.parametrize("cin, cout", [(6, 32), (34, 96), (64, 32)])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_gradients_against_float64(dev, s, cin, cout, B, H, W):
    _check(dev, B, cin, cout, s, H, W)


def test_depth_many_chunk_partials(dev):
    """B = 2, 41 x 37, 64 -> 32, s = 2: 128 chunks over 380 stages (two or three each), the last stage of an image part full."""
    B, cin, cout, s, H, W = 2, 64, 32, 2, 41, 37
    nchunks = lib.sessd_deconv_ks_wgrad_workspace_bytes(B, cin, H, W, cout, s) // (cin * cout * s * s * 4)
    stages = B * ((H * W + 7) // 8)
    assert nchunks == 128 and nchunks >= 3 and stages == 380 and stages % nchunks != 0 and (H * W) % 8 != 0
    _check(dev, B, cin, cout, s, H, W)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_function(dev, s):
    B, cin, cout, H, W = 2, 34, 96, 5, 7
    x, w, gout = _case(B, cin, cout, s, H, W, seed=7)
    gin64, gw64, bin_, bw_ = _reference(x, w, gout, s)
    xd, wd, gd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), gout.to(dev)
    y = ops.DeconvKsFunction.apply(xd, wd, s)
    want = torch.full((B, cout, s * H, s * W), float("nan"), device=dev)
    ops.deconv_ks_slice(xd.detach(), ops.pack_deconv_ks_slice(wd.detach(), s), None, None, False, want, 0)
    assert torch.equal(y.detach(), want)                                    # the forward kernel, bit for bit
    gx, gw = torch.autograd.grad(y, (xd, wd), gd, retain_graph=True)
    r_in, r_w = _ratio(gx, gin64, bin_), _ratio(gw, gw64, bw_)
    print("DeconvKsFunction s = %d: worst error / bound  gx %.3f  gw %.3f" % (s, r_in, r_w))
    assert r_in <= 1.0 and r_w <= 1.0
    # the incoming gradient as a non-contiguous channel slice of a wider map: what torch.cat's backward hands out
    wide = torch.randn(B, cout + 64, s * H, s * W, device=dev)
    wide[:, 32:32 + cout] = gd
    sl = wide[:, 32:32 + cout]
    assert not sl.is_contiguous() or B == 1
    gx2, gw2 = torch.autograd.grad(y, (xd, wd), sl, retain_graph=True)
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw)
    # needs_input_grad is honoured: the gradient that is not asked for is None (and its kernel is not launched)
    for need_x, need_w in ((False, True), (True, False)):
        class Ctx:
            needs_input_grad = (need_x, need_w, False)
            saved_tensors = (xd.detach(), wd.detach())
        Ctx.s = s
        got = ops.DeconvKsFunction.backward(Ctx, gd)
        assert (got[0] is None) == (not need_x) and (got[1] is None) == (not need_w) and got[2] is None
        if need_x:
            assert torch.equal(got[0], gx)
        if need_w:
            assert torch.equal(got[1], gw)
    # and through autograd: a weight-only / input-only graph
    y2 = ops.DeconvKsFunction.apply(xd.detach(), wd, s)
    assert torch.equal(torch.autograd.grad(y2, wd, gd)[0], gw)
    y3 = ops.DeconvKsFunction.apply(xd, wd.detach(), s)
    assert torch.equal(torch.autograd.grad(y3, xd, gd)[0], gx)


def test_wrappers_refuse_mismatched_shapes(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError):
        ops.deconv_ks_dgrad(z(2, 32, 8, 8), z(6, 32, 3, 3), 3)          # s
    with pytest.raises(ValueError):
        ops.deconv_ks_dgrad(z(2, 64, 8, 8), z(6, 32, 2, 2), 2)          # cout of grad_out
    with pytest.raises(ValueError):
        ops.deconv_ks_dgrad(z(2, 32, 7, 8), z(6, 32, 2, 2), 2)          # a map that is no multiple of s
    with pytest.raises(ValueError):
        ops.deconv_ks_wgrad(z(2, 6, 4, 4), z(2, 32, 8, 9), 2)           # grad_out is not s times x
    with pytest.raises(ValueError):
        ops.deconv_ks_wgrad(z(2, 5, 4, 4), z(2, 32, 8, 8), 2)           # odd cin
    with pytest.raises(ValueError):
        ops.deconv_ks_wgrad(z(2, 6, 4, 4).cpu(), z(2, 32, 8, 8), 2)     # a CPU tensor
    assert float(ops.deconv_ks_wgrad(z(0, 6, 4, 4), z(0, 32, 8, 8), 2).abs().max()) == 0.0   # the empty sum
