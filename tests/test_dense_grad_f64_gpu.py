"""The dense conv weight, data and bias gradients on the HIP kernels (csrc/dense_grad.hip, csrc/dense_wino_wgrad.hip,
ops.Conv2dFunction, ops.channel_sum) against float64 torch on the CPU, per element, inside the DERIVED bounds of
tests/dense_grad_ref.py (direct: gamma(K + 2) x the gradient of the absolute inputs; Winograd: gamma(n) x the absolute-value image of
the algorithm, n counted from the code). The shapes are the smallest that reach each branch of the kernels -- a single 8-pixel step per
row, the unroll-by-two tail at wout = 24, odd hin and hout = 1 at stride 2, ragged 32- and 64-blocks of channels, chunks that straddle
two images, a short last chunk, the reduce kernel's 16-wide tail, the LDS kernel's early-returning workgroups and odd stage counts --
and every case that names a branch re-derives the chunk count from a restatement of the entry point's rule and asserts the property,
so that a change of the rule fails here instead of silently testing less. tests/test_dense_grad_ref_cpu.py shows on the CPU that the
bounds can be met (float32 torch: 0.0005 .. 0.1) and that one zeroed pixel leaves them (36 .. 8e4).

Every case: shape, contiguity, worst error / bound <= 1 per tensor (printed), the same bits on a second call."""
import pytest
import torch
import torch.nn.functional as F

import dense_grad_ref as R
from sessd_hip import lib, ops

pytestmark = pytest.mark.gpu


def _wgrad_case(dev, name):
    k, s, B, ci, co, hi, wi, want = R.WGRAD_CASES[name]
    ho, wo = R.out_hw(k, s, hi, wi)
    kernel, nchunks, rpc, tiles = R.direct_chunks(B, ci, co, ho, k, s)
    assert (kernel, nchunks, rpc) == want                           # the branch the case is meant to reach
    assert nchunks * co * ci * k * k * 4 <= int(lib.sessd_conv2d_wgrad_workspace_bytes(co, ci, k))
    inp, gout = R.wgrad_inputs(name)
    ref, bound = R.wgrad_reference(inp, gout, k, s)
    xd, gd = inp.to(dev), gout.to(dev)
    got = ops.conv2d_wgrad(xd, gd, k, s, winograd=False)
    assert got.shape == (co, ci, k, k) and got.is_contiguous()
    r = R.ratio(got, ref, bound)
    print("conv2d_wgrad case %s (%s kernel, %d chunks of %d rows, %d tiles): worst error / bound %.3f" % (name, kernel, nchunks, rpc, tiles, r))
    assert r <= 1.0
    assert torch.equal(ops.conv2d_wgrad(xd, gd, k, s, winograd=False), got)
    return got, bound, (B, ho, wo, nchunks, rpc, tiles)


@pytest.mark.parametrize("name", ["1", "2", "5-odd", "5-even", "7-small", "7-64x34", "8", "9", "12"])
def test_wgrad_against_float64(dev, name):
    _wgrad_case(dev, name)


def test_wgrad_one_step_rows_and_ragged_blocks(dev):
    """Case 1: wout = 8 is one step per row; cout = 34 leaves a second 32-block with two live rows; ten chunks of one row.
    Case 2 (above): wout = 24, cin = 34. Case 9 (above): the 64 x 64 kernel with second blocks of 2 (cin) and 34 (cout) channels."""
    _, _, (B, ho, wo, nchunks, rpc, tiles) = _wgrad_case(dev, "1")
    assert wo == 8 and nchunks == 10 and rpc == 1 and R.WGRAD_CASES["1"][4] % 32 == 2
    assert R.out_hw(3, 1, *R.WGRAD_CASES["2"][5:7])[1] == 24 and R.WGRAD_CASES["2"][3] % 32 == 2
    assert R.WGRAD_CASES["9"][3] % 64 == 2 and R.WGRAD_CASES["9"][4] % 64 == 34 and R.WGRAD_CASES["9"][6] == 24


@pytest.mark.parametrize("name", ["3", "10", "13-two-tiles", "13-wide"])
def test_wgrad_ragged_chunks_across_images(dev, name):
    """69 (261) rows in chunks of two: the last chunk has one row, one chunk lies in two images, the number of chunks is no multiple
    of the reduce kernel's 16 loads in flight."""
    _, _, (B, ho, wo, nchunks, rpc, tiles) = _wgrad_case(dev, name)
    last, straddle = R.chunk_props(B, ho, nchunks, rpc)
    assert rpc == 2 and last == 1 and nchunks % 16 == 3 and nchunks > 16
    assert straddle == ([43] if name == "10" else [11])
    if name.startswith("13"):
        assert tiles == (2 if name == "13-two-tiles" else 1) and (rpc * (wo // 8)) % 2 == 0


@pytest.mark.parametrize("name,rows", [("4", [0, 2]), ("6", [0])])
def test_wgrad_tap_rows_that_are_always_outside(dev, name, rows):
    """One input row at stride 1 (ky = 0 and ky = 2 read rows -1 and 1) and hout = 1 at stride 2 (ky = 0 reads row -1): exact zeros."""
    got, bound, _ = _wgrad_case(dev, name)
    assert bool((bound[:, :, rows, :] == 0).all()) and bool((got[:, :, rows, :] == 0).all()) and bool((got[:, :, 1, :] != 0).all())


def test_wgrad_lds_kernel_one_stage_and_idle_workgroups(dev):
    """Case 11: six chunks of one stage each (S = 1: the second MMA of the loop body is skipped), a launch of 8 workgroups of which
    6 and 7 return at once. Case 12 (above): S = 3."""
    _, _, (B, ho, wo, nchunks, rpc, tiles) = _wgrad_case(dev, "11")
    stages = rpc * (wo // 8)
    launched = tiles * ((nchunks + 7) // 8 * 8)
    assert stages == 1 and nchunks == 6 and launched == 8 and launched - tiles * nchunks == 2
    k, s, B2, ci2, co2, hi2, wi2, _ = R.WGRAD_CASES["12"]
    assert R.direct_chunks(B2, ci2, co2, R.out_hw(k, s, hi2, wi2)[0], k, s)[2] * (R.out_hw(k, s, hi2, wi2)[1] // 8) == 3


@pytest.mark.parametrize("name,cin,cout", [("14-lds", 64, 128), ("14-general", 6, 34)])
def test_deconv_weight_gradient_with_the_roles_swapped(dev, name, cin, cout):
    """ConvTranspose2d(cin, cout, 3, 2, 1, 1) on x (2, cin, 3, 8): conv2d_wgrad(grad_out, x, 3, 2) is its (cin, cout, 3, 3) gradient."""
    got, _, _ = _wgrad_case(dev, name)
    gout, x = R.wgrad_inputs(name)          # the roles: inp = the layer's grad_out, gout = its input
    assert x.shape == (2, cin, 3, 8) and gout.shape == (2, cout, 6, 16) and got.shape == (cin, cout, 3, 3)
    ref, bound = R.deconv_wgrad_reference(x, gout)
    r = R.ratio(got, ref, bound)
    print("ConvTranspose2d %d -> %d weight gradient: worst error / bound %.3f" % (cin, cout, r))
    assert r <= 1.0


def _direct_entry(dev, wout, short=0):
    B, ci, co, h = 1, 2, 2, 4
    x = torch.randn(B, ci, h, wout, device=dev)
    g = torch.randn(B, co, h, wout, device=dev)
    gw = torch.full((co, ci, 3, 3), float("nan"), device=dev)
    need = int(lib.sessd_conv2d_wgrad_workspace_bytes(co, ci, 3))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.sessd_conv2d_wgrad(x.data_ptr(), B, ci, h, wout, g.data_ptr(), co, h, wout, 3, 1, gw.data_ptr(), ws.data_ptr(), need - short,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, gw


def test_entry_refuses_a_width_that_is_no_multiple_of_8(dev):
    """Today's wout % 8 rule: whoever lifts it changes this test on purpose."""
    rc, gw = _direct_entry(dev, 12)
    assert rc == -1 and bool(torch.isnan(gw).all())
    rc, gw = _direct_entry(dev, 16)
    assert rc == 0 and bool(torch.isfinite(gw).all())


def test_entry_refuses_a_short_workspace(dev):
    rc, gw = _direct_entry(dev, 16, short=1)
    assert rc == -2 and bool(torch.isnan(gw).all())


@pytest.mark.parametrize("B,cin,cout,H,W", list(R.WINO_WGRAD_CASES))
def test_winograd_domain_weight_gradient_against_float64(dev, B, cin, cout, H, W):
    """(1, 64, 64, 2, 16): one stage, one chunk, no row above or below. (5, 64, 64, 4, 18): 12 stages, the last with 2 tiles, 3 chunks.
    (3, 64, 128, 6, 22): tw = 11, stages straddle rows and images, 13 stages in chunks of 4 / 4 / 5, two co blocks.
    (2, 64, 64, 16, 32): 8 chunks, the XCD-placement branch."""
    stages, nchunks = R.wino_wgrad_chunks(B, cin, cout, H, W)
    assert (stages, nchunks) == R.WINO_WGRAD_CASES[(B, cin, cout, H, W)]
    assert int(lib.sessd_conv3x3_wgrad_winograd_workspace_bytes(B, cin, cout, H, W)) == nchunks * 16 * cin * cout * 4
    tiles = B * (H // 2) * (W // 2)
    cuts = [c * stages // nchunks for c in range(nchunks + 1)]
    if (B, H, W) == (1, 2, 16):
        assert stages == 1 and nchunks == 1 and H // 2 == 1
    elif (B, H, W) == (5, 4, 18):
        assert tiles - 8 * (stages - 1) == 2
    elif (B, H, W) == (3, 6, 22):
        assert W // 2 == 11 and [b - a for a, b in zip(cuts, cuts[1:])] == [4, 4, 5] and cout // 64 == 2 and (H // 2) * (W // 2) % 8
    else:
        assert nchunks & 7 == 0
    x, gout = R.wino_wgrad_inputs(B, cin, cout, H, W)
    ref = R.wgrad_reference(x, gout, 3, 1)[0]
    bound = R.wino_wgrad_bound(x, gout, nchunks)
    xd, gd = x.to(dev), gout.to(dev)
    got = ops.conv2d_wgrad(xd, gd, 3, 1, winograd=True)
    assert got.shape == (cout, cin, 3, 3) and got.is_contiguous()
    r = R.ratio(got, ref, bound)
    print("Winograd-domain weight gradient B %d, %d -> %d, %d x %d (%d stages, %d chunks, n = %d): worst error / bound %.3f"
          % (B, cin, cout, H, W, stages, nchunks, R.wino_wgrad_n(x, nchunks), r))
    assert r <= 1.0
    assert torch.equal(ops.conv2d_wgrad(xd, gd, 3, 1, winograd=True), got)
    if W % 8 == 0:   # the comparison tests/test_dense_grad_gpu.py makes: the direct kernel, 2e-4 of the largest entry
        direct = ops.conv2d_wgrad(xd, gd, 3, 1, winograd=False)
        assert float((got - direct).abs().max()) <= 2e-4 * max(1e-6, float(direct.abs().max()))


def test_automatic_choice_falls_to_the_direct_kernel_outside_the_winograd_shapes(dev):
    """winograd=None on a map of >= 4096 pixels whose channels are no multiples of 64 (16 -> 32 on 64 x 64): the direct kernel's bits,
    no ValueError -- that is kept for the caller's own winograd=True. (The automatic choice used to be taken for the caller's.)"""
    x, w, bias, gout = R.module_inputs("conv3x3-s1-16-32-winograd")
    xd, gd = x.to(dev), gout.to(dev)
    assert int(lib.sessd_conv3x3_wgrad_winograd_workspace_bytes(1, 16, 32, 64, 64)) == 0 and ops.USE_WINOGRAD and ops.USE_WINOGRAD_WGRAD
    assert torch.equal(ops.conv2d_wgrad(xd, gd, 3, 1), ops.conv2d_wgrad(xd, gd, 3, 1, winograd=False))
    with pytest.raises(ValueError):
        ops.conv2d_wgrad(xd, gd, 3, 1, winograd=True)


def _module(name, dev):
    tr, k, s, ci, co, has_bias, _, _ = R.MODULE_CASES[name]
    x, w, bias, gout = R.module_inputs(name)
    m = torch.nn.ConvTranspose2d(ci, co, 3, stride=2, padding=1, output_padding=1, bias=has_bias) if tr else \
        torch.nn.Conv2d(ci, co, k, stride=s, padding=k // 2, bias=has_bias)
    with torch.no_grad():
        m.weight.copy_(w)
        if has_bias:
            m.bias.copy_(bias)
    return m.to(dev), x, w, bias, gout


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_module_forward_and_gradients_against_float64(dev, name):
    tr, k, s, ci, co, has_bias, (B, H, W), (data, wg) = R.MODULE_CASES[name]
    m, x, w, bias, gout = _module(name, dev)
    ref, bound = R.module_bounds(name, x, w, bias, gout)
    # the kernel families MODULE_CASES names are the ones ops selects
    xd = x.to(dev).requires_grad_(True)
    if tr or s == 2:
        assert data == "direct"
    else:
        assert (ops._train_cfg(ops.pack_conv2d(m.weight, 1), xd) == 22) == (data == "winograd")
        assert (ops._train_cfg(ops.pack_conv2d(m.weight, 1, adjoint=True), gout.to(dev)) == 22) == (data == "winograd")
    assert bool(lib.sessd_conv3x3_wgrad_winograd_workspace_bytes(B, ci, co, H, W) and H * W >= 4096 and k == 3 and s == 1 and not tr) \
        == (wg == "winograd")
    params = (xd, m.weight, m.bias) if has_bias else (xd, m.weight)
    y = ops.conv2d_module(xd, m)
    grads = torch.autograd.grad(y, params, gout.to(dev), retain_graph=True)
    got = dict(zip(("y", "gx", "gw", "gb"), (y.detach(),) + tuple(grads)))
    assert set(got) == set(ref)
    for key in got:
        assert got[key].shape == ref[key].shape and got[key].is_contiguous()
        r = R.ratio(got[key], ref[key], bound[key])
        print("conv2d_module %s, %s (%s): worst error / bound %.3f" % (name, key, wg if key == "gw" else data if key != "gb" else "sum", r))
        assert r <= 1.0
    again = torch.autograd.grad(ops.conv2d_module(xd, m), params, gout.to(dev))
    assert all(torch.equal(a, b) for a, b in zip(again, grads))


def test_module_gradient_slices_and_unasked_gradients(dev):
    name = "conv1x1-34-6-bias"
    tr, k, s, ci, co, has_bias, (B, H, W), _ = R.MODULE_CASES[name]
    m, x, w, bias, gout = _module(name, dev)
    xd, gd = x.to(dev).requires_grad_(True), gout.to(dev)
    y = ops.conv2d_module(xd, m)
    gx, gw, gb = torch.autograd.grad(y, (xd, m.weight, m.bias), gd, retain_graph=True)
    # the incoming gradient as a non-contiguous channel slice of a wider map: what torch.cat's backward hands out
    wide = torch.randn(B, co + 10, H, W, device=dev)
    wide[:, 3:3 + co] = gd
    sl = wide[:, 3:3 + co]
    assert not sl.is_contiguous()
    gx2, gw2, gb2 = torch.autograd.grad(y, (xd, m.weight, m.bias), sl, retain_graph=True)
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    # a gradient that is not asked for is None
    for need in ((False, True, True), (True, False, False), (True, True, False)):
        class Ctx:
            needs_input_grad = need + (False, False)
            saved_tensors = (xd.detach(), m.weight)
            cfg = (False, 1, True)
        out = ops.Conv2dFunction.backward(Ctx, gd)
        assert [o is None for o in out] == [not n for n in need] + [True, True]
        for o, want in zip(out[:3], (gx, gw, gb)):
            assert o is None or torch.equal(o, want)
    # and through autograd: a weight-only and an input-only graph
    y2 = ops.Conv2dFunction.apply(xd.detach(), m.weight, None, False, 1)
    assert torch.equal(torch.autograd.grad(y2, m.weight, gd)[0], gw)
    y3 = ops.Conv2dFunction.apply(xd, m.weight.detach(), None, False, 1)
    assert torch.equal(torch.autograd.grad(y3, xd, gd)[0], gx)


@pytest.mark.parametrize("shape", [(3, 22, 6, 10), (2, 5, 7, 9)])
def test_channel_sum_against_float64(dev, shape):
    """(2, 5, 7, 9): a plane that is no multiple of 4"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
    ref, bound = R.channel_sum_reference(x)
    got = ops.channel_sum(x.to(dev))
    assert got.shape == (shape[1],) and got.is_contiguous()
    r = R.ratio(got, ref, bound)
    print("channel_sum %s: worst error / bound %.3f" % (shape, r))
    assert r <= 1.0
    assert torch.equal(ops.channel_sum(x.to(dev)), got)
