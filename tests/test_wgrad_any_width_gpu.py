"""The dense conv weight gradient at widths that are no multiple of 8 (sessd_conv2d_wgrad_any_width through
ops.conv2d_wgrad(..., any_width=True)) against float64 torch on the CPU, per element, inside the derived direct bound of
tests/dense_grad_ref.py. The cases (tests/wgrad_any_ref.py) are the smallest that reach each ragged path of the three kernels of
csrc/dense_grad.hip in each alignment class -- a 4-pixel group behind a full step, a group that ends inside the row (even and odd
widths), less than one step, the prefetch of the step past the row, a single column, the LDS kernel's partly empty last stage with
chunks of two rows that lie in two images -- and every case asserts the kernel branch the restated chunk rule names.
sessd_conv2d_wgrad refuses every one of them (EINVAL).

Every case: shape, contiguity, worst error / bound <= 1 (printed), the same bits on a second call."""
import pytest
import torch

import dense_grad_ref as R
import wgrad_any_ref as A
from sessd_hip import lib, ops
from sessd_hip._lib import SessdError

pytestmark = pytest.mark.gpu


def _case(dev, name):
    k, s, B, ci, co, hi, wi, want = A.ANY_WIDTH_CASES[name]
    ho, wo = R.out_hw(k, s, hi, wi)
    assert wo % 8 != 0
    kernel, nchunks, rpc, tiles = R.direct_chunks(B, ci, co, ho, k, s)
    assert (kernel, nchunks, rpc) == want                           # the branch the case is meant to reach
    assert nchunks * co * ci * k * k * 4 <= int(lib.sessd_conv2d_wgrad_workspace_bytes(co, ci, k))
    inp, gout, ref, bound = A.reference(name)
    xd, gd = inp.to(dev), gout.to(dev)
    got = ops.conv2d_wgrad(xd, gd, k, s, winograd=False, any_width=True)
    assert got.shape == (co, ci, k, k) and got.is_contiguous()
    r = R.ratio(got, ref, bound)
    print("conv2d_wgrad any width, case %s (wout %d, %s kernel, %d chunks of %d rows, %d tiles): worst error / bound %.3f"
          % (name, wo, kernel, nchunks, rpc, tiles, r))
    assert r <= 1.0
    assert torch.equal(ops.conv2d_wgrad(xd, gd, k, s, winograd=False, any_width=True), got)
    return got, bound, (B, ho, wo, nchunks, rpc, tiles)


@pytest.mark.parametrize("name", [n for n in A.ANY_WIDTH_CASES if n not in ("s1-w1", "lds-w7") and n not in A.DECONV_CASES])
def test_any_width_against_float64(dev, name):
    _case(dev, name)


def test_the_old_entry_refuses_every_case(dev):
    """the default path is today's: SessdError (EINVAL) from sessd_conv2d_wgrad, for each of these widths"""
    for name in ("s1-w12", "s2-w7", "1x1_64-w10", "lds-w4"):
        k, s = A.ANY_WIDTH_CASES[name][:2]
        inp, gout = A.inputs(name)
        with pytest.raises(SessdError, match="conv2d_wgrad failed: invalid argument"):
            ops.conv2d_wgrad(inp.to(dev), gout.to(dev), k, s, winograd=False)


def test_a_single_column(dev):
    """wout = 1: kx = 0 and kx = 2 read columns -1 and 1, which are padding: exact zeros, the centre column is not"""
    got, bound, _ = _case(dev, "s1-w1")
    assert bool((bound[:, :, :, [0, 2]] == 0).all()) and bool((got[:, :, :, [0, 2]] == 0).all()) and bool((got[:, :, :, 1] != 0).all())


def test_lds_kernel_ragged_stages_and_chunks_across_images(dev):
    """wout = 7: one partly empty stage per row; 69 rows in chunks of two: the last chunk has one row, chunk 11 lies in two images,
    two cout tiles. lds-w12 (above): 1.5 stages per row, i.e. two, the second half empty."""
    _, _, (B, ho, wo, nchunks, rpc, tiles) = _case(dev, "lds-w7")
    last, straddle = R.chunk_props(B, ho, nchunks, rpc)
    assert wo == 7 and rpc == 2 and last == 1 and straddle == [11] and tiles == 2


@pytest.mark.parametrize("name", list(A.DECONV_CASES))
def test_deconv_weight_gradient_with_the_roles_swapped(dev, name):
    """ConvTranspose2d(cin, cout, 3, 2, 1, 1) on x: conv2d_wgrad(grad_out, x, 3, 2, any_width=True) is its (cin, cout, 3, 3) gradient."""
    cin, cout, xshape = A.DECONV_CASES[name]
    got, _, _ = _case(dev, name)
    gout, x = A.inputs(name)          # the roles: inp = the layer's grad_out, gout = its input
    assert tuple(x.shape) == xshape and gout.shape == (xshape[0], cout, 2 * xshape[2], 2 * xshape[3]) and got.shape == (cin, cout, 3, 3)
    ref, bound = R.deconv_wgrad_reference(x, gout)
    r = R.ratio(got, ref, bound)
    print("ConvTranspose2d %d -> %d weight gradient, any width: worst error / bound %.3f" % (cin, cout, r))
    assert r <= 1.0


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_multiples_of_8_take_the_same_launches(dev, name):
    """wout % 8 == 0: the new entry dispatches to the kernels of sessd_conv2d_wgrad -- the same bits"""
    k, s = R.WGRAD_CASES[name][:2]
    inp, gout = R.wgrad_inputs(name)
    xd, gd = inp.to(dev), gout.to(dev)
    assert torch.equal(ops.conv2d_wgrad(xd, gd, k, s, winograd=False, any_width=True), ops.conv2d_wgrad(xd, gd, k, s, winograd=False))


def test_module_gradient_through_the_any_width_function(dev):
    """ops.conv2d_module(x, m, any_width=True) on a 10-wide map: the weight gradient is conv2d_wgrad(..., any_width=True)'s, the node is
    Conv2dFunctionAnyWidth's; with the default argument the backward raises as it always did."""
    k, s, B, ci, co, hi, wi, _ = A.ANY_WIDTH_CASES["s1-w10"]
    inp, gout, ref, bound = A.reference("s1-w10")
    m = torch.nn.Conv2d(ci, co, k, stride=s, padding=1, bias=False).to(dev)
    xd, gd = inp.to(dev), gout.to(dev)
    y = ops.conv2d_module(xd, m, any_width=True)
    assert type(y.grad_fn).__name__ == "Conv2dFunctionAnyWidthBackward"
    gw = torch.autograd.grad(y, m.weight, gd)[0]
    assert torch.equal(gw, ops.conv2d_wgrad(xd, gd, k, s, winograd=False, any_width=True)) and R.ratio(gw, ref, bound) <= 1.0
    y = ops.conv2d_module(xd, m)
    assert type(y.grad_fn).__name__ == "Conv2dFunctionBackward"
    with pytest.raises(SessdError, match="conv2d_wgrad failed: invalid argument"):
        torch.autograd.grad(y, m.weight, gd)
