"""The bounds of tests/dense_grad_ref.py can be met by a correct float32 implementation and are not vacuous (no GPU):
  - float32 torch on the CPU stays within every bound (ratio <= 1) on every case that tests/test_dense_grad_f64_gpu.py runs;
  - the same float32 run on a copy with ONE input pixel of the last image's last row (its last column: the right-neighbour and the
    bottom tap row) zeroed in every channel leaves the bound (ratio > 1);
  - float32 restatements of F(2x2,3x3) with the kernels' transforms, tile order and chunk sums stay within the Winograd bounds;
  - the restated chunk rules give the branch properties the case table names.
Every ratio is printed (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import dense_grad_ref as R


def _wgrad32(inp, gout, k, stride):
    w = torch.zeros(gout.shape[1], inp.shape[1], k, k, requires_grad=True)
    return torch.autograd.grad(F.conv2d(inp, w, stride=stride, padding=k // 2), w, gout)[0]


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_float32_meets_the_direct_bound_and_one_pixel_leaves_it(name):
    k, s = R.WGRAD_CASES[name][:2]
    inp, gout = R.wgrad_inputs(name)
    ref, bound = R.wgrad_reference(inp, gout, k, s)
    assert bool((bound >= 0).all()) and bool((bound > 0).any())
    r = R.ratio(_wgrad32(inp, gout, k, s), ref, bound)
    bad = inp.clone()
    bad[-1, :, -1, -1] = 0.0
    err = (_wgrad32(bad, gout, k, s).double() - ref).abs()
    m = float((err[bound > 0] / bound[bound > 0]).max())
    print("wgrad case %s: float32 / bound %.4f, one pixel zeroed %.3g, zero-bound entries %d" % (name, r, m, int((bound == 0).sum())))
    assert r <= 1.0
    assert m > 1.0


def test_the_exact_zero_entries():
    """hout = 1 with stride 2 (case 6): the ky = 0 taps read row -1 only; one row with stride 1 (case 4): ky = 0 and ky = 2."""
    for name, rows in (("6", [0]), ("4", [0, 2])):
        k, s = R.WGRAD_CASES[name][:2]
        bound = R.wgrad_reference(*R.wgrad_inputs(name), k, s)[1]
        assert bool((bound[:, :, rows, :] == 0).all()) and bool((bound[:, :, 1, 1] > 0).all())


@pytest.mark.parametrize("name", list(R.WGRAD_CASES))
def test_restated_chunk_rule_gives_the_named_branch(name):
    k, s, B, ci, co, hi, wi, want = R.WGRAD_CASES[name]
    ho, wo = R.out_hw(k, s, hi, wi)
    assert wo % 8 == 0
    assert R.direct_chunks(B, ci, co, ho, k, s)[:3] == want


def test_chunk_properties_of_the_ragged_cases():
    assert R.chunk_props(3, 23, 35, 2) == (1, [11])     # cases 3 and 13: 69 rows, chunk 11 = rows 22, 23 lies in images 0 and 1, the last chunk has one row
    assert R.chunk_props(3, 87, 131, 2) == (1, [43])    # case 10: chunk 43 = rows 86, 87
    assert 35 % 16 == 3 and 131 % 16 == 3                    # the reduce kernel's 16-wide tail
    assert [R.wino_wgrad_chunks(*c) for c in R.WINO_WGRAD_CASES] == list(R.WINO_WGRAD_CASES.values())


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_float32_module_meets_its_bounds(name):
    tr, k, s = R.MODULE_CASES[name][:3]
    x, w, bias, gout = R.module_inputs(name)
    ref, bound = R.module_bounds(name, x, w, bias, gout)
    got = dict(zip(("y", "gx", "gw", "gb"), R._grads(x, w, bias, gout, s, tr)))
    for key in ref:
        r = R.ratio(got[key], ref[key], bound[key])
        print("module case %s, %s: float32 / bound %.4f" % (name, key, r))
        assert r <= 1.0


@pytest.mark.parametrize("shape", list(R.WINO_WGRAD_CASES))
def test_float32_winograd_weight_gradient_meets_the_winograd_bound(shape):
    x, gout = R.wino_wgrad_inputs(*shape)
    nchunks = R.WINO_WGRAD_CASES[shape][1]
    ref = R.wgrad_reference(x, gout, 3, 1)[0]
    bound = R.wino_wgrad_bound(x, gout, nchunks)
    exact = R.wino_wgrad(x, gout, torch.float64, nchunks=nchunks)   # the algorithm itself, in float64, is the convolution's gradient
    assert float((exact - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    r = R.ratio(R.wino_wgrad(x, gout, torch.float32, nchunks=nchunks), ref, bound)
    bad = x.clone()
    bad[-1, :, -1, -1] = 0.0
    m = R.ratio(R.wino_wgrad(bad, gout, torch.float32, nchunks=nchunks), ref, bound)
    print("Winograd weight gradient %s, n = %d: float32 restatement / bound %.4f, one pixel zeroed %.3g"
          % (shape, R.wino_wgrad_n(x, nchunks), r, m))
    assert r <= 1.0
    assert m > 1.0


@pytest.mark.parametrize("B,cin,cout,H,W,bias", [(1, 16, 32, 64, 64, False), (2, 16, 34, 6, 10, True), (1, 64, 64, 8, 16, False)])
def test_float32_winograd_forward_meets_the_winograd_bound(B, cin, cout, H, W, bias):
    g = torch.Generator().manual_seed(cin + cout + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) * (1.0 / (3 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) if bias else None
    gout = torch.randn(B, cout, H, W, generator=g)
    ref = R.module_reference(x, w, b, gout, 1, False)[0]
    for what, inp, wt, bb, want in (("forward", x, w, b, ref["y"]), ("data gradient", gout, R.adjoint_weight(w), None, ref["gx"])):
        exact = R.wino_forward(inp, wt, bb, torch.float64)
        assert float((exact - want).abs().max()) <= 1e-9 * float(want.abs().max())
        r = R.ratio(R.wino_forward(inp, wt, bb, torch.float32), want, R.wino_forward_bound(inp, wt, bb))
        print("Winograd %s %d -> %d on %d x %d, n = %d: float32 restatement / bound %.4f"
              % (what, inp.shape[1], wt.shape[0], H, W, R.wino_forward_n(inp.shape[1]), r))
        assert r <= 1.0


def test_ratio_refuses_what_it_must():
    ref, bound = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([1e-6, 0.0], dtype=torch.float64)
    assert R.ratio(torch.tensor([1.0, 0.0]), ref, bound) == 0.0
    with pytest.raises(AssertionError):
        R.ratio(torch.tensor([1.0, 1e-30]), ref, bound)              # an entry whose bound is 0 must be exactly 0
    with pytest.raises(AssertionError):
        R.ratio(torch.tensor([float("nan"), 0.0]), ref, bound)
    assert R.gamma(1000) > 1000 * R.U
