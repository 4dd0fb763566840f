"""sessd_conv2d_wgrad_any_width and the opt-in switches around it, without a GPU:
  - the header declares the new entry and sessd_hip/_lib.py binds it (the dynamic check of tests/test_abi.py still holds);
  - its argument checks come before any device call (null / dummy pointers): a width that is no multiple of 8 gets as far as the
    workspace check (SESSD_EWORKSPACE), where sessd_conv2d_wgrad answers SESSD_EINVAL; everything else is refused as before;
  - ops.conv2d_train_covers(..., any_width=True) drops the wout % 8 condition and nothing else; the default is today's answer;
  - the bounds of tests/wgrad_any_ref.py can be met (float32 torch on the CPU: ratio <= 1) and are not vacuous: positive wherever a
    tap can reach the image, and one zeroed input pixel leaves them."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dense_grad_ref as R
import sessd_hip
import wgrad_any_ref as A
from det3d.models.necks.rpn_v1 import RPN
from sessd_hip import ops
from test_abi import test_header_symbols_exported_and_bound as _abi_check

lib = sessd_hip.lib
EINVAL, EWORKSPACE = -1, -2
P = 64   # a dummy, 16-byte aligned, never dereferenced pointer: every call below must return before a launch


def test_the_new_entry_is_declared_exported_and_bound():
    _abi_check()
    assert "sessd_conv2d_wgrad_any_width" in sessd_hip.SIGNATURES and hasattr(lib, "sessd_conv2d_wgrad_any_width")
    assert sessd_hip.SIGNATURES["sessd_conv2d_wgrad_any_width"] == sessd_hip.SIGNATURES["sessd_conv2d_wgrad"]


def _call(entry, wout=12, k=3, s=1, hout=4, win=None, hin=None, batch=1, cin=2, cout=2, ws_bytes=0):
    win = (wout * s if win is None else win)
    hin = (hout * s if hin is None else hin)
    return entry(P, batch, cin, hin, win, P, cout, hout, wout, k, s, P, P, ws_bytes, None)


def test_argument_checks_before_any_launch():
    new, old = lib.sessd_conv2d_wgrad_any_width, lib.sessd_conv2d_wgrad
    need = int(lib.sessd_conv2d_wgrad_workspace_bytes(2, 2, 3))
    # the width is accepted before the device is touched: a short workspace is the next refusal
    for wout in (12, 10, 7, 4, 1, 54, 16):
        assert _call(new, wout, ws_bytes=need - 1) == EWORKSPACE, wout
        assert _call(old, wout, ws_bytes=need - 1) == (EWORKSPACE if wout % 8 == 0 else EINVAL), wout
    assert _call(new, 6, s=2, ws_bytes=0) == EWORKSPACE and _call(old, 6, s=2, ws_bytes=0) == EINVAL
    assert _call(new, 7, k=1, ws_bytes=0) == EWORKSPACE and _call(old, 7, k=1, ws_bytes=0) == EINVAL
    # everything else stays refused
    assert _call(new, 6, s=2, win=11, ws_bytes=1 << 40) == EINVAL          # stride 2: win == 2 * wout (11 gives wout = 6, too)
    assert _call(new, 0, ws_bytes=1 << 40) == EINVAL and _call(new, 12, win=13, ws_bytes=1 << 40) == EINVAL
    assert _call(new, 12, k=5, ws_bytes=1 << 40) == EINVAL and _call(new, 12, k=1, s=2, ws_bytes=1 << 40) == EINVAL
    assert _call(new, 12, s=3, ws_bytes=1 << 40) == EINVAL and _call(new, 12, batch=0, ws_bytes=1 << 40) == EINVAL
    assert _call(new, 12, hout=5, hin=4, ws_bytes=1 << 40) == EINVAL
    assert _call(new, 500, hout=500, batch=64, cin=64, ws_bytes=1 << 40) == EINVAL    # 2 GiB


class _OnDevice:
    """What the predicates read of a tensor, claiming to be a float32 device tensor: the predicates touch no data."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


@pytest.fixture()
def device_stand_in(monkeypatch):
    """The predicates' two questions about WHERE things are, answered for CPU modules: everything else is theirs."""
    monkeypatch.setattr(ops, "_device_f32", lambda x: isinstance(x, _OnDevice) and x.dim() == 4)
    monkeypatch.setattr(ops, "_device_param", lambda t: t is None or t.dtype == torch.float32)


def test_conv2d_train_covers_any_width(device_stand_in):
    C = nn.Conv2d
    covers = ops.conv2d_train_covers
    pointpillars = [(C(64, 128, 3, stride=2, bias=False), _OnDevice(2, 64, 248, 216), True),      # wout 108
                    (C(128, 128, 3, padding=1, bias=False), _OnDevice(2, 128, 124, 108), False),  # 108
                    (C(256, 256, 3, padding=1, bias=False), _OnDevice(2, 256, 62, 54), False)]    # 54
    for m, x, padded in pointpillars:
        assert covers(m, x, padded=padded, any_width=True)
        assert not covers(m, x, padded=padded) and not covers(m, x, padded=padded, any_width=False)
    for w in (12, 5):
        assert covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(2, 64, 16, w), any_width=True)
        assert covers(C(64, 32, 1, bias=False), _OnDevice(2, 64, 16, w), any_width=True)
        assert not covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(2, 64, 16, w))
    assert covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 16, 8), any_width=True)           # wout = 4
    assert not covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 16, 8))
    # what the flag does not lift
    assert not covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 15, 16), any_width=True)      # stride 2: odd H
    assert not covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 16, 10 + 1), any_width=True)  # ... odd W
    assert not covers(C(63, 32, 3, padding=1, bias=False), _OnDevice(2, 63, 16, 12), any_width=True)                # odd cin
    assert not covers(C(64, 33, 3, padding=1, bias=False), _OnDevice(2, 64, 16, 12), any_width=True)                # odd cout
    assert not covers(C(64, 32, 5, padding=2, bias=False), _OnDevice(2, 64, 16, 12), any_width=True)
    assert not covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(64, 64, 512, 510), any_width=True)             # 2 GiB
    assert not covers(C(64, 32, 3, padding=1, bias=False), torch.zeros(2, 64, 16, 12), any_width=True)              # a CPU tensor
    # the default argument answers exactly as before on multiples of 8, too
    assert covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(2, 64, 16, 16)) and covers(C(64, 32, 3, padding=1, bias=False),
                                                                                         _OnDevice(2, 64, 16, 16), any_width=True)


def test_the_switch_is_off_by_default():
    assert RPN.train_any_width is False and RPN.fused_train is True


def _wgrad32(inp, gout, k, stride):
    w = torch.zeros(gout.shape[1], inp.shape[1], k, k, requires_grad=True)
    return torch.autograd.grad(F.conv2d(inp, w, stride=stride, padding=k // 2), w, gout)[0]


@pytest.mark.parametrize("name", list(A.ANY_WIDTH_CASES))
def test_float32_meets_the_bound_and_the_bound_is_not_vacuous(name):
    k, s, B, ci, co, hi, wi, want = A.ANY_WIDTH_CASES[name]
    ho, wo = R.out_hw(k, s, hi, wi)
    assert wo % 8 != 0 and (s == 1 or wi == 2 * wo)
    assert R.direct_chunks(B, ci, co, ho, k, s)[:3] == want
    inp, gout, ref, bound = A.reference(name)
    reach = A.reachable(k, s, hi, wi)
    assert bool((bound[:, :, reach] > 0).all()) and bool((bound[:, :, ~reach] == 0).all()) and bool(reach.any())
    r = R.ratio(_wgrad32(inp, gout, k, s), ref, bound)
    bad = inp.clone()
    bad[-1, :, -1, -1] = 0.0           # the last column of the last row: the pixel a ragged step is most likely to lose
    err = (_wgrad32(bad, gout, k, s).double() - ref).abs()
    m = float((err[bound > 0] / bound[bound > 0]).max())
    print("any-width case %s: float32 / bound %.4f, one pixel zeroed %.3g, zero-bound entries %d" % (name, r, m, int((bound == 0).sum())))
    assert r <= 1.0
    assert m > 1.0


def test_the_exact_zero_columns_of_a_single_column_map():
    k, s, B, ci, co, hi, wi, _ = A.ANY_WIDTH_CASES["s1-w1"]
    assert A.reachable(k, s, hi, wi).tolist() == [[False, True, False]] * 3
    bound = A.reference("s1-w1")[3]
    assert bool((bound[:, :, :, [0, 2]] == 0).all()) and bool((bound[:, :, :, 1] > 0).all())


def test_deconv_cases_are_the_layers_they_claim():
    for name, (cin, cout, xshape) in A.DECONV_CASES.items():
        k, s, B, ci, co, hi, wi, _ = A.ANY_WIDTH_CASES[name]
        gout, x = A.inputs(name)
        assert (k, s) == (3, 2) and tuple(x.shape) == xshape and tuple(gout.shape) == (B, cout, 2 * xshape[2], 2 * xshape[3])
        assert (ci, co) == (cout, cin)
        ref, bound = R.deconv_wgrad_reference(x, gout)
        conv_ref, conv_bound = A.reference(name)[2:]
        assert torch.equal(ref, conv_ref) or float((ref - conv_ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert ref.shape == (cin, cout, 3, 3) and bool((bound > 0).all())
