"""sessd_deconv_ks_dgrad / sessd_deconv_ks_wgrad: the argument checks come before any device call, so they run here with null or
dummy pointers and no GPU (as tests/test_abi.py does for the other entry points); and the two predicates of the train-mode RPN
neck, ops.deconv_ks_covers / ops.conv2d_train_covers, answer False for every refusal reason on CPU modules (and for a CPU tensor
as such: a stand-in that only claims to be a device tensor shows the rest)."""
import pytest
import torch
from torch import nn

import sessd_hip
from sessd_hip import ops

lib = sessd_hip.lib
EINVAL, OK = -1, 0
P = 64   # a dummy, 16-byte aligned, never dereferenced pointer: every call below must return before a launch


def dgrad(batch=2, cin=64, hin=8, win=8, s=2, cout=32, gout=P, wpk=P, gin=P):
    return lib.sessd_deconv_ks_dgrad(gout, batch, cin, hin, win, wpk, s, cout, gin, None)


def wgrad(batch=2, cin=64, hin=8, win=8, cout=32, s=2, x=P, gout=P, gw=P, ws=P, ws_bytes=0):
    return lib.sessd_deconv_ks_wgrad(x, gout, batch, cin, hin, win, cout, s, gw, ws, ws_bytes, None)


def test_einval_before_any_launch():
    for f in (dgrad, wgrad):
        assert f(s=3) == EINVAL and f(s=0) == EINVAL and f(s=8) == EINVAL
        assert f(cin=63) == EINVAL and f(cin=0) == EINVAL and f(cin=1) == EINVAL
        assert f(cout=48) == EINVAL and f(cout=0) == EINVAL and f(cout=16) == EINVAL
        assert f(batch=65536) == EINVAL and f(batch=-1) == EINVAL and f(hin=-1) == EINVAL
        # the empty call launches nothing, whatever the pointers
        assert f(batch=0) == OK and f(hin=0) == OK and f(win=0) == OK
    assert dgrad(batch=0, gout=None, wpk=None, gin=None) == OK and wgrad(hin=0, x=None, gout=None, gw=None, ws=None) == OK
    # NULL tensors on a non-empty call
    assert dgrad(gout=None) == EINVAL and dgrad(wpk=None) == EINVAL and dgrad(gin=None) == EINVAL
    assert wgrad(x=None) == EINVAL and wgrad(gout=None) == EINVAL and wgrad(gw=None) == EINVAL and wgrad(ws=None) == EINVAL
    # a grad_out that the float2 / float4 loads cannot take
    assert dgrad(gout=P + 4) == EINVAL and wgrad(gout=P + 8, s=4, ws_bytes=1 << 40) == EINVAL
    # tensors that 32-bit byte offsets cannot address: one image's grad_out (dgrad), the whole input / grad_out (wgrad), the weight
    assert dgrad(batch=1, cin=2, hin=2048, win=2048, s=4, cout=32) == EINVAL
    assert dgrad(batch=1, cin=16384, hin=1, win=1, s=4, cout=2048) == EINVAL
    assert wgrad(batch=64, cin=64, hin=512, win=512, cout=32, s=1, ws_bytes=1 << 40) == EINVAL
    assert wgrad(batch=64, cin=2, hin=256, win=256, cout=32, s=4, ws_bytes=1 << 40) == EINVAL
    assert wgrad(batch=1, cin=16384, hin=1, win=1, cout=2048, s=4, ws_bytes=1 << 40) == EINVAL
    # a workspace smaller than the query asks for
    need = lib.sessd_deconv_ks_wgrad_workspace_bytes(2, 64, 8, 8, 32, 2)
    assert need > 0 and wgrad(ws_bytes=need - 1) == EINVAL and wgrad(ws_bytes=0) == EINVAL


def test_workspace_bytes_follows_the_chunk_rule():
    wb = lib.sessd_deconv_ks_wgrad_workspace_bytes
    assert wb(2, 64, 8, 8, 32, 3) == 0 and wb(2, 63, 8, 8, 32, 2) == 0 and wb(2, 64, 8, 8, 48, 2) == 0 and wb(70000, 64, 8, 8, 32, 2) == 0
    for cin, cout, s, cap in ((64, 128, 1, 128), (128, 128, 2, 128), (256, 128, 4, 16), (6, 32, 2, 128), (1024, 1024, 4, 8)):
        per = cin * cout * s * s * 4
        assert wb(0, cin, 8, 8, cout, s) == per                 # positive inside the domain, the empty call included
        last = 0
        for hw in (1, 2, 3, 5, 8, 13, 40, 100, 300, 1000, 1100):   # one image of 1 x hw: ceil(hw / 8) stages
            got = wb(1, cin, 1, hw, cout, s)
            stages = (hw + 7) // 8
            assert got == min(stages, cap) * per, (cin, cout, s, hw)
            assert got >= last                                  # monotone in the pixel count, flat from the cap on
            last = got
        assert last == cap * per and wb(4, cin, 100, 100, cout, s) == cap * per
    # the three PointPillars up-samplers at batch 2
    assert wb(2, 64, 248, 216, 128, 1) == 128 * 64 * 128 * 4
    assert wb(2, 128, 124, 108, 128, 2) == 128 * 128 * 128 * 4 * 4
    assert wb(2, 256, 62, 54, 128, 4) == 16 * 256 * 128 * 16 * 4


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


def test_predicates_refuse_cpu_tensors_and_cpu_modules():
    up = nn.ConvTranspose2d(64, 128, 2, stride=2, bias=False)
    conv = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    assert not ops.deconv_ks_covers(up, torch.zeros(2, 64, 8, 8)) and not ops.conv2d_train_covers(conv, torch.zeros(2, 64, 8, 8))
    assert not ops.deconv_ks_covers(up, None) and not ops.conv2d_train_covers(conv, None)
    assert not ops.deconv_ks_covers(up, _OnDevice(2, 64, 8, 8)) and not ops.conv2d_train_covers(conv, _OnDevice(2, 64, 8, 8))


def test_deconv_ks_covers(device_stand_in):
    x = _OnDevice(2, 64, 8, 8)
    T = nn.ConvTranspose2d
    for cin, s, h, w in ((64, 1, 248, 216), (128, 2, 124, 108), (256, 4, 62, 54)):     # the PointPillars up-samplers
        assert ops.deconv_ks_covers(T(cin, 128, s, stride=s, bias=False), _OnDevice(2, cin, h, w))
    assert ops.deconv_ks_covers(T(64, 32, 4, stride=4, bias=False), _OnDevice(1, 64, 5, 7))           # any H, W
    assert not ops.deconv_ks_covers(T(64, 128, 3, stride=3, bias=False), x)                           # s
    assert not ops.deconv_ks_covers(T(64, 128, 3, stride=2, padding=1, output_padding=1, bias=False), x)   # kernel != stride
    assert not ops.deconv_ks_covers(T(64, 128, (2, 4), stride=(2, 4), bias=False), x)                 # two strides
    assert not ops.deconv_ks_covers(T(64, 128, 4, stride=4, padding=1, bias=False), x)                # padding
    assert not ops.deconv_ks_covers(T(64, 128, 2, stride=2, dilation=2, bias=False), x)               # dilation
    assert not ops.deconv_ks_covers(T(64, 128, 2, stride=2, groups=2, bias=False), x)                 # groups
    assert not ops.deconv_ks_covers(T(64, 128, 2, stride=2, bias=True), x)                            # bias
    assert not ops.deconv_ks_covers(T(62, 128, 2, stride=2, bias=False), x)                           # x has other channels
    assert not ops.deconv_ks_covers(T(63, 128, 2, stride=2, bias=False), _OnDevice(2, 63, 8, 8))      # odd cin
    assert not ops.deconv_ks_covers(T(64, 48, 2, stride=2, bias=False), x)                            # cout % 32
    assert not ops.deconv_ks_covers(T(64, 128, 2, stride=2, bias=False).double(), x)                  # a float64 weight
    assert not ops.deconv_ks_covers(nn.Conv2d(64, 128, 2, stride=2, bias=False), x)                   # the stride < 1 "up-sampler"
    with_output_padding = T(64, 128, 2, stride=2, bias=False)
    with_output_padding.output_padding = (1, 1)
    assert not ops.deconv_ks_covers(with_output_padding, x)


def test_conv2d_train_covers(device_stand_in):
    C = nn.Conv2d
    x = _OnDevice(2, 64, 16, 16)
    assert ops.conv2d_train_covers(C(64, 32, 3, padding=1, bias=False), x)
    assert ops.conv2d_train_covers(C(64, 32, 3, stride=2, padding=1, bias=False), x)                  # wout = 8
    assert ops.conv2d_train_covers(C(64, 32, 1, bias=False), x) and ops.conv2d_train_covers(C(64, 32, 3, padding=1), x)
    assert ops.conv2d_train_covers(C(64, 32, 3, stride=2, bias=False), x, padded=True)                # behind a ZeroPad2d(1)
    assert not ops.conv2d_train_covers(C(64, 32, 3, stride=2, bias=False), x)                         # ... and without one
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, bias=False), x, padded=True)           # padded twice
    assert not ops.conv2d_train_covers(C(64, 32, 1, bias=False), x, padded=True)
    assert not ops.conv2d_train_covers(C(64, 32, 5, padding=2, bias=False), x)                        # k
    assert not ops.conv2d_train_covers(C(64, 32, (1, 3), padding=(0, 1), bias=False), x)
    assert not ops.conv2d_train_covers(C(64, 32, 3, stride=4, padding=1, bias=False), x)              # stride
    assert not ops.conv2d_train_covers(C(64, 32, 1, stride=2, bias=False), x)                         # k = 1 is stride 1
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=2, bias=False), x)                        # padding
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding="same", bias=False), x)
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, padding_mode="reflect", bias=False), x)
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=2, dilation=2, bias=False), x)            # dilation
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, groups=2, bias=False), x)              # groups
    assert not ops.conv2d_train_covers(C(63, 32, 3, padding=1, bias=False), _OnDevice(2, 63, 16, 16))  # the packers: odd cin
    assert not ops.conv2d_train_covers(C(64, 33, 3, padding=1, bias=False), x)                        # ... odd cout (the adjoint layer)
    assert not ops.conv2d_train_covers(C(32, 32, 3, padding=1, bias=False), x)                        # x has other channels
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(2, 64, 16, 12))  # wout % 8
    assert not ops.conv2d_train_covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 16, 8))   # wout = 4
    assert not ops.conv2d_train_covers(C(64, 32, 3, stride=2, padding=1, bias=False), _OnDevice(2, 64, 15, 16))  # stride 2: odd H
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, bias=False), _OnDevice(64, 64, 512, 512))         # 2 GiB
    assert not ops.conv2d_train_covers(C(64, 32, 3, padding=1, bias=False).double(), x)
    assert not ops.conv2d_train_covers(nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False), x)
    # PointPillars at full size (the known limit): block 0 is covered, the 3x3 layers of blocks 1 and 2 are not (wout 108, 54)
    assert ops.conv2d_train_covers(C(64, 64, 3, stride=2, bias=False), _OnDevice(2, 64, 496, 432), padded=True)
    assert ops.conv2d_train_covers(C(64, 64, 3, padding=1, bias=False), _OnDevice(2, 64, 248, 216))
    assert not ops.conv2d_train_covers(C(64, 128, 3, stride=2, bias=False), _OnDevice(2, 64, 248, 216), padded=True)
    assert not ops.conv2d_train_covers(C(128, 128, 3, padding=1, bias=False), _OnDevice(2, 128, 124, 108))
    assert not ops.conv2d_train_covers(C(256, 256, 3, padding=1, bias=False), _OnDevice(2, 256, 62, 54))
    # the three-class SECOND neck (200 x 176, stride 1): covered
    assert ops.conv2d_train_covers(C(128, 128, 3, stride=1, bias=False), _OnDevice(2, 128, 200, 176), padded=True)
    assert ops.conv2d_train_covers(C(128, 128, 3, padding=1, bias=False), _OnDevice(2, 128, 200, 176))
