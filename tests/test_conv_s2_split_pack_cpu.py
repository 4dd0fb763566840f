"""ops.pack_conv2d_s2_split (the weights of sessd_conv2d_s2_split_active): the three bfloat16 planes sum in float64 to the
float32 weight EXACTLY, element for element, and lie in the fragment order csrc/dense_conv_s2_split.hip documents:
[ceil(cout/128)][cin/16][tap 9 = 3 ky + kx][plane 3][(cout/32)%4][lane = (cin/8)%2 * 32 + cout%32][cin%8]. No GPU."""
import numpy as np
import pytest
import torch

from sessd_hip import ops


def _unpack(planes, cin, cout):
    """the documented layout read back with numpy and this test's own index arithmetic -> (3, cout padded, cin, 3, 3) float64"""
    ng = (cout + 127) // 128
    assert tuple(planes.shape) == (ng, cin // 16, 9, 3, 4, 64, 8) and planes.dtype == torch.bfloat16
    p = planes.to(torch.float64).numpy()
    co, ci = np.arange(ng * 128), np.arange(cin)
    g, cb, c32 = co // 128, (co // 32) % 4, co % 32
    ks, half, c8 = ci // 16, (ci // 8) % 2, ci % 8
    out = np.zeros((3, ng * 128, cin, 3, 3))
    for pl in range(3):
        for ky in range(3):
            for kx in range(3):
                lane = half[None, :] * 32 + c32[:, None]
                out[pl, :, :, ky, kx] = p[g[:, None], ks[None, :], 3 * ky + kx, pl, cb[:, None], lane, c8[None, :]]
    return torch.from_numpy(out)


@pytest.mark.parametrize("cin,cout", [(128, 256), (32, 40), (16, 128)])
def test_split_planes_sum_to_the_weight_exactly(cin, cout):
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    planes = ops.pack_conv2d_s2_split(w)   # plain torch: here on the CPU (PackedConv.wsplit_s2() makes it on the weight's device)
    u = _unpack(planes, cin, cout)
    assert torch.equal(u[:, :cout].sum(0), w.to(torch.float64))
    assert not u[:, cout:].any()   # padded couts are zero
    # each term is the round-to-nearest bf16 of what the terms before it left
    assert torch.equal(u[0, :cout].float(), w.to(torch.bfloat16).float())
    r1 = w.double() - u[0, :cout]
    assert torch.equal(u[1, :cout].float(), r1.float().to(torch.bfloat16).float())
    r2 = r1 - u[1, :cout]
    assert torch.equal(u[2, :cout].float(), r2.float().to(torch.bfloat16).float())


def test_no_split_planes_for_cin_not_a_multiple_of_16():
    with pytest.raises(ValueError):
        ops.pack_conv2d_s2_split(torch.randn(32, 24, 3, 3))
    with pytest.raises(ValueError):
        ops.pack_conv2d_s2_split(torch.randn(32, 16, 1, 1))


def test_packed_conv_accessor_is_lazy_cached_and_none_when_not_eligible():
    w = torch.randn(40, 32, 3, 3)
    pc = ops.pack_conv2d(w, stride=2)
    planes = pc.wsplit_s2()
    assert planes is pc.wsplit_s2()
    assert torch.equal(planes.view(torch.int16), ops.pack_conv2d_s2_split(w).view(torch.int16))
    assert ops.pack_conv2d(torch.randn(32, 24, 3, 3), stride=2).wsplit_s2() is None    # cin % 16
    assert ops.pack_conv2d(torch.randn(32, 32, 3, 3), stride=1).wsplit_s2() is None    # stride 1: a Winograd layer
    assert ops.pack_conv2d(torch.randn(32, 32, 1, 1), stride=1).wsplit_s2() is None    # 1x1


def test_entry_point_rejects_bad_arguments_before_touching_the_device():
    import ctypes
    import sessd_hip
    one = ctypes.c_int32(1)
    p = ctypes.addressof(one)
    from sessd_hip._lib import ConvEpilogue, TileList
    f = lambda cin=32, hin=8, win=8, batch=1, cout=32, hout=4, wout=4, tl=p, nl=p, cap=4, w=p, x=p, out=p: \
        sessd_hip.lib.sessd_conv2d_s2_split_active(x, batch, cin, hin, win, w, out, cout, hout, wout, ConvEpilogue(relu=1),
                                                   TileList(tl, nl, cap), None)
    assert sessd_hip.lib.sessd_conv2d_s2_split_active(p, 1, 32, 8, 8, p, p, 32, 4, 4, None, None, None) == -1    # no list at all
    assert f(cin=24) == -1 and f(cin=0) == -1 and f(batch=0) == -1 and f(cout=0) == -1
    assert f(hout=3, hin=6) == -1 and f(wout=5, win=10) == -1            # odd output maps have no 2x2 tile grid
    assert f(hin=9) == -1 and f(hin=6) == -1 and f(win=9) == -1 and f(win=6) == -1   # hin in {2 hout - 1, 2 hout}
    assert f(tl=None) == -1 and f(nl=None) == -1 and f(cap=0) == -1 and f(w=None) == -1 and f(x=None) == -1 and f(out=None) == -1
    assert f(cin=16, hin=2048, win=2048, hout=1024, wout=1024, batch=8) == -1    # 32-bit buffer offsets (input)
    assert f(cin=16, hin=1024, win=1024, hout=512, wout=512, cout=4096) == -1    # ... (output)
