"""ops.pack_deconv2d_s2_split (the weights of sessd_deconv2d_s2_pair_split_active): the three bfloat16 planes sum in float64 to
the float32 weight EXACTLY, element for element, and lie in the fragment order csrc/dense_deconv_split.hip documents:
[ceil(cout/128)][cin/16][tap 9][plane 3][(cout/32)%4][lane = (cin/8)%2 * 32 + cout%32][cin%8]. No GPU."""
import pytest
import torch

from sessd_hip import ops


def _unpack(planes, cin, cout):
    """the documented layout read back with this test's own index arithmetic -> (3, cin, cout, 3, 3) float64"""
    ng, ks, nt, npl, ncb, nl, n8 = planes.shape
    assert (ng, ks, nt, npl, ncb, nl, n8) == ((cout + 127) // 128, cin // 16, 9, 3, 4, 64, 8) and planes.dtype == torch.bfloat16
    p = planes.to(torch.float64)
    out = torch.zeros(3, cin, ng * 128, 3, 3, dtype=torch.float64)
    for t, (ky, kx) in enumerate(ops.DECONV_SPLIT_TAPS):
        for g in range(ng):
            for cb in range(4):
                # [k-step][plane][lane half][cout % 32][cin % 8] -> [plane][cin = k-step * 16 + half * 8 + i][cout % 32]
                blk = p[g, :, t, :, cb].reshape(ks, 3, 2, 32, 8).permute(1, 0, 2, 4, 3).reshape(3, cin, 32)
                out[:, :, g * 128 + cb * 32:g * 128 + cb * 32 + 32, ky, kx] = blk
    return out


@pytest.mark.parametrize("cin,cout", [(256, 128), (32, 40), (16, 128)])
def test_split_planes_sum_to_the_weight_exactly(cin, cout):
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cin, cout, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    planes = ops.pack_deconv2d_s2_split(w)   # plain torch: here on the CPU (PackedConv.wsplit() makes it on the weight's device)
    assert sorted(ops.DECONV_SPLIT_TAPS) == [(ky, kx) for ky in range(3) for kx in range(3)]
    u = _unpack(planes, cin, cout)
    assert torch.equal(u[:, :, :cout].sum(0), w.to(torch.float64))
    assert not u[:, :, cout:].any()   # padded couts are zero
    # each term is the round-to-nearest bf16 of what the terms before it left
    assert torch.equal(u[0, :, :cout].float(), w.to(torch.bfloat16).float())
    r1 = w.double() - u[0, :, :cout]
    assert torch.equal(u[1, :, :cout].float(), r1.float().to(torch.bfloat16).float())


def test_no_split_planes_for_cin_not_a_multiple_of_16():
    with pytest.raises(ValueError):
        ops.pack_deconv2d_s2_split(torch.randn(24, 32, 3, 3))


def test_entry_point_rejects_bad_arguments_before_touching_the_device():
    import ctypes
    import sessd_hip
    one = ctypes.c_int32(1)
    p = ctypes.addressof(one)
    from sessd_hip._lib import ConvEpilogue, TileList
    f = lambda cin=32, hin=8, win=8, batch=1, cout=32, tl=p, nl=p, cap=4, wa=p, relu_b=1: sessd_hip.lib.sessd_deconv2d_s2_pair_split_active(
        p, batch, cin, hin, win, wa, p, p, p, cout, ConvEpilogue(relu=1), ConvEpilogue(relu=relu_b), TileList(tl, nl, cap), None)
    assert sessd_hip.lib.sessd_deconv2d_s2_pair_split_active(p, 1, 32, 8, 8, p, p, p, p, 32, None, None, None, None) == -1   # no list at all
    assert f(relu_b=0) == -1   # the kernel has one activation for both layers
    assert f(cin=24) == -1 and f(cin=0) == -1 and f(hin=7) == -1 and f(win=9) == -1 and f(batch=0) == -1 and f(cout=0) == -1
    assert f(tl=None) == -1 and f(nl=None) == -1 and f(cap=0) == -1 and f(wa=None) == -1
    assert f(cin=16, hin=1024, win=1024, batch=32) == -1 and f(cin=4096, hin=1024, win=1024, cout=1) == -1   # 32-bit buffer offsets
