"""sessd_deconv_ks_slice (csrc/deconv_ks.hip): ConvTranspose2d(cin, cout, s, stride=s) + folded BatchNorm + ReLU, s in {1, 2, 4}, in
ONE launch into a channel slice of a wider NCHW buffer, against torch float64.

Shapes: B = 2 (the batch axis of the grid), cout = 128 (four cout blocks: one workgroup's width for s = 1 / 2, four workgroups for
s = 4), the three (cin, s) of the PointPillars neck + (128, 4); (H, W) = (6, 10): 60 pixels, two 32-pixel tiles, the last one part
full, tiles that straddle image rows; (3, 33): one pixel past a tile in a row, 99 pixels -- odd, no multiple of 32.

Bound: 2e-4 * max |ref|, the project's figure for float32 dense layers (tests/test_pointpillars_neck_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from sessd_hip import SessdError, ops

pytestmark = pytest.mark.gpu

B, COUT, C_TOTAL = 2, 128, 384


def _case(cin, s, H, W):
    g = torch.Generator().manual_seed(1000 * s + cin + H)
    x = torch.randn(B, cin, H, W, generator=g)
    w = (torch.rand(cin, COUT, s, s, generator=g) * 2 - 1) * (3.0 / cin) ** 0.5
    scale = (torch.rand(COUT, generator=g) + 0.5) * torch.where(torch.rand(COUT, generator=g) < 0.2, -1.0, 1.0)
    shift = torch.randn(COUT, generator=g) * 0.3
    plain = F.conv_transpose2d(x.double(), w.double(), None, stride=s)
    ref = torch.relu(plain * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    return x, w, scale, shift, plain, ref


@pytest.mark.parametrize("H, W", [(6, 10), (3, 33)])
@pytest.mark.parametrize("cin, s", [(64, 1), (128, 2), (256, 4), (128, 4)])
def test_slice_against_float64(dev, cin, s, H, W):
    x, w, scale, shift, plain, ref = _case(cin, s, H, W)
    assert ref.shape == (B, COUT, s * H, s * W) and float(ref.max()) > 0 and bool((ref == 0).any())
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    pk = ops.pack_deconv_ks_slice(w.to(dev), s)
    assert (pk.cin, pk.cout, pk.stride) == (cin, COUT, s) and pk.wpk.numel() == w.numel()
    xd, sd, td = x.to(dev), scale.to(dev), shift.to(dev)
    bound = 2e-4 * float(ref.abs().max())
    for c_off in (0, 128, 256):
        out = torch.full((B, C_TOTAL, s * H, s * W), float("nan"), device=dev)
        got = ops.deconv_ks_slice(xd, pk, sd, td, True, out, c_off)
        assert got is out
        o = out.cpu()
        mine = o[:, c_off:c_off + COUT]
        assert bool(torch.isfinite(mine).all())
        err = float((mine.double() - ref).abs().max())
        print("s = %d, cin %d, %d x %d, c_off %d: max err %.3e, bound %.3e" % (s, cin, H, W, c_off, err, bound))
        assert err <= bound
        rest = torch.cat([o[:, :c_off], o[:, c_off + COUT:]], 1)
        assert rest.shape[1] == C_TOTAL - COUT and bool(torch.isnan(rest).all())    # nothing outside the slice is written
    # without scale / shift / ReLU: the plain transposed conv
    out = torch.full((B, C_TOTAL, s * H, s * W), float("nan"), device=dev)
    ops.deconv_ks_slice(xd, pk, None, None, False, out, 128)
    o = out.cpu()
    err0, bound0 = float((o[:, 128:256].double() - plain).abs().max()), 2e-4 * float(plain.abs().max())
    print("s = %d, cin %d, %d x %d, plain: max err %.3e, bound %.3e" % (s, cin, H, W, err0, bound0))
    assert err0 <= bound0 and bool((plain < 0).any())
    assert bool(torch.isnan(o[:, :128]).all()) and bool(torch.isnan(o[:, 256:]).all())


def test_bad_arguments_are_refused_on_the_host(dev):
    """SESSD_EINVAL surfaces as the binding's error before anything is launched: the NaN-filled output is untouched."""
    H, W = 4, 8
    wpk = torch.zeros(256 * COUT * 16, device=dev)
    scale = torch.ones(COUT, device=dev)

    def run(cin, s, c_off):
        x = torch.zeros(B, cin, H, W, device=dev)
        out = torch.full((B, C_TOTAL, s * H, s * W), float("nan"), device=dev)
        with pytest.raises(SessdError, match="invalid argument"):
            ops.deconv_ks_slice(x, ops.PackedDeconvKs(wpk, cin, COUT, s), scale, scale, True, out, c_off)
        assert bool(torch.isnan(out).all())

    run(128, 3, 0)        # s not in {1, 2, 4}
    run(63, 2, 0)         # odd cin
    run(128, 2, 320)      # c_off + cout > c_total
    with pytest.raises(ValueError):
        ops.pack_deconv_ks_slice(torch.zeros(128, COUT, 3, 3, device=dev), 3)
    with pytest.raises(ValueError):   # out's spatial size must be s times x's
        ops.deconv_ks_slice(torch.zeros(B, 128, H, W, device=dev), ops.pack_deconv_ks_slice(torch.zeros(128, COUT, 2, 2, device=dev), 2),
                            None, None, True, torch.zeros(B, C_TOTAL, 2 * H, 2 * W + 1, device=dev), 0)
    # an empty call is fine and launches nothing
    out = torch.full((B, C_TOTAL, 0, 16), float("nan"), device=dev)
    ops.deconv_ks_slice(torch.zeros(B, 128, 0, 8, device=dev), ops.PackedDeconvKs(wpk, 128, COUT, 2), None, None, True, out, 0)
