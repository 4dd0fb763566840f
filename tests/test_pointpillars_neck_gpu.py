"""The PointPillars neck on the device: the kernel-size = stride transposed up-samplers lowered by ops.pack_deconv2d_ks onto
sessd_conv2d_mfma (s * s output-parity launches of one tap each) against torch float64, and the mirror RPN with the config's
three blocks and up-samplers of stride 1 / 2 / 4 against the golden output of the reference's own class
(tests/golden/pillars_ref.npz).

Bound: 2e-4 * max |out|, the project's figure for float32 dense layers (tests/test_rpn_head_gpu.py holds the neck output to it)."""
import pytest
import torch
import torch.nn.functional as F

import pillars_ref as PR
from sessd_hip import ops

pytestmark = pytest.mark.gpu

B, H, W = 2, 6, 10


@pytest.mark.parametrize("cin", [128, 256])
@pytest.mark.parametrize("s", [2, 4])
def test_deconv_ks_against_float64(dev, s, cin):
    cout = 128
    g = torch.Generator().manual_seed(100 * s + cin)
    x = torch.randn(B, cin, H, W, generator=g)
    w = (torch.rand(cin, cout, s, s, generator=g) * 2 - 1) * (3.0 / cin) ** 0.5
    scale = (torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0)
    shift = torch.randn(cout, generator=g) * 0.3
    ref = torch.relu(F.conv_transpose2d(x.double(), w.double(), None, stride=s) * scale.double().view(1, -1, 1, 1)
                     + shift.double().view(1, -1, 1, 1))
    assert ref.shape == (B, cout, s * H, s * W) and float(ref.max()) > 0 and bool((ref == 0).any())
    pc = ops.pack_deconv2d_ks(w.to(dev), s)
    assert pc.kind == "deconv_ks" and pc.stride == s and len(pc.launches) == s * s
    assert all(la.ntaps == 1 and la.out_mul == s and la.in_mul == 1 and int(la.dy[0]) == 0 and int(la.dx[0]) == 0
               for la in pc.launches)
    assert sorted((la.py, la.px) for la in pc.launches) == [(py, px) for py in range(s) for px in range(s)]
    out = torch.full((B, cout, s * H, s * W), float("nan"), device=dev)
    got = ops.conv2d(x.to(dev), pc, scale.to(dev), shift.to(dev), True, out=out)
    assert got is out and bool(torch.isfinite(out).all())    # every output pixel belongs to one parity class
    err, bound = float((out.cpu().double() - ref).abs().max()), 2e-4 * float(ref.abs().max())
    print("deconv k = s = %d, cin %d: max err %.3e, bound %.3e" % (s, cin, err, bound))
    assert err <= bound
    # without BatchNorm / ReLU, and the families that do not cover it are refused
    plain = ops.conv2d(x.to(dev), pc, None, None, False)
    ref0 = F.conv_transpose2d(x.double(), w.double(), None, stride=s)
    assert float((plain.cpu().double() - ref0).abs().max()) <= 2e-4 * float(ref0.abs().max())
    with pytest.raises(ValueError):
        ops.conv2d(x.to(dev), pc, None, None, False, tile_cfg=22)


def test_mirror_rpn_three_blocks_against_the_reference(dev, golden_dir):
    from det3d.models.necks.rpn_v1 import RPN
    r = PR.load_golden(golden_dir)["rpn3"]
    neck = RPN(**PR.RPN3_ARGS)
    neck.load_state_dict(r["sd"])
    neck.eval().to(dev)
    with torch.no_grad():
        got = neck(r["x"].to(dev))
    ref = r["out"]
    assert got.shape == ref.shape == (2, 384, 8, 12)
    err, bound = float((got.cpu() - ref).abs().max()), 2e-4 * float(ref.abs().max())
    print("mirror RPN (3 blocks, up-samplers 1 / 2 / 4) vs reference: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    # every up-sampler went through the lowering: 1 + 4 + 16 launches
    kinds = {k: (v[1].kind, len(v[1].launches)) for k, v in neck._low._cache.items() if k.startswith("de")}
    assert kinds == {"de0.0": ("conv", 1), "de1.0": ("deconv_ks", 4), "de2.0": ("deconv_ks", 16)}, kinds
