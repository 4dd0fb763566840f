"""Stream-K Winograd shape 3 (tile_cfg 25; csrc/dense_wino_sk.hip SPLIT): shape 0's units, rounds and shares on the bf16 matrix
cores, f32 operands split three ways. Held to float64 torch at f32 accuracy: no worse than 2x the f32 shape 0 on the same input
and geometry, and within 2e-6 of the output scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sessd_hip import ops

pytestmark = pytest.mark.gpu


def _problem(cin, cout, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    return x, w, F.conv2d(x.double(), w.double(), padding=1)


def test_pack_planes_sum_to_f32_u(dev):
    """layout 4: the three bf16 planes add up (float64) to the f32 U of shape 0's packing, element for element"""
    for co, ci, adjoint in ((128, 128, False), (256, 128, True), (40, 32, False)):
        w = (torch.randn(co, ci, 3, 3, generator=torch.Generator().manual_seed(co + ci)) * 0.05).to(dev)
        u0 = ops.pack_winograd_sk(w, 0, adjoint=adjoint).cpu()   # [grp][ci/2][wave 8][h 2][j 32][cb 4][xl 2]
        if adjoint:
            co, ci = ci, co
        ng = (co + 127) // 128
        u0 = u0.view(ng, ci // 2, 8, 2, 32, 4, 2).permute(0, 5, 4, 1, 3, 2, 6).reshape(ng * 128, ci, 16)   # (cout, cin, xi)
        p = ops.pack_winograd_sk(w, 3, adjoint=adjoint)
        assert p.dtype == torch.bfloat16 and p.shape == (ng, 8, ci // 2, 3, 64, 8)
        s = p.cpu().double().view(ng, 8, ci // 16, 2, 4, 3, 2, 32, 8).sum(dim=5)   # [grp][wave][round][xl][cb][hh][i][e]
        s = s.permute(0, 4, 6, 2, 5, 7, 1, 3).reshape(ng * 128, ci, 16)          # (cout, cin, xi = 2 wave + xl)
        assert torch.equal(s, u0.double()), float((s - u0.double()).abs().max())


def _err(got, ref):
    return float((got.cpu().double() - ref).abs().max())


@pytest.mark.parametrize("cin,cout,B,H,W,wgs", [(128, 128, 1, 200, 176, 0), (256, 256, 1, 100, 88, 0), (128, 128, 1, 200, 176, 104),
                                                 (256, 256, 2, 100, 88, 64), (32, 128, 1, 8, 8, 16), (16, 40, 3, 10, 66, 8)])
def test_split_full_map(dev, cin, cout, B, H, W, wgs):
    x, w, ref = _problem(cin, cout, B, H, W, cin + H + wgs)
    pc = ops.pack_conv2d(w.to(dev), 1)
    xd = x.to(dev)
    ws3 = ops.winograd_sk_workspace(B, H, W, cout, dev, wgs, 3)
    ws0 = ops.winograd_sk_workspace(B, H, W, cout, dev, wgs, 0)
    a = ops.conv2d(xd, pc, None, None, False, tile_cfg=25, workspace=ws3, workgroups=wgs)
    b = ops.conv2d(xd, pc, None, None, False, tile_cfg=25, workspace=ws3, workgroups=wgs)
    f32 = ops.conv2d(xd, pc, None, None, False, tile_cfg=22, workspace=ws0, workgroups=wgs)
    torch.cuda.synchronize()
    units = B * (((H // 2) * (W // 2) + 31) // 32) * ((cout + 127) // 128)
    assert int(ws3[:units * 4].view(torch.int32).abs().sum().item()) == 0       # counters left at zero
    assert torch.equal(a, b)
    e3, e0, scale = _err(a, ref), _err(f32, ref), float(ref.abs().max())
    print("split err %.3e  f32 err %.3e  max|ref| %.3f" % (e3, e0, scale))
    assert e3 <= 2 * e0 and e3 <= 2e-6 * scale
    # the fused epilogue (BatchNorm, ReLU, residual) as the f32 shape's
    g = torch.Generator().manual_seed(1)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    res = torch.randn(B, cout, H, W, generator=g).to(dev)
    full = ops.conv2d(xd, pc, sc, sh, True, residual=res, tile_cfg=25, workspace=ws3, workgroups=wgs)
    want = torch.relu(ref * sc.cpu().double().view(1, -1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1)) + res.cpu().double()
    assert _err(full, want) <= 4e-6 * float(want.abs().max())


@pytest.mark.parametrize("cin,cout,H,W", [(128, 128, 200, 176), (256, 256, 100, 88)])
@pytest.mark.parametrize("min_rounds", [-1, 4])
def test_split_list(dev, cin, cout, H, W, min_rounds):
    """over a tile list (whole-unit shares / stream-K shares of 4 rounds): error bound as the full map; a whole-unit launch writes
    no partial sum; two launches give the same bits"""
    B = 1
    x, w, ref = _problem(cin, cout, B, H, W, cin + 7)
    pc = ops.pack_conv2d(w.to(dev), 1)
    xd = x.to(dev)
    nt = (H // 2) * (W // 2)
    rng = np.random.default_rng(3)
    tiles = np.sort(rng.choice(nt, nt * 2 // 5, replace=False)).astype(np.int32)
    tl = torch.from_numpy(tiles).to(dev)
    n = torch.tensor([len(tiles)], dtype=torch.int32, device=dev)
    ws = ops.winograd_sk_workspace(B, H, W, cout, dev, 0, 3)
    if min_rounds < 0:
        ws.fill_(0x7F)
        units = B * ((nt + 31) // 32) * ((cout + 127) // 128)
        ws[:units * 4].zero_()
    outs = []
    for _ in range(2):
        out = torch.full((B, cout, H, W), float("nan"), device=dev)
        ops.conv2d_winograd_sk_active(xd, pc.upk_sk(3), cout, None, None, False, out, 3, ws, tl, n, min_rounds=min_rounds)
        outs.append(out)
    torch.cuda.synchronize()
    if min_rounds < 0:
        assert bool((ws[units * 4:] == 0x7F).all()), "a whole-unit launch wrote a partial sum"
    ty, tx = torch.from_numpy(tiles // (W // 2)).long(), torch.from_numpy(tiles % (W // 2)).long()
    sel = lambda t: torch.stack([t[:, :, 2 * ty + a, 2 * tx + b] for a in (0, 1) for b in (0, 1)], -1)
    got = sel(outs[0].cpu().double())
    assert torch.isfinite(got).all() and torch.equal(got, sel(outs[1].cpu().double()))
    want = sel(ref)
    ws0 = ops.winograd_sk_workspace(B, H, W, cout, dev, 0, 0)
    f32 = torch.full((B, cout, H, W), float("nan"), device=dev)
    ops.conv2d_winograd_sk_active(xd, pc.upk_sk(0), cout, None, None, False, f32, 0, ws0, tl, n, min_rounds=min_rounds)
    e3, e0, scale = float((got - want).abs().max()), float((sel(f32.cpu().double()) - want).abs().max()), float(ref.abs().max())
    print("list split err %.3e  f32 err %.3e  max|ref| %.3f" % (e3, e0, scale))
    assert e3 <= 2 * e0 and e3 <= 2e-6 * scale


def test_split_list_equals_full_map(dev):
    """listed tiles (whole-unit shares) equal a full-map launch without cut units (8 workgroups, 4 units each) bit for bit: a
    tile's column of the MFMAs sees only its own patch, in the same order"""
    cin, cout, B, H, W = 128, 128, 1, 64, 64
    x, w, _ = _problem(cin, cout, B, H, W, 5)
    pc = ops.pack_conv2d(w.to(dev), 1)
    xd = x.to(dev)
    nt = (H // 2) * (W // 2)
    tiles = np.sort(np.random.default_rng(4).choice(nt, nt // 3, replace=False)).astype(np.int32)
    tl, n = torch.from_numpy(tiles).to(dev), torch.tensor([len(tiles)], dtype=torch.int32, device=dev)
    ws = ops.winograd_sk_workspace(B, H, W, cout, dev, 8, 3)
    full = ops.conv2d(xd, pc, None, None, False, tile_cfg=25, workspace=ws, workgroups=8)
    out = torch.full_like(full, float("nan"))
    ops.conv2d_winograd_sk_active(xd, pc.upk_sk(3), cout, None, None, False, out, 3, ws, tl, n, workgroups=8, min_rounds=-1)
    ty, tx = torch.from_numpy(tiles // (W // 2)).long().to(dev), torch.from_numpy(tiles % (W // 2)).long().to(dev)
    for a in (0, 1):
        for b in (0, 1):
            assert torch.equal(out[:, :, 2 * ty + a, 2 * tx + b], full[:, :, 2 * ty + a, 2 * tx + b])


def test_engine_reports_split_shape(dev):
    """force_active_tiles(): the 8-wave list layers run shape 3, and the packing it needs exists"""
    from sessd_hip import configs, engine, synth
    if not engine.WINO_SPLIT:
        pytest.skip("SESSD_WINO_SPLIT=0")
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0)
    eng = engine.InferenceEngine(model, VG["range"], VG["voxel_size"], 5, 16000, configs.TEST_CFG, 1, 20480, dev)
    eng.set_points([torch.from_numpy(synth.make_frame(1, 20000)).to(dev)])
    cfg = eng.force_active_tiles()
    assert {l: s for l, (s, _) in cfg.items() if l in (1, 5, 9)} == {1: 3, 5: 3, 9: 3}
    eng.enqueue()
    torch.cuda.synchronize()
    assert {1, 5, 9} <= set(eng._active_layers())
    assert torch.isfinite(eng.t["o0"]).all() and torch.isfinite(eng.t["o1"]).all()
