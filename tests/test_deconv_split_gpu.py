"""sessd_deconv2d_s2_pair_split_active (csrc/dense_deconv_split.hip): the transposed pair over a tile list on the bf16 matrix
cores with three-way split operands, held to float64 torch (F.conv_transpose2d(., 2, 1, 1) + scale / shift / ReLU + residual) and
to the f32 pair kernel (ops.deconv2d_s2_pair_active, tile_cfg 12) on the same inputs.

Accuracy rule, over the listed blocks, with e_split / e_f32 the largest absolute errors against float64:
e_split <= 2 e_f32 (the rule of tests/test_wino_split_gpu.py for the merged split shape) and e_split <= 2e-5 max|ref|
(the tolerance every list kernel is held to first hand, tests/test_dense_active_gpu.py). Both errors are printed."""
import numpy as np
import pytest
import torch

from sessd_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = [(16, 128, 1, 4, 4),      # one K step
          (32, 40, 3, 6, 10),      # cout not a multiple of 32, odd tile columns, several images in one list
          (256, 128, 1, 8, 12)]    # the layer's own channel counts
LISTS = ["empty", "one", "33", "all", "subset", "cap"]
_CASES = {}


def _case(shape):
    """inputs on the CPU and the float64 references, computed once per shape and left unchanged"""
    if shape not in _CASES:
        import torch.nn.functional as F
        cin, cout, B, hin, win = shape
        g = torch.Generator().manual_seed(1000 + cin + cout + hin)
        x = torch.randn(B, cin, hin, win, generator=g)
        lay = [(torch.randn(cin, cout, 3, 3, generator=g) / (3.0 * cin ** 0.5), 0.5 + torch.rand(cout, generator=g),
                torch.randn(cout, generator=g) * 0.3) for _ in range(2)]
        res = torch.randn(B, cout, 2 * hin, 2 * win, generator=g)
        ref = []
        for l, (w, sc, sh) in enumerate(lay):
            y = F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1, output_padding=1)
            y = torch.relu(y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
            ref.append(y + res.double() if l == 0 else y)   # the residual belongs to layer a only, after the ReLU
        _CASES[shape] = dict(x=x, lay=lay, res=res, ref=ref)
    return _CASES[shape]


def _entries(shape, kind):
    """(entries, count on the device, list_cap) of a list kind; entries = image * (hin/2 * win/2) + tile"""
    cin, cout, B, hin, win = shape
    th, tw = hin // 2, win // 2
    nt = B * th * tw
    last_row = [b * th * tw + (th - 1) * tw + c for b in range(B) for c in range(tw)]
    last_col = [b * th * tw + r * tw + tw - 1 for b in range(B) for r in range(th)]
    if kind == "empty":
        return list(range(nt)), 0, nt
    if kind == "one":
        return [nt - 1], 1, 1
    if kind == "33":
        # one past two units of 16 (and past the 32 entries of a unit of the f32 arm); a map with fewer tiles repeats entries (a repeated block is written twice with the same bits)
        rs = np.random.RandomState(3).permutation(nt)
        return [int(rs[i % nt]) for i in range(33)], 33, 33
    if kind == "all":
        return list(range(nt)), nt, nt
    if kind == "subset":
        # a random 40 % with the bottom-right tile and tiles of the last row and the last column: the zero taps at y + 1 = hin, x + 1 = win
        rs = np.random.RandomState(5)
        pick = set(int(v) for v in rs.permutation(nt)[:max(1, int(0.4 * nt))])
        pick |= {nt - 1, last_row[0], last_col[0]}
        return [int(v) for v in rs.permutation(sorted(pick))], len(pick), len(pick)
    if kind == "cap":
        # list_cap smaller than the device count: only the first list_cap entries are computed
        ent = [int(v) for v in np.random.RandomState(7).permutation(nt)]
        return ent, nt, max(1, nt // 2)
    raise ValueError(kind)


def _block_mask(shape, entries):
    cin, cout, B, hin, win = shape
    th, tw = hin // 2, win // 2
    m = torch.zeros(B, 1, 2 * hin, 2 * win, dtype=torch.bool)
    for e in entries:
        b, t = divmod(e, th * tw)
        r, c = divmod(t, tw)
        m[b, 0, 4 * r:4 * r + 4, 4 * c:4 * c + 4] = True
    return m


def _run(dev, shape, entries, count, cap, split=True, residual=True):
    cin, cout, B, hin, win = shape
    c = _case(shape)
    if "dev" not in c:
        c["dev"] = dict(x=c["x"].to(dev), res=c["res"].to(dev), sb=[(sc.to(dev), sh.to(dev)) for _, sc, sh in c["lay"]],
                        pc=[ops.pack_deconv2d_s2(w.to(dev)) for w, _, _ in c["lay"]])
    d = c["dev"]
    tl = torch.tensor(entries, dtype=torch.int32, device=dev)[:cap].contiguous()
    nl = torch.tensor([count], dtype=torch.int32, device=dev)
    oa = torch.full((B, cout, 2 * hin, 2 * win), float("nan"), device=dev)
    ob = torch.full((B, cout, 2 * hin, 2 * win), float("nan"), device=dev)
    res = d["res"] if residual else None
    if split:
        ops.deconv2d_s2_pair_split_active(d["x"], d["pc"][0], d["pc"][1], *d["sb"][0], *d["sb"][1], True, oa, ob, tl, nl, residual_a=res)
    else:
        ops.deconv2d_s2_pair_active(d["x"], d["pc"][0], d["pc"][1], *d["sb"][0], *d["sb"][1], True, oa, ob, tl, nl, residual_a=res, tile_cfg=12)
    torch.cuda.synchronize()
    return oa.cpu(), ob.cpu()


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_split_pair_over_a_tile_list(dev, shape, kind):
    c = _case(shape)
    entries, count, cap = _entries(shape, kind)
    listed = entries[:min(count, cap)]
    mask = _block_mask(shape, listed)
    got = _run(dev, shape, entries, count, cap)
    for l, o in enumerate(got):
        m = mask.expand_as(o)
        assert torch.isfinite(o[m]).all(), "layer %d: a listed block is not finite" % l
        assert torch.isnan(o[~m]).all(), "layer %d: a pixel outside the listed blocks was written" % l
    if not listed:
        return
    # two launches: the same bits
    again = _run(dev, shape, entries, count, cap)
    for o, o2 in zip(got, again):
        assert torch.equal(o[mask.expand_as(o)], o2[mask.expand_as(o)])
    # a listed block's bits do not depend on which other tiles are listed: against the list of every tile
    nt = shape[2] * (shape[3] // 2) * (shape[4] // 2)
    full = _run(dev, shape, list(range(nt)), nt, nt)
    for o, f in zip(got, full):
        assert torch.equal(o[mask.expand_as(o)], f[mask.expand_as(o)])
    # the residual is applied to layer a only: without it layer b keeps its bits, layer a loses exactly the residual's blocks
    nores = _run(dev, shape, entries, count, cap, residual=False)
    assert torch.equal(nores[1][mask.expand_as(nores[1])], got[1][mask.expand_as(got[1])])
    ma = mask.expand_as(got[0])
    assert float((got[0][ma].double() - nores[0][ma].double() - c["res"][ma].double()).abs().max()) <= 1e-6 * float(c["res"].abs().max() + c["ref"][0].abs().max())
    # accuracy against float64, beside the f32 pair kernel on the same inputs
    f32 = _run(dev, shape, entries, count, cap, split=False)
    for l in range(2):
        m = mask.expand_as(got[l])
        ref = c["ref"][l][m]
        e_split = float((got[l][m].double() - ref).abs().max())
        e_f32 = float((f32[l][m].double() - ref).abs().max())
        rmax = float(ref.abs().max())
        print("shape %s list %s layer %d: e_split %.3e  e_f32 %.3e  max|ref| %.3e" % (shape, kind, l, e_split, e_f32, rmax))
        assert e_split <= 2.0 * e_f32, (l, e_split, e_f32)
        assert e_split <= 2e-5 * rmax, (l, e_split, rmax)


def test_split_planes_are_built_once_on_the_device(dev):
    w = _case(SHAPES[1])["lay"][0][0]
    pc = ops.pack_deconv2d_s2(w.to(dev))
    planes = pc.wsplit()
    assert planes is pc.wsplit() and planes.is_cuda
    assert torch.equal(planes.cpu().view(torch.int16), ops.pack_deconv2d_s2_split(w).view(torch.int16))
    assert ops.pack_deconv2d_s2(torch.randn(24, 32, 3, 3).to(dev)).wsplit() is None   # cin % 16


def test_engine_runs_the_pair_on_the_split_kernel(dev):
    """An engine with the pair configuration PAIR_SPLIT_CFG set by hand against the same engine with the pair on the direct kernel
    (tile_cfg 12), every layer over its list: mid0 / mid1 within 2e-6 of their largest value (the bound tests/test_pipeline_gpu.py
    holds list engines to against full-map engines), the same detections under that test's allclose rule."""
    from sessd_hip import configs, synth
    from sessd_hip.engine import InferenceEngine, PAIR_SPLIT_CFG
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0)
    frames = [torch.from_numpy(synth.make_frame(51, 20000)).to(dev)]
    res = []
    for pair_cfg in (PAIR_SPLIT_CFG, 12):
        eng = InferenceEngine(model, VG["range"], VG["voxel_size"], 5, 16000, configs.TEST_CFG, 1, 20480, dev)
        eng.set_points(frames)
        cfg = dict(eng.DEFAULT_ACTIVE_CFG)
        cfg[eng.ACTIVE_PAIR] = (pair_cfg, 0)
        eng.force_active_tiles(cfg)
        for m in (eng.t["mid0"], eng.t["mid1"]):
            m.fill_(float("nan"))
        eng.enqueue()
        out = eng.results()
        assert sorted(eng._active_layers()) == sorted(eng.ACTIVE_SLOTS)   # every list layer ran over its list
        assert eng.active_cfg[eng.ACTIVE_PAIR][0] == pair_cfg
        mid = torch.cat([eng.t["mid0"].reshape(-1), eng.t["mid1"].reshape(-1)]).cpu()
        assert torch.isfinite(mid).all()
        res.append((mid, out))
    ref = float(res[1][0].abs().max())
    err = float((res[0][0] - res[1][0]).abs().max())
    print("mid0 / mid1: split against tile_cfg 12: max abs diff %.3e, max|ref| %.3e" % (err, ref))
    assert err <= 2e-6 * ref, (err, ref)
    for a, b in zip(res[0][1], res[1][1]):
        assert len(a["scores"]) == len(b["scores"])
        sa, sb = (np.asarray(v["scores"].cpu() if torch.is_tensor(v["scores"]) else v["scores"]) for v in (a, b))
        ba, bb = (np.asarray(v["box3d_lidar"].cpu() if torch.is_tensor(v["box3d_lidar"]) else v["box3d_lidar"]) for v in (a, b))
        assert np.allclose(ba, bb, rtol=1e-4, atol=1e-4) and np.allclose(sa, sb, rtol=1e-4)
