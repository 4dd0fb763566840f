"""sessd_conv2d_s2_split_active (csrc/dense_conv_s2_split.hip): Conv2d(cin, cout, 3, stride 2, padding 1) over a tile list on
the bf16 matrix cores with three-way split operands, held to float64 torch (F.conv2d(., stride 2, padding 1) + scale / shift /
ReLU + residual) and to the f32 list kernel (ops.conv2d_sk_active, tile_cfg 30) on the same inputs and the same list.

Accuracy rule, over the listed pixels, with e_split / e_f32 the largest absolute errors against float64:
e_split <= 2 e_f32 (the rule of tests/test_wino_split_gpu.py and tests/test_deconv_split_gpu.py for the merged split kernels) and
e_split <= 2e-5 max|ref| (the tolerance every list kernel is held to first hand, tests/test_dense_active_gpu.py). Both errors
are printed."""
import numpy as np
import pytest
import torch

from sessd_hip import ops

pytestmark = pytest.mark.gpu

SHAPES = [(16, 128, 1, 8, 8),       # one K step
          (32, 40, 3, 11, 20),      # cout no multiple of 32; odd hin: the bottom tap row falls outside; several images in one list
          (128, 256, 1, 16, 24)]    # the layer's own channel counts: two cout groups
LISTS = ["empty", "one", "33", "all", "subset", "cap"]
_CASES = {}


def _out_hw(shape):
    return (shape[3] + 1) // 2, (shape[4] + 1) // 2


def _case(shape):
    """inputs on the CPU and the float64 reference, computed once per shape and left unchanged"""
    if shape not in _CASES:
        import torch.nn.functional as F
        cin, cout, B, hin, win = shape
        ho, wo = _out_hw(shape)
        g = torch.Generator().manual_seed(2000 + cin + cout + hin)
        x = torch.randn(B, cin, hin, win, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
        sc, sh = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g) * 0.3
        res = torch.randn(B, cout, ho, wo, generator=g)
        y = F.conv2d(x.double(), w.double(), stride=2, padding=1)
        assert tuple(y.shape[2:]) == (ho, wo)
        ref = torch.relu(y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)) + res.double()   # the residual after the ReLU
        _CASES[shape] = dict(x=x, w=w, sc=sc, sh=sh, res=res, ref=ref)
    return _CASES[shape]


def _entries(shape, kind):
    """(entries, count on the device, list_cap) of a list kind; entries = image * (hout/2 * wout/2) + tile"""
    B = shape[2]
    ho, wo = _out_hw(shape)
    th, tw = ho // 2, wo // 2
    nt = B * th * tw
    if kind == "empty":
        return list(range(nt)), 0, nt
    if kind == "one":
        return [nt - 1], 1, 1
    if kind == "33":
        # one past two units of 16; a map with fewer tiles repeats entries (a repeated tile is written twice with the same bits)
        rs = np.random.RandomState(3).permutation(nt)
        return [int(rs[i % nt]) for i in range(33)], 33, 33
    if kind == "all":
        return list(range(nt)), nt, nt
    if kind == "subset":
        # a random 40 % with tiles of the first and the last row and column of tiles: the zero taps at iy = -1, ix = -1, iy = hin, ix = win
        rs = np.random.RandomState(5)
        pick = set(int(v) for v in rs.permutation(nt)[:max(1, int(0.4 * nt))])
        b = B - 1
        pick |= {0, nt - 1, b * th * tw + tw - 1, b * th * tw + (th - 1) * tw}                 # the four corners
        pick |= {tw // 2, (th // 2) * tw, (th // 2) * tw + tw - 1, (th - 1) * tw + tw // 2}    # an inner tile of each border
        return [int(v) for v in rs.permutation(sorted(pick))], len(pick), len(pick)
    if kind == "cap":
        # list_cap smaller than the device count: only the first list_cap entries are computed
        ent = [int(v) for v in np.random.RandomState(7).permutation(nt)]
        return ent, nt, max(1, nt // 2)
    raise ValueError(kind)


def _tile_mask(shape, entries):
    B = shape[2]
    ho, wo = _out_hw(shape)
    th, tw = ho // 2, wo // 2
    m = torch.zeros(B, 1, ho, wo, dtype=torch.bool)
    for e in entries:
        b, t = divmod(e, th * tw)
        r, c = divmod(t, tw)
        m[b, 0, 2 * r:2 * r + 2, 2 * c:2 * c + 2] = True
    return m


def _run(dev, shape, entries, count, cap, split=True, residual=True):
    cin, cout, B, hin, win = shape
    ho, wo = _out_hw(shape)
    c = _case(shape)
    if "dev" not in c:
        c["dev"] = dict(x=c["x"].to(dev), res=c["res"].to(dev), sc=c["sc"].to(dev), sh=c["sh"].to(dev),
                        pc=ops.pack_conv2d(c["w"].to(dev), stride=2), ws=ops.conv2d_sk_workspace(B, ho, wo, cout, 1, dev))
    d = c["dev"]
    tl = torch.tensor(entries, dtype=torch.int32, device=dev)[:cap].contiguous()
    nl = torch.tensor([count], dtype=torch.int32, device=dev)
    out = torch.full((B, cout, ho, wo), float("nan"), device=dev)
    res = d["res"] if residual else None
    if split:
        ops.conv2d_s2_split_active(d["x"], d["pc"], d["sc"], d["sh"], True, out, tl, nl, residual=res)
    else:
        ops.conv2d_sk_active(d["x"], d["pc"], d["sc"], d["sh"], True, out, d["ws"], tl, nl, residual=res)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_split_conv_over_a_tile_list(dev, shape, kind):
    c = _case(shape)
    entries, count, cap = _entries(shape, kind)
    listed = entries[:min(count, cap)]
    m = _tile_mask(shape, listed).expand_as(c["ref"])
    got = _run(dev, shape, entries, count, cap)
    assert torch.isfinite(got[m]).all(), "a listed pixel is not finite"
    assert torch.isnan(got[~m]).all(), "a pixel outside the listed tiles was written"
    if not listed:
        return
    # two launches: the same bits
    assert torch.equal(got[m], _run(dev, shape, entries, count, cap)[m])
    # a listed tile's bits do not depend on which other tiles are listed, nor on the list order: against the list of every tile
    nt = shape[2] * (_out_hw(shape)[0] // 2) * (_out_hw(shape)[1] // 2)
    assert torch.equal(got[m], _run(dev, shape, list(range(nt)), nt, nt)[m])
    # without the residual the difference is exactly the residual (one f32 addition after the ReLU)
    nores = _run(dev, shape, entries, count, cap, residual=False)
    assert torch.equal(got[m], (nores[m] + c["res"][m]))
    # accuracy against float64, beside the f32 list kernel on the same inputs and list
    f32 = _run(dev, shape, entries, count, cap, split=False)
    ref = c["ref"][m]
    e_split = float((got[m].double() - ref).abs().max())
    e_f32 = float((f32[m].double() - ref).abs().max())
    rmax = float(ref.abs().max())
    print("shape %s list %s: e_split %.3e  e_f32 %.3e  max|ref| %.3e" % (shape, kind, e_split, e_f32, rmax))
    assert e_split <= 2.0 * e_f32, (e_split, e_f32)
    assert e_split <= 2e-5 * rmax, (e_split, rmax)


def test_split_planes_are_built_once_on_the_device(dev):
    w = _case(SHAPES[1])["w"]
    pc = ops.pack_conv2d(w.to(dev), stride=2)
    planes = pc.wsplit_s2()
    assert planes is pc.wsplit_s2() and planes.is_cuda
    assert torch.equal(planes.cpu().view(torch.int16), ops.pack_conv2d_s2_split(w).view(torch.int16))
    assert ops.pack_conv2d(torch.randn(32, 24, 3, 3).to(dev), stride=2).wsplit_s2() is None   # cin % 16


def test_bad_arguments_return_the_error_code(dev):
    """a map that is not the stride-2 image of its input, and a layer without planes: refused, nothing launched or written"""
    cin, cout, B, hin, win = SHAPES[0]
    d = _case(SHAPES[0])
    x, pc = d["x"].to(dev), ops.pack_conv2d(d["w"].to(dev), stride=2)
    tl, nl = torch.zeros(4, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    out = torch.full((B, cout, 4, 4), float("nan"), device=dev)
    epi, lst = ops._epilogue(None, None, True, None), ops._tile_list(tl, nl)
    rc = ops.lib.sessd_conv2d_s2_split_active(x.data_ptr(), B, cin, hin, win, pc.wsplit_s2().data_ptr(), out.data_ptr(), cout, 4, 6,
                                              epi, lst, None)
    assert rc == -1
    rc = ops.lib.sessd_conv2d_s2_split_active(x.data_ptr(), B, 24, hin, win, pc.wsplit_s2().data_ptr(), out.data_ptr(), cout, 4, 4,
                                              epi, lst, None)
    assert rc == -1
    with pytest.raises(ValueError):
        ops.conv2d_s2_split_active(x, ops.pack_conv2d(d["w"].to(dev), stride=1), None, None, True, out, tl, nl)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def _np(v):
    return np.asarray(v.cpu() if torch.is_tensor(v) else v)


def test_engine_runs_b1_0_on_the_split_kernel(dev):
    """A benchmark-model engine with b1.0's configuration (S2_SPLIT_CFG, 0) set by hand against the same engine with (30, 4), every
    layer over its list: h["a"] within 2e-6 of its largest value (the bound tests/test_pipeline_gpu.py holds list engines to against
    full-map engines), the same detections under that test's allclose rule; a captured graph of the split engine replays the
    eager result's bits."""
    from sessd_hip import configs, synth
    from sessd_hip.engine import InferenceEngine, S2_SPLIT_CFG
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0)
    frames = [torch.from_numpy(synth.make_frame(51, 20000)).to(dev)]
    res = []
    for b10 in ((S2_SPLIT_CFG, 0), (30, 4)):
        eng = InferenceEngine(model, VG["range"], VG["voxel_size"], 5, 16000, configs.TEST_CFG, 1, 20480, dev)
        eng.set_points(frames)
        cfg = dict(eng.DEFAULT_ACTIVE_CFG)
        cfg[3] = b10
        eng.force_active_tiles(cfg)
        eng.h["a"].fill_(float("nan"))
        eng.enqueue()
        out = eng.results()
        assert sorted(eng._active_layers()) == sorted(eng.ACTIVE_SLOTS)   # every list layer ran over its list
        assert eng.active_cfg[3] == b10
        # the listed tiles of b1.0's output (the fill launch writes the layer's constant only where a reader can reach)
        m = eng.ta.mask_bool(eng.ACTIVE_MASK[3]).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, None].expand_as(eng.h["a"])
        assert bool(m.any()) and not bool(m.all())
        ha = eng.h["a"].cpu()[m]
        assert torch.isfinite(ha).all()
        res.append((ha, out))
        if b10[0] == S2_SPLIT_CFG:
            eng.capture()
            eng.h["a"].fill_(float("nan"))
            eng.replay()
            again = eng.results()
            assert torch.equal(eng.h["a"].cpu()[m], ha)
            for a, b in zip(out, again):
                for k in ("box3d_lidar", "scores", "label_preds"):
                    assert np.array_equal(_np(a[k]), _np(b[k])), k
    ref = float(res[1][0].abs().max())
    err = float((res[0][0] - res[1][0]).abs().max())
    print("h[a]: split against (30, 4): max abs diff %.3e, max|ref| %.3e" % (err, ref))
    assert err <= 2e-6 * ref, (err, ref)
    for a, b in zip(res[0][1], res[1][1]):
        assert len(a["scores"]) == len(b["scores"])
        assert np.allclose(_np(a["box3d_lidar"]), _np(b["box3d_lidar"]), rtol=1e-4, atol=1e-4)
        assert np.allclose(_np(a["scores"]), _np(b["scores"]), rtol=1e-4)


def test_force_active_tiles_refuses_the_split_configuration_where_it_has_no_planes(dev):
    from sessd_hip import configs
    from sessd_hip.engine import InferenceEngine, S2_SPLIT_CFG
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0)
    eng = InferenceEngine(model, VG["range"], VG["voxel_size"], 5, 16000, configs.TEST_CFG, 1, 20480, dev)
    for l in (6, 0, eng.ACTIVE_PAIR):   # a 1x1 layer, a Winograd layer, the transposed pair
        cfg = dict(eng.DEFAULT_ACTIVE_CFG)
        cfg[l] = (S2_SPLIT_CFG, 0)
        with pytest.raises(ValueError):
            eng.force_active_tiles(cfg)


def test_list_candidates_and_hand_set_configurations(dev):
    """What autotune() tries per list layer, in its order (default environment: all three SESSD_* switches on), and a configuration
    a layer cannot run -- from force_active_tiles, or written into active_cfg by hand -- refused by name: by _list_cfg_error, by
    _list_call, and by enqueue() before it launches anything (the frame's first launch clears the BEV map)."""
    from sessd_hip import configs, synth
    from sessd_hip.engine import InferenceEngine, PAIR_SPLIT_CFG, S2_SPLIT_CFG
    VG = configs.VOXEL_GENERATOR
    model = configs.build_synthetic_detector(dev, seed=0)
    eng = InferenceEngine(model, VG["range"], VG["voxel_size"], 5, 16000, configs.TEST_CFG, 1, 20480, dev)
    wino = [(shape, mr) for shape in (0, 1, 3) for mr in (1, 4, 8, 16, -1, -2)]
    direct, sk = [(3, 0), (4, 0), (11, 0), (12, 0)], [(30, 1), (30, 4), (30, 8), (30, 16)]
    want = {l: wino for l in (0, 1, 2, 4, 5)}
    want[3] = sk + ([(S2_SPLIT_CFG, 0)] if eng.lists[3].layer[0].wsplit_s2() is not None else [])
    want[6] = want[7] = direct + sk
    want[8] = direct + ([(PAIR_SPLIT_CFG, 0)] if all(pc.wsplit() is not None for pc, _, _ in eng.lists[8].layer) else [])
    want[9] = [(shape, mr) for shape in (0, 1, 3) for mr in (4, 8, 16, -1)]
    assert sorted(eng.lists) == list(range(10))
    for l in eng.lists:
        assert list(eng._list_candidates(l)) == want[l], l
        for cfg in want[l]:
            assert eng._list_cfg_error(l, cfg) is None, (l, cfg)
    assert want[3][-1] == (S2_SPLIT_CFG, 0) and want[8][-1] == (PAIR_SPLIT_CFG, 0)   # the benchmark model has both sets of planes
    for l in (6, 0, eng.ACTIVE_PAIR):
        assert "no split weight planes of a 3x3 stride-2 conv" in eng._list_cfg_error(l, (S2_SPLIT_CFG, 0))
        with pytest.raises(ValueError):
            eng._list_call(l, (S2_SPLIT_CFG, 0))
    # a Winograd shape whose packing is missing: a number that is no shape, and b0.1 with a 24-channel weight (cin % 16: no 8-wave
    # packing, the 4-wave one exists)
    assert "no stream-K Winograd packing for shape 7" in eng._list_cfg_error(1, (7, 1))
    _, scale, shift = eng.lists[1].layer
    narrow = ops.pack_conv2d(torch.randn(128, 24, 3, 3).to(dev), 1)
    assert narrow.upk_sk(0) is None and narrow.upk_sk(1) is not None
    # the hand-set configurations: nothing of the frame is launched
    eng.set_points([torch.from_numpy(synth.make_frame(51, 20000)).to(dev)])
    eng.force_active_tiles()
    row = eng.lists[1]
    for l, cfg, repl in ((0, (S2_SPLIT_CFG, 0), None), (eng.ACTIVE_PAIR, (S2_SPLIT_CFG, 0), None), (1, (0, 1), (narrow, scale, shift))):
        good = eng.active_cfg[l]
        eng.active_cfg[l] = cfg
        if repl is not None:
            eng.lists[1] = row._replace(layer=repl)
            assert "no stream-K Winograd packing for shape 0" in eng._list_cfg_error(1, (0, 1)) and eng._list_cfg_error(1, (1, 1)) is None
        eng.bev.fill_(float("nan"))
        with pytest.raises(ValueError):
            eng.enqueue()
        torch.cuda.synchronize()
        assert torch.isnan(eng.bev).all(), l
        eng.active_cfg[l], eng.lists[1] = good, row
    eng.enqueue()
    assert len(eng.results()) == 1 and not torch.isnan(eng.bev).any()
