"""One PFN layer in TRAIN mode on the device (csrc/pillar.hip: statistics, finalise, the eval kernel, backward select, backward
finalise, scatter backward; ops.pillar_features_train / pillar_scatter_train; the mirror modules) against the float64 closed
form of tests/pillars_train_ref.py, which tests/test_pillar_train_cpu.py holds to float64 autograd.

Inputs are tests/test_pillar_features_gpu.py::make_case's: NaN padding slots, NaN rows beyond N with an absurd point count and
cells far outside the canvas; every case is run with N as a host count (N rows) and through num_voxels_dev (N + 5 rows).

Forward bound: pillars_train_ref.forward_bound (derived there; never above (T + 32) u B per element).
Running statistics: 4 u max(|old|, |new|) per element against nn.BatchNorm1d in float64.
Gradients: e(t) = max|t - t64| / max|t64| for t in dW, dgamma, dbeta must stay within max(4 e_torch32, 64 u), e_torch32 being the
same figure for PillarFeatureNet._forward_torch in float32 on the CPU with the same upstream gradient. The upstream gradient is
zeroed on the (pillar, channel) pairs where float64 itself sees a near tie (pillars_train_ref.ill_posed_pairs); at most 2 % of
the pairs (2 of 64 for N = 1) may be, or the case is ill-posed and fails. Every case takes milliseconds."""
import functools

import numpy as np
import pytest
import torch

import pillars_ref as PR
import pillars_train_ref as TR
from sessd_hip import lib, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C = 64
BATCH, NX = 2, 12
SENT = -12345.0
GUARD = 64
F32 = lambda v: float(np.float32(v))
VX, VY, XO, YO = F32(0.2), F32(0.2), F32(0.2 / 2 + 0.0), F32(0.2 / 2 - 40.0)
GEOM = (VX, VY, XO, YO)
MOM = 0.01

SHAPES = [(T, N) for T in (2, 5, 64, 65, 100) for N in (1, 3, 257)] + [(1, 3), (1, 257)]


@functools.lru_cache(maxsize=None)
def prepared(T, N, with_distance):
    """The case, its float64 closed form, the forward bound and the near-tie mask: computed once, shared, never modified."""
    case = TR.make_train_case(1000 * T + N, N, T, with_distance)
    cf = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, with_distance)
    bound, cap = TR.forward_bound(case, cf)
    assert bool((bound <= cap).all())
    excl = TR.ill_posed_pairs(case, cf, bound)
    return case, cf, bound, excl


def upstream(case, excl, seed):
    """Random upstream gradient (N, C), zero on the near-tie pairs -- which must be few."""
    N = case["N"]
    n_excl = int(excl.sum())
    assert n_excl <= 2 if N == 1 else n_excl <= 0.02 * excl.numel(), "ill-posed case: %d of %d pairs near a tie" % (n_excl, excl.numel())
    g = np.random.RandomState(seed).randn(N, C)
    g[excl.numpy()] = 0.0
    return g.astype(np.float32)


def make_bn(case, dev):
    bn = torch.nn.BatchNorm1d(C, eps=TR.EPS, momentum=MOM).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(case["gamma"]))
        bn.bias.copy_(torch.from_numpy(case["beta"]))
        bn.running_mean.copy_(torch.from_numpy(case["running_mean"]))
        bn.running_var.copy_(torch.from_numpy(case["running_var"]))
    return bn


def run_device(case, dev, g=None, dev_count=True):
    """ops.pillar_features_train (+ backward with upstream gradient g (N, C)). dev_count: N + extra rows and the count on the
    device (the rows beyond N of g are NaN: they must not be read); else exactly N rows and the host count."""
    N = case["N"]
    rows = case["cap"] if dev_count else N
    vox, num, coors = (torch.from_numpy(case[k][:rows]).to(dev).contiguous() for k in ("voxels", "num", "coors"))
    n_dev = torch.tensor([N], dtype=torch.int32, device=dev) if dev_count else None
    w = torch.from_numpy(case["w"]).to(dev).requires_grad_(True)
    bn = make_bn(case, dev)
    out = ops.pillar_features_train(vox, num, coors, w, bn, *GEOM, with_distance=case["dist"], num_voxels_dev=n_dev)
    r = dict(out=out.detach().cpu(), rm=bn.running_mean.cpu(), rv=bn.running_var.cpu(), nbt=int(bn.num_batches_tracked))
    if g is not None:
        gg = torch.full((rows, C), float("nan"), dtype=torch.float32)
        gg[:N] = torch.from_numpy(g)
        out.backward(gg.to(dev))
        r.update(dW=w.grad.cpu(), dgamma=bn.weight.grad.cpu(), dbeta=bn.bias.grad.cpu())
    return r


def torch32(case, g, copies=1):
    """The yardstick: PillarFeatureNet._forward_torch in float32 on the CPU, train mode, the same upstream gradient (padding slots
    zeroed: that formulation multiplies them by 0). copies = R: the batch of R identical ranks, its gradients divided by R."""
    from det3d.models.readers.pillar_encoder import PillarFeatureNet
    net = PillarFeatureNet(num_filters=[C], with_distance=case["dist"], norm_cfg=None).train()
    pfn = net.pfn_layers[0]
    with torch.no_grad():
        pfn.linear.weight.copy_(torch.from_numpy(case["w"]))
        pfn.norm.weight.copy_(torch.from_numpy(case["gamma"]))
        pfn.norm.bias.copy_(torch.from_numpy(case["beta"]))
    assert (F32(net.vx), F32(net.vy), F32(net.x_offset), F32(net.y_offset)) == GEOM
    vox, num, coors = (torch.from_numpy(np.concatenate([a] * copies, 0)) for a in TR.live_args(case))
    out = net._forward_torch(torch.nan_to_num(vox, nan=0.0), num, coors)
    out.backward(torch.from_numpy(np.concatenate([g] * copies, 0)))
    return dict(dW=pfn.linear.weight.grad / copies, dgamma=pfn.norm.weight.grad / copies, dbeta=pfn.norm.bias.grad / copies)


def check_gradients(tag, got, ref64, ref32):
    worst = 0.0
    for k in ("dW", "dgamma", "dbeta"):
        t64 = ref64[k]
        den = float(t64.abs().max())
        assert den > 0, k
        e_dev = float((got[k].double() - t64).abs().max()) / den
        e_t32 = float((ref32[k].double() - t64).abs().max()) / den
        allowed = max(4 * e_t32, 64 * U)
        print("%s %s: e_device %.2e  e_torch32 %.2e  e_device / allowed %.3f" % (tag, k, e_dev, e_t32, e_dev / allowed))
        assert e_dev <= allowed, (tag, k, e_dev, e_t32)
        worst = max(worst, e_dev / allowed)
    return worst


@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("T,N", SHAPES)
def test_forward_and_running_statistics_against_float64(dev, T, N, with_distance):
    case, cf, bound, _ = prepared(T, N, with_distance)
    bn64 = torch.nn.BatchNorm1d(C, eps=TR.EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn64.running_mean.copy_(torch.from_numpy(case["running_mean"]))
        bn64.running_var.copy_(torch.from_numpy(case["running_var"]))
    bn64(cf["z"].reshape(N * T, C))
    for dev_count in (False, True):
        r = run_device(case, dev, dev_count=dev_count)
        got = r["out"]
        assert got.shape == ((case["cap"] if dev_count else N), C)
        assert bool((got[N:] == 0).all())                          # rows beyond the live count: zeros
        assert bool(torch.isfinite(got).all())                     # the NaN padding slots and rows were not read
        ratio = float(((got[:N].double() - cf["out"]).abs() / bound).max())
        print("T %d N %d dist %d dev_count %d: max error / bound = %.3f" % (T, N, with_distance, dev_count, ratio))
        assert ratio <= 1.0
        assert r["nbt"] == 1
        for name, new, old in (("running_mean", bn64.running_mean, case["running_mean"]), ("running_var", bn64.running_var, case["running_var"])):
            tol = 4 * U * torch.maximum(torch.from_numpy(old).double().abs(), new.abs())
            err = (r["rm" if name == "running_mean" else "rv"].double() - new).abs()
            print("   %s: max error / tolerance = %.3f" % (name, float((err / tol).max())))
            assert bool((err <= tol).all()), name


@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("T,N", SHAPES)
def test_gradients_against_float64(dev, T, N, with_distance):
    case, _, _, excl = prepared(T, N, with_distance)
    g = upstream(case, excl, 31 * T + N)
    ref64 = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, with_distance, g=g)
    ref32 = torch32(case, g)
    for dev_count in (False, True):
        got = run_device(case, dev, g=g, dev_count=dev_count)
        check_gradients("T %d N %d dist %d dev_count %d" % (T, N, with_distance, dev_count), got, ref64, ref32)


def test_selection_duplicated_points(dev):
    """Pillars whose two live points are identical: whichever of the two is selected, the gradient is the same."""
    case = TR.make_train_case(4242, 12, 5, True)
    twice = [i for i in range(12) if case["num"][i] >= 2]
    assert len(twice) >= 4
    for i in twice:
        case["num"][i] = 2
        case["voxels"][i, 1] = case["voxels"][i, 0]
        case["voxels"][i, 2:] = np.nan
    cf = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, True)
    bound, _ = TR.forward_bound(case, cf)
    y = cf["y"]
    assert bool((y[twice, 0] == y[twice, 1]).all())
    # near ties other than the duplicate itself: the pair's (one) value against the padding candidate, and the better one against 0
    best = torch.maximum(y[:, 0], cf["shift"][None])
    excl = ((y[:, 0] - cf["shift"][None]).abs() < 2 * bound) | (best.abs() < 2 * bound)
    only = torch.zeros(12, dtype=torch.bool)
    only[twice] = True
    g = np.random.RandomState(5).randn(12, C).astype(np.float32)
    g[(excl | ~only[:, None]).numpy()] = 0.0                          # the gradient enters through the duplicated pillars alone
    assert int((g != 0).sum()) >= 0.9 * len(twice) * C
    ref64 = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, True, g=g)
    live_sel = (ref64["sel"][twice] < 2) & (ref64["dy"][twice] != 0)
    assert int(live_sel.sum()) > 50                                    # the duplicated slots are selected
    check_gradients("duplicated points", run_device(case, dev, g=g), ref64, torch32(case, g))


def test_selection_padding_candidate_and_clamped_channels(dev):
    """Built like test_padding_rule: every live slot's Linear output is slightly negative (z = 1e-2 * fcx <= -1e-3), gamma = 1. In
    the even channels beta = +5: in a pillar with num_points < T the padding candidate (z = 0, value = shift) wins -- those pairs
    feed dbeta and dgamma (xhat = -mean * invstd) but not P, so with the gradient entering through them alone
    dW = -scale (dbeta / M S1 + dgamma / M invstd (G w - mean S1)). In the odd channels beta = -5: everything is clamped to 0 and
    every gradient of those channels is exactly 0."""
    T, N = 5, 12
    case = TR.make_train_case(77, N, T, False, small=True)
    even = torch.arange(C) % 2 == 0
    case["gamma"][:] = 1.0
    case["beta"][:] = np.where(np.arange(C) % 2 == 0, 5.0, -5.0)
    part = torch.from_numpy(case["num"][:N] < T)
    assert int(part.sum()) >= 4 and int((~part).sum()) >= 2
    cf = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, False)
    bound, _ = TR.forward_bound(case, cf)
    num = torch.from_numpy(case["num"][:N].astype(np.int64))
    # the conditions that make the case meaningful, on the float64 reference first
    assert bool((cf["z"][cf["live"]] < -5e-4).all())
    assert bool((cf["out"][part][:, even] == cf["shift"][even][None]).all()) and bool((cf["out"][:, ~even] == 0).all())
    assert bool((cf["y"][:, :, ~even] < -1).all())
    ill = TR.ill_posed_pairs(case, cf, bound)
    assert not bool(ill[part][:, even].any())          # the pairs this test is about are well separated
    ill = ill & even[None]                             # (a clamped channel's gradient is 0 whichever slot is selected)
    r = run_device(case, dev)
    assert bool((r["out"][:, ~even] == 0).all())
    for only_padding in (True, False):
        g = np.random.RandomState(9).randn(N, C).astype(np.float32)
        g[ill.numpy()] = 0.0                           # full pillars whose two best live slots lie within the bound
        if only_padding:
            g[~part.numpy()] = 0.0
        ref64 = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, False, g=g)
        assert bool((ref64["sel"][part][:, even] >= num[part][:, None]).all())          # a padding slot is selected
        if only_padding:
            assert float(ref64["P"].abs().max()) == 0.0 and float(ref64["dW"][even].abs().max()) > 0
        got = run_device(case, dev, g=g)
        check_gradients("padding rule (only padding pairs %d)" % only_padding, got, ref64, torch32(case, g))
        for k in ("dW", "dgamma", "dbeta"):
            assert float(got[k][~even].abs().max()) == 0.0, k                          # clamped channels: exactly zero
        want = torch.from_numpy(g).double()[:, even].sum(0)
        assert float((got["dbeta"][even].double() - want).abs().max()) <= 4 * U * float(want.abs().max())


def test_two_calls_give_the_same_bits(dev):
    case, _, _, excl = prepared(65, 257, True)
    g = upstream(case, excl, 3)
    a, b = run_device(case, dev, g=g), run_device(case, dev, g=g)
    for k in ("out", "rm", "rv", "dW", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k


def test_scatter_backward(dev):
    """grad_feat[p] = grad_canvas[b, :, y, x] bit for bit; a pillar outside the canvas gets a zero row (and reads nothing), rows
    beyond N are zero, the guard bands around the gradient buffer stay untouched."""
    case = TR.make_train_case(91, 9, 5, False)
    N, cap, ny = case["N"], case["cap"], case["ny"]
    gc = torch.from_numpy(np.random.RandomState(1).randn(BATCH, C, ny, NX).astype(np.float32))
    for bad_cell in ([BATCH - 1, 0, ny - 1, NX], [-1, 0, 0, 0], [BATCH, 0, 0, 0], [0, 0, -1, 3], [0, 0, ny, 0], [0, 0, 2, -1]):
        coors = case["coors"].copy()
        coors[4] = bad_cell
        want = torch.zeros(cap, C)
        for i in range(N):
            if i != 4:
                want[i] = gc[coors[i, 0], :, coors[i, 2], coors[i, 3]]
        co = torch.from_numpy(coors).to(dev)
        n_dev = torch.tensor([N], dtype=torch.int32, device=dev)
        buf = torch.full((cap * C + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
        view = buf[GUARD:GUARD + cap * C].view(cap, C)
        gcd = gc.to(dev)
        rc = lib.sessd_pillar_scatter_bwd(gcd.data_ptr(), co.data_ptr(), n_dev.data_ptr(), cap, C, BATCH, ny, NX, view.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + cap * C:] == SENT).all())
        assert torch.equal(view.cpu(), want)
        # through autograd, host count (N rows) and device count (all rows)
        for rows, nd in ((N, None), (cap, n_dev)):
            feat = torch.randn(rows, C, device=dev, requires_grad=True)
            canvas = ops.pillar_scatter_train(feat, co[:rows].contiguous(), BATCH, ny, NX, num_voxels_dev=nd)
            assert torch.equal(canvas, ops.pillar_scatter(feat.detach(), co[:rows].contiguous(), BATCH, ny, NX, num_voxels_dev=nd))
            canvas.backward(gcd)
            assert torch.equal(feat.grad.cpu(), want[:rows])


def test_sync_bn_two_identical_ranks_and_one_rank(dev):
    """reduce_fn doubles the totals: the float64 reference of two identical ranks (M, S1, G, dbeta, dgamma of the formula doubled;
    P and the bracket's S1, G this rank's own; dgamma / dbeta returned local). A reduce_fn that changes nothing: the plain form's
    bits."""
    T, N, dist = 5, 257, True
    case, cf1, _, excl = prepared(T, N, dist)
    g = upstream(case, excl, 17)
    plain = run_device(case, dev, g=g)
    state = ops.sync_bn_state()
    try:
        ops.set_sync_bn(True, reduce_fn=lambda t: None)
        same = run_device(case, dev, g=g)
        calls = []
        ops.set_sync_bn(True, reduce_fn=lambda t: (calls.append(t.numel()), t.mul_(2))[1])
        two = run_device(case, dev, g=g)
    finally:
        ops.restore_sync_bn(state)
    for k in plain:
        assert torch.equal(plain[k], same[k]) if torch.is_tensor(plain[k]) else plain[k] == same[k], k
    assert calls == [10 + 55 + 1, 2 * C]                              # one all-reduce in each direction
    cf2 = TR.closed_form(*TR.live_args(case), case["w"], case["gamma"], case["beta"], *GEOM, dist, g=g, ranks=2)
    bound2 = prepared(T, N, dist)[2]                                  # the same statistics, so the same bound
    # the statistics of the doubled batch are those of one copy but for M / (M - 1) in running_var
    assert float((cf2["mean"] - cf1["mean"]).abs().max()) <= 1e-12 * float(cf1["mean"].abs().max())
    ratio = float(((two["out"][:N].double() - cf2["out"]).abs() / bound2).max())
    print("two ranks: forward max error / bound = %.3f" % ratio)
    assert ratio <= 1.0
    rm, rv = TR.running_stats(cf2, torch.from_numpy(case["running_mean"]), torch.from_numpy(case["running_var"]), MOM)
    for got, new, old in ((two["rm"], rm, case["running_mean"]), (two["rv"], rv, case["running_var"])):
        tol = 4 * U * torch.maximum(torch.from_numpy(old).double().abs(), new.abs())
        assert bool(((got.double() - new).abs() <= tol).all())
    assert not torch.equal(two["rv"], plain["rv"])                    # M doubled: another unbiased variance
    check_gradients("two ranks", two, cf2, torch32(case, g, copies=2))


def _golden_net(golden_dir, dev, tag="plain"):
    from det3d.models.readers.pillar_encoder import PillarFeatureNet
    g = PR.load_golden(golden_dir)
    net = PillarFeatureNet(num_filters=[64], with_distance=tag == "dist", norm_cfg=None)
    net.load_state_dict(g[tag]["sd"])
    return g, net.to(dev)


def test_mirror_modules_train_on_the_device(dev, golden_dir):
    from det3d.models.readers.pillar_encoder import PointPillarsScatter
    for tag in ("plain", "dist"):
        g, net = _golden_net(golden_dir, dev, tag)
        sd = g[tag]["sd"]
        pfn = net.pfn_layers[0]
        vox, num, coors = (torch.from_numpy(g[k]).to(dev) for k in ("voxels", "num_points", "coors"))
        N, T = vox.shape[:2]
        case = dict(N=N, T=T, dist=tag == "dist", voxels=g["voxels"], num=g["num_points"], coors=g["coors"],
                    w=sd["pfn_layers.0.linear.weight"].numpy(), gamma=sd["pfn_layers.0.norm.weight"].numpy(),
                    beta=sd["pfn_layers.0.norm.bias"].numpy())
        par = (case["w"], case["gamma"], case["beta"])
        cf = TR.closed_form(*TR.live_args(case), *par, *GEOM, case["dist"])
        bound, _ = TR.forward_bound(case, cf)
        excl = TR.ill_posed_pairs(case, cf, bound)
        upstream(case, excl, 0)                                      # (the cap on near ties)
        gfeat = (~excl).numpy().astype(np.float32)                   # d(sum) / d(feature): 1, and 0 on the near ties
        ref64 = TR.closed_form(*TR.live_args(case), *par, *GEOM, case["dist"], g=gfeat)
        scat = PointPillarsScatter(num_input_features=64).to(dev)
        net.train(), scat.train()
        assert net.on_device_train_path(vox) and not net.on_device_path(vox)
        rm0 = pfn.norm.running_mean.clone()
        feat = net(vox, num, coors)
        assert type(feat.grad_fn).__name__.startswith("PillarFeaturesTrainFunction")
        out = scat(feat, coors, 2, [12, 8, 1])
        assert type(out.grad_fn).__name__.startswith("PillarScatterTrainFunction")
        assert not torch.equal(pfn.norm.running_mean, rm0) and int(pfn.norm.num_batches_tracked) == 1
        want = PR.scatter(cf["out"], g["coors"], 2, 8, 12)
        ratio = float(((out.detach().cpu().double() - want).abs() / PR.scatter(bound, g["coors"], 2, 8, 12).clamp_min(1e-300)).max())
        print("modules (%s): canvas max error / bound = %.3f" % (tag, ratio))
        assert ratio <= 1.0
        weight = PR.scatter(torch.from_numpy(gfeat), g["coors"], 2, 8, 12).to(dev)
        (out * weight).sum().backward()                              # = out.sum().backward() when no pair is near a tie
        got = dict(dW=pfn.linear.weight.grad.cpu(), dgamma=pfn.norm.weight.grad.cpu(), dbeta=pfn.norm.bias.grad.cpu())
        check_gradients("modules (%s)" % tag, got, ref64, torch32(case, gfeat))
        # fused_train = False: the torch formulation, as before
        _, net2 = _golden_net(golden_dir, dev, tag)
        net2.train()
        net2.fused_train = False
        assert not net2.on_device_train_path(vox)
        feat2 = net2(vox, num, coors)
        assert not type(feat2.grad_fn).__name__.startswith("PillarFeaturesTrainFunction")
        assert float((feat2.detach() - feat.detach()).abs().max()) <= 1e-4 * float(feat.detach().abs().max())
        # no_grad in train mode: the running statistics still move
        rm1 = pfn.norm.running_mean.clone()
        with torch.no_grad():
            f3 = net(vox, num, coors)
        assert not f3.requires_grad and not torch.equal(pfn.norm.running_mean, rm1) and int(pfn.norm.num_batches_tracked) == 2


def test_no_state_left_behind(dev, golden_dir):
    """After a train step the eval-mode output is the eval kernel's with the updated running statistics, bit for bit."""
    from sessd_hip.engine import fold_bn
    g, net = _golden_net(golden_dir, dev)
    vox, num, coors = (torch.from_numpy(g[k]).to(dev) for k in ("voxels", "num_points", "coors"))
    net.train()
    net(vox, num, coors).sum().backward()
    net.eval()
    pfn = net.pfn_layers[0]
    assert net.on_device_path(vox) and not net.on_device_train_path(vox)
    with torch.no_grad():
        got = net(vox, num, coors)
    scale, shift = fold_bn(pfn.norm)
    want = ops.pillar_features(vox, num.int(), coors.int(), pfn.linear.weight.detach().contiguous(), scale, shift, *GEOM)
    assert torch.equal(got, want)
    ref = PR.reader_forward(g["voxels"], g["num_points"], g["coors"], {"reader." + k: v.detach().cpu() for k, v in net.state_dict().items()})
    assert float((got.cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
