"""Train-mode PFN layer, the parts that need no GPU: the new entry points' argument checks (before any device call), the ops'
refusal of CPU tensors, the mirror module's predicate on the CPU, and the maths the kernels implement -- the closed form of
tests/pillars_train_ref.py (totals S1, G -> batch statistics; selected slot -> dbeta, dgamma, P -> dW) against torch float64
autograd of the reference formulation (Linear, F.batch_norm(training=True), ReLU, torch.max over the slots), to 1e-10 relative."""
import ctypes

import numpy as np
import pytest
import torch

import pillars_ref as PR
import pillars_train_ref as TR

F32 = lambda v: float(np.float32(v))
VX, VY, XO, YO = F32(0.2), F32(0.2), F32(0.2 / 2 + 0.0), F32(0.2 / 2 - 40.0)
GEOM = (VX, VY, XO, YO)


def test_entry_points_reject_bad_arguments_before_touching_the_device():
    import sessd_hip
    lib = sessd_hip.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)      # non-null, never dereferenced: every call below must fail first
    need = {d: lib.sessd_pillar_train_workspace_bytes(d) for d in (0, 1)}
    assert lib.sessd_pillar_train_totals(0) == 9 + 45 + 1 and lib.sessd_pillar_train_totals(1) == 10 + 55 + 1
    assert lib.sessd_pillar_train_bwd_totals(0) == 64 * 11 and lib.sessd_pillar_train_bwd_totals(1) == 64 * 12
    assert need[1] >= need[0] >= 256 + 8 * 64 * 11

    def stats(C=64, ndim=4, K=9, dist=0, vox=p, num=p, coors=p, tot=p, ws=p, nbytes=None, n=8, T=5):
        return lib.sessd_pillar_train_stats(vox, num, coors, None, n, T, ndim, VX, VY, XO, YO, C, K, dist, tot, ws,
                                            need[dist] if nbytes is None else nbytes, None)

    assert stats(C=32) == -1 and stats(ndim=5) == -1 and stats(K=10) == -1 and stats(K=9, dist=1) == -1
    assert stats(vox=None) == -1 and stats(num=None) == -1 and stats(coors=None) == -1 and stats(tot=None) == -1 and stats(ws=None) == -1
    assert stats(nbytes=need[0] - 1) == -1 and stats(K=10, dist=1, nbytes=need[1] - 1) == -1 and stats(n=0) == -1 and stats(T=0) == -1

    def fin(C=64, K=9, dist=0, ptrs=(p,) * 10):
        tot, w, g, b, rm, rv, mean, inv, sc, sh = ptrs
        return lib.sessd_pillar_train_finalize(tot, w, g, b, 1e-3, 0.01, C, K, dist, rm, rv, mean, inv, sc, sh, None)

    assert fin(C=128) == -1 and fin(K=10) == -1 and fin(K=9, dist=1) == -1
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        assert fin(ptrs=tuple(None if j == i else p for j in range(10))) == -1
    assert fin(ptrs=(p, p, p, p, p, None, p, p, p, p)) == -1 and fin(ptrs=(p, p, p, p, None, p, p, p, p, p)) == -1   # one of the pair

    def sel(C=64, ndim=4, K=9, dist=0, ptrs=(p,) * 10, nbytes=None):
        vox, num, coors, w, sc, sh, feat, grad, tot, ws = ptrs
        return lib.sessd_pillar_train_bwd_select(vox, num, coors, None, 8, 5, ndim, VX, VY, XO, YO, w, sc, sh, C, K, dist, feat, grad, tot,
                                                 ws, need[dist] if nbytes is None else nbytes, None)

    assert sel(C=63) == -1 and sel(ndim=3) == -1 and sel(K=10) == -1 and sel(K=9, dist=1) == -1 and sel(nbytes=255) == -1
    for i in range(10):
        assert sel(ptrs=tuple(None if j == i else p for j in range(10))) == -1

    def bfin(C=64, K=9, dist=0, ptrs=(p,) * 9):
        return lib.sessd_pillar_train_bwd_finalize(*ptrs[:6], 1e-3, C, K, dist, *ptrs[6:], None)

    assert bfin(C=0) == -1 and bfin(K=10) == -1 and bfin(K=9, dist=1) == -1
    for i in range(9):
        assert bfin(ptrs=tuple(None if j == i else p for j in range(9))) == -1

    sb = lambda C=64, gc=p, co=p, gf=p, n=8, b=2, ny=8, nx=12: lib.sessd_pillar_scatter_bwd(gc, co, None, n, C, b, ny, nx, gf, None)
    assert sb(C=32) == -1 and sb(gc=None) == -1 and sb(co=None) == -1 and sb(gf=None) == -1
    assert sb(n=0) == -1 and sb(b=0) == -1 and sb(ny=0) == -1 and sb(nx=0) == -1


def test_ops_refuse_cpu_tensors():
    from sessd_hip import ops
    bn = torch.nn.BatchNorm1d(64, eps=1e-3, momentum=0.01)
    vox, num, coors = torch.zeros(3, 5, 4), torch.ones(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.pillar_features_train(vox, num, coors, torch.zeros(64, 9), bn, VX, VY, XO, YO)
    assert int(bn.num_batches_tracked) == 0          # refused before the batch was counted
    with pytest.raises(ValueError):
        ops.pillar_scatter_train(torch.zeros(3, 64, requires_grad=True), coors, 2, 8, 12)


def test_cpu_modules_keep_the_torch_formulation(golden_dir):
    from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter
    g = PR.load_golden(golden_dir)
    vox, num, coors = (torch.from_numpy(g[k]) for k in ("voxels", "num_points", "coors"))
    assert PillarFeatureNet.fused_train is True
    nets = []
    for _ in range(2):
        net = PillarFeatureNet(num_filters=[64], norm_cfg=None)
        net.load_state_dict(g["plain"]["sd"])
        nets.append(net.train())
    assert not nets[0].on_device_train_path(vox) and not nets[0].on_device_path(vox)
    a = nets[0](vox, num, coors)
    b = nets[1]._forward_torch(vox, num, coors)
    assert a.grad_fn is not None and torch.equal(a, b)
    for k, v in nets[0].state_dict().items():          # the running statistics moved the same way
        assert torch.equal(v, nets[1].state_dict()[k]), k
    scat = PointPillarsScatter(num_input_features=64).train()
    canvas = scat(a, coors, 2, [12, 8, 1])
    assert canvas.grad_fn is not None and torch.equal(canvas.detach(), PR.scatter(a.detach(), g["coors"], 2, 8, 12))


CASES = [(5, 3, False), (5, 3, True), (2, 1, True), (1, 3, False), (65, 40, True), (100, 257, False)]


@pytest.mark.parametrize("T,N,with_distance", CASES)
@pytest.mark.parametrize("ranks", [1, 2])
def test_closed_form_equals_float64_autograd(T, N, with_distance, ranks):
    """ranks = 2: two identical ranks under SyncBN are one batch that holds every pillar twice -- the same statistics and output,
    and the whole batch's dW, dgamma, dbeta are twice one rank's local ones."""
    case = TR.make_train_case(1000 * T + N, N, T, with_distance)
    vox, num, coors = TR.live_args(case)
    rng = np.random.RandomState(N + T)
    g = rng.randn(N, 64)
    par = (case["w"], case["gamma"], case["beta"])
    cf = TR.closed_form(vox, num, coors, *par, *GEOM, with_distance, torch.float64, g=g, ranks=ranks)
    rep = lambda a: np.concatenate([a] * ranks, 0)
    ag = TR.formulation(rep(vox), rep(num), rep(coors), *par, *GEOM, with_distance, torch.float64, g=rep(g))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(torch.cat([cf["out"]] * ranks, 0), ag["out"]) <= 1e-10
    for k in ("dW", "dgamma", "dbeta"):
        e = rel(ranks * cf[k], ag[k])
        print("T %d N %d dist %d ranks %d %s: %.2e" % (T, N, with_distance, ranks, k, e))
        assert e <= 1e-10, k
    # the statistics, against torch's own BatchNorm1d in float64
    bn = torch.nn.BatchNorm1d(64, eps=TR.EPS, momentum=0.01).double().train()
    bn(cf["z"].reshape(N * T, 64))
    rm, rv = TR.running_stats(dict(cf, M=N * T), torch.zeros(64), torch.ones(64), 0.01)
    if ranks == 1:
        assert rel(rm, bn.running_mean) <= 1e-10 and rel(rv, bn.running_var) <= 1e-10
    assert bool(torch.isfinite(cf["out"]).all())       # the NaN padding slots were masked, not read
