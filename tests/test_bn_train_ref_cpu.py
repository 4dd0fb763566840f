"""The bounds of tests/bn_train_ref.py can be met by a correct float32 implementation and are not vacuous (no GPU).
  - A float32 restatement (numpy) of the kernels' arithmetic order -- float64 block partials in the blocks' order, the finisher in
    float64 cast once, every float32 operation of the apply kernels rounded on its own, the SSFA fma chains over channel quarters --
    meets every bound, on every case tests/test_bn_train_f64_gpu.py runs (worst error / bound <= 1).
  - Named single defects leave them by a clear factor: the variance formed in float32, running_var without n / (n - 1), one row
    block's / plane slice's / dot block's partial dropped, dgamma / N with the rank-local N in the two-rank form, the two attention
    weights exchanged.
  - The ambiguity condition of the backward (the share of |z64| <= E_z is at most 1 %) holds for every input family and case.
  - The restated block rules give the branch properties the GPU cases name.
Every ratio is printed (pytest -s). Measured here, worst error / bound. Restatement: sparse table y 0.864, dx 0.854, dgamma 0.747 (the
outputs that are one cast of a float64 value -- mean, invstd, running statistics, dbeta -- reach 0.94 .. 0.996, as a single rounding
may); dense map y 0.828, dx 0.664; two ranks y 0.793, dx 0.577; SSFA stage A 0.666 (smap) and 0.445 (dzmap), stage B 0.708 (stats), 0.510
(out), 0.498 (dx). The largest ambiguous share is 4.2e-5 (offset family, n = 3001). Defects: float32 variance at |mean| >> std invstd
4.8e4 .. 9.0e5, y 1.8e3 .. 3.5e3, dx 3.1e4 .. 1.6e5; running_var without n / (n - 1) 179 (n = 3001) .. 1.6e5 (n = 2); a dropped partial
3.7e3 .. 1.2e7 (sparse blocks 127 / 64 / 125 of n = 128 / 129 / 3001, dense slice 15), the last dot block's 1.1e5 (stats); the rank-local N
2.9e6 .. 3.5e6 (dx); the attention weights exchanged 1.1e8 (out)."""
import numpy as np
import pytest
import torch

import bn_train_ref as R

F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _sums64(cols, spans, drop):
    """float64 partial sums of each span, added in span order; drop: the index of a live span whose partial is left out"""
    tot = [np.zeros(c.shape[1:], np.float64) for c in cols]
    for i, (a, b) in enumerate(spans):
        if b > a and i != drop:
            for k, c in enumerate(cols):
                tot[k] = tot[k] + c[a:b].astype(np.float64).sum(0)
    return tot


def _finish(t0, t1, n, rm, rv, defect):
    """the finisher / bn_sync_finalize_kernel: -> mean_f, invstd_f, running_mean, running_var"""
    eps, mom = np.float64(F(R.EPS)), np.float64(F(R.MOMENTUM))
    m = t0 / n if n > 0 else np.zeros_like(t0)
    var = t1 / n - m * m if n > 0 else np.zeros_like(t0)
    if defect == "var32":
        var = (F(t1 / n) - F(m) * F(m)).astype(np.float64)
    var = np.maximum(var, 0.0)
    mean_f, is_f = F(m), F(1.0 / np.sqrt(var + eps))
    if n > 0:
        unbiased = var * n / (n - 1) if (n > 1 and defect != "no_bessel") else var
        rm, rv = F((1.0 - mom) * rm + mom * m), F((1.0 - mom) * rv + mom * unbiased)
    return mean_f, is_f, rm, rv


def _apply_fwd(x, mean_f, is_f, g, b, relu):
    z = (x - mean_f) * is_f * g + b          # float32 arrays: four roundings
    return np.maximum(z, F(0)) if relu else z


def _bwd_sums(x, dy, y, mean_f, is_f, relu, spans, drop):
    dz = np.where(y > 0, dy, F(0)) if relu else dy
    xhat = (x - mean_f) * is_f
    t0, t1 = _sums64([dz, dz.astype(np.float64) * xhat.astype(np.float64)], spans, drop)
    return dz, xhat, t0, t1


def _apply_bwd(dz, xhat, g, is_f, dbeta_f, dgamma_f, inv_n):
    return g * is_f * (dz - dbeta_f * inv_n - xhat * dgamma_f * inv_n)


def bn32(x, g, b, dy, relu, rm0, rv0, spans, defect=None, drop=None):
    """one rank, the fused form: the outputs tests hand to R.check_bn"""
    x, g, b, dy = (np.asarray(t, F) for t in (x, g, b, dy))
    n = x.shape[0]
    t0, t1 = _sums64([x, x.astype(np.float64) ** 2], spans, drop if defect == "drop_fwd" else None)
    mean_f, is_f, rm, rv = _finish(t0, t1, n, np.asarray(rm0, F), np.asarray(rv0, F), defect)
    y = _apply_fwd(x, mean_f, is_f, g, b, relu)
    dz, xhat, s0, s1 = _bwd_sums(x, dy, y, mean_f, is_f, relu, spans, drop if defect == "drop_bwd" else None)
    dbeta_f, dgamma_f = F(s0), F(s1)
    dx = _apply_bwd(dz, xhat, g, is_f, dbeta_f, dgamma_f, F(1) / F(max(n, 1)))
    return {k: _t(v) for k, v in dict(y=y, mean=mean_f, invstd=is_f, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma_f,
                                      dbeta=dbeta_f).items()}


def bn32_sync(xs, g, b, dys, relu, rm0, rv0, defect=None):
    """the split form on the parts of a batch: statistics per rank, the float64 totals added, finalise + apply per rank"""
    xs, dys = [np.asarray(t, F) for t in xs], [np.asarray(t, F) for t in dys]
    g, b = np.asarray(g, F), np.asarray(b, F)
    fw = [_sums64([x, x.astype(np.float64) ** 2], R.sparse_blocks(x.shape[0])[1], None) for x in xs]
    N = sum(x.shape[0] for x in xs)
    t0, t1 = sum(f[0] for f in fw), sum(f[1] for f in fw)
    outs, bw = [], []
    for x, dy in zip(xs, dys):
        mean_f, is_f, rm, rv = _finish(t0, t1, N, np.asarray(rm0, F), np.asarray(rv0, F), None)
        y = _apply_fwd(x, mean_f, is_f, g, b, relu)
        dz, xhat, s0, s1 = _bwd_sums(x, dy, y, mean_f, is_f, relu, R.sparse_blocks(x.shape[0])[1], None)
        outs.append(dict(y=y, mean=mean_f, invstd=is_f, running_mean=rm, running_var=rv, dgamma=F(s1), dbeta=F(s0)))
        bw.append((dz, xhat, s0, s1, is_f))
    S0, S1 = sum(w[2] for w in bw), sum(w[3] for w in bw)
    for x, o, (dz, xhat, _, _, is_f) in zip(xs, outs, bw):
        n_used = max(x.shape[0], 1) if defect == "local_n" else N
        o["dx"] = _apply_bwd(dz, xhat, g, is_f, F(S0), F(S1), F(1.0 / n_used))
    return [{k: _t(v) for k, v in o.items()} for o in outs]


def bn32_dense(x4, g, b, dy4, relu, rm0, rv0, defect=None, drop=None):
    """the dense map: the same arithmetic with the rows regrouped slice by slice (the order of the float64 partials)"""
    B, C, H, W = x4.shape
    plane = H * W
    _, sl = R.plane_slices(plane)
    order, spans, at = [], [], 0
    for q0, q1 in sl:
        idx = [bi * plane + p for bi in range(B) for p in range(4 * q0, 4 * q1)]
        order += idx
        spans.append((at, at + len(idx)))
        at += len(idx)
    order = np.asarray(order, np.int64)
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    xr, dyr = R.rows(x4).numpy()[order], R.rows(dy4).numpy()[order]
    got = bn32(xr, g, b, dyr, relu, rm0, rv0, spans, defect, drop)
    for k in ("y", "dx"):
        got[k] = got[k][_t(inv)]
    return got


def _worst(r):
    return max(r.values())


# ---- BatchNorm: the restatement meets the bounds -------------------------------------------------------------------------------------

@pytest.mark.parametrize("relu", [True, False])
def test_sparse_restatement_meets_every_bound(relu):
    worst = {}
    for C, n, cap, fam in R.SPARSE_CASES:
        x, g, b, dy = R.family_rows(fam, n, C, 1)
        rm0, rv0 = R.running_init(C)
        got = bn32(x, g, b, dy, relu, rm0, rv0, R.sparse_blocks(n)[1])
        r, st = R.check_bn(x, g, b, dy, relu, rm0, rv0, got)
        amb = R.ambiguity(st)
        print("sparse C %d n %d %s relu %d: %s ambiguous %.2g" % (C, n, fam, relu, {k: round(v, 3) for k, v in r.items()}, amb))
        assert _worst(r) <= 1.0 and amb <= 0.01
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if n == 0:
            assert torch.equal(got["running_mean"], rm0) and torch.equal(got["running_var"], rv0)
            assert float(got["dgamma"].abs().max()) == 0 and float(got["dbeta"].abs().max()) == 0
        if n == 1:
            assert torch.equal(got["y"], (b.clamp_min(0) if relu else b).view(1, -1))
    print("sparse restatement, worst per output:", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("shape,fam", R.DENSE_CASES)
def test_dense_restatement_meets_every_bound(shape, fam):
    x, g, b, dy = R.dense_inputs(shape, fam)
    rm0, rv0 = R.running_init(shape[1])
    for relu in (True, False):
        got = bn32_dense(x, g, b, dy, relu, rm0, rv0)
        r, st = R.check_bn(R.rows(x), g, b, R.rows(dy), relu, rm0, rv0, got)
        print("dense %s %s relu %d: %s ambiguous %.2g" % (shape, fam, relu, {k: round(v, 3) for k, v in r.items()}, R.ambiguity(st)))
        assert _worst(r) <= 1.0


@pytest.mark.parametrize("shape", R.DENSE_FALLBACK + [R.DENSE_REUSE])
def test_the_fallback_and_reuse_shapes_meet_the_ambiguity_condition(shape):
    """the fallback shapes with the float32 accumulation of torch's own BatchNorm in the bound (acc=R.U)"""
    x, g, b, dy = R.dense_inputs(shape, "ordinary")
    acc = R.U64 if shape == R.DENSE_REUSE else R.U
    assert R.ambiguity(R.bn_forward_reference(R.rows(x), g, b, True, acc=acc)) <= 0.01


def _sync_sparse_parts(C, n0, n1):
    x, g, b, dy = R.family_rows("ordinary", n0 + n1, C, 2)
    return [x[:n0], x[n0:]], g, b, [dy[:n0], dy[n0:]]


@pytest.mark.parametrize("C,n0,n1", R.SYNC_SPARSE)
def test_two_rank_restatement_meets_every_bound_and_the_local_n_leaves_it(C, n0, n1):
    xs, g, b, dys = _sync_sparse_parts(C, n0, n1)
    rm0, rv0 = R.running_init(C)
    r = R.check_bn_sync(xs, g, b, dys, True, rm0, rv0, bn32_sync(xs, g, b, dys, True, rm0, rv0))
    print("two ranks C %d, %d + %d rows: %s" % (C, n0, n1, {k: round(v, 3) for k, v in r.items()}))
    assert _worst(r) <= 1.0
    bad = R.check_bn_sync(xs, g, b, dys, True, rm0, rv0, bn32_sync(xs, g, b, dys, True, rm0, rv0, defect="local_n"))
    print("  dgamma / N with the rank-local N: dx %.3g" % bad["dx"])
    assert (bad["dx"] > 100.0) == (n1 > 0)          # with an empty second rank the first rank's N IS the global one


def test_two_rank_dense_parts_meet_the_ambiguity_condition():
    for C, H, W, b0, b1 in R.SYNC_DENSE:
        x, g, b, dy = R.dense_inputs((b0 + b1, C, H, W), "ordinary", seed=2)
        assert R.ambiguity(R.bn_forward_reference(R.rows(x), g, b, True)) <= 0.01


# ---- BatchNorm: single defects leave the bounds --------------------------------------------------------------------------------------

def test_a_float32_variance_leaves_the_bounds_where_the_mean_is_large():
    for C, n in ((4, 3001), (64, 129)):
        x, g, b, dy = R.family_rows("offset", n, C, 1)
        rm0, rv0 = R.running_init(C)
        r, _ = R.check_bn(x, g, b, dy, False, rm0, rv0, bn32(x, g, b, dy, False, rm0, rv0, R.sparse_blocks(n)[1], defect="var32"))
        print("float32 variance, offset family C %d n %d: invstd %.3g y %.3g dx %.3g" % (C, n, r["invstd"], r["y"], r["dx"]))
        assert r["invstd"] > 100.0 and r["y"] > 100.0 and r["dx"] > 100.0


def test_a_biased_running_var_leaves_its_bound():
    for n in (2, 127, 3001):
        x, g, b, dy = R.family_rows("ordinary", n, 4, 1)
        rm0, rv0 = R.running_init(4)
        r, _ = R.check_bn(x, g, b, dy, True, rm0, rv0, bn32(x, g, b, dy, True, rm0, rv0, R.sparse_blocks(n)[1], defect="no_bessel"))
        print("running_var without n / (n - 1), n %d: %.3g" % (n, r["running_var"]))
        assert r["running_var"] > 10.0 and max(v for k, v in r.items() if k != "running_var") <= 1.0


def test_a_dropped_partial_leaves_the_bounds():
    """the last live row block of a sparse table (one row at n = 129), the last plane slice of a dense map"""
    for n in (128, 129, 3001):
        x, g, b, dy = R.family_rows("ordinary", n, 4, 1)
        rm0, rv0 = R.running_init(4)
        spans = R.sparse_blocks(n)[1]
        last = max(i for i, (a, e) in enumerate(spans) if e > a)
        f, _ = R.check_bn(x, g, b, dy, False, rm0, rv0, bn32(x, g, b, dy, False, rm0, rv0, spans, "drop_fwd", last))
        w, _ = R.check_bn(x, g, b, dy, False, rm0, rv0, bn32(x, g, b, dy, False, rm0, rv0, spans, "drop_bwd", last))
        print("sparse n %d, block %d dropped: forward mean %.3g, backward dbeta %.3g dgamma %.3g" % (n, last, f["mean"], w["dbeta"], w["dgamma"]))
        assert f["mean"] > 100.0 and w["dbeta"] > 100.0 and w["dgamma"] > 100.0
    shape = (1, 2, 128, 132)          # the large dense map: one slice is 1 / 16 of the plane, inside the old atol = 2e-2
    x, g, b, dy = R.dense_inputs(shape, "ordinary")
    rm0, rv0 = R.running_init(2)
    w, _ = R.check_bn(R.rows(x), g, b, R.rows(dy), False, rm0, rv0, bn32_dense(x, g, b, dy, False, rm0, rv0, "drop_bwd", 15))
    print("dense %s, slice 15 dropped in the backward: dbeta %.3g dgamma %.3g" % (shape, w["dbeta"], w["dgamma"]))
    assert w["dbeta"] > 100.0 and w["dgamma"] > 100.0


# ---- the block rules ------------------------------------------------------------------------------------------------------------------

def test_restated_block_rules_give_the_named_branches():
    assert R.sparse_blocks(0)[0] == 0 and R.live(R.sparse_blocks(0)[1]) == []
    assert R.live(R.sparse_blocks(1)[1]) == [1]
    assert R.sparse_blocks(127)[0] == 1 and len(R.live(R.sparse_blocks(127)[1])) == 127          # one empty block
    assert R.live(R.sparse_blocks(128)[1]) == [1] * 128 and [n for _, n, _, _ in R.SPARSE_CASES if R.sparse_blocks(n)[1][127][1] > R.sparse_blocks(n)[1][127][0]]
    c, sp = R.sparse_blocks(129)
    assert c == 2 and R.live(sp) == [2] * 64 + [1] and len(sp) - len(R.live(sp)) == 63             # a one-row last live block
    assert R.sparse_blocks(3001)[0] == 24 and R.live(R.sparse_blocks(3001)[1])[-1] == 3001 - 24 * 125
    assert R.plane_slices(4) == (1, [(0, 1)] + [(1, 1)] * 15)                                      # one quad, 15 empty slices
    assert R.plane_slices(60)[0] == 1 and len(R.live(R.plane_slices(60)[1])) == 15
    assert R.plane_slices(36)[0] == 1 and len(R.live(R.plane_slices(36)[1])) == 9
    assert R.plane_slices(128 * 132)[0] == 264 > 256                                                # a second thread-stride pass
    assert R.plane_slices(256 * 260)[0] > 256 and R.dot_blocks(1, 256 * 260) == 260 > 256          # SSFA: both second passes
    assert R.dot_blocks(2, 60) == 1 and 2 * 15 < 64                                                 # dead lanes in the only dot block
    assert R.dot_blocks(3, 20) == 1 and R.dot_blocks(1, 240) == 1


# ---- SSFA tail ------------------------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """float32 fma through float64: the product of two float32 values is exact there"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def _dot32(x, w):
    """ssfa_dot_kernel: x (B, C, H, W); w (C) or a (B, C, H, W) map. fma chain per channel quarter, ((p0 + p1) + p2) + p3"""
    B, C, H, W = x.shape
    cper = C // 4
    parts = []
    for cq in range(4):
        acc = np.zeros((B, H, W), F)
        for c in range(cq * cper, (cq + 1) * cper):
            wc = w[c] if w.ndim == 1 else w[:, c]
            acc = (x[:, c].astype(np.float64) * np.asarray(wc, np.float64) + acc.astype(np.float64)).astype(F)
        parts.append(acc)
    return (((parts[0] + parts[1]) + parts[2]) + parts[3]).reshape(-1)


def _attention32(s0, s1, stats, gb, swapped):
    g0, b0, g1, b1 = (F(v) for v in gb)
    zh0, zh1 = (s0 - stats[0]) * stats[1], (s1 - stats[2]) * stats[3]
    z0, z1 = _fma(zh0, g0, np.full_like(zh0, b0)), _fma(zh1, g1, np.full_like(zh1, b1))
    m = np.maximum(z0, z1)
    e0, e1 = np.exp(z0 - m), np.exp(z1 - m)
    inv = F(1) / (e0 + e1)
    a0, a1 = e0 * inv, e1 * inv
    if swapped:
        a0 = e1 * inv
        a1 = F(1) - a0
    return a0, a1, zh0, zh1


def ssfa32(x0, x1, w0, w1, gb, grad, rm0, rv0, defect=None):
    x0, x1, w0, w1, grad = (t.numpy() for t in (x0, x1, w0, w1, grad))
    B, C, H, W = x0.shape
    n = B * H * W
    s = [_dot32(x0, w0), _dot32(x1, w1)]
    nb = R.dot_blocks(B, H * W)
    # a dot block = 64 consecutive quads = 256 consecutive pixels of the (b, pixel) order
    spans = [(256 * i, min(n, 256 * (i + 1))) for i in range(nb)]
    stats, rm, rv = [], [], []
    for k in range(2):
        t0, t1 = _sums64([s[k][:, None], s[k][:, None].astype(np.float64) ** 2], spans, nb - 1 if defect == "drop_fwd" else None)
        mean_f, is_f, m, v = _finish(t0, t1, n, rm0[k:k + 1].numpy(), rv0[k:k + 1].numpy(), None)
        stats += [mean_f[0], is_f[0]]
        rm.append(m[0]); rv.append(v[0])
    stats = np.asarray(stats, F)
    a0, a1, zh0, zh1 = _attention32(s[0], s[1], stats, gb, defect == "swapped")
    A0, A1 = a0.reshape(B, 1, H, W), a1.reshape(B, 1, H, W)
    out = x0 * A0 + x1 * A1
    r0, r1 = _dot32(x0, grad), _dot32(x1, grad)
    dz = a0 * a1 * (r0 - r1)
    dz64 = dz.astype(np.float64)[:, None]
    t = _sums64([dz64, dz64 * zh0.astype(np.float64)[:, None], dz64 * zh1.astype(np.float64)[:, None]], spans, None)
    dbeta = np.asarray([F(t[0][0]), F(-t[0][0])], F)
    dgamma = np.asarray([F(t[1][0]), F(-t[2][0])], F)
    g0, g1 = F(gb[0]), F(gb[2])
    inv_n = F(1) / F(n)
    k0, k1 = g0 * stats[1], g1 * stats[3]
    ds0 = k0 * (dz - dbeta[0] * inv_n - zh0 * (dgamma[0] * inv_n))
    ds1 = k1 * (-dz - dbeta[1] * inv_n - zh1 * (dgamma[1] * inv_n))
    D0, D1 = ds0.reshape(B, 1, H, W), ds1.reshape(B, 1, H, W)
    wv0, wv1 = w0.reshape(1, C, 1, 1), w1.reshape(1, C, 1, 1)
    dx0 = (wv0.astype(np.float64) * D0.astype(np.float64) + (grad * A0).astype(np.float64)).astype(F)
    dx1 = (wv1.astype(np.float64) * D1.astype(np.float64) + (grad * A1).astype(np.float64)).astype(F)
    dw0 = F((D0.astype(np.float64) * x0.astype(np.float64)).sum((0, 2, 3)))
    dw1 = F((D1.astype(np.float64) * x1.astype(np.float64)).sum((0, 2, 3)))
    got = dict(smap=np.stack(s), stats=stats, out=out, running_mean=np.asarray(rm, F), running_var=np.asarray(rv, F), dzmap=dz,
               dx0=dx0, dx1=dx1, dw0=dw0, dw1=dw1, dgamma=dgamma, dbeta=dbeta)
    return {k: _t(v) for k, v in got.items()}


def _ssfa_running():
    return torch.tensor([0.05, 0.1]), torch.tensor([0.7, 0.9])


@pytest.mark.parametrize("shape,kind", R.SSFA_CASES)
def test_ssfa_restatement_meets_both_stages(shape, kind):
    x0, x1, w0, w1, gb, grad = R.ssfa_inputs(shape, kind)
    rm0, rv0 = _ssfa_running()
    got = ssfa32(x0, x1, w0, w1, gb, grad, rm0, rv0)
    r, fw = R.check_ssfa(x0, x1, w0, w1, gb, grad, rm0, rv0, got)
    print("SSFA %s %s: %s" % (shape, kind, {k: round(v, 3) for k, v in r.items()}))
    assert _worst(r) <= 1.0
    assert bool((got["dbeta"][1] == -got["dbeta"][0]))
    z = fw["att"]["z"]
    if kind == "saturated":
        assert float((z[0] - z[1]).abs().max()) > 30.0
    if kind == "equal":
        assert float((fw["att"]["a"] - 0.5).abs().max()) < 0.45 and torch.equal(got["smap"][0], got["smap"][1])


def test_ssfa_defects_leave_the_bounds():
    shape, kind = (1, 4, 256, 260), "plain"
    x0, x1, w0, w1, gb, grad = R.ssfa_inputs(shape, kind)
    rm0, rv0 = _ssfa_running()
    sw, _ = R.check_ssfa(x0, x1, w0, w1, gb, grad, rm0, rv0, ssfa32(x0, x1, w0, w1, gb, grad, rm0, rv0, defect="swapped"))
    dr, _ = R.check_ssfa(x0, x1, w0, w1, gb, grad, rm0, rv0, ssfa32(x0, x1, w0, w1, gb, grad, rm0, rv0, defect="drop_fwd"))
    print("SSFA %s: attention weights exchanged: out %.3g dzmap %.3g; last dot block's partial dropped: stats %.3g" %
          (shape, sw["B.out"], sw["A.dzmap"], dr["B.stats"]))
    assert sw["B.out"] > 100.0 and dr["B.stats"] > 100.0 and sw["A.smap"] <= 1.0
