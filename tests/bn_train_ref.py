"""float64 references and DERIVED error bounds for the train-mode BatchNorm (+ ReLU) passes of csrc/bn_train.hip -- sparse table,
dense NCHW map, and their split SyncBN form -- and for the fused SSFA attention tail of csrc/ssfa_train.hip. No GPU is needed here:
tests/test_bn_train_ref_cpu.py checks that the bounds can be met and are not vacuous, tests/test_bn_train_f64_gpu.py holds the kernels
to them. The references are written from the formulas, not from torch.nn.BatchNorm*, so that n = 0, n = 1 and var = 0 are defined:
the biased variance normalises, the unbiased one goes into running_var only when n > 1, running statistics are untouched at n = 0,
rows >= n are zero.

Notation: u = 2^-24 and gamma(n) from tests/dense_grad_ref.py; u64 = 2^-53, gamma64(n) the same for float64. All tensors are laid out
as ROWS (n, C): a sparse table's valid rows, or a dense map through rows(). eps and momentum are the float32 values the C entry
points receive. Every bound is per element and input-aware; SLACK = 1 + 2^-16 covers the second-order terms of the first-order
derivations below.

STATISTICS (bn_stats; bn_stats_kernel / bn2d_stats_kernel / ssfa_dot_kernel<false> and their finishers, bn_sync_finalize_kernel):
    t0 = sum x, t1 = sum x^2   float64: `s0 += d; s1 += d * d` (the square of a float32 is exact in float64), lane tree, block
                               partials in block order: no path has more than n additions                gamma64(n) each
    m = t0 / n                 1 float64 rounding: e64_mu = gamma64(n + 2) sum|x| / n
    var = t1 / n - m * m       d_var = gamma64(2 n + 6) (sum x^2 / n + mu^2): NOT negligible against var when |mu| >> std
    save_mean = (float)m       E_mu = u |mu| + e64_mu
    save_invstd = (float)(1.0 / sqrt(var + eps))
                               rel_is = u + ((1 - d_var / (var + eps))^(-1/2) - 1) + 4 u64   (relative; d_var / (2 (var + eps)) to
                               first order)
    running_mean = (float)((1 - momentum) * running_mean + momentum * m)               E = u |new| + momentum e64_mu
    running_var  = (float)((1 - momentum) * running_var + momentum * unbiased)         E = u |new| + momentum d_var n / (n - 1)

FORWARD (bn_forward_reference; bn_apply_kernel `(xv - mean) * invstd * g + beta`, bn2d_z -- the file is compiled without fp
contraction: four roundings):
    d = x - mean_f             |mean_f - mu| <= E_mu, 1 rounding:             E_mu + u |x - mu|
    xhat_f = d * invstd_f      invstd_f = is (1 + rel_is), 1 rounding:        E_xhat = (2 u + rel_is) |xhat| + E_mu is
    z_f = xhat_f * g + beta    2 roundings:                                   E_z = |g| E_xhat + u |xhat g| + u |z|
    y = max(0, z): ReLU is 1-Lipschitz, E_y = E_z.

BACKWARD (bn_backward_reference; bn_stats_kernel<true> / bn2d_stats_kernel<1>, bn_apply_kernel<true> / bn2d_apply_kernel<true>).
The ReLU mask is DATA: the reference differentiates with the mask y_dev > 0 of the device's own forward output, after the test has
verified that it equals z64 > 0 wherever |z64| > E_z; ambiguity() is the share of {|z64| <= E_z}, a property of the inputs that
tests/test_bn_train_ref_cpu.py holds below 1 % for every input family.
    dbeta  = (float) sum dz               float64 sum, one cast:  E_dbeta = u |dbeta| + gamma64(n + 2) sum|dz|
    dgamma = (float) sum dz * xhat_f      `(double)g * (double)((xv - mu) * is)`: exact products of float32 values:
                                          E_dgamma = sum|dz| E_xhat + u |dgamma| + gamma64(n + 2) sum|dz xhat|
    dx = k * (dz - db - xhat_f * dg),  A = dz, Bt = dbeta / N, Ct = xhat dgamma / N:
        inv_n = 1.f / (float)N  (or (float)(1.0 / N), bn_sync_finalize_kernel)                      1 rounding
        db = dbeta_f * inv_n                                     E_B = E_dbeta / N + 2 u |Bt|
        xhat_f * dgamma_f * inv_n (two products, either order)   E_C = (E_xhat |dgamma| + |xhat| E_dgamma) / N + 3 u |Ct|
        the two subtractions                                     2 u (|A| + |Bt|) + u |Ct|
        k = g * invstd_f (1 rounding), the last product (1)      (rel_is + 2 u) |dx|
        E_dx = |g| is (E_B + E_C + 2 u (|A| + |Bt|) + u |Ct|) + (rel_is + 2 u) |dx|
SyncBN form: the statistics, dx and the sums in dx are those of the concatenated batch of all ranks (N = the global row count); a
rank's dgamma / dbeta are its local sums (local_param_grads).

SSFA TAIL, two stages against the C entry points, whose saved tensors (smap, stats, dzmap) are outputs one can read.
Stage A, from the inputs:
    smap_k = sum_c w_k[c] x_k[c]    ssfa_dot_kernel<false>: an fma chain over a channel quarter (C / 4 roundings), then
                                    `((p0 + p1) + p2) + p3` (3):   E = gamma(C / 4 + 3) sum_c |w_k[c] x_k[c]|
    dzmap = a0 a1 (da0 - da1)       ssfa_dot_kernel<true>: da_k = sum_c g[c] x_k[c] the same way, E_da = gamma(C / 4 + 3) sum_c |g x_k|;
                                    a from attention() on the device's own smap and stats (the stage A form of attention_reference:
                                    the float32 stats are data):
                                    E_dz = a0 a1 (E_da0 + E_da1) + (E_a0 a1 + a0 E_a1) |da0 - da1| + 3 u |dz|
Stage B, downstream from the device's smap and dzmap (float32 values taken as data), with the EXACT statistics of that smap:
    stats, running statistics       as STATISTICS above with C = 1
    attention()                     zh = (s - mean_f) * invstd_f: E_zh = E_xhat above (stage A form: 2 u |zh|);  z = fmaf(zh, g, b):
                                    E_z = |g| E_zh + u |z|;  m = max(z0, z1); e_k = expf(z_k - m): one of them is expf(0) = 1 exactly,
                                    the other has the subtraction's u |z0 - z1| in its exponent and expf's own error (2 ulp = 4 u
                                    allowed);  inv = 1.f / (e0 + e1) (2 roundings), a_k = e_k * inv (1);  d a_k / d z = +- a0 a1:
                                    E_a_k = a0 a1 (E_z0 + E_z1 + u |z0 - z1| + 4 u) + 3 u a_k   (+ 1e-37 where expf underflows)
    out = x0 a0 + x1 a1             ssfa_blend_kernel: two products and an add:  E_out = |x0| E_a0 + |x1| E_a1 + 2 u (|x0| a0 + |x1| a1)
    dbeta = [S, -S], S = sum dz; dgamma = [sum dz zh0, -sum dz zh1]   as BACKWARD above; dbeta[1] = -dbeta[0] exactly
    ds_k = k_k (dz_k - db_k - zh_k dg_k), dz_1 = -dz_0                as dx of BACKWARD above (ssfa_bwd_apply_kernel, same roundings)
    dx_k = fmaf(w_k, ds_k, g * a_k)                                   E = |w_k| E_ds_k + |g| E_a_k + u |g a_k| + u |dx_k|
    dw_k[c] = (float) sum ds_k x_k[c]   float64 sum of exact products, one cast:  E = sum |x_k| E_ds_k + u |dw| + gamma64(n + 2) sum |ds x|
"""
import torch

from dense_grad_ref import U, gamma, ratio  # noqa: F401  (ratio is re-exported for the tests)

U64 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -16
BN_BLOCKS = 128      # csrc/bn_train.hip
BN2D_SPLIT = 16      # csrc/bn_train.hip; SLICES of csrc/ssfa_train.hip
EPS, MOMENTUM = 1e-3, 0.01


def gamma64(n, acc=U64):
    return n * acc / (1.0 - n * acc)


def f32(v):
    """the float32 value a C `float` argument receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def rows(x):
    """(B, C, H, W) -> (B H W, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def unrows(r, B, H, W):
    return r.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ---- which rows each statistics block takes, restated (a change of the rule must fail the tests that name a branch) ------------------

def sparse_blocks(n):
    """bn_stats_kernel: chunk = divup(n, 128); block b takes rows [b chunk, min(n, (b + 1) chunk)). -> (chunk, [(r0, r1)] * 128)"""
    chunk = -(-n // BN_BLOCKS)
    return chunk, [(min(n, b * chunk), min(n, (b + 1) * chunk)) for b in range(BN_BLOCKS)]


def plane_slices(plane):
    """bn2d_stats_kernel, ssfa_bwd_apply_kernel: 16 slices of the plane's quads, chunk = divup(plane / 4, 16). -> (chunk, [(q0, q1)] * 16)"""
    quads = plane // 4
    chunk = -(-quads // BN2D_SPLIT)
    return chunk, [(min(quads, s * chunk), min(quads, (s + 1) * chunk)) for s in range(BN2D_SPLIT)]


def dot_blocks(B, plane):
    """ssfa_dot_kernel: blocks of 64 pixel quads over all images"""
    return -(-(B * (plane // 4)) // 64)


def live(spans):
    return [b - a for a, b in spans if b > a]


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------------

def bn_stats(x, eps=EPS, acc=U64):
    """x (n, C): float32 values. The float64 statistics and the bounds of what the finisher saves (see STATISTICS). acc: the unit
    roundoff of the accumulation -- u64 for the kernels, u for torch's own BatchNorm (the shapes ops.bn2d_relu_train hands to it)."""
    x = x.double()
    n, C = x.shape
    eps = f32(eps)
    if n:
        mu = x.mean(0)
        var = ((x - mu) ** 2).mean(0)     # two-pass: the reference's own float64 error stays far below d_var
        sabs, sq = x.abs().sum(0), (x * x).sum(0)
    else:
        mu = var = sabs = sq = torch.zeros(C, dtype=torch.float64)
    is_ = 1.0 / torch.sqrt(var + eps)
    e64_mu = gamma64(n + 2, acc) * sabs / max(n, 1)
    d_var = gamma64(2 * n + 6, acc) * (sq / max(n, 1) + mu * mu)
    r = d_var / (var + eps)
    assert float(r.max()) < 0.5
    rel_is = U + torch.expm1(-0.5 * torch.log1p(-r)) + 4 * acc      # (1 - r)^(-1/2) - 1: d_var / (2 (var + eps)) to first order
    xhat = (x - mu) * is_
    E_mu = U * mu.abs() + e64_mu
    return dict(n=n, acc=acc, mu=mu, var=var, invstd=is_, xhat=xhat, E_mu=SLACK * E_mu, E_invstd=SLACK * rel_is * is_, rel_is=rel_is,
                e64_mu=e64_mu, d_var=d_var, E_xhat=SLACK * ((2 * U + rel_is) * xhat.abs() + E_mu * is_))


def running_reference(st, running_mean, running_var, momentum=MOMENTUM):
    """((running_mean, running_var) after the update, their bounds); untouched (bound 0: the same bits) at n = 0"""
    rm, rv = running_mean.double(), running_var.double()
    n, mom = st["n"], f32(momentum)
    if n == 0:
        return (rm, rv), (torch.zeros_like(rm), torch.zeros_like(rv))
    bessel = n / (n - 1.0) if n > 1 else 1.0
    nm, nv = (1 - mom) * rm + mom * st["mu"], (1 - mom) * rv + mom * st["var"] * bessel
    if st["acc"] != U64:
        # torch's own update is float32 arithmetic, not one cast of a float64 expression: 1 - momentum, the two products and the sum
        # are 4 roundings on the absolute-value image, n / (n - 1) and its product 2 more for the variance
        im, iv = (1 - mom) * rm.abs() + mom * st["mu"].abs(), (1 - mom) * rv.abs() + mom * st["var"] * bessel
        return (nm, nv), (SLACK * (gamma(4) * im + mom * st["e64_mu"]), SLACK * (gamma(6) * iv + mom * st["d_var"] * bessel))
    return (nm, nv), (SLACK * (U * nm.abs() + mom * st["e64_mu"]), SLACK * (U * nv.abs() + mom * st["d_var"] * bessel))


def bn_forward_reference(x, g, b, relu, eps=EPS, acc=U64):
    """x (n, C) valid rows, g / b (C). -> (st with z, y, E_z added). E_y = E_z."""
    st = bn_stats(x, eps, acc)
    g, b = g.double(), b.double()
    z = st["xhat"] * g + b
    st.update(g=g, b=b, z=z, y=z.clamp_min(0) if relu else z,
              E_z=SLACK * (g.abs() * st["E_xhat"] + U * (st["xhat"] * g).abs() + U * z.abs()))
    return st


def ambiguity(st):
    """the share of elements whose ReLU decision the bound does not fix: |z64| <= E_z"""
    return float((st["z"].abs() <= st["E_z"]).double().mean()) if st["z"].numel() else 0.0


def mask_agrees(st, y_dev):
    """y_dev > 0 equals z64 > 0 wherever |z64| > E_z"""
    sure = st["z"].abs() > st["E_z"]
    return bool(((y_dev.detach().cpu() > 0) == (st["z"] > 0))[sure].all())


def _dx_bound(st, g, dz, dbeta, dgamma, E_dbeta, E_dgamma, N):
    """(dx, E_dx) of dx = g is (dz - dbeta / N - xhat dgamma / N), see BACKWARD"""
    xhat, is_ = st["xhat"], st["invstd"]
    A, Bt, Ct = dz, dbeta / N, xhat * dgamma / N
    dx = g * is_ * (A - Bt - Ct)
    E_B = E_dbeta / N + 2 * U * Bt.abs()
    E_C = (st["E_xhat"] * dgamma.abs() + xhat.abs() * E_dgamma) / N + 3 * U * Ct.abs()
    E_in = E_B + E_C + 2 * U * (A.abs() + Bt.abs()) + U * Ct.abs()
    return dx, SLACK * (g.abs() * is_ * E_in + (st["rel_is"] + 2 * U) * dx.abs())


def _sums(st, dz, lo, hi):
    n = hi - lo
    d, xh = dz[lo:hi], st["xhat"][lo:hi]
    dbeta, dgamma = d.sum(0), (d * xh).sum(0)
    E_dbeta = U * dbeta.abs() + gamma64(n + 2, st["acc"]) * d.abs().sum(0)
    E_dgamma = (d.abs() * st["E_xhat"][lo:hi]).sum(0) + U * dgamma.abs() + gamma64(n + 2, st["acc"]) * (d * xh).abs().sum(0)
    return dbeta, dgamma, SLACK * E_dbeta, SLACK * E_dgamma


def bn_backward_reference(st, dy, mask):
    """st: bn_forward_reference of the (concatenated) batch; dy (n, C); mask (n, C) bool (y_dev > 0) or None (no ReLU).
    -> ({dx, dgamma, dbeta, dz}, the bounds of the first three)"""
    dz = dy.double() if mask is None else dy.double() * mask.double()
    n = st["n"]
    dbeta, dgamma, E_dbeta, E_dgamma = _sums(st, dz, 0, n)
    dx, E_dx = _dx_bound(st, st["g"], dz, dbeta, dgamma, E_dbeta, E_dgamma, max(n, 1))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dz=dz), dict(dx=E_dx, dgamma=E_dgamma, dbeta=E_dbeta)


def local_param_grads(st, dz, lo, hi):
    """SyncBN: a rank's dgamma / dbeta are the sums over ITS rows [lo, hi) with the global statistics. -> ({dgamma, dbeta}, bounds)"""
    dbeta, dgamma, E_dbeta, E_dgamma = _sums(st, dz, lo, hi)
    return dict(dgamma=dgamma, dbeta=dbeta), dict(dgamma=E_dgamma, dbeta=E_dbeta)


# ---- the input families ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("ordinary", "offset", "constant", "zeros")


def family_rows(name, n, C, seed):
    """(x (n, C), gamma, beta, dy (n, C)) float32. ordinary: randn 1.7 + 0.3. offset: |mean| >> std (even channels 100 +- 0.1, odd
    channels -40 +- 1). constant: the last channel is 2.5 everywhere (var = 0). zeros: 90 % exact zeros (the mostly empty BEV map)."""
    gen = torch.Generator().manual_seed(seed * 7919 + n * 31 + C + FAMILIES.index(name) * 1000003)
    x = torch.randn(n, C, generator=gen) * 1.7 + 0.3
    if name == "offset":
        even = (torch.arange(C) % 2 == 0)
        x = torch.where(even, torch.randn(n, C, generator=gen) * 0.1 + 100.0, torch.randn(n, C, generator=gen) - 40.0)
    elif name == "constant":
        x[:, -1] = 2.5
    elif name == "zeros":
        x = x * (torch.rand(n, C, generator=gen) < 0.1)
    g, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.2
    return x.float().contiguous(), g, b, torch.randn(n, C, generator=gen)


def running_init(C, seed=3):
    gen = torch.Generator().manual_seed(seed + C)
    return torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5


# sparse table: (C, n, cap, family). C 1 / 2: VEC 1; 4 / 64 / 256: VEC 4; Q = C / VEC from 1 to 64; finisher G = 256 / C from 256 to 1.
# n = 128: the only count here at which block 127 has a row (127: chunk 1, block 127 empty; 129: 65 live blocks; 3001: 126) -- without it
# a finisher that leaves out the last block's partial passes every case.
SPARSE_CASES = [(C, n, n + 5, "ordinary") for C in (1, 2, 4, 64, 256) for n in (0, 1, 2, 127, 128, 129, 3001)] + \
               [(C, n, n + 3, fam) for fam in FAMILIES[1:] for C in (1, 4, 64) for n in (129, 3001)]
# dense map: ((B, C, H, W), family)
DENSE_CASES = [((1, 1, 2, 2), "ordinary"), ((3, 24, 6, 10), "ordinary"), ((2, 5, 4, 9), "ordinary"), ((1, 2, 128, 132), "ordinary"),
               ((1, 1024, 2, 2), "ordinary")] + [(s, fam) for fam in FAMILIES[1:] for s in ((3, 24, 6, 10), (1, 2, 128, 132))]
DENSE_FALLBACK = [(1, 1025, 2, 2), (2, 5, 3, 5)]     # more than 1024 channels; a plane that is no multiple of 4
DENSE_REUSE = (2, 3, 4, 6)                           # run in the workspace that has just served C = 1024
# two ranks in one process: sparse (C, rows of rank 0, rows of rank 1), dense (C, H, W, images of rank 0, images of rank 1)
SYNC_SPARSE = [(64, 300, 177), (64, 477, 0), (2, 300, 177)]
SYNC_DENSE = [(24, 6, 10, 2, 1)]


def dense_inputs(shape, fam, seed=1):
    B, C, H, W = shape
    x, g, b, dy = family_rows(fam, B * H * W, C, seed)
    return unrows(x, B, H, W), g, b, unrows(dy, B, H, W)


# ---- SSFA tail ------------------------------------------------------------------------------------------------------------------------

def ssfa_dot_reference(x0, x1, w0, w1):
    """x (B, C, H, W); w (C), or a (B, C, H, W) map (the backward's dot with grad_out). -> ((2, B H W) float64, bound): stage A."""
    C = x0.shape[1]
    out, bnd = [], []
    for x, w in ((x0, w0), (x1, w1)):
        p = x.double() * (w.double().view(1, -1, 1, 1) if w.dim() == 1 else w.double())
        out.append(p.sum(1).reshape(-1))
        bnd.append(gamma(C // 4 + 3) * p.abs().sum(1).reshape(-1))
    return torch.stack(out), torch.stack(bnd)


def attention_reference(smap, mean, invstd, E_zh, gb):
    """smap (2, n) float64; mean, invstd: two float64 numbers each; E_zh (2, n); gb = (g0, b0, g1, b1) floats.
    -> dict(a (2, n), zh, z, E_a (2, n))"""
    g = torch.tensor([float(gb[0]), float(gb[2])], dtype=torch.float64).view(2, 1)
    b = torch.tensor([float(gb[1]), float(gb[3])], dtype=torch.float64).view(2, 1)
    zh = (smap - mean.view(2, 1)) * invstd.view(2, 1)
    z = zh * g + b
    a = torch.softmax(z, 0)
    E_z = g.abs() * E_zh + U * z.abs()
    aa = a[0] * a[1]
    E_a = aa * (E_z[0] + E_z[1] + U * (z[0] - z[1]).abs() + 4 * U) + 3 * U * a + 1e-37
    return dict(a=a, zh=zh, z=z, g=g, E_a=SLACK * E_a)


def attention_stage_a(smap_dev, stats_dev, gb):
    """attention() from the device's smap AND the device's float32 stats [mean0, invstd0, mean1, invstd1] as data: E_zh = 2 u |zh|"""
    s, st = smap_dev.double(), stats_dev.double()
    mean, invstd = st[[0, 2]], st[[1, 3]]
    zh = (s - mean.view(2, 1)) * invstd.view(2, 1)
    return attention_reference(s, mean, invstd, 2 * U * zh.abs(), gb)


def ssfa_dz_reference(grad, x0, x1, att):
    """dzmap (B H W) and its stage A bound; att = attention_stage_a(...)"""
    da, E_da = ssfa_dot_reference(x0, x1, grad, grad)
    a, E_a = att["a"], att["E_a"]
    dz = a[0] * a[1] * (da[0] - da[1])
    E = a[0] * a[1] * (E_da[0] + E_da[1]) + (E_a[0] * a[1] + a[0] * E_a[1]) * (da[0] - da[1]).abs() + 3 * U * dz.abs()
    return dz, SLACK * E


def ssfa_stage_b(smap_dev, x0, x1, gb, eps=EPS):
    """Forward downstream from the device's smap: -> dict(st = [bn_stats of each branch], att, stats (4) + E_stats, out + E_out)"""
    s = smap_dev.double()
    st = [bn_stats(s[k].view(-1, 1), eps) for k in range(2)]
    mean, invstd = torch.stack([t["mu"][0] for t in st]), torch.stack([t["invstd"][0] for t in st])
    att = attention_reference(s, mean, invstd, torch.stack([t["E_xhat"][:, 0] for t in st]), gb)
    B, C, H, W = x0.shape
    a, E_a = att["a"].view(2, B, 1, H, W), att["E_a"].view(2, B, 1, H, W)
    X0, X1 = x0.double(), x1.double()
    out = X0 * a[0] + X1 * a[1]
    E_out = X0.abs() * E_a[0] + X1.abs() * E_a[1] + 2 * U * (X0.abs() * a[0] + X1.abs() * a[1])
    stats = torch.stack([st[0]["mu"][0], st[0]["invstd"][0], st[1]["mu"][0], st[1]["invstd"][0]])
    E_stats = torch.stack([st[0]["E_mu"][0], st[0]["E_invstd"][0], st[1]["E_mu"][0], st[1]["E_invstd"][0]])
    return dict(st=st, att=att, stats=stats, E_stats=E_stats, out=out, E_out=SLACK * E_out)


def ssfa_backward_stage_b(fw, dz_dev, grad, x0, x1, w0, w1):
    """fw = ssfa_stage_b(...); dz_dev (B H W): the device's dzmap as data. -> ({dx0, dx1, dw0, dw1, dgamma (2), dbeta (2)}, bounds)"""
    B, C, H, W = x0.shape
    n = B * H * W
    dz0 = dz_dev.double().view(-1, 1)
    G = grad.double()
    ref, bnd = {}, {}
    dgam, dbet, E_dgam, E_dbet = [], [], [], []
    for k, (x, w) in enumerate(((x0, w0), (x1, w1))):
        st = fw["st"][k]
        dz = dz0 if k == 0 else -dz0
        dbeta, dgamma, E_dbeta, E_dgamma = _sums(st, dz, 0, n)
        ds, E_ds = _dx_bound(st, fw["att"]["g"][k], dz, dbeta, dgamma, E_dbeta, E_dgamma, n)
        ds, E_ds = ds.view(B, 1, H, W), E_ds.view(B, 1, H, W)
        a, E_a = fw["att"]["a"][k].view(B, 1, H, W), fw["att"]["E_a"][k].view(B, 1, H, W)
        X, wv = x.double(), w.double().view(1, -1, 1, 1)
        dx = G * a + wv * ds
        ref["dx%d" % k] = dx
        bnd["dx%d" % k] = SLACK * (wv.abs() * E_ds + G.abs() * E_a + U * (G * a).abs() + U * dx.abs())
        dw = (ds * X).sum((0, 2, 3))
        ref["dw%d" % k] = dw
        bnd["dw%d" % k] = SLACK * ((X.abs() * E_ds).sum((0, 2, 3)) + U * dw.abs() + gamma64(n + 2) * (ds * X).abs().sum((0, 2, 3)))
        dgam.append(dgamma[0]); dbet.append(dbeta[0]); E_dgam.append(E_dgamma[0]); E_dbet.append(E_dbeta[0])
    ref["dgamma"], ref["dbeta"] = torch.stack(dgam), torch.stack(dbet)
    bnd["dgamma"], bnd["dbeta"] = torch.stack(E_dgam), torch.stack(E_dbet)
    return ref, bnd


# (B, C, H, W), kind. plain: x0 = randn 1.2 + 0.2, x1 = randn 0.8 - 0.1. saturated: |z0 - z1| > 30 on part of the map. equal: x1 = x0
# and w1 = w0, so a = 0.5 up to beta and gamma.
SSFA_CASES = [((2, 8, 6, 10), "plain"), ((3, 4, 4, 5), "plain"), ((1, 64, 20, 12), "plain"), ((1, 4, 256, 260), "plain"),
              ((2, 8, 6, 10), "saturated"), ((2, 8, 6, 10), "equal")]
SSFA_GB = {"plain": (1.3, -0.1, 0.8, 0.1), "saturated": (14.0, 3.0, 11.0, -2.0), "equal": (1.3, -0.1, 0.8, 0.1)}


def ssfa_inputs(shape, kind):
    """(x0, x1, w0, w1, (g0, b0, g1, b1), grad)"""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(B * 100 + C + H + len(kind))
    x0 = torch.randn(B, C, H, W, generator=gen) * 1.2 + 0.2
    x1 = torch.randn(B, C, H, W, generator=gen) * 0.8 - 0.1
    w0, w1 = (torch.rand(C, generator=gen) * 2 - 1) * (3.0 / C) ** 0.5, (torch.rand(C, generator=gen) * 2 - 1) * (3.0 / C) ** 0.5
    if kind == "equal":
        x1, w1 = x0.clone(), w0.clone()
    gb = tuple(f32(v) for v in SSFA_GB[kind])
    return x0, x1, w0, w1, gb, torch.randn(B, C, H, W, generator=gen)


# ---- verdicts: what a set of outputs (the device's, or a float32 restatement's) is held to --------------------------------------------

def _ratio(got, ref, bound):
    return ratio(got, ref, bound) if ref.numel() else 0.0


def check_bn(x, g, b, dy, relu, rm0, rv0, got, eps=EPS, momentum=MOMENTUM, acc=U64):
    """x, dy (n, C): the valid rows; got: y, mean, invstd, running_mean, running_var, dx, dgamma, dbeta as rows / (C) vectors.
    Asserts the ambiguity condition and the mask agreement. -> ({name: worst error / bound}, st)"""
    st = bn_forward_reference(x, g, b, relu, eps, acc)
    (nm, nv), (E_m, E_v) = running_reference(st, rm0, rv0, momentum)
    r = dict(y=_ratio(got["y"], st["y"], st["E_z"]), mean=_ratio(got["mean"], st["mu"], st["E_mu"]),
             invstd=_ratio(got["invstd"], st["invstd"], st["E_invstd"]),
             running_mean=_ratio(got["running_mean"], nm, E_m), running_var=_ratio(got["running_var"], nv, E_v))
    assert ambiguity(st) <= 0.01
    if "dx" in got:
        if relu:
            assert mask_agrees(st, got["y"])
        ref, bnd = bn_backward_reference(st, dy, (got["y"].detach().cpu() > 0) if relu else None)
        r.update({k: _ratio(got[k], ref[k], bnd[k]) for k in ("dx", "dgamma", "dbeta")})
    return r, st


def check_bn_sync(xs, g, b, dys, relu, rm0, rv0, gots, eps=EPS, momentum=MOMENTUM):
    """Two (or more) ranks: xs / dys / gots per rank; every output of every rank against the reference of the concatenated batch; the
    ranks' local dgamma / dbeta add up to the global ones. -> {name: worst ratio over the ranks}"""
    st = bn_forward_reference(torch.cat(xs), g, b, relu, eps)
    (nm, nv), (E_m, E_v) = running_reference(st, rm0, rv0, momentum)
    assert ambiguity(st) <= 0.01
    ycat = torch.cat([t["y"].detach().cpu() for t in gots])
    if relu:
        assert mask_agrees(st, ycat)
    ref, bnd = bn_backward_reference(st, torch.cat(dys), (ycat > 0) if relu else None)
    r, lo = {}, 0
    tot = {k: torch.zeros_like(ref[k]) for k in ("dgamma", "dbeta")}
    E_tot = {k: torch.zeros_like(ref[k]) for k in ("dgamma", "dbeta")}

    def note(k, v):
        r[k] = max(r.get(k, 0.0), v)
    for x, got in zip(xs, gots):
        hi = lo + x.shape[0]
        note("y", _ratio(got["y"], st["y"][lo:hi], st["E_z"][lo:hi]))
        note("mean", _ratio(got["mean"], st["mu"], st["E_mu"]))
        note("invstd", _ratio(got["invstd"], st["invstd"], st["E_invstd"]))
        note("running_mean", _ratio(got["running_mean"], nm, E_m))
        note("running_var", _ratio(got["running_var"], nv, E_v))
        note("dx", _ratio(got["dx"], ref["dx"][lo:hi], bnd["dx"][lo:hi]))
        loc, E_loc = local_param_grads(st, ref["dz"], lo, hi)
        for k in ("dgamma", "dbeta"):
            note(k, _ratio(got[k], loc[k], E_loc[k]))
            tot[k] += got[k].detach().cpu().double()
            E_tot[k] += E_loc[k]
        lo = hi
    for k in ("dgamma", "dbeta"):
        note(k + "_total", ratio(tot[k], ref[k], E_tot[k]))
    return r


def check_ssfa(x0, x1, w0, w1, gb, grad, rm0, rv0, got, eps=EPS, momentum=MOMENTUM):
    """got: smap (2, n), stats (4), out, running_mean (2), running_var (2), dzmap (n), dx0, dx1, dw0, dw1, dgamma (2), dbeta (2).
    -> ({"A.smap", "A.dzmap"}: stage A ratios, {"B.*"}: stage B ratios)"""
    smap, E_smap = ssfa_dot_reference(x0, x1, w0, w1)
    r = {"A.smap": ratio(got["smap"], smap, E_smap)}
    fw = ssfa_stage_b(got["smap"].detach().cpu(), x0, x1, gb, eps)
    r["B.stats"] = ratio(got["stats"], fw["stats"], fw["E_stats"])
    r["B.out"] = ratio(got["out"], fw["out"], fw["E_out"])
    for k in range(2):
        (nm, nv), (E_m, E_v) = running_reference(fw["st"][k], rm0[k:k + 1], rv0[k:k + 1], momentum)
        r["B.running_mean"] = max(r.get("B.running_mean", 0.0), ratio(got["running_mean"][k:k + 1], nm, E_m))
        r["B.running_var"] = max(r.get("B.running_var", 0.0), ratio(got["running_var"][k:k + 1], nv, E_v))
    if "dzmap" in got:
        att = attention_stage_a(got["smap"].detach().cpu(), got["stats"].detach().cpu(), gb)
        dz, E_dz = ssfa_dz_reference(grad, x0, x1, att)
        r["A.dzmap"] = ratio(got["dzmap"], dz, E_dz)
        ref, bnd = ssfa_backward_stage_b(fw, got["dzmap"].detach().cpu(), grad, x0, x1, w0, w1)
        for k in ref:
            r["B." + k] = ratio(got[k], ref[k], bnd[k])
    return r, fw
