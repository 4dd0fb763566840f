"""TEST INFRASTRUCTURE ONLY -- one PFN layer in TRAIN mode (Linear, BatchNorm1d over all N * T slots, ReLU, max over the slots) two
ways, in any float dtype on the same inputs:

  formulation   the reference formulation in torch ops with autograd: F.linear, F.batch_norm(training=True), relu,
                torch.max(dim=1)[0] on the masked decorated columns of tests/pillars_ref.py (pillar_encoder.py:42-57, 114-153)
  closed_form   what csrc/pillar.hip's train kernels compute, restated: the totals S1 = sum f_i, G = sum f_i f_i^T over the live
                slots, sum z = w . S1, sum z^2 = w^T G w, mean / var / invstd over M = N * T, scale = gamma * invstd,
                shift = beta - mean * scale; per (pillar, channel) the selected slot = the lowest slot index that attains the
                maximum (padding slots are the indices >= num_points), dy = g where the selected pre-ReLU value is > 0,
                dbeta = sum dy, dgamma = sum dy * xhat, P = sum over live selected slots of dy * f_s,
                dW = scale * [P - dbeta / M * S1 - dgamma / M * invstd * (G w - mean * S1)].
                ranks = R: R identical ranks under SyncBN -- M, S1, G, dbeta, dgamma of the formula are R times this rank's; P,
                the S1 and G inside the brackets and the returned dgamma / dbeta are this rank's own.

tests/test_pillar_train_cpu.py holds closed_form to formulation's autograd in float64 (1e-10); the GPU tests use closed_form in
float64 as the yardstick of the kernels."""
import torch
import torch.nn.functional as F

import pillars_ref as PR

EPS = PR.EPS


def formulation(voxels, num_points, coors, w, gamma, beta, vx, vy, xo, yo, with_distance, dtype=torch.float64, g=None):
    """-> dict(out (N, C)[, dW, dgamma, dbeta for the upstream gradient g (N, C)])"""
    f, _ = PR.pillar_columns(voxels, num_points, coors, vx, vy, xo, yo, with_distance, dtype)
    N, T, K = f.shape
    w, gamma, beta = (torch.as_tensor(t).to(dtype).clone().requires_grad_(True) for t in (w, gamma, beta))
    z = F.linear(f.reshape(N * T, K), w)
    y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    out = torch.max(torch.relu(y).reshape(N, T, -1), dim=1)[0]
    r = dict(out=out.detach())
    if g is not None:
        out.backward(torch.as_tensor(g).to(dtype))
        r.update(dW=w.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return r


def closed_form(voxels, num_points, coors, w, gamma, beta, vx, vy, xo, yo, with_distance, dtype=torch.float64, g=None, ranks=1):
    """-> dict(f, live, S1, G, M, mean, var, invstd, scale, shift, y (N, T, C) pre-ReLU values, out (N, C)
    [, dW, dgamma, dbeta, P, sel (N, C) selected slot, dy])"""
    f, live = PR.pillar_columns(voxels, num_points, coors, vx, vy, xo, yo, with_distance, dtype)   # padding rows are zero
    N, T, K = f.shape
    w, gamma, beta = (torch.as_tensor(t).to(dtype) for t in (w, gamma, beta))
    rows = f.reshape(N * T, K)
    S1, G, M = rows.sum(0), rows.t() @ rows, float(N * T)
    Ma, S1a, Ga = ranks * M, ranks * S1, ranks * G          # of all ranks
    mean = (w @ S1a) / Ma
    var = ((w @ Ga) * w).sum(1) / Ma - mean * mean
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    z = F.linear(f, w)                                       # (N, T, C); 0 in the padding slots
    y = z * scale + shift
    r = dict(f=f, live=live, S1=S1, G=G, M=Ma, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, z=z, y=y)
    val, sel = torch.max(torch.relu(y), dim=1)               # the first maximal slot
    r["out"] = val
    if g is not None:
        g = torch.as_tensor(g).to(dtype)
        ysel = torch.gather(y, 1, sel[:, None, :])[:, 0]     # (N, C)
        zsel = torch.gather(z, 1, sel[:, None, :])[:, 0]
        dy = torch.where(ysel > 0, g, torch.zeros((), dtype=dtype))
        xhat = (zsel - mean) * invstd                        # a padding slot: z = 0
        dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
        fsel = f[torch.arange(N)[:, None], sel]              # (N, C, K); zero rows where a padding slot is selected
        P = (dy[:, :, None] * fsel).sum(0)                   # (C, K)
        dba, dga = ranks * dbeta, ranks * dgamma
        Gw = w @ G                                           # (C, K), G symmetric
        dW = scale[:, None] * (P - (dba / Ma)[:, None] * S1[None] - (dga / Ma * invstd)[:, None] * (Gw - mean[:, None] * S1[None]))
        r.update(dW=dW, dgamma=dgamma, dbeta=dbeta, P=P, sel=sel, dy=dy)
    return r


def running_stats(ref, running_mean, running_var, momentum):
    """torch.nn.BatchNorm1d's update from a closed_form result."""
    M = ref["M"]
    unbiased = ref["var"] * M / (M - 1) if M > 1 else ref["var"]
    return ((1 - momentum) * running_mean.to(unbiased.dtype) + momentum * ref["mean"],
            (1 - momentum) * running_var.to(unbiased.dtype) + momentum * unbiased)


def make_train_case(seed, N, T, with_distance, **kw):
    """tests/test_pillar_features_gpu.py::make_case (NaN padding slots, NaN rows beyond N with an absurd count and off-canvas cells)
    with train-mode parameters: gamma of both signs (the case's folded scale), beta ~ N(0, 0.5), running statistics to update."""
    import numpy as np
    from test_pillar_features_gpu import make_case
    case = make_case(seed, N, T, with_distance, **kw)
    rng = np.random.RandomState(seed + 7919)
    C = case["w"].shape[0]
    case["gamma"] = case.pop("scale")
    case.pop("shift")
    case["beta"] = (rng.randn(C) * 0.5).astype(np.float32)
    case["running_mean"] = (rng.randn(C) * 0.3).astype(np.float32)
    case["running_var"] = (rng.rand(C) + 0.5).astype(np.float32)
    assert kw.get("small") or ((case["gamma"] > 0).any() and (case["gamma"] < 0).any())
    return case


def live_args(case):
    """The N live rows (padding slots still NaN: the references mask them before they read them)."""
    N = case["N"]
    return case["voxels"][:N], case["num"][:N], case["coors"][:N]


U = 2.0 ** -24


def forward_bound(case, cf):
    """Per-element bound (N, C) on |device train-mode output - cf["out"]| (float64 closed form on the same float32 inputs), and
    the cap it never exceeds. Three parts, first order in u = 2^-24:

      (T + 16) u B   the eval kernel's own bound (tests/test_pillar_features_gpu.py) with the train-mode scale and shift:
                     B = |scale_c| sum_k |W_ck| A_k + |shift_c|;
      2 u B          scale and shift are handed to that kernel as float32: |d scale| |z| + |d shift| <= u (|scale| |z| + |shift|),
                     and the affine then runs on the rounded values;
      S              the statistics' own error. The kernel forms the decorated rows in float64 from the float32 points and keeps
                     the totals in float64, so this is the rounding of float64 sums over the L live slots: a live slot's z,
                     as the statistics see it, is off by at most E_pc = (L + 16) 2^-53 sum_k |W_ck| A_pk (every addition of
                     the longest chain and the row's own handful of operations), and
                        |d mean_c| <= sum_p num_p E_pc / M
                        |d var_c|  <= 2 / M sum_{live i} |z_i - mean_c| E_pc      (var = sum z^2 / M - mean^2)
                        |d invstd| =  invstd^3 / 2 |d var|
                     out = gamma invstd (z_s - mean) + beta  =>  S_pc = |gamma_c| (invstd_c |d mean_c| + D_pc |d invstd_c|)
                     with D_pc the largest |z - mean_c| over the pillar's candidates (|mean_c| for a padding slot). S is
                     orders of magnitude below u B; it is computed, not assumed.

    The sum is capped at (T + 32) u B: whatever the derivation gives, the test never grants more than that."""
    N, T = case["N"], case["T"]
    cols, live = cf["f"], cf["live"]
    raw = cols[:, :, :4].abs().amax(dim=1)
    A = [raw, 2 * raw[:, :3], cols[:, 0, 7:9].abs()]
    if case["dist"]:
        A.append(cols[:, :, 9:10].abs().amax(dim=1))
    A = torch.cat(A, dim=1)                                   # (N, K)
    w = torch.from_numpy(case["w"]).double()
    gamma = torch.from_numpy(case["gamma"]).double()
    B = cf["scale"].abs()[None] * (A @ w.abs().t()) + cf["shift"].abs()[None]
    num = live.sum(1).double()
    E = (float(num.sum()) + 16) * 2.0 ** -53 * (A @ w.abs().t())   # (N, C)
    M, mean, invstd = cf["M"], cf["mean"], cf["invstd"]
    dev = (cf["z"] - mean).abs()                              # (N, T, C); a padding slot: |mean|
    d_mean = (num[:, None] * E).sum(0) / M
    d_var = 2.0 / M * ((dev * live[:, :, None]).sum(1) * E).sum(0)
    d_invstd = 0.5 * invstd ** 3 * d_var
    D = dev.amax(dim=1)
    S = gamma.abs()[None] * (invstd[None] * d_mean[None] + D * d_invstd[None])
    cap = (T + 32) * U * B
    return torch.minimum((T + 18) * U * B + S, cap), cap


def ill_posed_pairs(case, cf, bound):
    """(N, C) mask of the (pillar, channel) pairs where a float32 evaluation may legitimately select another slot or another side
    of the ReLU than float64 does: the gap between the two best candidates (the live slots' pre-ReLU values and, with
    num_points < T, ONE padding candidate), or the best one's distance from 0, is below twice the forward bound."""
    y, live = cf["y"], cf["live"]
    N, T, C = y.shape
    num = live.sum(1)
    slot = torch.arange(T)[None, :, None]
    keep = live[:, :, None] | (slot == num[:, None, None])    # the live slots and the first padding slot
    cand = torch.where(keep, y, torch.full((), -float("inf"), dtype=y.dtype))
    top = torch.topk(cand, min(2, T), dim=1)[0]
    best = top[:, 0]
    gap = best - top[:, 1] if T > 1 else torch.full_like(best, float("inf"))
    return (gap < 2 * bound) | (best.abs() < 2 * bound)
