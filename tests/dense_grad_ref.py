"""float64 references and DERIVED error bounds for the dense conv gradients (csrc/dense_grad.hip, csrc/dense_wino_wgrad.hip,
ops.Conv2dFunction, ops.channel_sum). No GPU is needed here: tests/test_dense_grad_ref_cpu.py checks that the bounds can be met and
are not vacuous, tests/test_dense_grad_f64_gpu.py holds the kernels to them.

Notation: u = 2^-24 (float32 unit roundoff), gamma(n) = n u / (1 - n u): a result that went through n float32 roundings on its
longest path differs from the exact one by at most gamma(n) times the ABSOLUTE-VALUE IMAGE of the computation (the same computation
with every input, every transform matrix and every subtraction replaced by its absolute value: no cancellation). gamma, not n u:
the two differ once n^2 u is no longer small.

DIRECT BOUND (wgrad_reference, module_reference, channel_sum_reference): the f32 MFMA kernels -- sessd_conv2d_wgrad's three kernels with their ordered chunk sums, the forward
kernels of sessd_conv2d_mfma that carry the data gradients, sessd_nchw_channel_sum. bound = gamma(K + 2) A, A = the same gradient in
float64 on |x|, |w|, |gout|, K = the number of products of one entry: B Hout Wout (weight gradient), 9 cout / cout (3x3 / 1x1 data
gradient), 9 cin / cin (+ 1 with a bias: the forward), B H W (bias gradient). An f32 fma chain of K terms added in any order, or cut
into partial sums that are added afterwards, has at most K roundings on any path; + 2 for what an MFMA may round inside one
instruction (its two products are added before they meet the accumulator).

WINOGRAD BOUND, weight gradient (wino_wgrad_bound; the count follows csrc/dense_wino_wgrad.hip line by line):
    dM = A dY A^T      SESSD_WW_TRANSFORM: r1 = gy[0] + gy[1] (1), rows[a].x + rows[a].y (1)                          2
    V  = B^T d B       SESSD_WW_TRANSFORM: tl[0] = pr[0].xy - pr[2].xy (1), tl[a].x - tr[a].x (1)                     2
    dU = sum dM V      v_mfma_f32_32x32x2f32 over the tiles of a chunk, then wino_wgrad_reduce_kernel's u[xi] += v[xi]
                       over the chunks: no path is longer than T + nchunks, T = B (H / 2) (W / 2) tiles              T + nchunks
                       (+ 2 inside the MFMA, as above)                                                                2
    dg = G^T dU G      wino_wgrad_reduce_kernel: hs = 0.5f * (u[4 + col] + u[8 + col]) (1; the product with 0.5 is exact),
                       t[0][col] = u[col] + hs (1); the same two for the columns                                      4
    n = T + nchunks + 10. The two operands of a product carry 2 roundings each and MULTIPLY, which is (1 + d)^4: counted as 4.
    Absolute image: |G^T| ( sum over tiles of (|A| |dY| |A^T|) . (|B^T| |d| |B|) ) |G|.

WINOGRAD BOUND, stream-K forward, tile_cfg 22 = shape 0 (wino_forward_bound; csrc/dense_wino_sk.hip, winograd_pack_body of
csrc/dense_conv.hip) -- the forward and, with the flipped, channel-swapped weight, the data gradient of a 3x3 stride-1 layer:
    U = G g G^T        winograd_pack_body: float64 arithmetic, out[dst] = (float)u[b] (1); the six float64 roundings before it
                       are 2^-29 u each: counted as one more                                                          2
    V = B^T d B        SESSD_SK_TRANSFORM: tl[0] = pr[0].xy - pr[2].xy (1), tl[a].x - tr[a].x (1)                     2
    M = sum U V        SESSD_SK_MMA over cin channels (+ 2 inside the MFMA)                                           cin + 2
    Y = A^T M A        epilogue: q0[c] = m[c] + m[4 + c] + m[8 + c] (2), y[0] = q0[0] + q0[1] + q0[2] (2)             4
    cut units          a unit of rpu = cin / 16 rounds can be cut between workgroups rpu - 1 times; each cut adds two
                       already-transformed partial outputs, z = (0.f + y) + o4 (1 each; the transform is linear, so the
                       absolute image is the same)                                                                    cin / 16 - 1
    bias               SESSD_SK_FINALIZE: fmaf(Y, 1.f, shift) (1); without a bias fmaf(Y, 1.f, 0.f) is exact           1
    n = cin + cin / 16 + 10. Absolute image: |A^T| ( sum over cin of (|G| |g| |G^T|) . (|B^T| |d| |B|) ) |A| + |bias|.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(n):
    nu = n * U
    assert nu < 1.0
    return nu / (1.0 - nu)


def ratio(got, ref, bound):
    """Worst err / bound. The error must be finite; where bound == 0 the entry must be exactly 0."""
    err = (got.detach().cpu().double() - ref).abs()
    assert bool(torch.isfinite(err).all())
    if float(bound.min()) > 0:
        return float((err / bound).max())
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


# ---- float64 references ------------------------------------------------------------------------------------------------------------

def _layer(x, w, b, stride, transposed):
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=stride, padding=w.shape[-1] // 2)


def _grads(x, w, b, gout, stride, transposed):
    """(y, gx, gw, gb) of the layer, float64, by torch.autograd.grad against gout"""
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = None if b is None else b.clone().requires_grad_(True)
    y = _layer(x, w, b, stride, transposed)
    g = torch.autograd.grad(y, (x, w) if b is None else (x, w, b), gout)
    return y.detach(), g[0], g[1], (g[2] if b is not None else None)


def wgrad_reference(inp, gout, k, stride):
    """(gw, bound) of ops.conv2d_wgrad(inp, gout, k, stride): Conv2d(k, stride, padding k // 2); float64; direct bound."""
    B, ci = inp.shape[:2]
    co, ho, wo = gout.shape[1:]
    z = torch.zeros(co, ci, k, k, dtype=torch.float64)
    gw = _grads(inp.double(), z, None, gout.double(), stride, False)[2]
    aw = _grads(inp.double().abs(), z, None, gout.double().abs(), stride, False)[2]
    return gw, gamma(B * ho * wo + 2) * aw


def module_reference(x, w, bias, gout, stride, transposed):
    """Conv2d(k, stride, padding k // 2) / ConvTranspose2d(3, 2, 1, 1) with weight w: ({y, gx, gw, gb}, the same keys' direct bounds)."""
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    ref = _grads(d(x), d(w), d(bias), d(gout), stride, transposed)
    ab = _grads(a(x), a(w), a(bias), a(gout), stride, transposed)
    taps = w.shape[-1] ** 2
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    B = x.shape[0]
    small = x if transposed else gout       # the map whose pixels the weight gradient sums over
    K = dict(y=taps * cin + (bias is not None), gx=taps * cout, gw=B * small.shape[2] * small.shape[3],
             gb=B * gout.shape[2] * gout.shape[3])
    keys = ("y", "gx", "gw", "gb")
    return ({k: v for k, v in zip(keys, ref) if v is not None},
            {k: gamma(K[k] + 2) * v for k, v in zip(keys, ab) if v is not None})


def channel_sum_reference(x):
    return x.double().sum((0, 2, 3)), gamma(x.shape[0] * x.shape[2] * x.shape[3] + 2) * x.double().abs().sum((0, 2, 3))


# ---- the entry points' chunk rules, restated (a change of the rule must fail the tests that name a branch) ----------------------------

def direct_chunks(B, cin, cout, hout, k, stride):
    """sessd_conv2d_wgrad: (kernel, nchunks, rows_per_chunk, tiles); kernel in {"1x1_64", "s2_lds", "general"}."""
    rows = B * hout
    if k == 1 and cin >= 64 and cout >= 64:
        kernel, tiles, budget, cap = "1x1_64", -(-cout // 64) * -(-cin // 64), 1024, 256
    elif k == 3 and stride == 2 and cin % 64 == 0 and cout % 64 == 0:
        kernel, tiles, budget, cap = "s2_lds", (cout // 64) * (cin // 64), 512, 64
    else:
        kernel, tiles, budget, cap = "general", -(-cout // 32) * -(-cin // 32), 2048, 64
    n = min(max(budget // tiles, 8), cap, rows)
    rpc = -(-rows // n)
    return kernel, -(-rows // rpc), rpc, tiles


def wino_wgrad_chunks(B, cin, cout, H, W):
    """sessd_conv3x3_wgrad_winograd (ww_chunks): (stages of 8 tiles, nchunks); chunk c owns stages [c S / n, (c + 1) S / n)."""
    stages = -(-(B * (H // 2) * (W // 2)) // 8)
    n = min(256 // ((cin // 64) * (cout // 64)), 64, stages // 4)
    if n >= 8:
        n &= ~7
    return stages, max(n, 1)


# ---- F(2x2,3x3) as the kernels perform it; absolute=True gives the absolute-value image ----------------------------------------------

def _ops(absolute):
    if absolute:
        return (lambda a, b: a + b), (lambda a: a)
    return (lambda a, b: a - b), (lambda a: -a)


def _patches(x):
    """(B, C, H, W) -> the 4x4 input patches of the 2x2 output tiles, zero padded: (B, C, H / 2, W / 2, 4, 4)"""
    return F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)


def _bt_d_b(p, absolute):
    sub, _ = _ops(absolute)
    r = torch.stack([sub(p[..., 0, :], p[..., 2, :]), p[..., 1, :] + p[..., 2, :], sub(p[..., 2, :], p[..., 1, :]),
                     sub(p[..., 1, :], p[..., 3, :])], -2)
    return torch.stack([sub(r[..., 0], r[..., 2]), r[..., 1] + r[..., 2], sub(r[..., 2], r[..., 1]), sub(r[..., 1], r[..., 3])], -1)


def _a_dy_at(g, absolute):
    """(..., 2, 2) -> (..., 4, 4): rows g0, g0 + g1, g0 - g1, -g1, then the same for the columns"""
    sub, neg = _ops(absolute)
    r = torch.stack([g[..., 0, :], g[..., 0, :] + g[..., 1, :], sub(g[..., 0, :], g[..., 1, :]), neg(g[..., 1, :])], -2)
    return torch.stack([r[..., 0], r[..., 0] + r[..., 1], sub(r[..., 0], r[..., 1]), neg(r[..., 1])], -1)


def _gt_du_g(u, absolute):
    """(..., 4, 4) -> (..., 3, 3) as wino_wgrad_reduce_kernel: hs = 0.5 (u1 + u2), hd = 0.5 (u1 - u2); u0 + hs, hd, hs + u3"""
    sub, _ = _ops(absolute)

    def stage(v, dim):
        a, b, c, d = v.unbind(dim)
        hs, hd = 0.5 * (b + c), 0.5 * sub(b, c)
        return torch.stack([a + hs, hd, hs + d], dim)
    return stage(stage(u, -2), -1)


def _at_m_a(m, absolute):
    """(..., 4, 4) -> (..., 2, 2) as the stream-K epilogue: q0 = m0 + m1 + m2, q1 = m1 - m2 - m3, the same for the columns"""
    sub, _ = _ops(absolute)

    def stage(v, dim):
        a, b, c, d = v.unbind(dim)
        return torch.stack([a + b + c, sub(sub(b, c), d)], dim)
    return stage(stage(m, -2), -1)


def wino_wgrad(x, gout, dtype, absolute=False, nchunks=1):
    """The Winograd-domain weight gradient in `dtype`, tiles in the kernel's order (b, ty, tx), padded to stages of 8 and summed
    chunk by chunk, the chunk partials added in chunk order."""
    x, gout = x.to(dtype), gout.to(dtype)
    if absolute:
        x, gout = x.abs(), gout.abs()
    B, ci, H, W = x.shape
    co = gout.shape[1]
    V = _bt_d_b(_patches(x), absolute).permute(0, 2, 3, 1, 4, 5).reshape(-1, ci, 16)                                  # [tile][ci][xi]
    dM = _a_dy_at(gout.unfold(2, 2, 2).unfold(3, 2, 2), absolute).permute(0, 2, 3, 1, 4, 5).reshape(-1, co, 16)      # [tile][co][xi]
    T = V.shape[0]
    stages = -(-T // 8)
    dU = torch.zeros(co, ci, 16, dtype=dtype)
    for c in range(nchunks):
        t0, t1 = min(T, 8 * (c * stages // nchunks)), min(T, 8 * ((c + 1) * stages // nchunks))
        dU = dU + torch.einsum("tox,tcx->ocx", dM[t0:t1], V[t0:t1])
    return _gt_du_g(dU.reshape(co, ci, 4, 4), absolute)


def wino_wgrad_n(x, nchunks):
    B, _, H, W = x.shape
    return B * (H // 2) * (W // 2) + nchunks + 10


def wino_wgrad_bound(x, gout, nchunks):
    return gamma(wino_wgrad_n(x, nchunks)) * wino_wgrad(x, gout, torch.float64, absolute=True)


def _g_g_gt(w, absolute):
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
    if absolute:
        G, w = G.abs(), w.abs()
    return torch.einsum("ia,ocab,jb->ocij", G, w.double(), G)


def wino_forward(x, w, bias, dtype, absolute=False):
    """Conv2d(3, 1, 1) as the stream-K Winograd forward performs it: U = G g G^T in float64, rounded once to `dtype`."""
    U_ = _g_g_gt(w, absolute).to(dtype)
    x = x.to(dtype)
    if absolute:
        x = x.abs()
    B, ci, H, W = x.shape
    co = w.shape[0]
    V = _bt_d_b(_patches(x), absolute)                                    # (B, ci, th, tw, 4, 4)
    M = torch.einsum("ocij,bcyxij->boyxij", U_, V)
    Y = _at_m_a(M, absolute).permute(0, 1, 2, 4, 3, 5).reshape(B, co, H, W)
    if bias is not None:
        b = bias.to(dtype)
        Y = Y + (b.abs() if absolute else b).view(1, -1, 1, 1)
    return Y


def wino_forward_n(cin):
    return cin + cin // 16 + 10


def wino_forward_bound(x, w, bias=None):
    return gamma(wino_forward_n(x.shape[1])) * wino_forward(x, w, bias, torch.float64, absolute=True)


def adjoint_weight(w):
    """the weight of the stride-1 layer whose forward is this layer's data gradient: taps flipped, channels swapped"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def deconv_wgrad_reference(x, gout):
    """(gw (cin, cout, 3, 3), bound) of ConvTranspose2d(3, 2, 1, 1): x (B, cin, H, W), gout (B, cout, 2 H, 2 W); direct bound."""
    z = torch.zeros(x.shape[1], gout.shape[1], 3, 3, dtype=torch.float64)
    gw = _grads(x.double(), z, None, gout.double(), 2, True)[2]
    aw = _grads(x.double().abs(), z, None, gout.double().abs(), 2, True)[2]
    return gw, gamma(x.shape[0] * x.shape[2] * x.shape[3] + 2) * aw


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# ops.conv2d_wgrad(inp, gout, k, stride, winograd=False): id -> (k, stride, B, cin, cout, Hin, Win, (kernel, nchunks, rows per chunk)).
# 14a / 14b are the two ConvTranspose2d(3, 2, 1, 1) layers with the roles swapped: inp = the layer's grad_out (B, cout, 2 H, 2 W),
# gout = its input (B, cin, H, W), so "cin" here is the layer's cout and the result is the layer's (cin, cout, 3, 3) gradient.
WGRAD_CASES = {
    "1": (3, 1, 2, 6, 34, 5, 8, ("general", 10, 1)),
    "2": (3, 1, 3, 34, 6, 3, 24, ("general", 9, 1)),
    "3": (3, 1, 3, 2, 2, 23, 8, ("general", 35, 2)),
    "4": (3, 1, 1, 1, 1, 1, 8, ("general", 1, 1)),
    "5-odd": (3, 2, 2, 6, 34, 5, 16, ("general", 6, 1)),
    "5-even": (3, 2, 2, 6, 34, 6, 16, ("general", 6, 1)),
    "6": (3, 2, 1, 6, 34, 2, 48, ("general", 1, 1)),
    "7-small": (1, 1, 2, 6, 34, 5, 8, ("general", 10, 1)),
    "7-64x34": (1, 1, 2, 64, 34, 5, 8, ("general", 10, 1)),
    "8": (1, 1, 2, 64, 64, 5, 8, ("1x1_64", 10, 1)),
    "9": (1, 1, 2, 66, 98, 5, 24, ("1x1_64", 10, 1)),
    "10": (1, 1, 3, 64, 64, 87, 8, ("1x1_64", 131, 2)),
    "11": (3, 2, 2, 64, 64, 5, 16, ("s2_lds", 6, 1)),
    "12": (3, 2, 2, 64, 128, 6, 48, ("s2_lds", 6, 1)),
    "13-two-tiles": (3, 2, 3, 128, 64, 46, 16, ("s2_lds", 35, 2)),
    "13-wide": (3, 2, 3, 64, 64, 46, 48, ("s2_lds", 35, 2)),
    "14-lds": (3, 2, 2, 128, 64, 6, 16, ("s2_lds", 6, 1)),
    "14-general": (3, 2, 2, 34, 6, 6, 16, ("general", 6, 1)),
}


def out_hw(k, stride, hin, win):
    p = k // 2
    return (hin + 2 * p - k) // stride + 1, (win + 2 * p - k) // stride + 1


def wgrad_inputs(name):
    """(inp, gout) of a WGRAD_CASES entry: float32 standard normals from a seed of the case's own"""
    k, s, B, ci, co, hi, wi, _ = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(sorted(WGRAD_CASES).index(name) + 100)
    ho, wo = out_hw(k, s, hi, wi)
    return torch.randn(B, ci, hi, wi, generator=g), torch.randn(B, co, ho, wo, generator=g)


def chunk_props(B, hout, nchunks, rpc):
    """(rows of the last chunk, the chunks whose rows lie in two images)"""
    rows = B * hout
    straddle = [c for c in range(nchunks) if (c * rpc) // hout != (min(rows, (c + 1) * rpc) - 1) // hout]
    return rows - (nchunks - 1) * rpc, straddle


# ops.conv2d_wgrad(x, gout, 3, 1, winograd=True): (B, cin, cout, H, W) -> (stages, nchunks)
WINO_WGRAD_CASES = {
    (1, 64, 64, 2, 16): (1, 1),
    (5, 64, 64, 4, 18): (12, 3),
    (3, 64, 128, 6, 22): (13, 3),
    (2, 64, 64, 16, 32): (32, 8),
}


def wino_wgrad_inputs(B, cin, cout, H, W):
    g = torch.Generator().manual_seed(B * 1000 + cin + cout + H + W)
    return torch.randn(B, cin, H, W, generator=g), torch.randn(B, cout, H, W, generator=g)


# ops.conv2d_module: name -> (transposed, k, stride, cin, cout, bias, (B, H, W) of x, kernels of (y and gx, gw))
MODULE_CASES = {
    "conv3x3-s1-6-34": (False, 3, 1, 6, 34, False, (2, 5, 8), ("direct", "direct")),
    "conv3x3-s2-6-34": (False, 3, 2, 6, 34, False, (2, 6, 16), ("direct", "direct")),
    "deconv-6-34": (True, 3, 2, 6, 34, False, (2, 3, 8), ("direct", "direct")),
    "conv1x1-34-6-bias": (False, 1, 1, 34, 6, True, (2, 5, 8), ("direct", "direct")),
    "conv3x3-s1-16-32-winograd": (False, 3, 1, 16, 32, False, (1, 64, 64), ("winograd", "direct")),
    "conv3x3-s1-64-64-winograd": (False, 3, 1, 64, 64, False, (1, 64, 64), ("winograd", "winograd")),
}


def module_inputs(name):
    """(x, w, bias, gout) of a MODULE_CASES entry; the weight uniform with variance 1 / fan-in"""
    tr, k, s, ci, co, has_bias, (B, H, W), _ = MODULE_CASES[name]
    g = torch.Generator().manual_seed(sorted(MODULE_CASES).index(name) + 200)
    x = torch.randn(B, ci, H, W, generator=g)
    w = (torch.rand((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * 2 - 1) * (3.0 / (ci * k * k)) ** 0.5
    bias = torch.randn(co, generator=g) if has_bias else None
    ho, wo = (2 * H, 2 * W) if tr else out_hw(k, s, H, W)
    return x, w, bias, torch.randn(B, co, ho, wo, generator=g)


def module_bounds(name, x, w, bias, gout):
    """module_reference with the Winograd bounds put where MODULE_CASES says the Winograd kernels run"""
    tr, k, s, ci, co, _, (B, H, W), (data, wg) = MODULE_CASES[name]
    ref, bound = module_reference(x, w, bias, gout, s, tr)
    if data == "winograd":
        bound["y"] = wino_forward_bound(x, w, bias)
        bound["gx"] = wino_forward_bound(gout, adjoint_weight(w))
    if wg == "winograd":
        bound["gw"] = wino_wgrad_bound(x, gout, wino_wgrad_chunks(B, ci, co, H, W)[1])
    return ref, bound
