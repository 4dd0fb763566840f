"""The train-mode BatchNorm + ReLU passes (csrc/bn_train.hip: sparse table, dense map, the split SyncBN form) and the fused SSFA
attention tail (csrc/ssfa_train.hip) on the device against float64 references written from the formulas, per element, inside the
DERIVED bounds of tests/bn_train_ref.py. tests/test_bn_train_ref_cpu.py shows without a GPU that a float32 restatement of the kernels
meets every bound and that single defects (a float32 variance, a missing n / (n - 1), a dropped block partial, the rank-local N, the
attention weights exchanged) leave them by factors of 50 to 1e8.

The shapes are the smallest that reach each branch, and each case that names a branch asserts it from the restated block rule
(R.sparse_blocks, R.plane_slices, R.dot_blocks): C = 1 .. 256 (VEC 1 and 4, Q 1 .. 64, finisher G 256 .. 1); n = 0, 1, 2, 127 (one
empty block), 128 (every block live), 129 (63 empty blocks, a one-row last live block), 3001; *n_dev past the capacity; one quad and 15 empty slices; a
264-quad slice (second thread-stride pass); the last counter word at C = 1024; 260 dot blocks (second finisher pass). Input families:
ordinary, |mean| >> std, a constant channel, 90 % exact zeros.

Every raw call: the counter region of the workspace is read back and is all zero. Every kernel runs twice: equal bits. Every case
prints its worst error / bound per output and the running worst of its family. Measured on the MI355X: sparse table 0.864 (y), 0.854
(dx), 0.996 on the outputs that are one cast of a float64 value; dense map 0.828 (y), 0.999; two ranks 0.793 (y), 0.94; SSFA stage A
0.666 (smap), 0.445 (dzmap); stage B 0.708 (stats), 0.510 (out)."""
import pytest
import torch

import bn_train_ref as R
from sessd_hip import lib, ops
from sessd_hip._lib import SessdError, check

pytestmark = pytest.mark.gpu

_WORST = {}


def _note(family, what, r):
    w = max(r.values())
    _WORST[family] = max(_WORST.get(family, 0.0), w)
    print("%s | %s: %s | worst of the family so far %.3f" % (family, what, {k: round(v, 3) for k, v in r.items()}, _WORST[family]))
    assert w <= 1.0, (family, what, r)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes, dev):
    return torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)


def _counters_zero(ws, nbytes):
    torch.cuda.synchronize()
    return int(ws[:nbytes].to(torch.int64).sum()) == 0


def _cpu(d):
    return {k: v.detach().cpu() for k, v in d.items()}


def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ---- sparse table -----------------------------------------------------------------------------------------------------------------------

def _sparse_table(x, dy, cap, fill=1e6):
    n, C = x.shape
    xf, dyf = torch.full((cap, C), fill), torch.full((cap, C), -3.0)
    xf[:n], dyf[:n] = x, dy
    return xf, dyf


def _sparse_raw(dev, xf, dyf, n_dev_value, g, b, relu, rm0, rv0, ws):
    """sessd_bn_relu_train_fwd, then _bwd, on a table of cap rows; the counter words are checked after each call"""
    cap, C = xf.shape
    xd, dyd, gd, bd = xf.to(dev), dyf.to(dev), g.to(dev), b.to(dev)
    nd = torch.tensor([n_dev_value], dtype=torch.int32, device=dev)
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    y, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    mean, invstd, dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(4))
    check(lib.sessd_bn_relu_train_fwd(xd.data_ptr(), nd.data_ptr(), cap, C, gd.data_ptr(), bd.data_ptr(), R.EPS, R.MOMENTUM, int(relu),
                                      rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _st()), "fwd")
    assert _counters_zero(ws, 256)
    check(lib.sessd_bn_relu_train_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), nd.data_ptr(), cap, C, gd.data_ptr(), mean.data_ptr(),
                                      invstd.data_ptr(), int(relu), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _st()), "bwd")
    assert _counters_zero(ws, 256)
    return _cpu(dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dg, dbeta=db))


def _valid(full, n):
    """the outputs over the valid rows; rows >= n of y and dx must be exact zeros"""
    assert float(full["y"][n:].abs().sum()) == 0 and float(full["dx"][n:].abs().sum()) == 0
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    return dict(full, y=full["y"][:n], dx=full["dx"][:n])


def _sparse_case(dev, C, n, cap, fam, relu):
    x, g, b, dy = R.family_rows(fam, n, C, 1)
    rm0, rv0 = R.running_init(C)
    xf, dyf = _sparse_table(x, dy, cap)
    ws = _ws(lib.sessd_bn_relu_train_workspace_bytes(C), dev)
    full = _sparse_raw(dev, xf, dyf, n, g, b, relu, rm0, rv0, ws)
    assert _same_bits(full, _sparse_raw(dev, xf, dyf, n, g, b, relu, rm0, rv0, ws))
    got = _valid(full, n)
    r, st = R.check_bn(x, g, b, dy, relu, rm0, rv0, got)
    _note("sparse", "C %d n %d cap %d %s relu %d" % (C, n, cap, fam, relu), r)
    return got, st, (x, g, b, dy, rm0, rv0)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C,n,cap,fam", R.SPARSE_CASES)
def test_sparse_table_against_float64(dev, C, n, cap, fam, relu):
    assert cap > n
    got, st, (x, g, b, dy, rm0, rv0) = _sparse_case(dev, C, n, cap, fam, relu)
    chunk, spans = R.sparse_blocks(n)
    if n == 0:
        assert R.live(spans) == []
        assert torch.equal(got["running_mean"], rm0) and torch.equal(got["running_var"], rv0)       # bit for bit
        assert float(got["dgamma"].abs().max()) == 0 and float(got["dbeta"].abs().max()) == 0
        assert float(got["mean"].abs().max()) == 0
    elif n == 1:
        assert torch.equal(got["y"], (b.clamp_min(0) if relu else b).view(1, C))                   # y = relu(beta)
        want = (1 - R.f32(R.MOMENTUM)) * rv0.double()                                                # towards 0: the biased value
        assert float((got["running_var"].double() - want).abs().max()) <= 2 * R.U * float(want.abs().max())
    elif n == 127:
        assert chunk == 1 and len(R.live(spans)) == 127
    elif n == 128:
        assert chunk == 1 and spans[127] == (127, 128)                 # the last block's partial counts
    elif n == 129:
        assert chunk == 2 and R.live(spans) == [2] * 64 + [1]
    if fam == "constant":
        assert float(st["var"][-1]) == 0.0
    if fam == "offset":
        assert float((st["mu"].abs() / st["var"].sqrt()).min()) > 30.0


@pytest.mark.parametrize("C", [1, 4, 64])
def test_sparse_row_count_past_the_capacity_is_clamped(dev, C):
    """*n_dev = cap + 7 gives the bits of n = cap"""
    cap = 133
    x, g, b, dy = R.family_rows("ordinary", cap, C, 4)
    rm0, rv0 = R.running_init(C)
    ws = _ws(lib.sessd_bn_relu_train_workspace_bytes(C), dev)
    a = _sparse_raw(dev, x, dy, cap, g, b, True, rm0, rv0, ws)
    c = _sparse_raw(dev, x, dy, cap + 7, g, b, True, rm0, rv0, ws)
    assert _same_bits(a, c)
    r, _ = R.check_bn(x, g, b, dy, True, rm0, rv0, c)
    _note("sparse", "C %d *n_dev = cap + 7" % C, r)


def _bn_module(cls, C, g, b, rm0, rv0, dev):
    bn = cls(C, eps=R.EPS, momentum=R.MOMENTUM).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(g); bn.bias.copy_(b); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    return bn


@pytest.mark.parametrize("C,n,fam", [(1, 129, "ordinary"), (64, 3001, "offset"), (4, 0, "ordinary"), (256, 1, "ordinary")])
def test_sparse_table_through_autograd(dev, C, n, fam):
    """ops.bn_relu_train: the same bounds through BnReluTrainFunction; the cached workspace's counter words are zero afterwards"""
    cap = n + 5
    x, g, b, dy = R.family_rows(fam, n, C, 1)
    rm0, rv0 = R.running_init(C)
    xf, dyf = _sparse_table(x, dy, cap)
    bn = _bn_module(torch.nn.BatchNorm1d, C, g, b, rm0, rv0, dev)
    xd = xf.to(dev).requires_grad_(True)
    nd = torch.tensor([n], dtype=torch.int32, device=dev)
    y = ops.bn_relu_train(xd, nd, bn, relu=True)
    y.backward(dyf.to(dev))
    assert _counters_zero(ops.zeroed_workspace(lib.sessd_bn_relu_train_workspace_bytes(C), dev, "bn"), 256)
    full = _cpu(dict(y=y, running_mean=bn.running_mean, running_var=bn.running_var, dx=xd.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad))
    st = R.bn_forward_reference(x, g, b, True)
    full.update(mean=st["mu"].float(), invstd=st["invstd"].float())     # not handed out by the autograd form
    r, _ = R.check_bn(x, g, b, dy, True, rm0, rv0, _valid(full, n))
    _note("sparse", "ops.bn_relu_train C %d n %d %s" % (C, n, fam), r)
    assert int(bn.num_batches_tracked) == 1


def test_sparse_channel_count_that_is_no_power_of_two_raises(dev):
    x = torch.randn(40, 24, device=dev)
    nd = torch.tensor([40], dtype=torch.int32, device=dev)
    bn = torch.nn.BatchNorm1d(24, eps=R.EPS, momentum=R.MOMENTUM).to(dev).train()
    with pytest.raises(SessdError):
        ops.bn_relu_train(x, nd, bn)
    y = torch.full_like(x, float("nan"))
    m = torch.full((24,), float("nan"), device=dev)
    ws = _ws(lib.sessd_bn_relu_train_workspace_bytes(32), dev)
    rc = lib.sessd_bn_relu_train_fwd(x.data_ptr(), nd.data_ptr(), 40, 24, bn.weight.data_ptr(), bn.bias.data_ptr(), R.EPS, R.MOMENTUM, 1,
                                     None, None, y.data_ptr(), m.data_ptr(), m.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(y).all()) and bool(torch.isnan(m).all())


# ---- dense map ------------------------------------------------------------------------------------------------------------------------

def _dense_raw(dev, x, dy, g, b, relu, rm0, rv0, ws):
    """sessd_bn2d_relu_train_fwd, then sessd_bn2d_relu_train_bwd with the mask read from y"""
    B, C, H, W = x.shape
    xd, dyd, gd, bd = x.to(dev), dy.to(dev), g.to(dev), b.to(dev)
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    y, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    mean, invstd, dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(4))
    check(lib.sessd_bn2d_relu_train_fwd(xd.data_ptr(), B, C, H * W, gd.data_ptr(), bd.data_ptr(), R.EPS, R.MOMENTUM, int(relu),
                                        rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _st()), "fwd")
    assert _counters_zero(ws, 4096)
    check(lib.sessd_bn2d_relu_train_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), B, C, H * W, gd.data_ptr(), mean.data_ptr(),
                                        invstd.data_ptr(), int(relu), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _st()), "bwd")
    assert _counters_zero(ws, 4096)
    return _cpu(dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dg, dbeta=db))


def _as_rows(got):
    return dict(got, y=R.rows(got["y"]), dx=R.rows(got["dx"]))


def _dense_ops(dev, x, dy, g, b, relu, rm0, rv0):
    """ops.bn2d_relu_train through autograd: the default backward re-derives the mask from x"""
    bn = _bn_module(torch.nn.BatchNorm2d, x.shape[1], g, b, rm0, rv0, dev)
    xd = x.to(dev).requires_grad_(True)
    y = ops.bn2d_relu_train(xd, bn, relu)
    y.backward(dy.to(dev))
    return _cpu(dict(y=y, running_mean=bn.running_mean, running_var=bn.running_var, dx=xd.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape,fam", R.DENSE_CASES)
def test_dense_map_against_float64(dev, shape, fam, relu):
    B, C, H, W = shape
    chunk, sl = R.plane_slices(H * W)
    if shape == (1, 1, 2, 2):
        assert R.live(sl) == [1]
    elif shape == (3, 24, 6, 10):
        assert R.live(sl) == [1] * 15
    elif shape == (2, 5, 4, 9):
        assert R.live(sl) == [1] * 9 and C % 2 == 1
    elif shape == (1, 2, 128, 132):
        assert chunk == 264 > 256
    else:
        assert C == 1024 == int(lib.sessd_bn2d_relu_train_workspace_bytes(0)) // 4
    x, g, b, dy = R.dense_inputs(shape, fam)
    rm0, rv0 = R.running_init(C)
    ws = _ws(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev)
    raw = _dense_raw(dev, x, dy, g, b, relu, rm0, rv0, ws)
    assert _same_bits(raw, _dense_raw(dev, x, dy, g, b, relu, rm0, rv0, ws))
    r, st = R.check_bn(R.rows(x), g, b, R.rows(dy), relu, rm0, rv0, _as_rows(raw))
    _note("dense", "%s %s relu %d, mask from y" % (shape, fam, relu), r)
    assert ops.BN_MASK_FROM_X
    viaops = _dense_ops(dev, x, dy, g, b, relu, rm0, rv0)
    assert _counters_zero(ops.zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev, "bn2d"), 4096)
    assert all(torch.equal(viaops[k], raw[k]) for k in viaops)          # the mask from x: the same bits as the mask from y
    if fam == "constant":
        assert float(st["var"][-1]) == 0.0


def test_dense_workspace_serves_another_channel_count(dev):
    """C = 1024 (the last counter word), then the same workspace at C = 3"""
    ws = _ws(lib.sessd_bn2d_relu_train_workspace_bytes(1024), dev)
    for shape in ((1, 1024, 2, 2), R.DENSE_REUSE):
        x, g, b, dy = R.dense_inputs(shape, "ordinary")
        rm0, rv0 = R.running_init(shape[1])
        raw = _dense_raw(dev, x, dy, g, b, True, rm0, rv0, ws)
        r, _ = R.check_bn(R.rows(x), g, b, R.rows(dy), True, rm0, rv0, _as_rows(raw))
        _note("dense", "%s in the workspace of C = 1024" % (shape,), r)
    assert R.DENSE_REUSE[1] == 3


@pytest.mark.parametrize("shape", R.DENSE_FALLBACK)
def test_dense_shapes_outside_the_kernel_take_the_torch_fallback_and_meet_the_reference(dev, shape):
    """More than 1024 channels, a plane that is no multiple of 4: torch's own BatchNorm accumulates in float32, so the same
    derivation holds with gamma in place of gamma64 (acc=R.U)."""
    B, C, H, W = shape
    assert C > ops.BN2D_MAX_CHANNELS or (H * W) % 4
    x, g, b, dy = R.dense_inputs(shape, "ordinary")
    rm0, rv0 = R.running_init(C)
    got = _dense_ops(dev, x, dy, g, b, True, rm0, rv0)
    st = R.bn_forward_reference(R.rows(x), g, b, True, acc=R.U)
    got.update(mean=st["mu"].float(), invstd=st["invstd"].float())
    r, _ = R.check_bn(R.rows(x), g, b, R.rows(dy), True, rm0, rv0, _as_rows(got), acc=R.U)
    _note("dense fallback", "%s" % (shape,), r)


# ---- two ranks in one process: the split entry points, the float64 totals added with torch ---------------------------------------------

def _sync_sparse(dev, xs, dys, caps, g, b, relu, rm0, rv0):
    C = g.numel()
    gd, bd = g.to(dev), b.to(dev)
    ws = _ws(lib.sessd_bn_relu_train_workspace_bytes(C), dev)
    ranks = []
    for x, dy, cap in zip(xs, dys, caps):
        xf, dyf = _sparse_table(x, dy, cap)
        k = dict(x=xf.to(dev), dy=dyf.to(dev), n=torch.tensor([x.shape[0]], dtype=torch.int32, device=dev), cap=cap,
                 sums=torch.full((2 * C + 1,), float("nan"), dtype=torch.float64, device=dev),
                 bsums=torch.full((2 * C,), float("nan"), dtype=torch.float64, device=dev),
                 rm=rm0.clone().to(dev), rv=rv0.clone().to(dev), y=torch.full((cap, C), float("nan"), device=dev),
                 dx=torch.full((cap, C), float("nan"), device=dev))
        for name in ("mean", "invstd", "dg", "db"):
            k[name] = torch.full((C,), float("nan"), device=dev)
        ranks.append(k)
    for k in ranks:
        check(lib.sessd_bn_relu_train_stats(k["x"].data_ptr(), k["n"].data_ptr(), k["cap"], C, k["sums"].data_ptr(), ws.data_ptr(),
                                            ws.numel(), _st()), "stats")
        assert _counters_zero(ws, 256)
    total = sum(k["sums"] for k in ranks)                         # the all-reduce
    for k in ranks:
        check(lib.sessd_bn_relu_train_apply(k["x"].data_ptr(), k["n"].data_ptr(), k["cap"], C, gd.data_ptr(), bd.data_ptr(), R.EPS,
                                            R.MOMENTUM, int(relu), total.data_ptr(), k["rm"].data_ptr(), k["rv"].data_ptr(),
                                            k["y"].data_ptr(), k["mean"].data_ptr(), k["invstd"].data_ptr(), _st()), "apply")
        check(lib.sessd_bn_relu_train_bwd_stats(k["dy"].data_ptr(), k["x"].data_ptr(), k["y"].data_ptr(), k["n"].data_ptr(), k["cap"], C,
                                                k["mean"].data_ptr(), k["invstd"].data_ptr(), int(relu), k["dg"].data_ptr(),
                                                k["db"].data_ptr(), k["bsums"].data_ptr(), ws.data_ptr(), ws.numel(), _st()), "bwd_stats")
        assert _counters_zero(ws, 256)
    btotal = sum(k["bsums"] for k in ranks)
    scratch = _ws(lib.sessd_bn_sync_scratch_bytes(C), dev)
    outs = []
    for k in ranks:
        check(lib.sessd_bn_relu_train_bwd_apply(k["dy"].data_ptr(), k["x"].data_ptr(), k["y"].data_ptr(), k["n"].data_ptr(), k["cap"], C,
                                                gd.data_ptr(), k["mean"].data_ptr(), k["invstd"].data_ptr(), int(relu), btotal.data_ptr(),
                                                total.data_ptr(), k["dx"].data_ptr(), scratch.data_ptr(), scratch.numel(), _st()),
              "bwd_apply")
        n = int(k["n"])
        outs.append(_valid(_cpu(dict(y=k["y"], mean=k["mean"], invstd=k["invstd"], running_mean=k["rm"], running_var=k["rv"],
                                     dx=k["dx"], dgamma=k["dg"], dbeta=k["db"])), n))
    return outs


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C,n0,n1", R.SYNC_SPARSE)
def test_two_ranks_sparse_equal_the_concatenated_batch(dev, C, n0, n1, relu):
    """An empty rank gets the global mean and invstd, updates its running statistics with the global n and writes only zeros."""
    x, g, b, dy = R.family_rows("ordinary", n0 + n1, C, 2)
    rm0, rv0 = R.running_init(C)
    xs, dys = [x[:n0], x[n0:]], [dy[:n0], dy[n0:]]
    outs = _sync_sparse(dev, xs, dys, [n0 + 3, n1 + 8], g, b, relu, rm0, rv0)
    again = _sync_sparse(dev, xs, dys, [n0 + 3, n1 + 8], g, b, relu, rm0, rv0)
    assert all(_same_bits(a, c) for a, c in zip(outs, again))
    r = R.check_bn_sync(xs, g, b, dys, relu, rm0, rv0, outs)
    _note("two ranks", "sparse C %d, %d + %d rows, relu %d" % (C, n0, n1, relu), r)
    for k in ("mean", "invstd", "running_mean", "running_var"):
        assert torch.equal(outs[0][k], outs[1][k])
    if n1 == 0:
        assert float(outs[1]["dgamma"].abs().max()) == 0 and float(outs[1]["dbeta"].abs().max()) == 0
        assert not torch.equal(outs[1]["running_mean"], rm0)


@pytest.mark.parametrize("C,H,W,b0,b1", R.SYNC_DENSE)
def test_two_ranks_dense_equal_the_concatenated_batch(dev, C, H, W, b0, b1):
    x, g, b, dy = R.dense_inputs((b0 + b1, C, H, W), "ordinary", seed=2)
    rm0, rv0 = R.running_init(C)
    gd, bd = g.to(dev), b.to(dev)
    ws = _ws(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev)
    plane = H * W

    def run():
        ranks = []
        for lo, hi in ((0, b0), (b0, b0 + b1)):
            k = dict(x=x[lo:hi].contiguous().to(dev), dy=dy[lo:hi].contiguous().to(dev), B=hi - lo,
                     sums=torch.full((2 * C + 1,), float("nan"), dtype=torch.float64, device=dev),
                     bsums=torch.full((2 * C,), float("nan"), dtype=torch.float64, device=dev), rm=rm0.clone().to(dev), rv=rv0.clone().to(dev))
            k["y"], k["dx"] = torch.full_like(k["x"], float("nan")), torch.full_like(k["x"], float("nan"))
            for name in ("mean", "invstd", "dg", "db"):
                k[name] = torch.full((C,), float("nan"), device=dev)
            ranks.append(k)
        for k in ranks:
            check(lib.sessd_bn2d_relu_train_stats(k["x"].data_ptr(), k["B"], C, plane, k["sums"].data_ptr(), ws.data_ptr(), ws.numel(), _st()), "stats")
            assert _counters_zero(ws, 4096)
        total = sum(k["sums"] for k in ranks)
        for k in ranks:
            check(lib.sessd_bn2d_relu_train_apply(k["x"].data_ptr(), k["B"], C, plane, gd.data_ptr(), bd.data_ptr(), R.EPS, R.MOMENTUM, 1,
                                                  total.data_ptr(), k["rm"].data_ptr(), k["rv"].data_ptr(), k["y"].data_ptr(),
                                                  k["mean"].data_ptr(), k["invstd"].data_ptr(), _st()), "apply")
            check(lib.sessd_bn2d_relu_train_bwd_stats(k["dy"].data_ptr(), k["x"].data_ptr(), None, k["B"], C, plane, gd.data_ptr(), bd.data_ptr(),
                                                      k["mean"].data_ptr(), k["invstd"].data_ptr(), 1, k["dg"].data_ptr(), k["db"].data_ptr(),
                                                      k["bsums"].data_ptr(), ws.data_ptr(), ws.numel(), _st()), "bwd_stats")
            assert _counters_zero(ws, 4096)
        btotal = sum(k["bsums"] for k in ranks)
        scratch = _ws(lib.sessd_bn_sync_scratch_bytes(C), dev)
        outs = []
        for k in ranks:
            check(lib.sessd_bn2d_relu_train_bwd_apply(k["dy"].data_ptr(), k["x"].data_ptr(), None, k["B"], C, plane, gd.data_ptr(), bd.data_ptr(),
                                                      k["mean"].data_ptr(), k["invstd"].data_ptr(), 1, btotal.data_ptr(), total.data_ptr(),
                                                      k["dx"].data_ptr(), scratch.data_ptr(), scratch.numel(), _st()), "bwd_apply")
            outs.append(_as_rows(_cpu(dict(y=k["y"], mean=k["mean"], invstd=k["invstd"], running_mean=k["rm"], running_var=k["rv"],
                                           dx=k["dx"], dgamma=k["dg"], dbeta=k["db"]))))
        return outs

    outs, again = run(), run()
    assert all(_same_bits(a, c) for a, c in zip(outs, again))
    xs = [R.rows(x[:b0]), R.rows(x[b0:])]
    dys = [R.rows(dy[:b0]), R.rows(dy[b0:])]
    r = R.check_bn_sync(xs, g, b, dys, True, rm0, rv0, outs)
    _note("two ranks", "dense C %d %d x %d, %d + %d images" % (C, H, W, b0, b1), r)


# ---- SSFA tail ------------------------------------------------------------------------------------------------------------------------

SSFA_COUNTER_BYTES = 256 + 4096


def _ssfa_raw(dev, x0, x1, w0, w1, gb, grad, rm0, rv0, ws):
    B, C, H, W = x0.shape
    plane, n = H * W, B * H * W
    d = [t.to(dev) for t in (x0, x1, w0, w1, grad)]
    gbd = [torch.tensor([v], device=dev) for v in gb]
    rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, smap, stats, dz = nan(B, C, H, W), nan(2, n), nan(4), nan(n)
    dx0, dx1, dw0, dw1, dg, db = nan(B, C, H, W), nan(B, C, H, W), nan(C), nan(C), nan(2), nan(2)
    check(lib.sessd_ssfa_fuse_train_fwd(d[0].data_ptr(), d[1].data_ptr(), B, C, plane, d[2].data_ptr(), d[3].data_ptr(), gbd[0].data_ptr(),
                                        gbd[1].data_ptr(), gbd[2].data_ptr(), gbd[3].data_ptr(), R.EPS, R.MOMENTUM, rm[0:1].data_ptr(),
                                        rv[0:1].data_ptr(), rm[1:2].data_ptr(), rv[1:2].data_ptr(), out.data_ptr(), smap.data_ptr(),
                                        stats.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "ssfa fwd")
    assert _counters_zero(ws, SSFA_COUNTER_BYTES)
    check(lib.sessd_ssfa_fuse_train_bwd(d[4].data_ptr(), d[0].data_ptr(), d[1].data_ptr(), B, C, plane, d[2].data_ptr(), d[3].data_ptr(),
                                        gbd[0].data_ptr(), gbd[1].data_ptr(), gbd[2].data_ptr(), gbd[3].data_ptr(), smap.data_ptr(),
                                        stats.data_ptr(), dz.data_ptr(), dx0.data_ptr(), dx1.data_ptr(), dw0.data_ptr(), dw1.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "ssfa bwd")
    assert _counters_zero(ws, SSFA_COUNTER_BYTES)
    return _cpu(dict(smap=smap, stats=stats, out=out, running_mean=rm, running_var=rv, dzmap=dz, dx0=dx0, dx1=dx1, dw0=dw0, dw1=dw1,
                     dgamma=dg, dbeta=db))


SSFA_RUNNING = (torch.tensor([0.05, 0.1]), torch.tensor([0.7, 0.9]))


@pytest.mark.parametrize("shape,kind", R.SSFA_CASES)
def test_ssfa_tail_against_float64_in_two_stages(dev, shape, kind):
    B, C, H, W = shape
    nb, (chunk, sl) = R.dot_blocks(B, H * W), R.plane_slices(H * W)
    if shape == (2, 8, 6, 10):
        assert nb == 1 and B * H * W // 4 < 64                      # dead lanes in the only dot block
    elif shape == (3, 4, 4, 5):
        assert C // 4 == 1
    elif shape == (1, 4, 256, 260):
        assert nb == 260 > 256 and chunk > 256
    need = int(lib.sessd_ssfa_fuse_train_workspace_bytes(B, C, H * W))
    assert need == SSFA_COUNTER_BYTES + max(nb * 4, C * 16 * 2) * 8  # the two launches of the backward share the partials region
    x0, x1, w0, w1, gb, grad = R.ssfa_inputs(shape, kind)
    rm0, rv0 = SSFA_RUNNING
    ws = _ws(need, dev)
    got = _ssfa_raw(dev, x0, x1, w0, w1, gb, grad, rm0, rv0, ws)
    assert _same_bits(got, _ssfa_raw(dev, x0, x1, w0, w1, gb, grad, rm0, rv0, ws))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    r, fw = R.check_ssfa(x0, x1, w0, w1, gb, grad, rm0, rv0, got)
    _note("SSFA stage A", "%s %s" % (shape, kind), {k: v for k, v in r.items() if k.startswith("A.")})
    _note("SSFA stage B", "%s %s" % (shape, kind), {k: v for k, v in r.items() if k.startswith("B.")})
    assert bool(got["dbeta"][1] == -got["dbeta"][0])
    z = fw["att"]["z"]
    if kind == "saturated":
        assert float((z[0] - z[1]).abs().max()) > 30.0
    if kind == "equal":
        assert torch.equal(got["smap"][0], got["smap"][1]) and float((fw["att"]["a"] - 0.5).abs().max()) < 0.45


def test_ssfa_tail_through_autograd_gives_the_entry_points_bits(dev):
    """ops.ssfa_fuse_train: output, running statistics and every gradient are the raw calls' bits, each on the right parameter"""
    shape, kind = (1, 64, 20, 12), "plain"
    B, C, H, W = shape
    x0, x1, w0, w1, gb, grad = R.ssfa_inputs(shape, kind)
    rm0, rv0 = SSFA_RUNNING
    raw = _ssfa_raw(dev, x0, x1, w0, w1, gb, grad, rm0, rv0, _ws(lib.sessd_ssfa_fuse_train_workspace_bytes(B, C, H * W), dev))
    mods = []
    for k, w in enumerate((w0, w1)):
        conv = torch.nn.Conv2d(C, 1, 1, bias=False).to(dev)
        bn = torch.nn.BatchNorm2d(1, eps=R.EPS, momentum=R.MOMENTUM).to(dev).train()
        with torch.no_grad():
            conv.weight.copy_(w.view(1, C, 1, 1))
            bn.weight.fill_(gb[2 * k]); bn.bias.fill_(gb[2 * k + 1]); bn.running_mean.fill_(float(rm0[k])); bn.running_var.fill_(float(rv0[k]))
        mods += [conv, bn]
    a0, a1 = x0.to(dev).requires_grad_(True), x1.to(dev).requires_grad_(True)
    out = ops.ssfa_fuse_train(a0, a1, *mods)
    out.backward(grad.to(dev))
    assert _counters_zero(ops.zeroed_workspace(lib.sessd_ssfa_fuse_train_workspace_bytes(B, C, H * W), dev, "ssfa_train"), SSFA_COUNTER_BYTES)
    assert torch.equal(out.detach().cpu(), raw["out"])
    assert torch.equal(a0.grad.cpu(), raw["dx0"]) and torch.equal(a1.grad.cpu(), raw["dx1"])
    for k in range(2):
        conv, bn = mods[2 * k], mods[2 * k + 1]
        assert torch.equal(conv.weight.grad.cpu().view(-1), raw["dw%d" % k])
        assert torch.equal(bn.weight.grad.cpu(), raw["dgamma"][k:k + 1]) and torch.equal(bn.bias.grad.cpu(), raw["dbeta"][k:k + 1])
        assert torch.equal(bn.running_mean.cpu(), raw["running_mean"][k:k + 1]) and torch.equal(bn.running_var.cpu(), raw["running_var"][k:k + 1])
        assert int(bn.num_batches_tracked) == 1
