"""sessd_pillar_features (csrc/pillar.hip) alone: the PFN layer + scatter kernel against tests/pillars_ref.py run in float64 on the
same float32 inputs.

Bound (per element, derived, nothing measured). u = 2^-24. For pillar p and channel c let

    B = |scale_c| * sum_k |W_ck| * A_k + |shift_c|

with A_k = the pillar's max |value| over its live points for the raw columns x, y, z, r; 2 * max |coordinate| for the three
mean-centred columns; |centre| for the two centre columns; max |xyz| for the distance column. The kernel's error is at most
(T + 16) * u * B:
  * the mean of n <= T float32 values, summed in any order and divided once: (n + 2) * u * max |coordinate| relative to the
    column's size, which the mean-centred columns inherit (A_k = 2 * max covers |x - m| and the subtraction's rounding);
  * the dot product of K <= 10 terms adds at most 10 * u * sum_k |W_ck| A_k;
  * the affine (one multiply, one add) at most 2 * u * B;
  * max and relu are exact.
(n + 2) + 10 + 2 <= T + 14; the remaining 2 u cover the square root and the three products of the distance column and the two
operations of a centre column. vx, vy and the offsets are given to both sides as the SAME float32 values.

Pillars lie in distinct cells, as a voxelizer leaves them: B = 2 frames of ny = 8 x nx = 12 hold 192, so the N = 257 cases use
ny = 16 (the canvas test with duplicate cells would have no defined answer). Every case takes milliseconds."""
import numpy as np
import pytest
import torch

import pillars_ref as PR
from sessd_hip import lib, ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C = 64
BATCH, NX = 2, 12
SENT = -12345.0
GUARD = 64
F32 = lambda v: float(np.float32(v))
VX, VY, XO, YO = F32(0.2), F32(0.2), F32(0.2 / 2 + 0.0), F32(0.2 / 2 - 40.0)   # the reader's defaults, as float32


def make_case(seed, N, T, with_distance, ny=None, extra=5, small=False):
    """N live pillars (frames interleaved, distinct cells, (0, 0) and (ny - 1, nx - 1) taken) in N + extra rows: the padding slots
    hold NaN, the rows beyond N hold NaN points, an absurd point count and cells far outside the canvas."""
    rng = np.random.RandomState(seed)
    ny = (8 if N <= 192 else 16) if ny is None else ny
    total = BATCH * ny * NX
    assert N <= total
    ids = np.concatenate([[0, total - 1][:N], rng.permutation(total - 2)[:max(N - 2, 0)] + 1]).astype(np.int64)[:N]
    ids = ids[rng.permutation(N)]                 # the two frames' pillars interleaved
    b, cells = ids // (ny * NX), ids % (ny * NX)
    coors = np.stack([b, np.zeros(N, np.int64), cells // NX, cells % NX], 1)
    kinds = sorted({1, max(T - 1, 1), T})
    num = np.array([kinds[i % len(kinds)] for i in rng.permutation(N)])
    vox = rng.rand(N, T, 4) * np.array([70.4, 80.0, 4.0, 1.0]) + np.array([0.0, -40.0, -3.0, 0.0])
    cap = N + extra
    voxels = np.full((cap, T, 4), np.nan, np.float32)
    for i in range(N):
        voxels[i, :num[i]] = vox[i, :num[i]]
    num_cap = np.full(cap, 1 << 20, np.int32)
    num_cap[:N] = num
    coors_cap = np.full((cap, 4), -7, np.int32)
    coors_cap[:N] = coors
    K = 10 if with_distance else 9
    w = ((rng.rand(C, K) * 2 - 1) * (1e-6 if small else 0.6)).astype(np.float32)
    scale = ((rng.rand(C) + 0.5) * np.where(rng.rand(C) < 0.25, -1, 1)).astype(np.float32)
    shift = (rng.randn(C) * 2.0).astype(np.float32)   # both signs
    if small:
        w[:, 7] = 1e-2   # on the centre column fcx <= -0.1: every live slot's dot product is negative (the rest is < 4e-4)
        scale[:] = 1.0
        shift[:] = np.where(np.arange(C) % 2 == 0, 5.0, -0.5)
    return dict(N=N, T=T, cap=cap, ny=ny, dist=with_distance, voxels=voxels, num=num_cap, coors=coors_cap, w=w, scale=scale, shift=shift)


def reference(case):
    """float64 features (N, C) of the live rows and the per-element bound."""
    N, T = case["N"], case["T"]
    args = (case["voxels"][:N], case["num"][:N], case["coors"][:N])
    ref = PR.pillar_features(*args, case["w"], case["scale"], case["shift"], VX, VY, XO, YO, case["dist"], torch.float64)
    cols, _ = PR.pillar_columns(*args, VX, VY, XO, YO, case["dist"], torch.float64)
    raw = cols[:, :, :4].abs().amax(dim=1)                                  # (N, 4) max over the live slots (padding is 0)
    A = [raw, 2 * raw[:, :3], cols[:, 0, 7:9].abs()]
    if case["dist"]:
        A.append(cols[:, :, 9:10].abs().amax(dim=1))
    A = torch.cat(A, dim=1)                                                 # (N, K)
    w, s, t = (torch.from_numpy(case[k]).double() for k in ("w", "scale", "shift"))
    bound = (T + 16) * U * (s.abs()[None] * (A @ w.abs().t()) + t.abs()[None])
    return ref, bound


class Buffers:
    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        g = lambda k: torch.from_numpy(case[k]).to(dev)
        self.voxels, self.num, self.coors, self.w, self.scale, self.shift = (g(k) for k in ("voxels", "num", "coors", "w", "scale", "shift"))
        self.n_dev = torch.tensor([case["N"]], dtype=torch.int32, device=dev)

    def canvas(self):
        """A cleared (B, C, ny, nx) canvas inside a buffer with a guard band of sentinels on both sides."""
        n = BATCH * C * self.case["ny"] * NX
        buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=self.dev)
        view = buf[GUARD:GUARD + n].view(BATCH, C, self.case["ny"], NX)
        view.zero_()
        return buf, view

    def launch(self, feat=None, canvas=None, err=None):
        c = self.case
        p = lambda t: 0 if t is None else t.data_ptr()
        rc = lib.sessd_pillar_features(self.voxels.data_ptr(), self.num.data_ptr(), self.coors.data_ptr(), self.n_dev.data_ptr(), c["cap"],
                                       c["T"], 4, VX, VY, XO, YO, self.w.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), C,
                                       1 if c["dist"] else 0, BATCH, c["ny"], NX, p(feat), p(canvas), p(err),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc


def check_canvas(case, buf, view, feat_rows, skip=()):
    """Guard band untouched; the live pillars' columns equal their feature rows bit for bit; every other cell exactly 0."""
    n = view.numel()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())
    got = view.cpu()
    want = torch.zeros_like(got)
    co = case["coors"]
    for i in range(case["N"]):
        if i not in skip:
            want[co[i, 0], :, co[i, 2], co[i, 3]] = feat_rows[i]
    assert torch.equal(got, want)


@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("N", [1, 3, 257])
@pytest.mark.parametrize("T", [1, 5, 64, 65, 100])
def test_features_and_canvas_against_float64(dev, T, N, with_distance):
    case = make_case(1000 * T + N, N, T, with_distance)
    ref, bound = reference(case)
    bufs = Buffers(case, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    # feat only
    feat = torch.full((case["cap"], C), SENT, dtype=torch.float32, device=dev)
    bufs.launch(feat=feat, err=err)
    got = feat.cpu()
    assert bool((got[N:] == SENT).all())                      # rows beyond the live count: not written
    assert bool(torch.isfinite(got[:N]).all())                # the NaN padding slots were not read
    ratio = float(((got[:N].double() - ref).abs() / bound).max())
    print("T %d N %d dist %d: max error / bound = %.3f" % (T, N, with_distance, ratio))
    assert ratio <= 1.0
    # both: the same feature bits, the canvas holds them
    feat2 = torch.full_like(feat, SENT)
    buf, view = bufs.canvas()
    bufs.launch(feat=feat2, canvas=view, err=err)
    assert torch.equal(feat2.cpu(), got)
    check_canvas(case, buf, view, got)
    # canvas only
    buf3, view3 = bufs.canvas()
    bufs.launch(canvas=view3, err=err)
    check_canvas(case, buf3, view3, got)
    assert int(err.item()) == 0
    present = {case["num"][i] for i in range(N)}
    assert N < 3 or present == {1, max(T - 1, 1), T}


def test_padding_rule(dev):
    """Small weights that make every live slot's dot product slightly negative, scale 1, shift +5 in the even channels: a pillar with
    num_points < T outputs exactly shift[c] there (the padding slots' candidate relu(0 * scale + shift) wins), a full pillar stays
    below it; in the odd channels (shift -0.5) everything is 0."""
    T, N = 5, 12
    case = make_case(77, N, T, False, small=True)
    ref, bound = reference(case)
    num = case["num"][:N]
    part, full = torch.from_numpy(num < T), torch.from_numpy(num == T)
    assert int(part.sum()) >= 4 and int(full.sum()) >= 2
    even = torch.arange(C) % 2 == 0
    # the condition that makes the case meaningful, on the float64 reference first
    assert bool((ref[part][:, even] == 5.0).all()) and bool((ref[full][:, even] != 5.0).all())
    assert bool((ref[full][:, even] > 5.0 - 0.1).all()) and bool((ref[:, ~even] >= 0).all())
    bufs = Buffers(case, dev)
    feat = torch.full((case["cap"], C), SENT, dtype=torch.float32, device=dev)
    bufs.launch(feat=feat)
    got = feat.cpu()[:N]
    assert bool((got[part][:, even] == 5.0).all())
    assert bool((got[full][:, even] != 5.0).all())
    ratio = float(((got.double() - ref).abs() / bound).max())
    print("padding rule: max error / bound = %.3f" % ratio)
    assert ratio <= 1.0


def test_out_of_range_cell_is_skipped_and_flagged(dev):
    """One pillar with x = nx in the last row of the last frame (a linear index would land past its plane, the last channel's
    past the canvas): nothing is stored for it, the flag is set, every other cell is right, the guard band is untouched. The input
    is refused by design -- no out-of-bounds access is attempted."""
    T, N = 5, 9
    case = make_case(91, N, T, False)
    bad = 4
    case["coors"][bad] = [BATCH - 1, 0, case["ny"] - 1, NX]
    bufs = Buffers(case, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    feat = torch.full((case["cap"], C), SENT, dtype=torch.float32, device=dev)
    buf, view = bufs.canvas()
    bufs.launch(feat=feat, canvas=view, err=err)
    assert int(err.item()) == 1
    got = feat.cpu()
    assert bool(torch.isfinite(got[:N]).all()) and bool((got[N:] == SENT).all())   # its feature row is still computed
    check_canvas(case, buf, view, got, skip=(bad,))
    # negative and batch-overflow cells likewise, through the scatter-alone form, without a flag pointer
    for cell in ([-1, 0, 0, 0], [BATCH, 0, 0, 0], [0, 0, -1, 3], [0, 0, case["ny"], 0], [0, 0, 2, -1]):
        case["coors"][bad] = cell
        b2 = Buffers(case, dev)
        buf2, view2 = b2.canvas()
        rc = lib.sessd_pillar_features(0, 0, b2.coors.data_ptr(), b2.n_dev.data_ptr(), case["cap"], 1, 4, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, C, 0,
                                       BATCH, case["ny"], NX, feat.data_ptr(), view2.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        check_canvas(case, buf2, view2, got, skip=(bad,))


def test_ops_wrappers_and_mirror_modules(dev, golden_dir):
    """ops.pillar_features / ops.pillar_scatter give the direct launch's bits; the mirror's reader + scatter on the device give the
    golden canvas of the reference's own classes within twice the bound (both sides are float32 evaluations)."""
    case = make_case(5, 40, 7, True, extra=0)
    bufs = Buffers(case, dev)
    feat = torch.empty((case["cap"], C), dtype=torch.float32, device=dev)
    buf, view = bufs.canvas()
    bufs.launch(feat=feat, canvas=view)
    canvas = torch.zeros((BATCH, C, case["ny"], NX), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.pillar_features(bufs.voxels, bufs.num, bufs.coors, bufs.w, bufs.scale, bufs.shift, VX, VY, XO, YO, with_distance=True,
                              num_voxels_dev=bufs.n_dev, canvas=canvas, err_flag=err)
    assert torch.equal(got, feat) and torch.equal(canvas, view) and int(err.item()) == 0
    assert torch.equal(ops.pillar_scatter(feat, bufs.coors, BATCH, case["ny"], NX), view)
    with pytest.raises(ValueError):
        ops.pillar_features(bufs.voxels, bufs.num, bufs.coors, bufs.w[:, :9].contiguous(), bufs.scale, bufs.shift, VX, VY, XO, YO,
                            with_distance=True)
    # the mirror modules on the device
    from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter
    g = PR.load_golden(golden_dir)
    for tag in ("plain", "dist"):
        net = PillarFeatureNet(num_filters=[64], with_distance=tag == "dist", norm_cfg=None)
        net.load_state_dict(g[tag]["sd"])
        net.eval().to(dev)
        vox, num, coors = (torch.from_numpy(g[k]).to(dev) for k in ("voxels", "num_points", "coors"))
        assert net.on_device_path(vox)
        with torch.no_grad():
            f = net(vox, num, coors)
        sd = g[tag]["sd"]
        scale, shift = PR.fold_bn(sd, "pfn_layers.0.norm", torch.float32)
        c = dict(N=vox.shape[0], T=vox.shape[1], dist=tag == "dist", voxels=g["voxels"], num=g["num_points"], coors=g["coors"],
                 w=sd["pfn_layers.0.linear.weight"].numpy(), scale=scale.numpy(), shift=shift.numpy())
        _, bound = reference(c)
        ratio = float(((f.cpu().double() - g[tag]["out"].double()).abs() / (2 * bound)).max())
        print("mirror reader (%s) on the device vs reference: max error / (2 * bound) = %.3f" % (tag, ratio))
        assert f.shape == (vox.shape[0], 64) and ratio <= 1.0
        assert net(vox[:1], num[:1], coors[:1]).shape == (1, 64)
        if tag == "plain":
            canvas = PointPillarsScatter(num_input_features=64)(f, coors, 2, [12, 8, 1])
            assert torch.equal(canvas.cpu(), PR.scatter(f.cpu(), g["coors"], 2, 8, 12))


def test_empty_pillar_set(dev):
    """N = 0 (an empty frame): a (0, 64) tensor and a cleared canvas, no error (an empty tensor's pointer is null)."""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
    w, scale, shift = z(C, 9), z(C), z(C)
    f = ops.pillar_features(z(0, 5, 4), z(0, dtype=torch.int32), z(0, 4, dtype=torch.int32), w, scale, shift, VX, VY, XO, YO)
    assert f.shape == (0, C)
    canvas = torch.full((1, C, 4, 6), 3.0, device=dev)
    f = ops.pillar_features(z(0, 5, 4), z(0, dtype=torch.int32), z(0, 4, dtype=torch.int32), w, scale, shift, VX, VY, XO, YO, canvas=canvas)
    assert f.shape == (0, C) and bool((canvas == 3.0).all())    # the caller clears; nothing was written
    out = ops.pillar_scatter(f, z(0, 4, dtype=torch.int32), 2, 4, 6)
    assert out.shape == (2, C, 4, 6) and float(out.abs().max()) == 0.0


def test_training_mode_and_gradients_take_the_torch_path(dev, golden_dir):
    """Training mode, or a feature tensor that carries a gradient, runs the torch formulation: the canvas keeps its graph and the
    gradient reaches the PFN layer's weight. Eval mode without a gradient runs the kernels and agrees with it."""
    from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter
    g = PR.load_golden(golden_dir)
    net = PillarFeatureNet(num_filters=[64], norm_cfg=None)
    net.load_state_dict(g["plain"]["sd"])
    net.to(dev)
    scat = PointPillarsScatter(num_input_features=64).to(dev)
    vox, num, coors = (torch.from_numpy(g[k]).to(dev) for k in ("voxels", "num_points", "coors"))
    net.eval(), scat.eval()
    with torch.no_grad():
        ref = scat(net(vox, num, coors), coors, 2, [12, 8, 1])
    feat = net._forward_torch(vox, num, coors)          # eval mode, parameters require grad: the features carry a graph
    assert feat.requires_grad
    canvas = scat(feat, coors, 2, [12, 8, 1])
    assert canvas.grad_fn is not None
    assert float((canvas.detach() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    net.train(), scat.train()
    assert not net.on_device_path(vox)
    out = scat(net(vox, num, coors), coors, 2, [12, 8, 1])
    assert out.grad_fn is not None and out.shape == ref.shape
    out.sum().backward()
    gw = net.pfn_layers[0].linear.weight.grad
    assert gw is not None and float(gw.abs().max()) > 0
