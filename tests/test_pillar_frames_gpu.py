"""sessd_pillar_frames (ops.pillar_frames): staged clouds -> canvas without the (N, T, 4) pillar tensor, against
(1) the existing device path ops.voxelize_frames + ops.pillar_features(canvas=), bit for bit, and
(2) the oracle chain: oracle.capi.points_to_voxel for the pillars (coors, num_points, prefix exactly), then tests/pillars_ref.py in
    float64 for the features -- through `reference` of tests/test_pillar_features_gpu.py, which runs PR.pillar_features, the body of
    PR.reader_forward, on given weights and derives the per-element bound (T + 16) u B stated there -- and PR.scatter for the canvas.

The cloud is hand-built on the 48 x 32 grid of tests/test_pointpillars_detector_gpu.py: seven pillars in the grid's first row with
1, 63, 64, 65, T, T + 1 and 2 T + 3 points for T = 100 (so that every T in {5, 64, 100} meets counts below, at and above it and the
64-lane round), some 1400 background points in the other rows, points below, above and exactly on the upper range bound, one NaN
row; 2000-odd rows, shuffled with a fixed seed so that a pillar's points arrive interleaved with the others'. What the cases need
from the seed is asserted on the oracle alone, before the device is touched.

The NaN row goes to the device only. The oracle restates the reference's loop, whose range test lets a NaN through (both
comparisons are false) and then indexes its cell map with int(NaN): it cannot take such a row. The device kernels drop it, so
the oracle is given the same cloud without that row -- the remaining rows keep their order, which is all its outputs depend on."""
import numpy as np
import pytest
import torch

import pillars_ref as PR
import test_pillar_features_gpu as TF
from test_pointpillars_detector_gpu import VRANGE, VSIZE
from oracle import capi
from sessd_hip import ops

pytestmark = pytest.mark.gpu

NX, NY = 48, 32
TS = (5, 64, 100)
COUNTS = (1, 63, 64, 65, 100, 101, 203)           # 1, 63, 64, 65, T, T + 1, 2 T + 3 at T = 100
MAXV, MAXV_CUT = 2000, 150
SEED = 3
C = 64
SENT = -12345.0
GUARD = 4096


def build_cloud():
    rng = np.random.RandomState(SEED)
    rows, cells = [], []

    def in_cell(cx, cy, n):
        u = rng.rand(n, 2) * 0.8 + 0.1            # well inside the cell: no float32 rounding onto a neighbour
        return np.stack([VRANGE[0] + (cx + u[:, 0]) * VSIZE[0], VRANGE[1] + (cy + u[:, 1]) * VSIZE[1],
                         rng.rand(n) * 3.8 - 2.9, rng.rand(n)], 1)

    for k, c in enumerate(COUNTS):                # the special pillars: row 0, every sixth column
        rows.append(in_cell(6 * k + 2, 0, c))
        cells += [(6 * k + 2, 0)] * c
    nb = 1400                                     # background: rows 1 .. 31, a few points per pillar
    bx, by = rng.randint(0, NX, nb), rng.randint(1, NY, nb)
    for x, y in zip(bx, by):
        rows.append(in_cell(x, y, 1))
        cells.append((x, y))
    edge = np.array([[VRANGE[0] - 0.1, 0.0, 0.0, 0.5],       # below the lower bound in x
                     [VRANGE[3] + 0.3, 0.0, 0.0, 0.5],       # above the upper bound in x
                     [5.0, VRANGE[1] - 1.0, 0.0, 0.5], [5.0, VRANGE[4] + 1.0, 0.0, 0.5],
                     [5.0, 0.0, VRANGE[2] - 0.5, 0.5], [5.0, 0.0, VRANGE[5] + 0.5, 0.5],
                     [VRANGE[3], 0.0, 0.0, 0.5], [5.0, VRANGE[4], 0.0, 0.5], [5.0, 0.0, VRANGE[5], 0.5],   # exactly on the upper bounds
                     [np.nan, np.nan, np.nan, np.nan]])
    rows.append(edge)
    cells += [None] * len(edge)
    pts = np.concatenate(rows).astype(np.float32)
    perm = rng.permutation(len(pts))
    return pts[perm], [cells[i] for i in perm]


CLOUD, CELLS = build_cloud()
SHORT = np.ascontiguousarray(CLOUD[np.random.RandomState(SEED + 1).permutation(len(CLOUD))[:901]])
OUTSIDE = np.tile(np.array([[-100.0, 0.0, 0.0, 0.5]], np.float32), (300, 1))
N_EDGE = 10


def oracle_pillars(clouds, T, max_voxels):
    vs, cs, ns, prefix = [], [], [], [0]
    for b, pts in enumerate(clouds):
        pts = np.ascontiguousarray(pts[~np.isnan(pts).any(1)])    # (module docstring: the NaN row is the device's alone)
        v, c, n = capi.points_to_voxel(pts, VSIZE, VRANGE, T, max_voxels)
        vs.append(v), ns.append(n), cs.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
        prefix.append(prefix[-1] + len(c))
    return np.concatenate(vs), np.concatenate(ns), np.concatenate(cs), prefix


@pytest.fixture(scope="module")
def oracle():
    """(T, cut) -> oracle pillars of [CLOUD, SHORT]; the conditions on the seed, asserted here on the oracle alone."""
    assert 2000 <= len(CLOUD) <= 2100 and int(np.isnan(CLOUD).any(1).sum()) == 1
    out = {}
    for T in TS:
        for mv in (MAXV, MAXV_CUT):
            out[T, mv] = oracle_pillars([CLOUD, SHORT], T, mv)
        vox, num, coors, prefix = out[T, MAXV]
        m0 = prefix[1]
        assert m0 > MAXV_CUT                                       # the cut below cuts
        assert sum(c is None for c in CELLS) == N_EDGE
        # every count class is there, cut to T ...
        assert {min(c, T) for c in COUNTS} <= set(num[:m0].tolist())
        # ... and truncation keeps the T smallest indices, in order
        for k, c in enumerate(COUNTS):
            idx = [i for i, cell in enumerate(CELLS) if cell == (6 * k + 2, 0)]
            assert len(idx) == c
            row = int(np.nonzero((coors[:m0, 3] == 6 * k + 2) & (coors[:m0, 2] == 0))[0][0])
            keep = min(c, T)
            assert num[row] == keep and np.array_equal(vox[row, :keep], CLOUD[idx[:keep]])
        # max_voxels below the pillar count: the kept pillars are the first ones, and one of them loses points behind the cut
        _, num_c, coors_c, prefix_c = out[T, MAXV_CUT]
        assert prefix_c[1] == MAXV_CUT and np.array_equal(coors_c[:MAXV_CUT], coors[:MAXV_CUT])
        assert (num_c[:MAXV_CUT] <= num[:MAXV_CUT]).all() and (num_c[:MAXV_CUT] < num[:MAXV_CUT]).any()
    return out


def weights(with_distance, dev):
    rng = np.random.RandomState(11 + int(with_distance))
    K = 10 if with_distance else 9
    w = ((rng.rand(C, K) * 2 - 1) * 0.6).astype(np.float32)
    scale = ((rng.rand(C) + 0.5) * np.where(rng.rand(C) < 0.25, -1, 1)).astype(np.float32)
    shift = (rng.randn(C) * 2.0).astype(np.float32)
    return (w, scale, shift), tuple(torch.from_numpy(a).to(dev) for a in (w, scale, shift))


GEOM = (TF.VX, TF.VY, TF.XO, TF.YO)


def fused(clouds, T, max_voxels, wd, with_distance, dev, **kw):
    pts = [torch.from_numpy(c).to(dev) for c in clouds]
    return ops.pillar_frames(pts, VSIZE, VRANGE, T, max_voxels, *wd, *GEOM, with_distance=with_distance, **kw)


def tensor_path(clouds, T, max_voxels, wd, with_distance, dev):
    """the existing device path: voxelize_frames, then pillar_features with the canvas in its launch"""
    pts = [torch.from_numpy(c).to(dev) for c in clouds]
    B = len(pts)
    r = ops.voxelize_frames(pts, VSIZE, VRANGE, T, max_voxels)
    canvas = torch.zeros((B, C, NY, NX), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    feat = ops.pillar_features(r["voxels"], r["num_points"], r["coors"], *wd, *GEOM, with_distance=with_distance,
                               num_voxels_dev=r["prefix"][B:], canvas=canvas, err_flag=err)
    assert int(err.item()) == 0
    return dict(canvas=canvas, prefix=r["prefix"], coors=r["coors"], num_points=r["num_points"], feat=feat)


def assert_same(got, want, B):
    assert torch.equal(got["prefix"], want["prefix"])
    m = int(want["prefix"][B])
    assert torch.equal(got["canvas"], want["canvas"])
    for k in ("coors", "num_points", "feat"):
        assert torch.equal(got[k][:m], want[k][:m]), k
    return m


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("T", TS)
def test_bit_equality_with_the_tensor_path(oracle, dev, T, with_distance, B):
    _, wd = weights(with_distance, dev)
    sets = [[CLOUD, SHORT][:B]] + ([[OUTSIDE, CLOUD], [SHORT, OUTSIDE]] if B == 2 else [])
    for clouds in sets:
        for mv in (MAXV, MAXV_CUT):
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            got = fused(clouds, T, mv, wd, with_distance, dev, err_flag=err)
            m = assert_same(got, tensor_path(clouds, T, mv, wd, with_distance, dev), B)
            assert int(err.item()) == 0 and m > 0
            if clouds[0] is CLOUD:
                assert got["prefix"].cpu().tolist() == oracle[T, mv][3][:B + 1]


@pytest.mark.parametrize("with_distance", [False, True])
@pytest.mark.parametrize("T", TS)
def test_oracle_chain(oracle, dev, T, with_distance):
    (w, scale, shift), wd = weights(with_distance, dev)
    for mv in (MAXV, MAXV_CUT):
        vox, num, coors, prefix = oracle[T, mv]
        got = fused([CLOUD, SHORT], T, mv, wd, with_distance, dev)
        m = prefix[2]
        assert got["prefix"].cpu().tolist() == prefix
        assert np.array_equal(got["coors"][:m].cpu().numpy(), coors) and np.array_equal(got["num_points"][:m].cpu().numpy(), num)
        case = dict(N=m, T=T, dist=with_distance, voxels=vox, num=num, coors=coors, w=w, scale=scale, shift=shift)
        ref, bound = TF.reference(case)
        feat = got["feat"][:m].cpu()
        ratio = float(((feat.double() - ref).abs() / bound).max())
        print("T %d dist %d max_voxels %d: %d pillars, max error / bound = %.3f" % (T, with_distance, mv, m, ratio))
        assert ratio <= 1.0
        assert torch.equal(got["canvas"].cpu(), PR.scatter(feat, coors, 2, NY, NX))


def test_only_the_pillars_columns_are_written(oracle, dev):
    T = 100
    _, wd = weights(False, dev)
    _, _, coors, prefix = oracle[T, MAXV]
    canvas = torch.full((2, C, NY, NX), SENT, dtype=torch.float32, device=dev)
    got = fused([CLOUD, SHORT], T, MAXV, wd, False, dev, canvas=canvas)
    assert got["canvas"] is canvas
    named = torch.zeros((2, NY, NX), dtype=torch.bool)
    co = torch.from_numpy(coors).long()
    named[co[:, 0], co[:, 2], co[:, 3]] = True
    assert int(named.sum()) == prefix[2]
    c = canvas.cpu()
    assert bool((c.permute(0, 2, 3, 1)[~named] == SENT).all())
    assert bool((c.permute(0, 2, 3, 1)[named] != SENT).all())


def test_cells_outside_the_canvas_are_skipped_and_flagged(oracle, dev):
    """A canvas of 20 rows under the 32-row grid, inside a guard tensor: the pillars of rows >= 20 store nothing and set the flag;
    the others' columns are those of the full canvas. No out-of-bounds access is attempted -- the cell test comes before the store."""
    T, ny = 64, 20
    _, wd = weights(False, dev)
    coors = oracle[T, MAXV][2]
    assert (coors[:, 2] >= ny).any() and (coors[:, 2] < ny).any()
    full = fused([CLOUD], T, MAXV, wd, False, dev)
    n = C * ny * NX
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
    view = buf[GUARD:GUARD + n].view(1, C, ny, NX)
    view.zero_()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    got = fused([CLOUD], T, MAXV, wd, False, dev, canvas=view, err_flag=err)
    assert int(err.item()) == 1
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())
    assert torch.equal(view, full["canvas"][:, :, :ny]) and torch.equal(got["prefix"], full["prefix"])
    assert torch.equal(got["feat"][:int(got["prefix"][1])], full["feat"][:int(full["prefix"][1])])   # the rows are still computed


def test_no_state_is_left_between_calls(oracle, dev):
    T = 5
    _, wd = weights(True, dev)
    P = len(CLOUD)
    shared = dict(hash=ops.VoxelHash(P, dev), prefix=torch.zeros(2, dtype=torch.int32, device=dev),
                  coors=torch.empty((MAXV_CUT, 4), dtype=torch.int32, device=dev))
    shared["workspace"] = torch.empty(int(ops.lib.sessd_pillar_frames_workspace_bytes(shared["hash"].capacity, 1, P, T, MAXV_CUT)),
                                      dtype=torch.uint8, device=dev)
    second = np.tile(OUTSIDE[:1], (P, 1))                           # another cloud of the same length: a hundred points, twice
    second[:100], second[500:600] = SHORT[:100], SHORT[99::-1]
    staged = lambda c: torch.from_numpy(np.ascontiguousarray(c)).to(dev)[None]
    ops.pillar_frames(staged(CLOUD), VSIZE, VRANGE, T, MAXV_CUT, *wd, *GEOM, with_distance=True, **shared)   # hits the cut
    got = ops.pillar_frames(staged(second), VSIZE, VRANGE, T, MAXV_CUT, *wd, *GEOM, with_distance=True, **shared)
    fresh = ops.pillar_frames(staged(second), VSIZE, VRANGE, T, MAXV_CUT, *wd, *GEOM, with_distance=True)
    assert 0 < assert_same(got, fresh, 1) < MAXV_CUT               # the second cloud is NOT cut: the first one's break index is gone
