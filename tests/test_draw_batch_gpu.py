"""sessd_draw_batch (ops.DrawBatch) on the device against tests/draw_batch_ref.py: moved points, kept box rows, classes, counts and
the recorded augmentation BIT FOR BIT at the kernel's edges (one point, one short of / exactly / one past a 256-thread block,
several blocks; scene counts 0, 1, P - 1, P; one box, a partial wave, both waves full; box counts 0 and G; both flip values; boxes
wholly outside and with exactly one corner inside). Every case keeps each corner MARGIN from the range edges by the float64
restatement alone -- asserted on the CPU before the device is used -- so cosf against torch.cos cannot flip a decision. And
ops.voxelize_staged against ops.voxelize_frames."""
import numpy as np
import pytest
import torch

import draw_batch_ref as DR
from sessd_hip import ops, synth

pytestmark = pytest.mark.gpu
S, T = 5, 6
NAMES = ("pool_points", "pool_point_count", "pool_boxes", "pool_classes", "pool_box_count", "choice", "par")
OUT = ("staged", "gt_boxes", "gt_classes", "gt_count", "transformation")


def _draw(case, dev):
    return ops.DrawBatch(*[case[k].to(dev) for k in NAMES], case["range_xy"])


def _same(got, want, where=""):
    for k in OUT:
        assert torch.equal(got[k].cpu(), want[k]), (k, where)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [1, 15, 128])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_draw_equals_the_reference_bit_for_bit(dev, P, G, B):
    case = DR.make_case(S, P, G, T, B, seed=7 * P + G + B)
    flags = DR.slot_flags(case)
    margin = min(float(mg.min()) for _, mg in flags)
    print("smallest corner margin %.4f m" % margin)
    assert margin > DR.MARGIN                      # by the float64 restatement alone, before the device is used
    assert {0, G} <= set(case["pool_box_count"].tolist())
    assert {0, 1, max(P - 1, 0), P} <= set(case["pool_point_count"].tolist())
    assert set(case["par"][:, :, 0].reshape(-1).tolist()) == {0.0, 1.0} or T * B < 2
    if G >= 15:
        counts = np.concatenate([ins.sum(1) for ins, _ in flags])
        assert (counts == 0).any() and (counts == 1).any() and (counts == 4).any()
    draw = _draw(case, dev)
    for it in range(T):
        _same(draw.run(it), DR.reference(case, it), "iteration %d" % it)


@pytest.fixture(scope="module")
def mid(dev):
    case = DR.make_case(S, 257, 15, T, 3, seed=11)
    assert DR.min_margin(case) > DR.MARGIN
    return case, _draw(case, dev), [DR.reference(case, it) for it in range(T)]


def test_iteration_by_host_value_by_device_counter_and_modulo_the_table(mid, dev):
    case, draw, want = mid
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in (0, 1, 4):
        counter.fill_(it)
        a = {k: v.clone() for k, v in draw.run(it).items()}
        b = draw.run(iter_dev=counter)
        _same(a, want[it]), _same(b, want[it])
    _same(draw.run(T + 1), want[1])                # it = T + 1 gives the bits of it = 1
    counter.fill_(T + 1)
    _same(draw.run(iter_dev=counter), want[1])     # also when the device counter says so
    counter.fill_(-1)
    _same(draw.run(iter_dev=counter), want[T - 1])
    draw.cursor = 2
    _same(draw.run(), want[2])                     # default: the next one
    assert draw.cursor == 3


def test_every_output_element_is_written_and_two_calls_give_the_same_bits(mid, dev):
    case, draw, want = mid
    B, P, G = 3, 257, 15
    nan_f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    junk_i = lambda *s: torch.full(s, -0x5A5A5A5B, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        out = dict(staged=nan_f(B, P, 4), gt_boxes=nan_f(B, G, 7), gt_classes=junk_i(B, G), gt_count=junk_i(B), transformation=nan_f(B, 5))
        got = draw.run(3, out=out)
        assert all(got[k] is out[k] for k in OUT)
        _same(got, want[3])                        # equality with the reference: no NaN, no junk word is left anywhere
        outs.append(got)
    for k in OUT:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_captured_with_a_device_counter_replays_the_next_batch(mid, dev):
    case, draw, want = mid
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    draw.run(iter_dev=counter)                     # (warm: nothing is allocated inside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = draw.run(iter_dev=counter)
    for it in (2, 3, T + 4):
        counter.fill_(it)
        g.replay()
        _same(got, want[it % T], "replay %d" % it)


def test_refusals(mid, dev):
    case, draw, _ = mid
    t = {k: case[k].to(dev) for k in NAMES}
    build = lambda **kw: ops.DrawBatch(*[kw.get(k, t[k]) for k in NAMES], case["range_xy"])
    with pytest.raises(ValueError):                # G = 129
        build(pool_boxes=torch.zeros((S, 129, 7), device=dev), pool_classes=torch.zeros((S, 129), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):                # wrong dtype
        build(choice=t["choice"].long())
    with pytest.raises(ValueError):
        build(par=t["par"].double())
    with pytest.raises(ValueError):                # CPU tensor among device tensors
        build(pool_point_count=case["pool_point_count"])
    with pytest.raises(ValueError):                # wrong shape
        build(par=t["par"][:, :, :4].contiguous())
    with pytest.raises(ValueError):
        draw.run(0, out=dict(staged=torch.zeros((3, 257, 4))))
    with pytest.raises(ValueError):
        draw.run(0, out=dict(gt_count=torch.zeros(3, dtype=torch.int64, device=dev)))
    with pytest.raises(ValueError):
        draw.run(iter_dev=torch.zeros(1, dtype=torch.int64, device=dev))


def test_voxelize_staged_equals_voxelize_frames(dev):
    vsize, vrange, mp, mv = [0.16, 0.16, 4.0], [4.0, -2.56, -3.0, 11.68, 2.56, 1.0], 100, 2000
    clouds = [torch.from_numpy(synth.make_frame(s, n)).to(dev) for s, n in ((5, 20000), (6, 15000))]
    B, P = 2, 20000
    want = ops.voxelize_frames(clouds, vsize, vrange, mp, mv)
    staged = torch.tensor(DR.PAD_POINT, dtype=torch.float32, device=dev).repeat(B, P, 1)
    for b, c in enumerate(clouds):
        staged[b, :c.shape[0]] = c
    m = int(want["prefix"][B].item())
    assert 1000 < m <= B * mv

    def same(got):
        assert torch.equal(got["prefix"], want["prefix"])
        for k in ("voxels", "coors", "num_points"):
            assert torch.equal(got[k][:m], want[k][:m]), k

    got = ops.voxelize_staged(staged, vsize, vrange, mp, mv)
    same(got)
    assert torch.equal(got["mean"][:m], want["mean"][:m])
    cap = B * mv
    out = dict(voxels=torch.full((cap, mp, 4), float("nan"), device=dev), coordinates=torch.full((cap, 4), -7, dtype=torch.int32, device=dev),
               num_points=torch.full((cap,), -7, dtype=torch.int32, device=dev), prefix=torch.zeros(B + 1, dtype=torch.int32, device=dev),
               hash=ops.VoxelHash(P * B, dev))
    for _ in range(2):                             # the caller's tensors, twice: the hash is cleared by every call
        got = ops.voxelize_staged(staged, vsize, vrange, mp, mv, out=out)
        assert got["voxels"] is out["voxels"] and got["coors"] is out["coordinates"] and got["prefix"] is out["prefix"]
        same(got)
    assert bool((out["coordinates"][m:] == -7).all())   # rows at or beyond the count are not written
    with pytest.raises(ValueError):
        ops.voxelize_staged(staged, vsize, vrange, mp, mv, out=dict(voxels=torch.zeros((cap, mp, 4), device=dev, dtype=torch.float64)))
    with pytest.raises(ValueError):
        ops.voxelize_staged(staged[0], vsize, vrange, mp, mv)
