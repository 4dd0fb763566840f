"""sessd_draw_batch without a GPU: (1) its reference (tests/draw_batch_ref.py) IS the loader arithmetic it replaces --
DeviceBatcher._student_cloud / _student_boxes / _in_range on CPU tensors, bit for bit, kept rows taken in order; (2) the float64
restatement agrees with the float32 keep decision on cases generated away from the edges, which hold the kinds of boxes they claim;
(3) the new symbol is exported with the argument types the header spells, and the entry refuses bad arguments before any device
call (null / dummy device pointers)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import draw_batch_ref as DR
from conftest import ROOT


def _device_batcher(range_xy):
    """DeviceBatcher's arithmetic without its constructor (which uploads a scene pool): the three methods read lo / hi only"""
    from sessd_hip.trainloop import DeviceBatcher
    db = object.__new__(DeviceBatcher)
    db.lo = torch.tensor(range_xy[:2], dtype=torch.float32)
    db.hi = torch.tensor(range_xy[2:], dtype=torch.float32)
    return db


@pytest.mark.parametrize("P,G,B", [(257, 15, 3), (1000, 128, 1), (1, 1, 3)])
def test_reference_is_the_loader_arithmetic_bit_for_bit(P, G, B):
    from sessd_hip.trainloop import FAR
    case = DR.make_case(5, P, G, 6, B, seed=3)
    db = _device_batcher(case["range_xy"])
    seen_flips = set()
    for it in range(6):
        ref = DR.reference(case, it)
        for b in range(B):
            s, p = int(case["choice"][it, b]), case["par"][it, b]
            seen_flips.add(float(p[0]))
            n, m = int(case["pool_point_count"][s]), int(case["pool_box_count"][s])
            assert torch.equal(ref["staged"][b, :n], db._student_cloud(case["pool_points"][s, :n], p))
            assert bool((ref["staged"][b, n:] == torch.tensor(DR.PAD_POINT)).all())
            parked = db._in_range(db._student_boxes(case["pool_boxes"][s, :m], p))
            kept = parked[:, 0] > FAR / 2
            k = int(ref["gt_count"][b])
            assert k == int(kept.sum())
            assert torch.equal(ref["gt_boxes"][b, :k], parked[kept])
            assert torch.equal(ref["gt_classes"][b, :k], case["pool_classes"][s, :m][kept])
            assert not bool(ref["gt_boxes"][b, k:].any()) and not bool(ref["gt_classes"][b, k:].any())
        assert torch.equal(ref["transformation"], case["par"][it])
    assert seen_flips == {0.0, 1.0}


def test_cases_keep_their_margin_and_hold_every_kind_of_box():
    case = DR.make_case(5, 256, 15, 6, 3, seed=0)
    assert DR.min_margin(case) > DR.MARGIN
    counts = np.concatenate([ins.sum(1) for ins, _ in DR.slot_flags(case)])
    assert (counts == 0).any() and (counts == 1).any() and (counts == 4).any()   # wholly outside, one corner, wholly inside
    assert sorted(case["pool_point_count"].tolist()) == [0, 1, 128, 255, 256]
    assert {0, 15} <= set(case["pool_box_count"].tolist())
    # the float32 decision is the float64 one (the margin makes it so)
    for it in range(6):
        for b in range(3):
            s, p = int(case["choice"][it, b]), case["par"][it, b]
            m = int(case["pool_box_count"][s])
            if m:
                ins, _ = DR.corner_margins_f64(case["pool_boxes"][s, :m].numpy(), p.numpy(), case["range_xy"])
                assert np.array_equal(DR.keep_mask(DR.move_boxes(case["pool_boxes"][s, :m], p), case["range_xy"]).numpy(), ins.any(1))


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_symbol_is_exported_with_the_headers_argument_types():
    import sessd_hip
    from sessd_hip._lib import SIGNATURES, f32, i32, vp
    assert hasattr(sessd_hip.lib, "sessd_draw_batch")
    res, args = SIGNATURES["sessd_draw_batch"]
    assert res is i32 and sessd_hip.lib.sessd_draw_batch.argtypes == args
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sessd_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+sessd_draw_batch\s*\(([^)]*)\)", txt).group(1)
    kinds = [vp if "*" in a or "sessd_stream_t" in a else {"int": i32, "float": f32}[a.split()[0]] for a in decl.split(",")]
    assert kinds == args and len(args) == 21


def _call(**kw):
    import sessd_hip
    r = (C.c_float * 4)(*DR.RANGE_XY)
    v = dict(pool_points=4096, pool_point_count=256, pool_boxes=256, pool_classes=256, pool_box_count=256, choice=256, par=256,
             S=5, P=1000, G=15, T=6, B=3, range_xy=C.cast(r, C.c_void_p), iter_host=0, iter_dev=None, staged=4096, gt_boxes=256,
             gt_classes=256, gt_count=256, transformation=256)   # dummy non-null addresses: the call must fail before using them
    v.update(kw)
    return sessd_hip.lib.sessd_draw_batch(*[v[k] for k in ("pool_points", "pool_point_count", "pool_boxes", "pool_classes", "pool_box_count",
                                                            "choice", "par", "S", "P", "G", "T", "B", "range_xy", "iter_host", "iter_dev",
                                                            "staged", "gt_boxes", "gt_classes", "gt_count", "transformation")], None)


def test_entry_refuses_bad_arguments_before_any_device_call():
    EINVAL = -1
    assert _call(G=129) == EINVAL and _call(G=0) == EINVAL
    for k in ("S", "P", "T", "B"):
        assert _call(**{k: 0}) == EINVAL and _call(**{k: -3}) == EINVAL, k
    assert _call(B=65536) == EINVAL
    assert _call(S=1 << 15, P=1 << 14) == EINVAL and _call(B=1 << 15, P=1 << 14) == EINVAL and _call(T=1 << 14, B=1 << 14) == EINVAL
    for k in ("pool_points", "pool_point_count", "pool_boxes", "pool_classes", "pool_box_count", "choice", "par", "range_xy", "staged",
              "gt_boxes", "gt_classes", "gt_count", "transformation"):
        assert _call(**{k: None}) == EINVAL, k
    assert _call(pool_points=4100) == EINVAL and _call(staged=4104) == EINVAL   # one 16-byte row per thread


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_and_too_many_boxes():
    from sessd_hip import ops
    case = DR.make_case(5, 16, 4, 3, 2, seed=1)
    names = ("pool_points", "pool_point_count", "pool_boxes", "pool_classes", "pool_box_count", "choice", "par")
    with pytest.raises(ValueError):
        ops.DrawBatch(*[case[k] for k in names], case["range_xy"])   # CPU tensors
    with pytest.raises(ValueError):
        ops.voxelize_staged(torch.zeros(2, 8, 4), [0.16, 0.16, 4.0], [0, -2, -3, 8, 2, 1], 5, 100)
