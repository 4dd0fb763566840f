"""sessd_supervised_loss: the argument checks come before any device call, so they can be exercised without a GPU (null or dummy
device pointers). SESSD_EINVAL = -1, SESSD_EWORKSPACE = -2; the workspace query returns 0 for what it refuses. And the ctypes
mirrors of the two structs have the layout the header spells."""
import ctypes as C

import pytest

import sessd_hip
from sessd_hip._lib import SupervisedLossCfg, SupervisedTask

lib = sessd_hip.lib


def _cfg(**kw):
    v = dict(batch=2, num_anchors=600, num_tasks=3, labels_i64=1, pos_cls_weight=1.0, neg_cls_weight=1.0, focal_alpha=0.25,
             focal_gamma=2.0, smooth_l1_sigma=3.0, cls_loss_weight=1.0, loc_loss_weight=2.0, dir_loss_weight=0.2, direction_offset=0.0)
    v.update(kw)
    return SupervisedLossCfg(**v)


def _tasks(n, **null):
    arr = (SupervisedTask * 4)()
    for t in range(n):
        for name, _ in SupervisedTask._fields_:
            setattr(arr[t], name, 256)   # non-null, never dereferenced: the call must fail first
    for name, t in null.items():
        setattr(arr[t], name, None)
    return arr


def test_struct_mirrors_have_the_header_layout():
    assert [n for n, _ in SupervisedTask._fields_] == ["box", "cls", "dir", "labels", "reg_targets", "anchors", "grad_box", "grad_cls",
                                                       "grad_dir"]
    assert C.sizeof(SupervisedTask) == 9 * 8 and C.sizeof(SupervisedLossCfg) == 4 * 4 + 9 * 4   # LP64
    assert [n for n, _ in SupervisedLossCfg._fields_][:4] == ["batch", "num_anchors", "num_tasks", "labels_i64"]


def test_workspace_query_refuses_what_the_kernels_do_not_cover():
    wb = lambda c: lib.sessd_supervised_loss_workspace_bytes(C.addressof(c) if c is not None else None)
    assert wb(None) == 0
    assert wb(_cfg(batch=0)) == 0 and wb(_cfg(batch=-1)) == 0 and wb(_cfg(num_anchors=0)) == 0
    assert wb(_cfg(num_tasks=0)) == 0 and wb(_cfg(num_tasks=5)) == 0
    assert wb(_cfg(batch=1024, num_anchors=1 << 21)) == 0        # batch * anchors past 2^31
    # counts per block and sample, twelve doubles per block: 3 tasks x 2 samples x 3 blocks, each array rounded up to 256 bytes
    assert wb(_cfg()) == 256 + 256 + 256 * ((3 * 2 * 3 * 12 * 8 + 255) // 256)
    assert 0 < wb(_cfg(num_tasks=1, num_anchors=107136)) < 1 << 20 and 0 < wb(_cfg(num_anchors=70400)) < 1 << 20
    for T in (1, 2, 3, 4):
        assert wb(_cfg(num_tasks=T)) > 0


def test_entry_refuses_bad_arguments_before_any_device_call():
    ws, rec = 4096, 512   # dummy non-null addresses; ws is 256-byte aligned
    call = lambda c, tasks, record=rec, workspace=ws, nbytes=1 << 20: lib.sessd_supervised_loss(
        C.addressof(c) if c is not None else None, C.addressof(tasks) if tasks is not None else None, record, workspace, nbytes, None)
    good = _tasks(3)
    assert call(None, good) == -1 and call(_cfg(), None) == -1
    assert call(_cfg(batch=0), good) == -1 and call(_cfg(num_anchors=0), good) == -1
    assert call(_cfg(num_tasks=0), good) == -1 and call(_cfg(num_tasks=5), good) == -1
    assert call(_cfg(), good, record=None) == -1 and call(_cfg(), good, workspace=None) == -1
    for name, _ in SupervisedTask._fields_:       # a null pointer in any task, also the last one
        assert call(_cfg(), _tasks(3, **{name: 2})) == -1, name
        assert call(_cfg(), _tasks(3, **{name: 0})) == -1, name
    c0 = _cfg()
    need = lib.sessd_supervised_loss_workspace_bytes(C.addressof(c0))
    assert need > 0 and call(_cfg(), good, nbytes=need - 1) == -2 and call(_cfg(), good, nbytes=0) == -2
    assert call(_cfg(), good, workspace=4100) == -1   # not 256-byte aligned
    # a task past num_tasks is not looked at: two tasks with the third one's pointers null pass every check up to the workspace
    assert call(_cfg(num_tasks=2), _tasks(3, box=2), nbytes=0) == -2


def test_ops_wrapper_refuses_cpu_and_uncovered_configurations():
    import torch
    from sessd_hip import ops
    cfg = dict(pos_cls_weight=1.0, neg_cls_weight=1.0, focal_alpha=0.25, focal_gamma=2.0, smooth_l1_sigma=3.0, cls_loss_weight=1.0,
               loc_loss_weight=2.0, dir_loss_weight=0.2, direction_offset=0.0)
    with pytest.raises(ValueError):
        ops.SupervisedLoss(2, 600, 5, torch.device("cuda:0"), True, cfg)
    with pytest.raises(ValueError):
        ops.SupervisedLoss(0, 600, 1, torch.device("cuda:0"), True, cfg)
    with pytest.raises(ValueError):
        ops.SupervisedLoss(2, 600, 1, torch.device("cpu"), True, cfg)
    assert ops.SUPERVISED_LOSS_RECORD["loss"] == 0 and ops.SUPERVISED_LOSS_RECORD["loc_loss_elem"] == slice(6, 13)
