"""HIP kernels of the numba-convention rotated IoU / NMS family (AP-evaluation side) vs the oracle.
Tolerance 2e-5 on IoU-like outputs, 2e-4 m^2 on areas (device sinf/cosf/sqrtf vs libm)."""
import numpy as np
import pytest
import torch

import oracle
from sessd_hip import ops, synth

pytestmark = pytest.mark.gpu


def _boxes(n, seed):
    return np.ascontiguousarray(synth.clustered_boxes7(n, seed=seed)[:, [0, 1, 3, 4, 6]], np.float32)


@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
@pytest.mark.parametrize("n,k", [(1, 1), (37, 64), (300, 129)])
def test_rotate_iou_eval(dev, criterion, n, k):
    b, q = _boxes(n, n), _boxes(k, k + 7)
    want = oracle.rotate_iou_eval(b, q, criterion)
    got = ops.rotate_iou_eval(torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev), criterion).cpu().numpy()
    tol = 2e-4 if criterion == 2 else 2e-5
    assert np.abs(got - want).max() < tol
    assert ((got > 0) == (want > 0)).mean() > 0.999


def test_mirror_numpy_api(dev):
    from det3d.ops.nms.nms_gpu import nms_gpu, rotate_iou_gpu, rotate_iou_gpu_eval, rotate_nms_gpu
    b = _boxes(200, 3)
    iou = rotate_iou_gpu(b, b)
    # NB: on IDENTICAL boxes the reference algorithm is ill-conditioned (duplicate vertices: the golden vectors hold
    # 0, 1/3 and 1 on the diagonal), so only distinct pairs are compared
    off = ~np.eye(200, dtype=bool)
    assert iou.shape == (200, 200) and np.abs(iou - oracle.rotate_iou_eval(b, b, -1))[off].max() < 2e-5
    assert rotate_iou_gpu_eval(b[:0], b).shape == (0, 200)
    # rotate_nms_gpu: greedy on devRotateIoU > thresh over score order
    # box seed 5 (seed 3 above has a pair 4.8e-5 from the threshold): the oracle matrix has no entry within 1e-4 of 0.3 -- the
    # closest is 5.7e-4, thirty times the 2e-5 the device's IoU is held to -- so the keep list must be IDENTICAL
    bn = _boxes(200, 5)
    rng = np.random.RandomState(0)
    dets = np.concatenate([bn, rng.rand(200, 1).astype(np.float32)], 1)
    keep = rotate_nms_gpu(dets, 0.3)
    order = dets[:, 5].argsort()[::-1]
    ref_iou = oracle.rotate_iou_eval(bn[order], bn[order], -1).T  # [i][j] = IoU(box_i, box_j) in sorted order
    alive, want = np.ones(200, bool), []
    for i in range(200):
        if alive[i]:
            want.append(order[i])
            alive[i + 1:] &= ~(ref_iou[i, i + 1:] > 0.3)
    assert int((np.abs(ref_iou - 0.3) < 1e-4).sum()) == 0 and len(want) < 100
    assert list(keep) == want
    # nms_gpu: axis aligned, +1 convention
    aa = np.stack([b[:, 0] * 10, b[:, 1] * 10 + 400, b[:, 0] * 10 + b[:, 2] * 12, b[:, 1] * 10 + 400 + b[:, 3] * 12, dets[:, 5]], 1).astype(np.float32)
    keep2 = nms_gpu(aa, 0.4)
    order = aa[:, 4].argsort()[::-1]
    s = aa[order]
    alive, want = np.ones(200, bool), []
    for i in range(200):
        if not alive[i]:
            continue
        want.append(order[i])
        for j in range(i + 1, 200):
            w = max(min(s[i, 2], s[j, 2]) - max(s[i, 0], s[j, 0]) + 1, 0.0)
            h = max(min(s[i, 3], s[j, 3]) - max(s[i, 1], s[j, 1]) + 1, 0.0)
            sa = (s[i, 2] - s[i, 0] + 1) * (s[i, 3] - s[i, 1] + 1)
            sb = (s[j, 2] - s[j, 0] + 1) * (s[j, 3] - s[j, 1] + 1)
            if np.float32(w * h) / np.float32(sa + sb - w * h) > 0.4:
                alive[j] = False
    assert list(keep2) == want
