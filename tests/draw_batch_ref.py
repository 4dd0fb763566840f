"""Reference for sessd_draw_batch (csrc/draw_batch.hip): torch on the CPU in float32, ONE torch op per rounding, in the order the
header states -- which is the order of sessd_hip.trainloop.DeviceBatcher._student_cloud / _student_boxes / _in_range
(tests/test_draw_batch_cpu.py holds the two to each other bit for bit). Beside it a float64 restatement of the keep decision that
returns every corner's distance to the nearest range edge: the GPU test generates its boxes so that no corner lies within MARGIN of
an edge BY THAT RESTATEMENT ALONE, so cosf on the device against torch.cos here cannot flip a decision.

make_case builds resident tables at the kernel's edges: scene point counts 0, 1, P - 1, P; box counts 0 and G; both flip values;
boxes wholly inside, wholly outside (centre >= 15 m out) and with exactly one corner inside (designed in the moved frame of the
first slot that draws the scene, then carried back through the inverse move)."""
import math

import numpy as np
import torch

RANGE_XY = [0.0, -40.0, 70.4, 40.0]     # [x_lo, y_lo, x_hi, y_hi]
MARGIN = 1e-3                           # metres; float32 arithmetic on |values| < 128 m errs by < 1e-4
PAD_POINT = (-1.0e6, -1.0e6, -1.0e6, 0.0)
_SIGNS = ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))


def _move(x, y, p):
    yf = torch.where(p[0] != 0, -y, y)
    return (x * p[1] + yf * p[2]) * p[4], ((-x) * p[2] + yf * p[1]) * p[4]


def move_points(pts, p):
    """pts (n, 4) float32, p (5,) float32 [flipped, cos, sin, rotation, scale]"""
    out = torch.empty_like(pts)
    x, y = _move(pts[:, 0], pts[:, 1], p)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x, y, pts[:, 2] * p[4], pts[:, 3]
    return out


def move_boxes(b, p):
    out = torch.empty_like(b)
    x, y = _move(b[:, 0], b[:, 1], p)
    out[:, 0], out[:, 1] = x, y
    out[:, 2:6] = b[:, 2:6] * p[4]
    pi = torch.tensor(math.pi, dtype=torch.float32)
    yaw = torch.where(p[0] != 0, (-b[:, 6]) + pi, b[:, 6])
    out[:, 6] = yaw + p[3]
    return out


def keep_mask(b, range_xy):
    """moved boxes (n, 7) float32 -> bool (n): any BEV corner strictly inside"""
    lo_x, lo_y, hi_x, hi_y = (torch.tensor(v, dtype=torch.float32) for v in range_xy)
    c, s = torch.cos(b[:, 6]), torch.sin(b[:, 6])
    keep = torch.zeros(b.shape[0], dtype=torch.bool)
    for fx, fy in _SIGNS:
        dx, dy = fx * b[:, 3], fy * b[:, 4]
        x = (dx * c + dy * s) + b[:, 0]
        y = ((-dx) * s + dy * c) + b[:, 1]
        keep |= (x > lo_x) & (x < hi_x) & (y > lo_y) & (y < hi_y)
    return keep


def corner_margins_f64(b_src, p, range_xy):
    """The move and the keep decision in float64 on the float32 inputs: (inside (n, 4) bool, margin (n, 4) float64 = each corner's
    distance to the nearest range edge along an axis: a decision can only flip where a coordinate crosses an edge)."""
    b, p = np.asarray(b_src, np.float64).reshape(-1, 7), np.asarray(p, np.float64)
    yf = np.where(p[0] != 0, -b[:, 1], b[:, 1])
    X, Y = (b[:, 0] * p[1] + yf * p[2]) * p[4], (-b[:, 0] * p[2] + yf * p[1]) * p[4]
    w, l = b[:, 3] * p[4], b[:, 4] * p[4]
    yaw = np.where(p[0] != 0, -b[:, 6] + float(np.float32(math.pi)), b[:, 6]) + p[3]
    c, s = np.cos(yaw), np.sin(yaw)
    lo_x, lo_y, hi_x, hi_y = range_xy
    inside, margin = [], []
    for fx, fy in _SIGNS:
        dx, dy = fx * w, fy * l
        x, y = dx * c + dy * s + X, -dx * s + dy * c + Y
        inside.append((x > lo_x) & (x < hi_x) & (y > lo_y) & (y < hi_y))
        margin.append(np.minimum(np.minimum(np.abs(x - lo_x), np.abs(x - hi_x)), np.minimum(np.abs(y - lo_y), np.abs(y - hi_y))))
    return np.stack(inside, 1), np.stack(margin, 1)


def reference(case, it):
    """dict(staged (B, P, 4), gt_boxes (B, G, 7), gt_classes (B, G), gt_count (B), transformation (B, 5)) of row it mod T"""
    S, P, G, T, B = case["dims"]
    row = it % T
    staged = torch.tensor(PAD_POINT, dtype=torch.float32).repeat(B, P, 1)
    gt_boxes, gt_classes = torch.zeros((B, G, 7), dtype=torch.float32), torch.zeros((B, G), dtype=torch.int32)
    gt_count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        s, p = int(case["choice"][row, b]), case["par"][row, b]
        n, m = int(case["pool_point_count"][s]), int(case["pool_box_count"][s])
        staged[b, :n] = move_points(case["pool_points"][s, :n], p)
        moved = move_boxes(case["pool_boxes"][s, :m], p)
        keep = keep_mask(moved, case["range_xy"])
        k = int(keep.sum())
        gt_boxes[b, :k], gt_classes[b, :k], gt_count[b] = moved[keep], case["pool_classes"][s, :m][keep], k
    return dict(staged=staged, gt_boxes=gt_boxes, gt_classes=gt_classes, gt_count=gt_count, transformation=case["par"][row].clone())


def _unmove(X, Y, w, l, yaw, p):
    """float64 inverse of the move: the source (x, y, w, l, yaw) whose moved box is the designed one"""
    flip, c, s, rot, k = (float(v) for v in p)
    u, v = X / k, Y / k
    x, yf = u * c - v * s, u * s + v * c
    return x, (-yf if flip else yf), w / k, l / k, ((math.pi - (yaw - rot)) if flip else (yaw - rot))


def _design(kind, rng, range_xy):
    """a box in the MOVED frame: (X, Y, w, l, yaw)"""
    lo_x, lo_y, hi_x, hi_y = range_xy
    w, l = rng.uniform(1.4, 2.0), rng.uniform(3.5, 4.5)
    if kind == 0:     # wholly inside
        return rng.uniform(lo_x + 10, hi_x - 10), rng.uniform(lo_y + 10, hi_y - 10), w, l, rng.uniform(-math.pi, math.pi)
    if kind == 1:     # wholly outside: the centre at least 15 m out, the half diagonal is < 2.5 m
        side = rng.randint(4)
        X = (lo_x - rng.uniform(15, 40), hi_x + rng.uniform(15, 40), rng.uniform(lo_x, hi_x), rng.uniform(lo_x, hi_x))[side]
        Y = (rng.uniform(lo_y, hi_y), rng.uniform(lo_y, hi_y), lo_y - rng.uniform(15, 40), hi_y + rng.uniform(15, 40))[side]
        return X, Y, w, l, rng.uniform(-math.pi, math.pi)
    # exactly one corner inside: axis-aligned in the moved frame, that corner 0.3 m inside a corner of the range
    sx, sy = (-1, 1)[rng.randint(2)], (-1, 1)[rng.randint(2)]
    cx, cy = (lo_x if sx < 0 else hi_x), (lo_y if sy < 0 else hi_y)
    return cx + sx * (w / 2 - 0.3), cy + sy * (l / 2 - 0.3), w, l, 0.0


def make_case(S, P, G, T, B, seed=0, range_xy=RANGE_XY):
    """Resident tables (CPU tensors) with every live corner of every (iteration, slot) at least MARGIN from a range edge by the
    float64 restatement: the seed is advanced until that holds (checked again by the caller's assert_margins)."""
    for attempt in range(64):
        case = _make_case(S, P, G, T, B, seed + 1000 * attempt, range_xy)
        if min_margin(case) > MARGIN:
            return case
    raise AssertionError("no case with every corner %g m from the range edges" % MARGIN)


def _make_case(S, P, G, T, B, seed, range_xy):
    rng = np.random.RandomState(seed)
    npts = np.array(([0, 1, max(P - 1, 0), P] + [P // 2] * S)[:S], np.int32)
    nbox = np.array(([0, G, G, rng.randint(0, G + 1)] + [G] * S)[:S], np.int32)
    pts = np.stack([rng.uniform(-10, 80, (S, P)), rng.uniform(-50, 50, (S, P)), rng.uniform(-3, 1, (S, P)), rng.uniform(0, 1, (S, P))], -1)
    for s in range(S):
        pts[s, npts[s]:] = 7.0           # rows at or beyond the count: finite, never to be seen in an output
    shift = rng.randint(S)
    choice = np.array([[(t * B + b + shift) % S for b in range(B)] for t in range(T)], np.int32)
    flip = np.array([[(t + b) % 2 for b in range(B)] for t in range(T)], np.float64)
    rot, scale = rng.uniform(-math.pi / 4, math.pi / 4, (T, B)), rng.uniform(0.95, 1.05, (T, B))
    par = np.stack([flip, np.cos(rot), np.sin(rot), rot, scale], -1).astype(np.float32)
    boxes, classes = np.full((S, G, 7), 3.0), np.full((S, G), 9, np.int32)
    for s in range(S):
        slots = np.argwhere(choice == s)
        p = par[slots[0][0], slots[0][1]] if len(slots) else par[0, 0]
        for g in range(nbox[s]):
            kind = (g + s) % 3 if G > 1 else rng.randint(3)
            X, Y, w, l, yaw = _design(kind, rng, range_xy)
            x, y, w0, l0, yaw0 = _unmove(X, Y, w, l, yaw, p)
            boxes[s, g] = [x, y, rng.uniform(-1.5, -0.5), w0, l0, rng.uniform(1.4, 1.8), yaw0]
            classes[s, g] = 1 + rng.randint(3)
    t = torch.from_numpy
    return dict(dims=(S, P, G, T, B), range_xy=[float(v) for v in range_xy], pool_points=t(pts.astype(np.float32)),
                pool_point_count=t(npts), pool_boxes=t(boxes.astype(np.float32)), pool_classes=t(classes), pool_box_count=t(nbox),
                choice=t(choice), par=t(par))


def slot_flags(case):
    """[(inside (m, 4), margin (m, 4))] of the float64 restatement for every (iteration, slot) with live boxes"""
    S, P, G, T, B = case["dims"]
    out = []
    for row in range(T):
        for b in range(B):
            s = int(case["choice"][row, b])
            m = int(case["pool_box_count"][s])
            if m:
                out.append(corner_margins_f64(case["pool_boxes"][s, :m].numpy(), case["par"][row, b].numpy(), case["range_xy"]))
    return out


def min_margin(case):
    return min([float(mg.min()) for _, mg in slot_flags(case)] + [float("inf")])
