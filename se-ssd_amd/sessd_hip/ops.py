"""Thin torch-facing wrappers over the C ABI: one function per entry point of include/sessd_hip.h.

torch is plumbing only (device memory + the current HIP stream). Inputs must be contiguous CUDA
tensors of the stated dtype; nothing here copies to the host or synchronises.
"""
import ctypes
import os

import torch

from ._lib import lib, check, SessdError, ConvEpilogue, TileList, StreamK


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _addr(arr):
    """address of a ctypes array, as the integer the C entries take for a host pointer"""
    return ctypes.cast(arr, ctypes.c_void_p).value


def _req(t, dtype, name):
    if not t.is_cuda:
        raise ValueError("%s must be a CUDA (HIP) tensor: the SE-SSD hot path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


_ws_cache = {}
_CAPTURE_EPOCH = [0]


def new_capture_epoch():
    """Call before a stream capture begins (InferenceEngine.capture, TrainStep.capture). A scratch buffer that the module-level
    caches below hand out DURING a capture is allocated from that graph's private memory pool, and its initialisation
    (torch.zeros of a stream-K workspace) is a captured launch, not an executed one: a later capture must not find it in the cache
    -- torch uses ONE process-wide capture stream, so the (device, stream) key alone cannot tell two captures apart. Entries made
    while capturing therefore carry the epoch of their capture."""
    _CAPTURE_EPOCH[0] += 1
    # entries of earlier captures: the graphs that use them keep working without the cache's reference (their private pools
    # stay reserved for them), and no later capture may pick them up
    for cache in (_ws_cache, _SK_WS):
        for key in [k for k in cache if k[1][1] != 0]:
            del cache[key]
    return _CAPTURE_EPOCH[0]


def _cache_scope():
    """(stream, capture epoch or 0): the part of a scratch-cache key that separates eager use from each capture"""
    st = _stream()
    return (st, _CAPTURE_EPOCH[0] if torch.cuda.is_current_stream_capturing() else 0)


_MASKED_STREAMS = []   # (torch ExternalStream, raw handle): kept alive for the life of the process


def _destroy_masked_streams():
    """At interpreter exit, UNDER A PROFILER ONLY (rocprofv3 preloads its tool library: ROCP_TOOL_LIBRARIES is set; or
    SESSD_DESTROY_MASKED_STREAMS=1): drain and destroy the CU-masked streams. Measured in round 5, both ways: left to the runtime's
    own teardown the streams crashed the process in __cxa_finalize under rocprofv3 (the trace was complete, the exit code 139);
    destroyed here they exit cleanly under the profiler -- but a plain process that still holds events recorded on those streams
    (scripts/hostio_probe.py) crashed when they were destroyed first, and exits cleanly when they are left alone. A plain run
    therefore leaves them to the runtime."""
    import os
    if not (os.environ.get("ROCP_TOOL_LIBRARIES") or os.environ.get("SESSD_DESTROY_MASKED_STREAMS")):
        return
    try:
        if _MASKED_STREAMS and torch.cuda.is_available():
            torch.cuda.synchronize()
            # the caching allocator keeps free blocks (and their events) per stream: give them back before the streams go, or its
            # own teardown touches destroyed streams (a probe that dropped its engines before exit crashed there)
            import gc
            gc.collect()
            torch.cuda.empty_cache()
        while _MASKED_STREAMS:
            _, h = _MASKED_STREAMS.pop()
            lib.sessd_stream_destroy(h)
    except Exception:
        pass


import atexit as _atexit
_atexit.register(_destroy_masked_streams)


def close_masked_streams():
    """Deterministic end of life of every CU-masked stream of this process (round 6; bench.py calls it last): device idle, the
    caching allocator's free blocks (which carry events of the streams they were used on) returned, then hipStreamDestroy on each
    handle. The caller drops what was recorded ON those streams first -- captured graphs, engines, its torch.cuda.Event objects,
    a process group whose collectives ran on them (dist.destroy_process_group) -- and must not use the ExternalStream objects
    afterwards. After this the exit hook above finds nothing to do, with or without a profiler attached. Returns the number of
    streams destroyed."""
    import gc
    n = 0
    if _MASKED_STREAMS and torch.cuda.is_available():
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
    while _MASKED_STREAMS:
        _, h = _MASKED_STREAMS.pop()
        check(lib.sessd_stream_destroy(h), "stream_destroy")
        n += 1
    return n


def cu_masked_stream(part, parts, device=None, layout="contiguous"):
    """A torch stream (ExternalStream over hipExtStreamCreateWithCUMask) whose kernels run on the `part`-th of `parts` equal,
    disjoint sets of the device's compute units. layout: 'contiguous' = CU numbers [part * n, (part + 1) * n), 'interleaved' = every
    parts-th CU. Returns (stream, CUs in the set). Several frames in flight on such streams never wait for each other's CUs."""
    import ctypes
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    n = total // parts
    words = (ctypes.c_uint32 * ((total + 31) // 32))()
    cus = range(part * n, (part + 1) * n) if layout == "contiguous" else range(part, n * parts, parts)
    for c in cus:
        words[c >> 5] |= 1 << (c & 31)
    h = ctypes.c_void_p()
    with torch.cuda.device(dev):
        check(lib.sessd_stream_create_cu_mask(len(words), ctypes.cast(words, ctypes.c_void_p), ctypes.byref(h)), "stream_create_cu_mask")
    st = torch.cuda.ExternalStream(h.value, device=dev)
    _MASKED_STREAMS.append((st, h))
    return st, n


def workspace(nbytes, device, tag="default"):
    """A cached per-(device, stream, capture, tag) byte workspace, grown on demand (never shrinks)."""
    key = (device.index, _cache_scope(), tag)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def zeroed_workspace(nbytes, device, tag):
    """workspace() for the entry points whose contract is "counter words zero on entry, left zero on return" (the train-mode
    BatchNorm statistics kernels): cleared ONCE when (re)allocated, by our own fill kernel (inside a capture that launch is part
    of the graph; a torch memset would be a memset node, see sum_all)."""
    key = (device.index, _cache_scope(), tag)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        n = (max(int(nbytes), 256) + 15) // 16 * 16
        ws = torch.empty(n, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            check(lib.sessd_fill_u32(ws.data_ptr(), 0, n // 4, _stream()), "fill_u32")
        _ws_cache[key] = ws
    return ws


# ------------------------------------------------------------------ voxelizer
class VoxelHash:
    """Open-addressing cell -> row hash shared by a batch of frames (and by SpMiddleFHD level 0)."""

    def __init__(self, max_items, device, keys=None, vals=None):
        self.capacity = int(lib.sessd_hash_capacity(int(max_items)))
        self.keys = keys if keys is not None else torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.vals = vals if vals is not None else torch.empty(self.capacity, dtype=torch.int32, device=device)
        assert self.keys.numel() == self.capacity and self.vals.numel() == self.capacity

    def clear(self):
        check(lib.sessd_hash_clear(self.keys.data_ptr(), self.vals.data_ptr(), self.capacity, _stream()), "hash_clear")


def voxelize_batch(points_list, voxel_size, coors_range, max_points, max_voxels, with_batch_index=True,
                   want_mean=True):
    """points_list: list of (P_b, ndim) float32 CUDA tensors. Returns a dict of device tensors:
    voxels (cap,max_points,ndim), coors (cap,4|3) int32, num_points (cap,), mean (cap,ndim) or None,
    prefix (B+1,) int32 (prefix[b]..prefix[b+1] = rows of frame b; prefix[B] = total), hash.
    cap = B*max_voxels; rows beyond prefix[B] are unspecified."""
    B = len(points_list)
    dev = points_list[0].device
    ndim = points_list[0].shape[1]
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    cr = torch.tensor(coors_range, dtype=torch.float32)
    grid = torch.round((cr[3:] - cr[:3]) / vs).to(torch.int32)  # voxel_generator.py:15-16 (float32 math)
    cap = B * max_voxels
    maxp = max(int(p.shape[0]) for p in points_list)
    h = VoxelHash(maxp * B if B > 1 else maxp, dev)
    h.clear()
    voxels = torch.empty((cap, max_points, ndim), dtype=torch.float32, device=dev)
    cs = 4 if with_batch_index else 3
    coors = torch.empty((cap, cs), dtype=torch.int32, device=dev)
    nump = torch.empty((cap,), dtype=torch.int32, device=dev)
    mean = torch.empty((cap, ndim), dtype=torch.float32, device=dev) if want_mean else None
    prefix = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    need = lib.sessd_voxelize_workspace_bytes(h.capacity, maxp, max_points, max_voxels)
    ws = workspace(need, dev, "voxelize")
    range_h, vs_h, grid_h = cr.contiguous(), vs.contiguous(), grid.contiguous()
    for b, pts in enumerate(points_list):
        _req(pts, torch.float32, "points")
        check(lib.sessd_voxelize_frame(pts.data_ptr(), pts.shape[0], ndim, range_h.data_ptr(), vs_h.data_ptr(),
                                       grid_h.data_ptr(), max_points, max_voxels, b, h.keys.data_ptr(),
                                       h.vals.data_ptr(), h.capacity, voxels.data_ptr(), coors.data_ptr(), cs,
                                       nump.data_ptr(), _p(mean), prefix.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream()), "voxelize_frame")
    return dict(voxels=voxels, coors=coors, num_points=nump, mean=mean, prefix=prefix, hash=h, grid=grid)


def voxelize_frames(points_list, voxel_size, coors_range, max_points, max_voxels):
    """voxelize_batch with ALL frames in four launches (sessd_voxelize_frames): the clouds are staged into one
    (B, P_cap, 4) buffer, shorter ones padded with out-of-range rows. Same dict, same bits."""
    B = len(points_list)
    dev = points_list[0].device
    ndim = points_list[0].shape[1]
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    cr = torch.tensor(coors_range, dtype=torch.float32)
    grid = torch.round((cr[3:] - cr[:3]) / vs).to(torch.int32)
    cap = B * max_voxels
    P = max(1, max(int(p.shape[0]) for p in points_list))
    if ndim != 4:
        raise ValueError("voxelize_frames stages (x, y, z, r) rows; use voxelize_batch for other layouts")
    staged = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
    for b, pts in enumerate(points_list):
        _req(pts, torch.float32, "points")
        check(lib.sessd_stage_points(pts.data_ptr(), pts.shape[0], staged[b].data_ptr(), P, _stream()), "stage_points")
    h = VoxelHash(P * B, dev)
    h.clear()
    voxels = torch.empty((cap, max_points, ndim), dtype=torch.float32, device=dev)
    coors = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    nump = torch.empty((cap,), dtype=torch.int32, device=dev)
    mean = torch.empty((cap, ndim), dtype=torch.float32, device=dev)
    prefix = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    ws = workspace(lib.sessd_voxelize_frames_workspace_bytes(h.capacity, B, P, max_points, max_voxels), dev, "voxelize_frames")
    check(lib.sessd_voxelize_frames(staged.data_ptr(), B, P, ndim, cr.data_ptr(), vs.data_ptr(), grid.data_ptr(), max_points, max_voxels,
                                    h.keys.data_ptr(), h.vals.data_ptr(), h.capacity, voxels.data_ptr(), coors.data_ptr(), 4,
                                    nump.data_ptr(), mean.data_ptr(), prefix.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "voxelize_frames")
    return dict(voxels=voxels, coors=coors, num_points=nump, mean=mean, prefix=prefix, hash=h, grid=grid)


def voxelize_staged(staged, voxel_size, coors_range, max_points, max_voxels, out=None):
    """voxelize_frames on clouds that are staged already: staged (B, P, 4) float32, every frame padded to P rows with
    out-of-range rows (sessd_stage_points, DrawBatch). Same dict, same bits; no kernel of its own (sessd_voxelize_frames).
    out: a dict whose tensors are written in place of fresh ones -- voxels (B * max_voxels, max_points, 4), coors or coordinates
    (B * max_voxels, 4) int32, num_points (B * max_voxels) int32, prefix (B + 1) int32 with prefix[0] == 0, optionally mean
    (B * max_voxels, 4) and hash (a VoxelHash over B * P items); with all of them given a call allocates nothing after the
    first (the workspace is cached). Rows at or beyond prefix[B] are unspecified (not written)."""
    _req(staged, torch.float32, "staged")
    if staged.dim() != 3 or staged.shape[2] != 4 or staged.shape[0] < 1 or staged.shape[1] < 1:
        raise ValueError("voxelize_staged: staged points must be (B, P, 4) with B, P >= 1")
    dev = staged.device
    B, P = int(staged.shape[0]), int(staged.shape[1])
    max_points, max_voxels = int(max_points), int(max_voxels)
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    cr = torch.tensor(coors_range, dtype=torch.float32)
    grid = torch.round((cr[3:] - cr[:3]) / vs).to(torch.int32)
    cap = B * max_voxels
    out = {} if out is None else out
    coors_key = "coordinates" if "coordinates" in out else "coors"
    want = dict(voxels=((cap, max_points, 4), torch.float32), num_points=((cap,), torch.int32), prefix=((B + 1,), torch.int32),
                mean=((cap, 4), torch.float32))
    want[coors_key] = ((cap, 4), torch.int32)
    got = {}
    for k, (shape, dt) in want.items():
        t = out.get(k)
        if t is None:
            if k == "mean" and out:   # a caller that brings its own tensors and no mean does not want one
                got[k] = None
                continue
            t = torch.zeros(shape, dtype=dt, device=dev) if k == "prefix" else torch.empty(shape, dtype=dt, device=dev)
        elif not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("voxelize_staged: out[%r] must be a contiguous %s device tensor of shape %s, got %s %s %s"
                             % (k, dt, shape, t.device, t.dtype, tuple(t.shape)))
        got[k] = t
    h = out.get("hash")
    if h is None:
        h = VoxelHash(P * B, dev)
    elif h.capacity < 2 * P * B:
        raise ValueError("voxelize_staged: out['hash'] holds %d slots, %d needed" % (h.capacity, 2 * P * B))
    h.clear()
    ws = workspace(lib.sessd_voxelize_frames_workspace_bytes(h.capacity, B, P, max_points, max_voxels), dev, "voxelize_frames")
    check(lib.sessd_voxelize_frames(staged.data_ptr(), B, P, 4, cr.data_ptr(), vs.data_ptr(), grid.data_ptr(), max_points, max_voxels,
                                    h.keys.data_ptr(), h.vals.data_ptr(), h.capacity, got["voxels"].data_ptr(), got[coors_key].data_ptr(),
                                    4, got["num_points"].data_ptr(), _p(got["mean"]), got["prefix"].data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream()), "voxelize_frames")
    return dict(voxels=got["voxels"], coors=got[coors_key], num_points=got["num_points"], mean=got["mean"], prefix=got["prefix"], hash=h,
                grid=grid)


DRAW_MAX_GT = 128   # sessd_draw_batch: box rows per scene (one 128-thread block per frame)


class DrawBatch:
    """One training batch's clouds and ground truth drawn from resident scene tables in two launches (sessd_draw_batch): the global
    augmentation (flip about x, rotation about z, scaling) of points and boxes and the ground-truth range filter, for every frame of
    the batch, nothing read back. Tables (device, kept here): pool_points (S, P, 4) float32 with pool_point_count (S) int32;
    pool_boxes (S, G, 7) float32, pool_classes (S, G) int32, pool_box_count (S) int32; choice (T, B) int32 scene per slot and
    iteration; par (T, B, 5) float32 rows [flipped, cos, sin, rotation, scale]. range_xy: [x_lo, y_lo, x_hi, y_hi]. The outputs
    -- staged (B, P, 4), gt_boxes (B, G, 7), gt_classes (B, G), gt_count (B), transformation (B, 5) -- are allocated here, once:
    usable inside a captured graph."""

    _OUT = ("staged", "gt_boxes", "gt_classes", "gt_count", "transformation")

    def __init__(self, pool_points, pool_point_count, pool_boxes, pool_classes, pool_box_count, choice, par, range_xy):
        f32, i32 = torch.float32, torch.int32
        if pool_points.dim() != 3 or pool_boxes.dim() != 3 or choice.dim() != 2:
            raise ValueError("DrawBatch: pool_points (S, P, 4), pool_boxes (S, G, 7), choice (T, B) expected")
        S, P = int(pool_points.shape[0]), int(pool_points.shape[1])
        G, (T, B) = int(pool_boxes.shape[1]), (int(v) for v in choice.shape)
        if G > DRAW_MAX_GT:
            raise ValueError("DrawBatch holds at most %d boxes per scene, got %d" % (DRAW_MAX_GT, G))
        self.dev = pool_points.device
        self.S, self.P, self.G, self.T, self.B = S, P, G, T, B
        for v, name, dt, shape in ((pool_points, "pool_points", f32, (S, P, 4)), (pool_point_count, "pool_point_count", i32, (S,)),
                                   (pool_boxes, "pool_boxes", f32, (S, G, 7)), (pool_classes, "pool_classes", i32, (S, G)),
                                   (pool_box_count, "pool_box_count", i32, (S,)), (choice, "choice", i32, (T, B)),
                                   (par, "par", f32, (T, B, 5))):
            self._check(v, name, dt, shape)
        if min(S, P, G, T, B) < 1:
            raise ValueError("DrawBatch: S, P, G, T and B must be at least 1")
        r = [float(v) for v in range_xy]
        if len(r) != 4:
            raise ValueError("DrawBatch: range_xy is [x_lo, y_lo, x_hi, y_hi]")
        self._range = (ctypes.c_float * 4)(*r)
        self.tables = (pool_points, pool_point_count, pool_boxes, pool_classes, pool_box_count, choice, par)
        self.out = dict(staged=torch.zeros((B, P, 4), dtype=f32, device=self.dev), gt_boxes=torch.zeros((B, G, 7), dtype=f32, device=self.dev),
                        gt_classes=torch.zeros((B, G), dtype=i32, device=self.dev), gt_count=torch.zeros((B,), dtype=i32, device=self.dev),
                        transformation=torch.zeros((B, 5), dtype=f32, device=self.dev))
        self.cursor = 0

    def _check(self, v, name, dtype, shape):
        if not v.is_cuda or v.device != self.dev or v.dtype != dtype or tuple(v.shape) != shape or not v.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s, got %s %s %s"
                             % (name, dtype, shape, self.dev if self.dev.type == "cuda" else "the HIP device", v.device, v.dtype,
                                tuple(v.shape)))

    def run(self, it=None, iter_dev=None, out=None):
        """Draw batch `it` (default: the next one; row it mod T of choice / par), or the one a DEVICE int32[1] counter `iter_dev`
        names when the launch executes. out: dict with any of staged / gt_boxes / gt_classes / gt_count / transformation written
        in place of this object's own. Returns the dict of the five outputs; every element of each is written."""
        B, P, G = self.B, self.P, self.G
        shapes = dict(staged=((B, P, 4), torch.float32), gt_boxes=((B, G, 7), torch.float32), gt_classes=((B, G), torch.int32),
                      gt_count=((B,), torch.int32), transformation=((B, 5), torch.float32))
        res = {}
        for k in self._OUT:
            v = None if out is None else out.get(k)
            if v is None:
                v = self.out[k]
            else:
                self._check(v, "out[%r]" % k, shapes[k][1], shapes[k][0])
            res[k] = v
        if iter_dev is not None:
            self._check(iter_dev, "iter_dev", torch.int32, tuple(iter_dev.shape) if iter_dev.numel() == 1 else (1,))
            it = 0
        else:
            it = self.cursor if it is None else int(it)
            self.cursor = it + 1
        t = self.tables
        check(lib.sessd_draw_batch(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
                                   t[6].data_ptr(), self.S, P, G, self.T, B, _addr(self._range), it % self.T, _p(iter_dev) or None,
                                   res["staged"].data_ptr(), res["gt_boxes"].data_ptr(), res["gt_classes"].data_ptr(),
                                   res["gt_count"].data_ptr(), res["transformation"].data_ptr(), _stream()), "draw_batch")
        return res


def vfe_mean(voxels, num_points, num_features=4, num_voxels_dev=None):
    _req(voxels, torch.float32, "voxels")
    _req(num_points, torch.int32, "num_points")
    M, MP, ndim = voxels.shape
    out = torch.empty((M, num_features), dtype=torch.float32, device=voxels.device)
    check(lib.sessd_vfe_mean(voxels.data_ptr(), num_points.data_ptr(), _p(num_voxels_dev), M, MP, ndim, num_features,
                             out.data_ptr(), _stream()), "vfe_mean")
    return out


PILLAR_CHANNELS = 64   # sessd_pillar_features: one lane per output channel


def fill_zero(t):
    """Clear a contiguous float32 tensor with the library's own fill (a kernel launch, not a memset node)."""
    if t.numel() == 0:
        return t
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    check(lib.sessd_fill_u32(t.data_ptr(), 0, t.numel(), _stream()), "fill_u32")
    return t


def pillar_features(voxels, num_points, coors, weight, scale, shift, vx, vy, x_offset, y_offset, with_distance=False,
                    num_voxels_dev=None, canvas=None, err_flag=None):
    """PillarFeatureNet with one PFNLayer in eval mode (sessd_pillar_features): voxels (N, T, 4), num_points (N) int32, coors (N, 4)
    int32 [b, z, y, x], weight (64, 9 | 10) as nn.Linear stores it, scale / shift (64) the folded BatchNorm1d -> (N, 64).
    num_voxels_dev: device int32 live count (rows beyond it are not written). canvas (B, 64, ny, nx), cleared by the caller: the
    pillars' columns are written in the same launch; err_flag (device int32[1], zeroed by the caller) is set when a pillar's cell
    is outside it."""
    _req(voxels, torch.float32, "voxels")
    _req(num_points, torch.int32, "num_points")
    _req(coors, torch.int32, "coors")
    _req(weight, torch.float32, "weight")
    _req(scale, torch.float32, "scale")
    _req(shift, torch.float32, "shift")
    N, T, ndim = voxels.shape
    C, K = weight.shape
    if K != (10 if with_distance else 9) or scale.numel() != C or shift.numel() != C:
        raise ValueError("pillar_features: weight (C, %d), scale (C), shift (C) expected" % (10 if with_distance else 9))
    if num_points.numel() != N or tuple(coors.shape) != (N, 4):
        raise ValueError("pillar_features: num_points (N), coors (N, 4) expected")
    B = ny = nx = 0
    if canvas is not None:
        _req(canvas, torch.float32, "canvas")
        B, cc, ny, nx = canvas.shape
        if cc != C:
            raise ValueError("pillar_features: canvas must have %d channels" % C)
    if err_flag is not None:
        _req(err_flag, torch.int32, "err_flag")
    if num_voxels_dev is not None:
        _req(num_voxels_dev, torch.int32, "num_voxels_dev")
    feat = torch.empty((N, C), dtype=torch.float32, device=voxels.device)
    if N == 0:   # no pillars: nothing to launch (an empty tensor's pointer is null, which the entry point reads as "absent")
        return feat
    check(lib.sessd_pillar_features(voxels.data_ptr(), num_points.data_ptr(), coors.data_ptr(), _p(num_voxels_dev), N, T, ndim,
                                    float(vx), float(vy), float(x_offset), float(y_offset), weight.data_ptr(), scale.data_ptr(),
                                    shift.data_ptr(), C, 1 if with_distance else 0, B, ny, nx, feat.data_ptr(), _p(canvas),
                                    _p(err_flag), _stream()), "pillar_features")
    return feat


_byte_workspace = workspace   # (pillar_frames has a `workspace` argument of its own)


def pillar_frames(points, voxel_size, coors_range, max_points, max_voxels, weight, scale, shift, vx, vy, x_offset, y_offset,
                  with_distance=False, canvas=None, err_flag=None, hash=None, workspace=None, prefix=None, coors=None,
                  num_points=None, feat=None):
    """Clouds -> canvas in one call (sessd_pillar_frames): voxelize_frames + pillar_features(canvas=) without the (N, T, 4) tensor,
    the same bits. points: a list of (P_i, 4) float32 device clouds (staged here, shorter ones padded with out-of-range rows) or a
    staged (B, P, 4) tensor. weight (64, 9 | 10), scale / shift (64), vx .. y_offset: as pillar_features. What is not given is
    allocated, and cleared where the entry point wants it cleared: canvas (B, 64, ny, nx) of the voxel grid (a given canvas is the
    caller's to clear, as is a given err_flag), hash (a VoxelHash over B * P items; a given one is cleared here, every call),
    workspace (bytes), prefix (B + 1, prefix[0] = 0), coors (B * max_voxels, 4), num_points (B * max_voxels), feat
    (B * max_voxels, 64). Returns dict(canvas, prefix, coors, num_points, feat); rows beyond prefix[B] are unspecified."""
    staged = points
    if isinstance(points, (list, tuple)):
        for p in points:
            _req(p, torch.float32, "points")
            if p.dim() != 2 or p.shape[1] != 4:
                raise ValueError("pillar_frames: every cloud must be (P, 4) [x, y, z, r]")
        dev = points[0].device
        B, P = len(points), max(1, max(int(p.shape[0]) for p in points))
        staged = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
        for b, p in enumerate(points):
            check(lib.sessd_stage_points(p.data_ptr(), p.shape[0], staged[b].data_ptr(), P, _stream()), "stage_points")
    _req(staged, torch.float32, "points")
    if staged.dim() != 3 or staged.shape[2] != 4 or staged.shape[0] < 1 or staged.shape[1] < 1:
        raise ValueError("pillar_frames: staged points must be (B, P, 4) with B, P >= 1")
    for t, name in ((weight, "weight"), (scale, "scale"), (shift, "shift")):
        _req(t, torch.float32, name)
    dev = staged.device
    B, P = int(staged.shape[0]), int(staged.shape[1])
    C, K = weight.shape
    if C != PILLAR_CHANNELS or K != (10 if with_distance else 9) or scale.numel() != C or shift.numel() != C:
        raise ValueError("pillar_frames: weight (%d, %d), scale (%d), shift (%d) expected" % (PILLAR_CHANNELS, 10 if with_distance else 9,
                                                                                            PILLAR_CHANNELS, PILLAR_CHANNELS))
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    cr = torch.tensor(coors_range, dtype=torch.float32)
    grid = torch.round((cr[3:] - cr[:3]) / vs).to(torch.int32)
    cap = B * int(max_voxels)
    if canvas is None:
        canvas = fill_zero(torch.empty((B, C, int(grid[1]), int(grid[0])), dtype=torch.float32, device=dev))
    _req(canvas, torch.float32, "canvas")
    if canvas.dim() != 4 or canvas.shape[0] != B or canvas.shape[1] != C:
        raise ValueError("pillar_frames: canvas must be (%d, %d, ny, nx)" % (B, C))
    ny, nx = int(canvas.shape[2]), int(canvas.shape[3])
    if hash is None:
        hash = VoxelHash(P * B, dev)
    hash.clear()
    need = int(lib.sessd_pillar_frames_workspace_bytes(hash.capacity, B, P, int(max_points), int(max_voxels)))
    if workspace is None:
        workspace = _byte_workspace(need, dev, "pillar_frames")
    if prefix is None:
        prefix = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
    if coors is None:
        coors = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    if num_points is None:
        num_points = torch.empty((cap,), dtype=torch.int32, device=dev)
    if feat is None:
        feat = torch.empty((cap, C), dtype=torch.float32, device=dev)
    for t, dt, name, n in ((workspace, torch.uint8, "workspace", need), (prefix, torch.int32, "prefix", B + 1),
                           (coors, torch.int32, "coors", cap * 4), (num_points, torch.int32, "num_points", cap),
                           (feat, torch.float32, "feat", cap * C)):
        _req(t, dt, name)
        if t.numel() < n:
            raise ValueError("pillar_frames: %s holds %d elements, %d needed" % (name, t.numel(), n))
    if err_flag is not None:
        _req(err_flag, torch.int32, "err_flag")
    check(lib.sessd_pillar_frames(staged.data_ptr(), B, P, 4, cr.data_ptr(), vs.data_ptr(), grid.data_ptr(), int(max_points),
                                  int(max_voxels), hash.keys.data_ptr(), hash.vals.data_ptr(), hash.capacity, float(vx), float(vy),
                                  float(x_offset), float(y_offset), weight.data_ptr(), scale.data_ptr(), shift.data_ptr(), C,
                                  1 if with_distance else 0, ny, nx, canvas.data_ptr(), coors.data_ptr(), prefix.data_ptr(),
                                  num_points.data_ptr(), feat.data_ptr(), _p(err_flag), workspace.data_ptr(), workspace.numel(),
                                  _stream()), "pillar_frames")
    return dict(canvas=canvas, prefix=prefix, coors=coors, num_points=num_points, feat=feat)


def pillar_scatter(feat, coors, batch, ny, nx, num_voxels_dev=None, err_flag=None):
    """PointPillarsScatter: feat (N, 64), coors (N, 4) int32 [b, z, y, x] -> (batch, 64, ny, nx), zero where no pillar lies (cleared
    by sessd_fill_u32, then the scatter-alone form of sessd_pillar_features)."""
    _req(feat, torch.float32, "feat")
    _req(coors, torch.int32, "coors")
    N, C = feat.shape
    if tuple(coors.shape) != (N, 4):
        raise ValueError("pillar_scatter: coors (N, 4) expected")
    canvas = fill_zero(torch.empty((int(batch), C, int(ny), int(nx)), dtype=torch.float32, device=feat.device))
    if N == 0:
        return canvas
    check(lib.sessd_pillar_features(0, 0, coors.data_ptr(), _p(num_voxels_dev), N, 1, 4, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, C, 0,
                                    int(batch), int(ny), int(nx), feat.data_ptr(), canvas.data_ptr(), _p(err_flag), _stream()),
          "pillar_scatter")
    return canvas


class PillarFeaturesTrainFunction(torch.autograd.Function):
    """One PFN layer in train mode (csrc/pillar.hip): statistics over the live points -> [all-reduce under SyncBN] -> mean, invstd,
    scale, shift -> the eval kernel with them; backward by recomputation of the selected slot. Saves the inputs, the float64 totals,
    mean, invstd, scale, shift and the (N, 64) output: nothing of size N * T * 64."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, voxels, num_points, coors, running_mean, running_var, eps, momentum, geom, with_distance,
                num_voxels_dev):
        dev = voxels.device
        N, T, ndim = voxels.shape
        C, K = weight.shape
        dist = 1 if with_distance else 0
        w = weight.detach().float().contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        vx, vy, xo, yo = geom
        totals = torch.empty(int(lib.sessd_pillar_train_totals(dist)), dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_pillar_train_workspace_bytes(dist), dev, "pillar_train")
        check(lib.sessd_pillar_train_stats(voxels.data_ptr(), num_points.data_ptr(), coors.data_ptr(), _p(num_voxels_dev), N, T, ndim,
                                           vx, vy, xo, yo, C, K, dist, totals.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "pillar_train_stats")
        sync = sync_bn_active()
        totals_all = totals
        if sync:   # S1, G and M are additive over the ranks; this rank's own copy stays for the backward's dW
            totals_all = totals.clone()
            _sync_reduce(totals_all)
        mean, invstd, scale, shift = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4))
        check(lib.sessd_pillar_train_finalize(totals_all.data_ptr(), w.data_ptr(), g.data_ptr(), b.data_ptr(), float(eps),
                                              float(momentum), C, K, dist, _p(running_mean), _p(running_var), mean.data_ptr(),
                                              invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), _stream()), "pillar_train_finalize")
        feat = fill_zero(torch.empty((N, C), dtype=torch.float32, device=dev))   # rows >= *num_voxels_dev stay zero
        check(lib.sessd_pillar_features(voxels.data_ptr(), num_points.data_ptr(), coors.data_ptr(), _p(num_voxels_dev), N, T, ndim,
                                        vx, vy, xo, yo, w.data_ptr(), scale.data_ptr(), shift.data_ptr(), C, dist, 0, 0, 0,
                                        feat.data_ptr(), 0, 0, _stream()), "pillar_features")
        saved = [voxels, num_points, coors, w, g, totals, totals_all, mean, invstd, scale, shift, feat]
        if num_voxels_dev is not None:
            saved.append(num_voxels_dev)
        ctx.save_for_backward(*saved)
        ctx.geom, ctx.dist, ctx.sync, ctx.eps = geom, dist, sync, float(eps)
        return feat

    @staticmethod
    def backward(ctx, grad):
        voxels, num_points, coors, w, gamma, totals, totals_all, _mean, _invstd, scale, shift, feat = ctx.saved_tensors[:12]
        n_dev = ctx.saved_tensors[12] if len(ctx.saved_tensors) > 12 else None
        dev = voxels.device
        N, T, ndim = voxels.shape
        C, K = w.shape
        vx, vy, xo, yo = ctx.geom
        grad = grad.float().contiguous()
        bwd = torch.empty(int(lib.sessd_pillar_train_bwd_totals(ctx.dist)), dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_pillar_train_workspace_bytes(ctx.dist), dev, "pillar_train")
        check(lib.sessd_pillar_train_bwd_select(voxels.data_ptr(), num_points.data_ptr(), coors.data_ptr(), _p(n_dev), N, T, ndim, vx, vy,
                                                xo, yo, w.data_ptr(), scale.data_ptr(), shift.data_ptr(), C, K, ctx.dist,
                                                feat.data_ptr(), grad.data_ptr(), bwd.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _stream()), "pillar_train_bwd_select")
        bwd_all = bwd
        if ctx.sync:   # the sums of dy and dy * z of all ranks go into dW; P stays this rank's
            bwd_all = bwd[:2 * C].clone()
            _sync_reduce(bwd_all)
        dw = torch.empty((C, K), dtype=torch.float32, device=dev)
        dg, db = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        check(lib.sessd_pillar_train_bwd_finalize(bwd.data_ptr(), bwd_all.data_ptr(), totals.data_ptr(), totals_all.data_ptr(),
                                                  w.data_ptr(), gamma.data_ptr(), ctx.eps, C, K, ctx.dist, dw.data_ptr(), dg.data_ptr(),
                                                  db.data_ptr(), _stream()), "pillar_train_bwd_finalize")
        return (dw, dg, db) + (None,) * 10


def pillar_features_train(voxels, num_points, coors, linear_weight, bn, vx, vy, x_offset, y_offset, with_distance=False,
                          num_voxels_dev=None):
    """PillarFeatureNet with one PFNLayer in TRAIN mode: voxels (N, T, 4), num_points (N) int32, coors (N, 4) int32, linear_weight
    (64, 9 | 10), bn the layer's nn.BatchNorm1d (batch statistics over all N * T slots; its running statistics are updated in place
    and the batch is counted) -> (N, 64) features that carry a graph to linear_weight, bn.weight and bn.bias. The points carry no
    gradient. num_voxels_dev: device int32 live count; feature rows beyond it are zero. Under set_sync_bn the float64 totals pass
    through ONE all-reduce in each direction."""
    _req(voxels, torch.float32, "voxels")
    _req(num_points, torch.int32, "num_points")
    _req(coors, torch.int32, "coors")
    for t, name in ((linear_weight, "linear_weight"), (bn.weight, "bn.weight"), (bn.bias, "bn.bias")):
        if t is None or not t.is_cuda:
            raise ValueError("%s must be a CUDA (HIP) tensor: the SE-SSD hot path has no CPU fallback" % name)
    if voxels.dim() != 3 or voxels.shape[2] != 4 or voxels.shape[0] < 1 or voxels.shape[1] < 1:
        raise ValueError("pillar_features_train: voxels (N >= 1, T >= 1, 4) expected")
    N = voxels.shape[0]
    K = 10 if with_distance else 9
    C = PILLAR_CHANNELS
    if tuple(linear_weight.shape) != (C, K) or bn.weight.numel() != C or bn.bias.numel() != C:
        raise ValueError("pillar_features_train: linear_weight (%d, %d) and a BatchNorm1d(%d) expected" % (C, K, C))
    if num_points.numel() != N or tuple(coors.shape) != (N, 4):
        raise ValueError("pillar_features_train: num_points (N), coors (N, 4) expected")
    if num_voxels_dev is not None:
        _req(num_voxels_dev, torch.int32, "num_voxels_dev")
    mom = _bn_momentum(bn)
    geom = (float(vx), float(vy), float(x_offset), float(y_offset))
    return PillarFeaturesTrainFunction.apply(linear_weight, bn.weight, bn.bias, voxels, num_points, coors, bn.running_mean,
                                             bn.running_var, bn.eps, mom, geom, bool(with_distance), num_voxels_dev)


class PillarScatterTrainFunction(torch.autograd.Function):
    """pillar_scatter with its gradient: grad_feat[p] = the canvas gradient's column at pillar p's cell (sessd_pillar_scatter_bwd)."""

    @staticmethod
    def forward(ctx, feat, coors, batch, ny, nx, num_voxels_dev):
        ctx.save_for_backward(*([coors] if num_voxels_dev is None else [coors, num_voxels_dev]))
        ctx.shape = (int(batch), int(ny), int(nx))
        return pillar_scatter(feat, coors, batch, ny, nx, num_voxels_dev=num_voxels_dev)

    @staticmethod
    def backward(ctx, grad):
        coors = ctx.saved_tensors[0]
        n_dev = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        batch, ny, nx = ctx.shape
        N, C = coors.shape[0], PILLAR_CHANNELS
        grad = grad.float().contiguous()
        out = torch.empty((N, C), dtype=torch.float32, device=grad.device)
        if N > 0:
            check(lib.sessd_pillar_scatter_bwd(grad.data_ptr(), coors.data_ptr(), _p(n_dev), N, C, batch, ny, nx, out.data_ptr(), _stream()),
                  "pillar_scatter_bwd")
        return out, None, None, None, None, None


def pillar_scatter_train(feat, coors, batch, ny, nx, num_voxels_dev=None):
    """ops.pillar_scatter that keeps the graph: feat (N, 64) -> (batch, 64, ny, nx); the backward gathers the canvas gradient's
    columns (zero rows for pillars outside the canvas and for rows beyond *num_voxels_dev)."""
    _req(feat, torch.float32, "feat")
    _req(coors, torch.int32, "coors")
    if feat.dim() != 2 or feat.shape[1] != PILLAR_CHANNELS or tuple(coors.shape) != (feat.shape[0], 4):
        raise ValueError("pillar_scatter_train: feat (N, %d), coors (N, 4) expected" % PILLAR_CHANNELS)
    if num_voxels_dev is not None:
        _req(num_voxels_dev, torch.int32, "num_voxels_dev")
    return PillarScatterTrainFunction.apply(feat, coors, int(batch), int(ny), int(nx), num_voxels_dev)


# ------------------------------------------------------------------ iou3d operators
def boxes_pairwise(mode, a, b, out=None):
    w = 7 if mode in (2, 3) else 5
    _req(a, torch.float32, "boxes_a")
    _req(b, torch.float32, "boxes_b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != w or b.shape[1] != w:
        raise ValueError("boxes must be (N,%d)" % w)
    if out is None:
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    else:
        _req(out, torch.float32, "out")
    check(lib.sessd_boxes_pairwise(mode, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(), _stream()),
          "boxes_pairwise")
    return out


def di_nms(boxes, corners, standup_iou, scores, iou_preds, labels, dirs, anchors=None, cnt_thresh=2.6,
           sigma_dist_interval=(0, 20, 40, 60), sigma_square=(0.0009, 0.009, 0.1, 1), suppressed_thresh=0.3):
    """DI-NMS core (nms_cpu.h:173-384) on the device: boxes (n,7), corners (n,4,2), standup_iou (n,n), scores / iou_preds (n) float32,
    labels / dirs (n) int32, anchors (n,>=2) or None. Returns (boxes (k,7), scores (k,), labels (k,), dirs (k,), keep (k,) int64)."""
    import ctypes
    import numpy as np
    for t, nm in ((boxes, "boxes"), (corners, "corners"), (standup_iou, "standup_iou"), (scores, "scores"), (iou_preds, "iou_preds")):
        _req(t, torch.float32, nm)
    n = boxes.shape[0]
    dev = boxes.device
    if n > 1024:
        raise ValueError("di_nms handles at most 1024 boxes (one 1024-thread workgroup walks the reference's sequential loop; the "
                         "post-processor calls it after its top-k with nms_pre_max_size = 1000): pass pre_max_size <= 1024")
    labels = labels.to(torch.int32).contiguous()
    dirs = dirs.to(torch.int32).contiguous()
    if anchors is not None:
        _req(anchors, torch.float32, "anchors")
    iv = np.ascontiguousarray(np.asarray(sigma_dist_interval, np.float32))
    sg = np.ascontiguousarray(np.asarray(sigma_square, np.float32))
    if sg.shape[0] < iv.shape[0] - 1:
        raise ValueError("sigma_square needs one entry per distance interval")
    cap = max(n, 1)
    out_b = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    out_s = torch.empty((cap,), dtype=torch.float32, device=dev)
    out_l = torch.empty((cap,), dtype=torch.int32, device=dev)
    out_d = torch.empty((cap,), dtype=torch.int32, device=dev)
    keep = torch.empty((cap,), dtype=torch.int32, device=dev)
    nk = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sessd_di_nms_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    check(lib.sessd_di_nms(boxes.data_ptr(), corners.data_ptr(), standup_iou.data_ptr(), n, scores.data_ptr(), iou_preds.data_ptr(),
                           labels.data_ptr(), dirs.data_ptr(), _p(anchors), 0 if anchors is None else anchors.shape[1],
                           float(cnt_thresh), iv.ctypes.data_as(ctypes.c_void_p), int(iv.shape[0]), sg.ctypes.data_as(ctypes.c_void_p),
                           float(suppressed_thresh), 0 if anchors is None else 1, out_b.data_ptr(), out_s.data_ptr(),
                           out_l.data_ptr(), out_d.data_ptr(), keep.data_ptr(), nk.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "di_nms")
    k = int(nk.item())
    return out_b[:k], out_s[:k], out_l[:k], out_d[:k], keep[:k].long()


def quads_pairwise(mode, corners_a, corners_b, standup_iou, standup_thresh=0.0):
    """mode 0: IoU, 1: intersection area of convex quads (n,4,2) x (k,4,2); 0 where standup_iou <= standup_thresh."""
    _req(corners_a, torch.float32, "corners_a")
    _req(corners_b, torch.float32, "corners_b")
    _req(standup_iou, torch.float32, "standup_iou")
    n, k = corners_a.shape[0], corners_b.shape[0]
    if tuple(corners_a.shape[1:]) != (4, 2) or tuple(corners_b.shape[1:]) != (4, 2) or tuple(standup_iou.shape) != (n, k):
        raise ValueError("corners must be (n,4,2) / (k,4,2) and standup_iou (n,k)")
    out = torch.empty((n, k), dtype=torch.float32, device=corners_a.device)
    check(lib.sessd_quads_pairwise(int(mode), corners_a.data_ptr(), n, corners_b.data_ptr(), k, standup_iou.data_ptr(),
                                   float(standup_thresh), out.data_ptr(), _stream()), "quads_pairwise")
    return out


def boxes_aligned_overlap_bev(a, b, out=None):
    _req(a, torch.float32, "boxes_a")
    _req(b, torch.float32, "boxes_b")
    if a.shape != b.shape or a.shape[1] != 5:
        raise ValueError("aligned boxes must both be (N,5)")
    if out is None:
        out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    check(lib.sessd_boxes_aligned_overlap_bev(a.data_ptr(), b.data_ptr(), a.shape[0], out.data_ptr(), _stream()),
          "boxes_aligned_overlap_bev")
    return out


def rotate_iou_eval(boxes, query, criterion=-1):
    """numba-convention rotated IoU: boxes (N,5), query (K,5) [cx,cy,w,l,angle] -> (N,K) float32 on the device."""
    _req(boxes, torch.float32, "boxes")
    _req(query, torch.float32, "query")
    out = torch.zeros((boxes.shape[0], query.shape[0]), dtype=torch.float32, device=boxes.device)
    check(lib.sessd_rotate_iou_eval(boxes.data_ptr(), boxes.shape[0], query.data_ptr(), query.shape[0], int(criterion),
                                    out.data_ptr(), _stream()), "rotate_iou_eval")
    return out


def nms_sorted(mode, boxes, thresh):
    """boxes sorted by descending score. Returns (keep int64[N] device, num_keep int32[1] device)."""
    _req(boxes, torch.float32, "boxes")
    n = boxes.shape[0]
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    num = torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    need = lib.sessd_nms_workspace_bytes(n)
    ws = workspace(need, boxes.device, "nms")
    check(lib.sessd_nms_sorted(mode, boxes.data_ptr(), n, float(thresh), keep.data_ptr(), num.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream()), "nms_sorted")
    return keep, num


def nms_axis_eps_sorted(boxes, thresh, eps):
    """Axis-aligned greedy NMS of nms_cpu.h:24-70: boxes (N, >=4) sorted by descending score, IoU with eps-widened extents,
    suppress at >= thresh. Returns (keep int64[N] device, num_keep int32[1] device)."""
    _req(boxes, torch.float32, "boxes")
    n = boxes.shape[0]
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=boxes.device)
    num = torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    ws = workspace(lib.sessd_nms_workspace_bytes(n), boxes.device, "nms")
    check(lib.sessd_nms_axis_eps_sorted(boxes.data_ptr(), boxes.shape[1], n, float(thresh), float(eps), keep.data_ptr(),
                                        num.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nms_axis_eps_sorted")
    return keep, num


# ------------------------------------------------------------------ sparse 3-D convolution
def _i3(v):
    v = [int(v)] * 3 if isinstance(v, int) else [int(x) for x in v]
    return torch.tensor(v, dtype=torch.int32)


# Parameters written through raw pointers (sessd_adam_ema_step: student AND teacher) do not bump torch's tensor versions.
# Every cache of packed / folded weights includes this counter in its key; whoever writes parameters behind torch's back
# calls bump_param_generation().
_PARAM_GENERATION = [0]


def param_generation():
    return _PARAM_GENERATION[0]


def bump_param_generation():
    _PARAM_GENERATION[0] += 1


class SiteHash:
    """cell -> row hash of one resolution level. dims = (D,H,W) used for the linear key."""

    def __init__(self, capacity, dims, device, keys=None, vals=None):
        self.capacity = int(capacity)
        self.dims = [int(d) for d in dims]
        self.keys = keys if keys is not None else torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.vals = vals if vals is not None else torch.empty(self.capacity, dtype=torch.int32, device=device)
        self._dims_t = _i3(self.dims)


def sparse_hash_build(indices, n_dev, dims):
    _req(indices, torch.int32, "indices")
    n_cap = indices.shape[0]
    h = SiteHash(lib.sessd_hash_capacity(max(n_cap, 1)), dims, indices.device)
    check(lib.sessd_hash_clear(h.keys.data_ptr(), h.vals.data_ptr(), h.capacity, _stream()), "hash_clear")
    check(lib.sessd_sparse_hash_build(indices.data_ptr(), _p(n_dev), n_cap, h._dims_t.data_ptr(), h.keys.data_ptr(),
                                      h.vals.data_ptr(), h.capacity, _stream()), "sparse_hash_build")
    return h


def sparse_downsample_sites(in_indices, n_in_dev, ksize, stride, pad, out_dims, n_out_cap, err_flag=None):
    """Output sites of a strided sparse conv. Returns (out_indices (cap,4), n_out_dev (1,), out_hash, err_flag)."""
    _req(in_indices, torch.int32, "in_indices")
    dev = in_indices.device
    n_in_cap = in_indices.shape[0]
    ks, st, pd, od = _i3(ksize), _i3(stride), _i3(pad), _i3(out_dims)
    kv = int(ks.prod())
    h = SiteHash(lib.sessd_hash_capacity(n_out_cap), out_dims, dev)
    out_idx = torch.empty((n_out_cap, 4), dtype=torch.int32, device=dev)
    n_out = torch.zeros((1,), dtype=torch.int32, device=dev)
    if err_flag is None:
        err_flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    need = lib.sessd_sparse_downsample_workspace_bytes(n_in_cap, kv, h.capacity)
    ws = workspace(need, dev, "downsample")
    check(lib.sessd_sparse_downsample_sites(in_indices.data_ptr(), n_in_dev.data_ptr(), n_in_cap, ks.data_ptr(),
                                            st.data_ptr(), pd.data_ptr(), od.data_ptr(), h.keys.data_ptr(),
                                            h.vals.data_ptr(), h.capacity, out_idx.data_ptr(), n_out_cap,
                                            n_out.data_ptr(), err_flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "sparse_downsample_sites")
    return out_idx, n_out, h, err_flag


def sparse_rulebook(out_indices, n_out_dev, ksize, stride, pad, in_hash):
    """nbr (kv, n_out_cap) int32 and tile_mask (ceil(cap/16),) for a conv whose input level is in_hash."""
    _req(out_indices, torch.int32, "out_indices")
    dev = out_indices.device
    cap = out_indices.shape[0]
    ks, st, pd = _i3(ksize), _i3(stride), _i3(pad)
    kv = int(ks.prod())
    nbr = torch.empty((kv, cap), dtype=torch.int32, device=dev)
    tmask = torch.empty(((cap + 15) // 16,), dtype=torch.int32, device=dev)
    check(lib.sessd_sparse_rulebook(out_indices.data_ptr(), n_out_dev.data_ptr(), cap, ks.data_ptr(), st.data_ptr(),
                                    pd.data_ptr(), in_hash.keys.data_ptr(), in_hash.vals.data_ptr(), in_hash.capacity,
                                    in_hash._dims_t.data_ptr(), nbr.data_ptr(), tmask.data_ptr(), _stream()),
          "sparse_rulebook")
    return nbr, tmask


class _SparseToDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, indices, spatial_shape, batch_size, n_dev):
        feats = features.float().contiguous()
        n, c = feats.shape
        dims = _i3(spatial_shape)
        out = torch.zeros([int(batch_size), c] + [int(v) for v in spatial_shape], dtype=torch.float32, device=feats.device)
        check(lib.sessd_sparse_to_dense_dev(feats.data_ptr(), indices.data_ptr(), n, _p(n_dev), c, dims.data_ptr(), out.data_ptr(),
                                            _stream()), "sparse_to_dense")
        ctx.save_for_backward(indices, n_dev) if n_dev is not None else ctx.save_for_backward(indices)
        ctx.shape = [int(v) for v in spatial_shape]
        ctx.nc = (n, c)
        return out

    @staticmethod
    def backward(ctx, grad):
        indices = ctx.saved_tensors[0]
        n_dev = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        n, c = ctx.nc
        g = grad.float().contiguous()
        dims = _i3(ctx.shape)
        gf = torch.empty((n, c), dtype=torch.float32, device=g.device)
        check(lib.sessd_dense_to_sparse_dev(g.data_ptr(), indices.data_ptr(), n, _p(n_dev), c, dims.data_ptr(), gf.data_ptr(),
                                            _stream()), "dense_to_sparse")
        return gf, None, None, None, None


def sparse_to_dense(features, indices, spatial_shape, batch_size, n_dev=None):
    """SparseConvTensor.dense(): (n,C) features at (n,4) int32 sites -> (B,C,D,H,W); differentiable w.r.t. the features.
    n_dev (1,) int32 on the device: only the first n_dev[0] rows are sites (capacity-based tables)."""
    _req(indices, torch.int32, "indices")
    if not features.is_cuda:
        raise ValueError("features must be on the HIP device")
    return _SparseToDense.apply(features, indices, spatial_shape, batch_size, n_dev)


class SparseChain:
    """Sites and rulebooks of a chain of strided sparse convs in four launches (csrc/sparse_sites.hip).

    steps: list of (ksize, stride, pad) of the SparseConv3d layers, level l-1 -> level l; shape0: spatial shape of level 0;
    caps: row capacity per deeper level. jobs: list of (in_level, out_level, ksize, stride, pad) neighbour tables to build.
    Buffers are allocated once; `run()` enqueues on the current stream (no synchronisation, no allocation)."""

    def __init__(self, shape0, steps, caps, batch, jobs, device, workspace_tensor=None):
        from ._lib import ChainLevel, RulebookJob
        self.batch, self.dev = int(batch), device
        self.shapes = [[int(v) for v in shape0]]
        self.levels = (ChainLevel * len(steps))()
        self.indices, self.n_dev, self.caps = [], [], [int(c) for c in caps]
        counters = torch.zeros((len(steps),), dtype=torch.int32, device=device)
        for l, ((ks, st, pd), cap) in enumerate(zip(steps, caps)):
            ks, st, pd = _t3(ks), _t3(st), _t3(pd)
            shp = [(d + 2 * p - k) // s + 1 for d, k, s, p in zip(self.shapes[-1], ks, st, pd)]
            self.shapes.append(shp)
            idx = torch.empty((int(cap), 4), dtype=torch.int32, device=device)
            self.indices.append(idx)
            self.n_dev.append(counters[l:l + 1])
            L = self.levels[l]
            for d in range(3):
                L.ksize[d], L.stride[d], L.pad[d], L.out_dims[d] = ks[d], st[d], pd[d], shp[d]
            L.cap, L.indices, L.n_dev = int(cap), idx.data_ptr(), self.n_dev[l].data_ptr()
        self.ws_bytes = int(lib.sessd_sparse_chain_workspace_bytes(self.batch, len(steps), self.levels))
        if self.ws_bytes == 0:
            raise ValueError("invalid sparse chain (kernel < stride, empty level or more than 2^31 cells)")
        self.ws = workspace_tensor if workspace_tensor is not None else torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        assert self.ws.numel() >= self.ws_bytes
        self.jobs = (RulebookJob * len(jobs))()
        self.nbr, self.tile_mask = [], []
        # offset-pattern tiles (sessd_rulebook_job_t.perm): per job the sites' offset patterns, the position -> row table of the
        # sorted 256-row groups and the tile masks of that order; built by one more launch of run_rulebooks when sort_tiles is set
        self.sort_tiles = False
        self.site_mask, self.perm, self.tile_mask_sorted = [None] * len(jobs), [None] * len(jobs), [None] * len(jobs)
        for j, (li, lo, ks, st, pd) in enumerate(jobs):
            ks, st, pd = _t3(ks), _t3(st), _t3(pd)
            cap = None if lo == 0 else self.caps[lo - 1]
            self.nbr.append(None)
            self.tile_mask.append(None)
            J = self.jobs[j]
            J.in_level, J.out_level = int(li), int(lo)
            for d in range(3):
                J.ksize[d], J.stride[d], J.pad[d] = ks[d], st[d], pd[d]
        self._job_spec = [(int(li), int(lo), _t3(ks)) for (li, lo, ks, st, pd) in jobs]

    @staticmethod
    def workspace_bytes(shape0, steps, caps, batch):
        from ._lib import ChainLevel
        lv = (ChainLevel * len(steps))()
        shp = [int(v) for v in shape0]
        for l, ((ks, st, pd), cap) in enumerate(zip(steps, caps)):
            ks, st, pd = _t3(ks), _t3(st), _t3(pd)
            shp = [(d + 2 * p - k) // s + 1 for d, k, s, p in zip(shp, ks, st, pd)]
            for d in range(3):
                lv[l].ksize[d], lv[l].stride[d], lv[l].pad[d], lv[l].out_dims[d] = ks[d], st[d], pd[d], shp[d]
            lv[l].cap = int(cap)
        return int(lib.sessd_sparse_chain_workspace_bytes(int(batch), len(steps), lv))

    def bind_tables(self, n0_cap):
        """allocate nbr / tile_mask of every job (level-0 capacity is only known to the caller)"""
        for j, (li, lo, ks) in enumerate(self._job_spec):
            cap = int(n0_cap) if lo == 0 else self.caps[lo - 1]
            kv = ks[0] * ks[1] * ks[2]
            self.nbr[j] = torch.empty((kv, cap), dtype=torch.int32, device=self.dev)
            self.tile_mask[j] = torch.empty(((cap + 15) // 16,), dtype=torch.int32, device=self.dev)
            self.jobs[j].nbr, self.jobs[j].tile_mask = self.nbr[j].data_ptr(), self.tile_mask[j].data_ptr()
            if self.sort_tiles:
                groups = (cap + 255) // 256
                self.site_mask[j] = torch.zeros((cap,), dtype=torch.int32, device=self.dev)
                self.perm[j] = torch.zeros((groups * 256,), dtype=torch.uint8, device=self.dev)
                self.tile_mask_sorted[j] = torch.zeros((groups * 16,), dtype=torch.int32, device=self.dev)
                self.jobs[j].site_mask, self.jobs[j].perm = self.site_mask[j].data_ptr(), self.perm[j].data_ptr()
                self.jobs[j].tile_mask_sorted = self.tile_mask_sorted[j].data_ptr()

    def run(self, indices0, n0_dev_ptr, n0_cap, hash0, err_flag, clear=True, stream=None):
        self.run_sites(indices0, n0_dev_ptr, n0_cap, err_flag, clear, stream)
        self.run_rulebooks(indices0, n0_dev_ptr, n0_cap, hash0, 0, len(self.jobs), stream)

    def run_sites(self, indices0, n0_dev_ptr, n0_cap, err_flag, clear=True, stream=None):
        """the site tables of every deeper level (mark / gather / count / scan / emit)"""
        s = _stream() if stream is None else stream
        if self.nbr and self.nbr[0] is None:
            self.bind_tables(n0_cap)
        check(lib.sessd_sparse_chain_sites(indices0.data_ptr(), n0_dev_ptr, int(n0_cap), self.batch, len(self.levels),
                                           self.levels, self.ws.data_ptr(), self.ws.numel(), 1 if clear else 0,
                                           err_flag.data_ptr(), s), "sparse_chain_sites")

    def run_rulebooks(self, indices0, n0_dev_ptr, n0_cap, hash0, job_lo, job_hi, stream=None):
        """the neighbour tables of jobs [job_lo, job_hi) in one launch. Jobs whose levels are both 0 (the submanifold table of the
        voxels) need the voxelizer's hash only, not run_sites()."""
        import ctypes
        from ._lib import RulebookJob
        s = _stream() if stream is None else stream
        if self.nbr and self.nbr[0] is None:
            self.bind_tables(n0_cap)
        n = int(job_hi) - int(job_lo)
        if n <= 0:
            return
        sub = (RulebookJob * n).from_address(ctypes.addressof(self.jobs) + int(job_lo) * ctypes.sizeof(RulebookJob))
        check(lib.sessd_sparse_chain_rulebooks(indices0.data_ptr(), n0_dev_ptr, int(n0_cap), hash0.keys.data_ptr(),
                                               hash0.vals.data_ptr(), hash0.capacity, hash0._dims_t.data_ptr(), self.batch,
                                               len(self.levels), self.levels, self.ws.data_ptr(), n, sub, s), "sparse_chain_rulebooks")


def _t3(v):
    return [int(v)] * 3 if isinstance(v, int) else [int(x) for x in v]


# ------------------------------------------------------------------ batched re-packing of a training iteration's weights
# The training step re-packs every conv weight after every update: 14 sparse layers x (teacher forward, student forward, student
# data gradient) + the SSFA layers' tap / Winograd layouts in three roles = 95 launches of ~5 us per iteration. Inside
# `with ops.batched_repack(registry)` (TrainStep wraps an iteration in it) the packed objects of PARAMETER weights are kept, every
# packing they were made with is recorded as a job, and the first access after an update re-runs ALL jobs as two launches
# (sessd_sparse_pack_batch, sessd_dense_pack_batch). Staleness = ops.param_generation() (the fused update writes through raw
# pointers) or the accessed parameter's `_version` (any other in-place change).
_REPACK = [None]


class RepackRegistry:
    def __init__(self):
        self.objects = {}
        self.jobs = {"dense": [], "sparse": []}
        self._table = {"dense": None, "sparse": None}   # (device tensor, n_jobs, total_blocks), rebuilt when jobs were added
        self.versions = {}                               # id(parameter) -> [parameter, _version at the last refresh]
        self.gen = -1
        self._creating = 0
        self.refreshes = 0

    # -- recording (called by the low-level pack wrappers)
    def recording(self):
        return self._creating > 0

    def note(self, kind, job):
        self.jobs[kind].append(job)
        self._table[kind] = None

    # -- access
    def cached(self, key, weight, factory):
        self.ensure_fresh(weight)
        obj = self.objects.get(key)
        if obj is None:
            self._creating += 1
            try:
                obj = factory()
            finally:
                self._creating -= 1
            self.objects[key] = obj
            self.versions[id(weight)] = [weight, weight._version]
            if isinstance(obj, PackedConv):
                obj._registry = self   # its lazily made packings (and its launches', through their owner) go through create()
        return obj

    def create(self, factory):
        """A lazily made member of a cached object (a Winograd layout first asked for by a launch): record its packing too."""
        self._creating += 1
        try:
            return factory()
        finally:
            self._creating -= 1

    def ensure_fresh(self, weight=None):
        seen = self.versions.get(id(weight)) if weight is not None else None
        if self.gen == _PARAM_GENERATION[0] and (seen is None or seen[1] == weight._version):
            return
        self.refresh()

    def prepare(self):
        """Upload the job tables now (a host-to-device copy: not allowed inside a stream capture)."""
        for kind in ("sparse", "dense"):
            if self.jobs[kind] and self._table[kind] is None:
                self._table[kind] = _repack_table(kind, self.jobs[kind])

    def refresh(self):
        for kind in ("sparse", "dense"):
            jobs = self.jobs[kind]
            if not jobs:
                continue
            if self._table[kind] is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("RepackRegistry: a packing was recorded that no eager iteration has run yet; run one warm-up "
                                       "iteration (or registry.prepare()) before capturing")
                self._table[kind] = _repack_table(kind, jobs)
            table, n, blocks = self._table[kind]
            fn = lib.sessd_sparse_pack_batch if kind == "sparse" else lib.sessd_dense_pack_batch
            with torch.cuda.device(table.device):
                check(fn(table.data_ptr(), n, blocks, _stream()), "%s_pack_batch" % kind)
        self.gen = _PARAM_GENERATION[0]
        for rec in self.versions.values():
            rec[1] = rec[0]._version
        self.refreshes += 1


def _repack_table(kind, jobs):
    import ctypes
    i32, vp, i64 = ctypes.c_int32, ctypes.c_void_p, ctypes.c_longlong
    if kind == "dense":
        class Job(ctypes.Structure):
            _fields_ = [("w", vp), ("out", vp), ("so", i64), ("sc", i64), ("tap_off", i32 * 16), ("cout", i32), ("cin", i32),
                        ("ntaps", i32), ("kind", i32), ("flip", i32), ("layout", i32), ("block_start", i32), ("pad_", i32)]
    else:
        class Job(ctypes.Structure):
            _fields_ = [("w", vp), ("out", vp), ("kv", i32), ("cin", i32), ("cout", i32), ("adjoint", i32), ("reverse_k", i32),
                        ("block_start", i32)]
    arr = (Job * len(jobs))()
    start = 0
    for a, j in zip(arr, jobs):
        a.w, a.out, a.block_start = j["w"].data_ptr(), j["out"].data_ptr(), start
        if kind == "dense":
            a.so, a.sc, a.cout, a.cin, a.kind, a.flip, a.layout = j["so"], j["sc"], j["cout"], j["cin"], j["kind"], j["flip"], j["layout"]
            a.ntaps = len(j["taps"])
            for t, off in enumerate(j["taps"]):
                a.tap_off[t] = int(off)
            cp = (j["cout"] + 31) // 32 * 32
            if j["kind"] == 0:
                total = (j["cin"] // 2) * len(j["taps"]) * 2 * cp
            else:
                cpad = cp if j["layout"] == 0 else ((j["cout"] + 127) // 128 * 128 if j["layout"] in (1, 4) else (j["cout"] + 63) // 64 * 64)
                total = cpad * j["cin"]
        else:
            a.kv, a.cin, a.cout, a.adjoint, a.reverse_k = j["kv"], j["cin"], j["cout"], j["adjoint"], j["reverse_k"]
            total = j["kv"] * j["cin"] * j["cout"]
        start += (total + 255) // 256
    dev = jobs[0]["out"].device
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return table, len(jobs), start


class batched_repack:
    """Context: packed weights of parameters are cached in `registry` and re-packed together (see RepackRegistry)."""

    def __init__(self, registry):
        self.registry = registry

    def __enter__(self):
        self.prev = _REPACK[0]
        _REPACK[0] = self.registry
        return self.registry

    def __exit__(self, *exc):
        _REPACK[0] = self.prev
        return False


def _repack_note(group, **job):
    reg = _REPACK[0]
    if reg is not None and reg.recording():
        reg.note(group, job)


def _registry_for(weight):
    """The active registry if `weight` is a parameter (a stable pointer worth caching), else None."""
    reg = _REPACK[0]
    return reg if reg is not None and isinstance(weight, torch.nn.Parameter) and weight.is_cuda else None


def packed_sparse_weight(weight, mode="fwd"):
    """Packed weight of a sparse conv layer (mode "fwd") or of its data-gradient conv ("adj": strided layers, "adj_rev": submanifold
    layers): through the active re-pack registry for parameters, a fresh packing otherwise."""
    make = {"fwd": lambda: sparse_pack_weight(weight), "adj": lambda: sparse_pack_weight_adjoint(weight, False),
            "adj_rev": lambda: sparse_pack_weight_adjoint(weight, True)}[mode]
    reg = _registry_for(weight)
    if reg is None:
        return make()
    return reg.cached(("sparse", weight.data_ptr(), tuple(weight.shape), mode), weight, make)


def packed_conv2d(weight, stride=1, adjoint=False, transposed=False):
    """pack_conv2d / pack_deconv2d_s2 through the active re-pack registry (parameters), else a fresh packing."""
    make = (lambda: pack_deconv2d_s2(weight)) if transposed else (lambda: pack_conv2d(weight, stride, adjoint=adjoint))
    reg = _registry_for(weight)
    if reg is None:
        return make()
    return reg.cached(("dense", weight.data_ptr(), tuple(weight.shape), int(stride), bool(adjoint), bool(transposed)), weight, make)


def sparse_pack_weight(weight):
    """weight (kz,ky,kx,Cin,Cout) (spconv v1 layout) on the device -> packed MFMA-fragment order."""
    w = weight.detach().to(torch.float32).contiguous()
    if not w.is_cuda:
        raise ValueError("weight must be on the HIP device")
    cin, cout = w.shape[-2], w.shape[-1]
    kv = w.numel() // (cin * cout)
    out = torch.empty_like(w).view(-1)
    check(lib.sessd_sparse_pack_weight(w.data_ptr(), kv, cin, cout, out.data_ptr(), _stream()), "sparse_pack_weight")
    _repack_note("sparse", w=w, out=out, kv=kv, cin=cin, cout=cout, adjoint=0, reverse_k=0)
    return out


def sparse_pack_weight_adjoint(weight, reverse_offsets):
    """Packed weight of the (Cout -> Cin) conv that computes the data gradient of the layer with `weight` (kz,ky,kx,Cin,Cout):
    per offset W_k^T, offsets reversed for a submanifold layer (whose gradient runs on the forward neighbour table). One launch
    from the stored weight (no flip / transpose copies)."""
    w = weight.detach().to(torch.float32).contiguous()
    cin, cout = w.shape[-2], w.shape[-1]
    kv = w.numel() // (cin * cout)
    out = torch.empty_like(w).view(-1)
    check(lib.sessd_sparse_pack_weight_adjoint(w.data_ptr(), kv, cin, cout, 1 if reverse_offsets else 0, out.data_ptr(), _stream()),
          "sparse_pack_weight_adjoint")
    _repack_note("sparse", w=w, out=out, kv=kv, cin=cin, cout=cout, adjoint=1, reverse_k=1 if reverse_offsets else 0)
    return out


def sparse_conv(in_feat, nbr, tile_mask, n_out_dev, packed_weight, cin, cout, scale=None, shift=None, relu=True,
                out=None, dense_out=None, out_indices=None, dense_dims=None, cout_split=0, depth=0, offset_split=0, share_w=0, perm=None, tiles_per_wave=1):
    """tiles_per_wave = 2 / 4 (large levels; plain tiles only): a wave walks that many tiles and fetches the next tile's neighbour
    rows under the current tile's MFMAs -- the same bits. perm (with tile_mask = the job's tile_mask_sorted): offset-pattern tiles of a SparseChain built with sort_tiles -- the same
    bits as the plain tiles. cout_split (0 heuristic | 1, 2, 4) and depth (0 default | 2..4 operand sets in flight) only tune the launch: results are
    bit-identical for every choice. offset_split = 1 (small levels; ignored with dense_out): the four waves of a workgroup split
    the kernel offsets of a tile by k % 4 -- the same bits for every cout_split / depth, last-bit differences from offset_split 0.
    share_w = 1 (large levels; ignored with dense_out or where cin % 16 != 0): the four tiles of a workgroup share W[k] through LDS --
    the same bits as the plain kernel."""
    _req(in_feat, torch.float32, "in_feat")
    kv, cap = nbr.shape
    dd = None
    if dense_out is None:
        if out is None:
            out = torch.empty((cap, cout), dtype=torch.float32, device=in_feat.device)
    else:
        dd = _i3(dense_dims)
    check(lib.sessd_sparse_conv_sorted(in_feat.data_ptr(), cin, nbr.data_ptr(), tile_mask.data_ptr(), kv, n_out_dev.data_ptr(),
                                       cap, packed_weight.data_ptr(), _p(scale), _p(shift), 1 if relu else 0, _p(out), cout,
                                       _p(out_indices), _p(dense_out), 0 if dd is None else dd.data_ptr(),
                                       int(cout_split) + 256 * int(depth) + 65536 * int(bool(offset_split)) + 131072 * int(bool(share_w))
                                       + ({1: 0, 2: 1, 4: 2}[int(tiles_per_wave)] << 20), _p(perm), _stream()),
          "sparse_conv")
    return out if dense_out is None else dense_out


def sparse_renumber_sites(indices, n_dev, feat, site_hash, batch):
    """EXPERIMENTAL (not yet validated on hardware): the level's sites renumbered by (batch, z, y) grid row. Returns
    (out_indices, out_feat); `site_hash` (SiteHash of the level) is updated in place to the new rows."""
    _req(indices, torch.int32, "indices")
    _req(feat, torch.float32, "feat")
    cap, ch = indices.shape[0], feat.shape[1]
    out_idx, out_feat = torch.empty_like(indices), torch.empty_like(feat)
    ws = workspace(lib.sessd_sparse_renumber_workspace_bytes(int(batch), site_hash._dims_t.data_ptr()), indices.device, "renumber")
    check(lib.sessd_sparse_renumber_sites(indices.data_ptr(), n_dev.data_ptr(), cap, int(batch), site_hash._dims_t.data_ptr(),
                                          feat.data_ptr(), ch, site_hash.keys.data_ptr(), site_hash.vals.data_ptr(),
                                          site_hash.capacity, out_idx.data_ptr(), out_feat.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _stream()), "sparse_renumber_sites")
    return out_idx, out_feat


class BnReluTrainFunction(torch.autograd.Function):
    """Train-mode BatchNorm1d + optional ReLU over the first *n_dev rows of a sparse feature table, statistics and both passes on
    the HIP kernels of csrc/bn_train.hip; running statistics are updated in place like torch.nn.BatchNorm1d does."""

    @staticmethod
    def forward(ctx, x, n_dev, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.float().contiguous()
        _req(x, torch.float32, "x")
        cap, C = x.shape
        dev = x.device
        y = torch.empty_like(x)   # the kernel writes rows >= *n_dev as zeros
        mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = zeroed_workspace(lib.sessd_bn_relu_train_workspace_bytes(C), dev, "bn")
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        check(lib.sessd_bn_relu_train_fwd(x.data_ptr(), n_dev.data_ptr(), cap, C, g.data_ptr(), b.data_ptr(), float(eps),
                                          float(momentum), 1 if relu else 0, _p(running_mean), _p(running_var), y.data_ptr(),
                                          mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "bn_relu_train_fwd")
        ctx.save_for_backward(x, y, g, mean, invstd, n_dev)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, g, mean, invstd, n_dev = ctx.saved_tensors
        dy = dy.float().contiguous()
        cap, C = x.shape
        dx = torch.empty_like(x)
        dg, db = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
        ws = zeroed_workspace(lib.sessd_bn_relu_train_workspace_bytes(C), x.device, "bn")
        check(lib.sessd_bn_relu_train_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), n_dev.data_ptr(), cap, C, g.data_ptr(),
                                          mean.data_ptr(), invstd.data_ptr(), 1 if ctx.relu else 0, dx.data_ptr(), dg.data_ptr(),
                                          db.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "bn_relu_train_bwd")
        return dx, None, dg, db, None, None, None, None, None


_NBT_DEFER = [False]
_NBT_PENDING = []


class deferred_batch_counts:
    """Inside this context the `num_batches_tracked += 1` of every fused train-mode BatchNorm call is collected and applied as ONE
    multi-tensor launch on exit (56 one-element launches per SE-SSD iteration otherwise). Layers with momentum=None need the
    count at once and are not deferred."""

    def __enter__(self):
        self.prev = _NBT_DEFER[0]
        _NBT_DEFER[0] = True
        return self

    def __exit__(self, *exc):
        _NBT_DEFER[0] = self.prev
        if not self.prev and _NBT_PENDING:
            counts = {}   # a layer applied twice appears twice: one entry per tensor (duplicates in one multi-tensor launch race)
            for t in _NBT_PENDING:
                counts[id(t)] = (t, counts.get(id(t), (t, 0))[1] + 1)
            _NBT_PENDING.clear()
            torch._foreach_add_([t for t, _ in counts.values()], [n for _, n in counts.values()])
        return False


def _bn_momentum(bn):
    """Counts the batch (torch.nn.modules.batchnorm._BatchNorm.forward) and returns the layer's update factor."""
    nbt = bn.num_batches_tracked
    if bn.momentum is not None:
        if nbt is not None:
            if _NBT_DEFER[0]:
                _NBT_PENDING.append(nbt)
            else:
                nbt.add_(1)
        return bn.momentum
    if nbt is None:
        return 0.0
    nbt.add_(1)   # momentum=None: cumulative moving average, factor 1 / number of batches seen
    return 1.0 / float(nbt.item())


def bn_relu_train(x, n_dev, bn, relu=True):
    """x (cap, C) float32 on the device, rows < n_dev[0] valid; bn: a torch.nn.BatchNorm1d in train mode (its running statistics are
    updated in place, num_batches_tracked incremented)."""
    mom = _bn_momentum(bn)
    if sync_bn_active():
        return SyncBnReluTrainFunction.apply(x, n_dev, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, relu)
    return BnReluTrainFunction.apply(x, n_dev, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, relu)


# ---------------------------------------------------------------------------------------------------------------- SyncBN
# The reference's distributed training converts every BatchNorm to SyncBN (det3d/torchie/apis/train_sessd.py:286-294; semantics
# det3d/ops/syncbn/syncbn.py:37-103): batch statistics over the batches of ALL ranks. set_sync_bn(True) switches the fused
# train-mode BatchNorm passes (sparse tables and dense maps) to their split form -- statistics launch, ONE all-reduce of the
# float64 totals (2C + 1 numbers forward, 2C backward), finalise + apply -- in every process group of more than one rank; with
# one rank the all-reduce is skipped and the result equals the fused form bit for bit.
_SYNC_BN = {"on": False, "group": None, "reduce": None}


_KEEP = object()


def set_sync_bn(on=True, group=_KEEP, reduce_fn=_KEEP):
    """Switch the split (statistics | all-reduce | apply) BatchNorm passes on or off. group: the process group of the all-reduce
    (None = WORLD); reduce_fn(tensor) (tests): replaces dist.all_reduce on the float64 totals. An argument that is not passed
    keeps its current value, so that toggling the switch (TrainStep does, around every iteration) does not forget a configured
    group (round-4 advisor finding)."""
    _SYNC_BN["on"] = bool(on)
    if group is not _KEEP:
        _SYNC_BN["group"] = group
    if reduce_fn is not _KEEP:
        _SYNC_BN["reduce"] = reduce_fn


def sync_bn_state():
    """(on, group, reduce_fn): hand the tuple back to restore_sync_bn()."""
    return (_SYNC_BN["on"], _SYNC_BN["group"], _SYNC_BN["reduce"])


def restore_sync_bn(state):
    _SYNC_BN.update(on=bool(state[0]), group=state[1], reduce=state[2])


def sync_bn_active():
    return _SYNC_BN["on"]


def _sync_reduce(t):
    if _SYNC_BN["reduce"] is not None:
        _SYNC_BN["reduce"](t)
        return
    from .dist import collectives_enabled
    import torch.distributed as dist
    if collectives_enabled(_SYNC_BN["group"]):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SyncBN all-reduces cannot be captured in a hipGraph here: run the iteration eagerly at world size > 1 "
                               "(TrainStep.capture refuses it), or switch SyncBN off (rank-local statistics)")
        dist.all_reduce(t, group=_SYNC_BN["group"])


class SyncBnReluTrainFunction(torch.autograd.Function):
    """BnReluTrainFunction with the statistics of ALL ranks (sessd_bn_relu_train_stats / _apply / _bwd_stats / _bwd_apply)."""

    @staticmethod
    def forward(ctx, x, n_dev, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.float().contiguous()
        _req(x, torch.float32, "x")
        cap, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_bn_relu_train_workspace_bytes(C), dev, "bn")
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        check(lib.sessd_bn_relu_train_stats(x.data_ptr(), n_dev.data_ptr(), cap, C, sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "bn_relu_train_stats")
        _sync_reduce(sums)
        check(lib.sessd_bn_relu_train_apply(x.data_ptr(), n_dev.data_ptr(), cap, C, g.data_ptr(), b.data_ptr(), float(eps), float(momentum),
                                            1 if relu else 0, sums.data_ptr(), _p(running_mean), _p(running_var), y.data_ptr(),
                                            mean.data_ptr(), invstd.data_ptr(), _stream()), "bn_relu_train_apply")
        ctx.save_for_backward(x, y, g, mean, invstd, n_dev, sums)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, g, mean, invstd, n_dev, fwd_sums = ctx.saved_tensors
        dy = dy.float().contiguous()
        cap, C = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_bn_relu_train_workspace_bytes(C), dev, "bn")
        scratch = torch.empty(int(lib.sessd_bn_sync_scratch_bytes(C)), dtype=torch.uint8, device=dev)
        check(lib.sessd_bn_relu_train_bwd_stats(dy.data_ptr(), x.data_ptr(), y.data_ptr(), n_dev.data_ptr(), cap, C, mean.data_ptr(),
                                                invstd.data_ptr(), 1 if ctx.relu else 0, dg.data_ptr(), db.data_ptr(), sums.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream()), "bn_relu_train_bwd_stats")
        _sync_reduce(sums)
        check(lib.sessd_bn_relu_train_bwd_apply(dy.data_ptr(), x.data_ptr(), y.data_ptr(), n_dev.data_ptr(), cap, C, g.data_ptr(),
                                                mean.data_ptr(), invstd.data_ptr(), 1 if ctx.relu else 0, sums.data_ptr(),
                                                fwd_sums.data_ptr(), dx.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()),
              "bn_relu_train_bwd_apply")
        return dx, None, dg, db, None, None, None, None, None


class SyncBn2dReluTrainFunction(torch.autograd.Function):
    """Bn2dReluTrainFunction with the statistics of ALL ranks (the dense layout's split entry points; ReLU mask from x)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.float().contiguous()
        _req(x, torch.float32, "x")
        B, C, H, W = x.shape
        dev = x.device
        y = torch.empty_like(x)
        mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev, "bn2d")
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        check(lib.sessd_bn2d_relu_train_stats(x.data_ptr(), B, C, H * W, sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "bn2d_relu_train_stats")
        _sync_reduce(sums)
        check(lib.sessd_bn2d_relu_train_apply(x.data_ptr(), B, C, H * W, g.data_ptr(), b.data_ptr(), float(eps), float(momentum),
                                              1 if relu else 0, sums.data_ptr(), _p(running_mean), _p(running_var), y.data_ptr(),
                                              mean.data_ptr(), invstd.data_ptr(), _stream()), "bn2d_relu_train_apply")
        ctx.save_for_backward(x, g, b, mean, invstd, sums)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, mean, invstd, fwd_sums = ctx.saved_tensors
        dy = dy.float().contiguous()
        B, C, H, W = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        ws = zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev, "bn2d")
        scratch = torch.empty(int(lib.sessd_bn_sync_scratch_bytes(C)), dtype=torch.uint8, device=dev)
        check(lib.sessd_bn2d_relu_train_bwd_stats(dy.data_ptr(), x.data_ptr(), 0, B, C, H * W, g.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                  invstd.data_ptr(), 1 if ctx.relu else 0, dg.data_ptr(), db.data_ptr(), sums.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream()), "bn2d_relu_train_bwd_stats")
        _sync_reduce(sums)
        check(lib.sessd_bn2d_relu_train_bwd_apply(dy.data_ptr(), x.data_ptr(), 0, B, C, H * W, g.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                  invstd.data_ptr(), 1 if ctx.relu else 0, sums.data_ptr(), fwd_sums.data_ptr(),
                                                  dx.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()), "bn2d_relu_train_bwd_apply")
        return dx, dg, db, None, None, None, None, None


BN_MASK_FROM_X = os.environ.get("SESSD_BN_MASK_FROM_Y", "0") == "0"   # dense train-mode BatchNorm backward: ReLU mask from x, not y


class Bn2dReluTrainFunction(torch.autograd.Function):
    """Train-mode BatchNorm2d + optional ReLU on a dense (B, C, H, W) map (H * W % 4 == 0), both passes on csrc/bn_train.hip."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        x = x.float().contiguous()
        _req(x, torch.float32, "x")
        B, C, H, W = x.shape
        dev = x.device
        y = torch.empty_like(x)
        mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), dev, "bn2d")
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        check(lib.sessd_bn2d_relu_train_fwd(x.data_ptr(), B, C, H * W, g.data_ptr(), b.data_ptr(), float(eps), float(momentum),
                                            1 if relu else 0, _p(running_mean), _p(running_var), y.data_ptr(), mean.data_ptr(),
                                            invstd.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "bn2d_relu_train_fwd")
        # the backward re-derives the ReLU mask from x (sessd_bn2d_relu_train_bwd_x): y is not kept for it
        ctx.mask_from_x = BN_MASK_FROM_X
        ctx.save_for_backward(x, g, b, mean, invstd, *(() if ctx.mask_from_x else (y,)))
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, mean, invstd = ctx.saved_tensors[:5]
        dy = dy.float().contiguous()
        B, C, H, W = x.shape
        dx = torch.empty_like(x)
        dg, db = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
        ws = zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), x.device, "bn2d")
        if not ctx.mask_from_x:
            y = ctx.saved_tensors[5]
            check(lib.sessd_bn2d_relu_train_bwd(dy.data_ptr(), x.data_ptr(), y.data_ptr(), B, C, H * W, g.data_ptr(), mean.data_ptr(),
                                                invstd.data_ptr(), 1 if ctx.relu else 0, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream()), "bn2d_relu_train_bwd")
            return dx, dg, db, None, None, None, None, None
        check(lib.sessd_bn2d_relu_train_bwd_x(dy.data_ptr(), x.data_ptr(), B, C, H * W, g.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                              invstd.data_ptr(), 1 if ctx.relu else 0, dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream()), "bn2d_relu_train_bwd_x")
        return dx, dg, db, None, None, None, None, None


BN2D_MAX_CHANNELS = 1024  # csrc/bn_train.hip: per-channel arrival counters of the finisher block


def bn2d_relu_train(x, bn, relu=True):
    """x (B, C, H, W) float32 on the device; bn: a torch.nn.BatchNorm2d in train mode with affine parameters (running statistics
    updated in place, num_batches_tracked incremented). Falls back to the torch module where the kernel's layout assumption
    (H * W divisible by 4, at most BN2D_MAX_CHANNELS = 1024 channels) does not hold."""
    if (x.shape[2] * x.shape[3]) % 4 or bn.weight is None or x.shape[1] > BN2D_MAX_CHANNELS:
        y = bn(x)
        return torch.relu(y) if relu else y
    mom = _bn_momentum(bn)
    if sync_bn_active():
        return SyncBn2dReluTrainFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, relu)
    return Bn2dReluTrainFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, relu)


def points_in_bodies(points, planes):
    """points (P, >=3) float32 on the device, planes (M, F, 4) float32 on the device [nx, ny, nz, d] with inward normals ->
    (P, M) bool on the device (strictly inside every face)."""
    _req(points, torch.float32, "points")
    _req(planes, torch.float32, "planes")
    P, M, F = points.shape[0], planes.shape[0], planes.shape[1]
    words = (M + 31) // 32
    mask = torch.zeros((P, words), dtype=torch.int32, device=points.device)
    check(lib.sessd_points_in_bodies(points.data_ptr(), P, points.shape[1], planes.data_ptr(), M, F, mask.data_ptr(), _stream()),
          "points_in_bodies")
    bit = torch.arange(M, device=points.device)
    return ((mask[:, bit // 32] >> (bit % 32)) & 1).bool()


def box3d_overlap_eval(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0):
    """det3d/datasets/utils/eval.py:324-367 on the device: boxes (N,7), qboxes (K,7) float64 device tensors -> (N,K) float64."""
    _req(boxes, torch.float64, "boxes")
    _req(qboxes, torch.float64, "qboxes")
    out = torch.empty((boxes.shape[0], qboxes.shape[0]), dtype=torch.float64, device=boxes.device)
    check(lib.sessd_box3d_overlap_eval(boxes.data_ptr(), boxes.shape[0], qboxes.data_ptr(), qboxes.shape[0], int(criterion),
                                       int(z_axis), float(z_center), out.data_ptr(), _stream()), "box3d_overlap_eval")
    return out


class KittiStatistics:
    """Device side of eval_class_v3 (det3d/datasets/kitti/eval.py:174-319) for one (class, difficulty): the frames' overlap
    matrices and cleaned annotations uploaded once (CSR layout), then per overlap threshold: first matching pass -> recall
    thresholds -> second pass over (frame, threshold) -> ordered reduction. Only the final (T,4) table returns to the host."""

    def __init__(self, overlaps, gt_datas, dt_datas, ign_gts, ign_dets, dontcares, device):
        import numpy as np
        F = len(overlaps)
        self.F, self.dev = F, device
        n_gt = np.array([g.shape[0] for g in gt_datas], np.int64)
        n_dt = np.array([d.shape[0] for d in dt_datas], np.int64)
        n_dc = np.array([c.shape[0] for c in dontcares], np.int64)
        off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        self.gt_off_h, self.dt_off_h = off(n_gt), off(n_dt)
        ov_sizes = n_gt * n_dt
        ov_off = np.concatenate([[0], np.cumsum(ov_sizes)[:-1]]).astype(np.int64) if F else np.zeros((0,), np.int64)
        # overlaps[i] is (n_det, n_gt) (calculate_iou_partly(dt, gt)), float64 as the host code carries them
        flat = np.concatenate([np.ascontiguousarray(o, np.float64).reshape(-1) for o in overlaps]) if F else np.zeros((0,), np.float64)
        cat = lambda lst, w, dt: (np.concatenate(lst, 0) if len(lst) and sum(x.shape[0] for x in lst) else np.zeros((0, w), dt)).astype(dt)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.ov, self.ov_off = t(flat if flat.size else np.zeros((1,), np.float64)), t(ov_off if F else np.zeros((1,), np.int64))
        self.gt_off, self.dt_off, self.dc_off = t(self.gt_off_h), t(self.dt_off_h), t(off(n_dc))
        pad = lambda a, w, dt: a if a.shape[0] else np.zeros((1, w), dt)
        self.gt = t(pad(cat(gt_datas, 5, np.float64), 5, np.float64))
        self.dt = t(pad(cat(dt_datas, 6, np.float64), 6, np.float64))
        self.dc = t(pad(cat(dontcares, 4, np.float64), 4, np.float64))
        ig = np.concatenate(ign_gts).astype(np.int32) if F else np.zeros((0,), np.int32)
        idt = np.concatenate(ign_dets).astype(np.int32) if F else np.zeros((0,), np.int32)
        self.ig, self.idt = t(ig if ig.size else np.zeros((1,), np.int32)), t(idt if idt.size else np.zeros((1,), np.int32))
        self.n_gt_total = int(n_gt.sum())
        self.err = torch.zeros((1,), dtype=torch.int32, device=device)

    def _run(self, metric, min_overlap, thresholds, compute_fp, compute_aos, tp_scores, stats):
        check(lib.sessd_kitti_statistics(self.ov.data_ptr(), self.ov_off.data_ptr(), self.gt_off.data_ptr(), self.dt_off.data_ptr(),
                                         self.dc_off.data_ptr(), self.gt.data_ptr(), self.dt.data_ptr(), self.ig.data_ptr(),
                                         self.idt.data_ptr(), self.dc.data_ptr(), self.F, int(metric), float(min_overlap),
                                         _p(thresholds), 0 if thresholds is None else int(thresholds.shape[0]),
                                         1 if compute_fp else 0, 1 if compute_aos else 0, _p(tp_scores), _p(stats),
                                         self.err.data_ptr(), _stream()), "kitti_statistics")

    def precision_table(self, metric, min_overlap, num_valid_gt, compute_aos=False, num_pts=41):
        """-> (thresholds (n,), pr (n,4) [tp, fp, fn, similarity]) as numpy float64, n <= num_pts."""
        import numpy as np
        tp_scores = torch.empty((max(self.n_gt_total, 1),), dtype=torch.float64, device=self.dev)
        self._run(metric, min_overlap, None, False, False, tp_scores, None)
        sc = tp_scores[:self.n_gt_total]
        sc = sc[~torch.isnan(sc)]
        if sc.numel() == 0 or num_valid_gt <= 0:
            return np.zeros((0,)), np.zeros((0, 4))
        sc, _ = torch.sort(sc, descending=True)
        thr = torch.zeros((num_pts,), dtype=torch.float64, device=self.dev)
        n_thr = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        check(lib.sessd_kitti_thresholds(sc.data_ptr(), int(sc.numel()), int(num_valid_gt), int(num_pts), thr.data_ptr(),
                                         n_thr.data_ptr(), _stream()), "kitti_thresholds")
        n = int(n_thr.item())
        thr = thr[:n].contiguous()
        stats = torch.empty((self.F, n, 4), dtype=torch.float64, device=self.dev)
        self._run(metric, min_overlap, thr, True, compute_aos, None, stats)
        pr = torch.empty((n, 4), dtype=torch.float64, device=self.dev)
        check(lib.sessd_kitti_reduce(stats.data_ptr(), self.F, n, pr.data_ptr(), _stream()), "kitti_reduce")
        if int(self.err.item()):
            raise SessdError("a frame has more than 256 detections: not supported by the device evaluation")
        return thr.cpu().numpy(), pr.cpu().numpy()


def points_rigid_moves_(points, planes, centers, loc, rot, valid):
    """In place on the device: preprocess.py:544-560 points_transform_. points (P, >=3) f32 device; planes (M,6,4) f32 device;
    centers / loc (M,3), rot (M,) yaw changes and valid (M,) given as host arrays (float64 as the sampler draws them)."""
    import numpy as np
    _req(points, torch.float32, "points")
    _req(planes, torch.float32, "planes")
    M = planes.shape[0]
    dev = points.device
    rot = np.asarray(rot, np.float64)
    sc = np.stack([np.sin(rot), np.cos(rot)], 1).astype(np.float32)  # numpy casts sin / cos of the float64 angle to the point dtype
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)
    c, l, r, v = t(centers, np.float64), t(loc, np.float64), t(sc, np.float32), t(np.asarray(valid).astype(np.uint8), np.uint8)
    check(lib.sessd_points_rigid_moves(points.data_ptr(), points.shape[0], points.shape[1], planes.data_ptr(), c.data_ptr(),
                                       l.data_ptr(), r.data_ptr(), v.data_ptr(), M, _stream()), "points_rigid_moves")
    return points


def points_global_transform_(points, flip, angle, scale, raw_copy=None):
    """In place on the device: random_flip_v2 + global_rotation_v3 + global_scaling_v3 (preprocess.py:896-945) with the host's
    draws; raw_copy (same shape, device) optionally receives the untransformed cloud."""
    import numpy as np
    _req(points, torch.float32, "points")
    if raw_copy is not None:
        _req(raw_copy, torch.float32, "raw_copy")
    check(lib.sessd_points_global_transform(points.data_ptr(), points.shape[0], points.shape[1], 1 if flip else 0,
                                            float(np.float32(np.sin(angle))), float(np.float32(np.cos(angle))),
                                            float(np.float32(scale)), _p(raw_copy), _stream()), "points_global_transform")
    return points


def farthest_point_sample(points, k):
    """Indices (k,) int64 on the device of k of the rows of points (n, >=3) float32 device tensor, n <= 4096: sa_da_v2's thinning
    (start at row 0, farthest from the selection next, lowest index on ties)."""
    _req(points, torch.float32, "points")
    n = points.shape[0]
    out = torch.empty((k,), dtype=torch.int32, device=points.device)
    check(lib.sessd_farthest_point_sample(points.data_ptr(), n, points.shape[1], int(k), out.data_ptr(), _stream()), "farthest_point_sample")
    return out.long()


def points_compact(points, keep, out=None):
    """Order-preserving compaction on the device: rows of points (P, C) whose keep flag (P,) bool / uint8 is set.
    Returns (out (cap, C), n_out device int32 (1,)); nothing synchronises."""
    _req(points, torch.float32, "points")
    k = keep.to(torch.uint8).contiguous()
    P, C = points.shape
    if out is None:
        out = torch.empty((max(P, 1), C), dtype=torch.float32, device=points.device)
    n_out = torch.zeros((1,), dtype=torch.int32, device=points.device)
    ws = workspace(lib.sessd_points_compact_workspace_bytes(P), points.device, "compact")
    check(lib.sessd_points_compact(points.data_ptr(), k.data_ptr(), P, C, out.data_ptr(), out.shape[0], n_out.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream()), "points_compact")
    return out, n_out


def sparse_rulebook_transpose(nbr, n_out_dev, n_in_cap):
    """Rulebook of the data-gradient pass: nbr_t (kv, n_in_cap) with nbr_t[k][i] = j <=> nbr[k][j] = i, and its tile masks."""
    kv, cap = nbr.shape
    nbr_t = torch.empty((kv, n_in_cap), dtype=torch.int32, device=nbr.device)
    tm_t = torch.empty(((n_in_cap + 15) // 16,), dtype=torch.int32, device=nbr.device)
    check(lib.sessd_sparse_rulebook_transpose(nbr.data_ptr(), kv, n_out_dev.data_ptr(), cap, n_in_cap, nbr_t.data_ptr(),
                                              tm_t.data_ptr(), _stream()), "sparse_rulebook_transpose")
    return nbr_t, tm_t


def sparse_conv_wgrad(in_feat, grad_out, nbr, tile_mask, n_out_dev, cin, cout):
    """grad_weight (kv, cin, cout) of sparse_conv(in_feat, nbr, ...) given grad_out (n_out_cap, cout)."""
    _req(in_feat, torch.float32, "in_feat")
    _req(grad_out, torch.float32, "grad_out")
    kv, cap = nbr.shape
    if grad_out.shape[0] < cap or grad_out.shape[1] != cout or in_feat.shape[1] != cin:
        raise ValueError("grad_out must be (n_out_cap, cout) and in_feat (n_in, cin)")
    gw = torch.empty((kv, cin, cout), dtype=torch.float32, device=in_feat.device)
    ws = torch.empty(int(lib.sessd_sparse_conv_wgrad_workspace_bytes(kv, cin, cout)), dtype=torch.uint8, device=in_feat.device)
    check(lib.sessd_sparse_conv_wgrad(in_feat.data_ptr(), cin, grad_out.data_ptr(), cout, nbr.data_ptr(), tile_mask.data_ptr(),
                                      kv, n_out_dev.data_ptr(), cap, gw.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "sparse_conv_wgrad")
    return gw


# ------------------------------------------------------------------ dense BEV convolutions
class Launch:
    """One sessd_conv2d_mfma launch of a PackedConv: the taps' input offsets dy / dx (int32 host tensors), the step of its tile
    space in the input (in_mul) and output (out_mul) maps, the output parity class (py, px) it writes, and `view` = (weight,
    out_stride, in_stride, tap offsets): the strided view of the stored weight that its packings are made from.
    wpk, the weight in MFMA fragment order, is packed when first read: a 3x3 stride-1 layer that runs on a Winograd kernel never
    needs it (21 wasted pack launches per training iteration before)."""
    __slots__ = ("dy", "dx", "in_mul", "out_mul", "py", "px", "ntaps", "view", "_wpk", "_owner")

    def __init__(self, dy, dx, in_mul, out_mul, py, px, view):
        self.dy, self.dx, self.in_mul, self.out_mul, self.py, self.px, self.view = dy, dx, in_mul, out_mul, py, px, view
        self.ntaps = len(view[3])
        self._wpk = self._owner = None   # the owner is the PackedConv that takes the launch

    @property
    def wpk(self):
        if self._wpk is None:
            pc = self._owner
            self._wpk = pc._make(lambda: _pack_taps_view(*self.view, pc.cout, pc.cin))
        return self._wpk


class PackedConv:
    """A conv layer lowered to one or more sessd_conv2d_mfma launches, with every other packing of its weight that a dense kernel
    family takes. kind "conv": Conv2d(k in {1, 3}, stride, padding k // 2), one launch; "deconv": ConvTranspose2d(3, 2, 1, 1), one
    launch per output parity class; "deconv_ks": ConvTranspose2d(s, stride s), s * s one-tap launches.
    w3 = (weight, adjoint) of a 3x3 stride-1 conv: what the Winograd packings are made from, on demand; wt = the (cin, cout, 3, 3)
    weight of a "deconv": its launches are packed now, for the argument block of the merged launch, the split planes on demand."""

    def __init__(self, launches, cin, cout, kind, stride, w3=None, wt=None):
        self.launches = launches  # list of Launch
        self.cin, self.cout, self.kind, self.stride = cin, cout, kind, stride
        self._w3, self._wt = w3, wt
        self._upk = None
        self._upk_sk = [None, None, None, None]
        self._sk = None      # argument block of sessd_conv2d_sk (tile_cfg 30), made when first asked for
        self._wsplit = None
        self._wsplit_s2 = None
        self._registry = None  # RepackRegistry that keeps this object fresh (training step), else None
        for la in launches:
            la._owner = self
        self.wpk4 = self.ntaps4 = self.dy4 = self.dx4 = None
        if wt is not None:   # host-side argument blocks of the single merged launch (sessd_deconv2d_s2_mfma)
            self.wpk4 = (ctypes.c_void_p * 4)(*[la.wpk.data_ptr() for la in launches])
            self.ntaps4 = torch.tensor([la.ntaps for la in launches], dtype=torch.int32)
            self.dy4 = torch.zeros((4, 4), dtype=torch.int32)
            self.dx4 = torch.zeros((4, 4), dtype=torch.int32)
            for c, la in enumerate(launches):
                self.dy4[c, :la.ntaps] = la.dy
                self.dx4[c, :la.ntaps] = la.dx

    def _make(self, make):
        """Make a packing now -- through the registry, which records it as a job of its batched re-pack, if there is one."""
        return self._registry.create(make) if self._registry is not None else make()

    def out_hw(self, H, W):
        """(Ho, Wo) of the layer on an (H, W) map"""
        s = self.stride
        return ((H + s - 1) // s, (W + s - 1) // s) if self.kind == "conv" else (s * H, s * W)

    def tile_hw(self, H, W):
        """The pixel space the launches cut their tiles from: the output map of a conv, the INPUT map of a transposed conv (each of
        its launches writes one output parity class)."""
        return self.out_hw(H, W) if self.kind == "conv" else (H, W)

    @property
    def is_3x3_s1(self):
        """a 3x3 stride-1 conv: the layers the Winograd kernels (tile_cfg 20 - 25) and the LDS variant (10) are written for"""
        return self._w3 is not None

    @property
    def upk(self):
        """U = G g G^T packed for sessd_conv3x3_winograd (tile_cfg 20 / 21); None if the layer is not eligible."""
        if self._upk is None and self.is_3x3_s1 and self.cin % 8 == 0:
            self._upk = self._make(lambda: pack_winograd(self._w3[0], adjoint=self._w3[1]))
        return self._upk

    def upk_sk(self, shape):
        """U packed for sessd_conv3x3_winograd_sk (tile_cfg 22 / 23 / 24 / 25 = shape 0 / 1 / 2 / 3); None if not eligible."""
        if self._upk_sk[shape] is None and self.is_3x3_s1 and self.cin % (16, 8, 16, 16)[shape] == 0:
            self._upk_sk[shape] = self._make(lambda: pack_winograd_sk(self._w3[0], shape, adjoint=self._w3[1]))
        return self._upk_sk[shape]

    def wsplit(self):
        """A ConvTranspose2d(3, 2, 1, 1) weight as three bf16 planes for sessd_deconv2d_s2_pair_split_active
        (pack_deconv2d_s2_split), made when first asked for; None if the layer is not eligible (not that layer kind, cin % 16)."""
        if self._wt is None or self.cin % 16:
            return None
        if self._registry is not None:   # a training step's weights change under the registry, which has no job for this packing
            return pack_deconv2d_s2_split(self._wt)
        if self._wsplit is None:
            self._wsplit = pack_deconv2d_s2_split(self._wt)
        return self._wsplit

    def wsplit_s2(self):
        """A Conv2d(3, stride 2, padding 1) weight as three bf16 planes for sessd_conv2d_s2_split_active (pack_conv2d_s2_split),
        made when first asked for; None if the layer is not eligible (not a 3x3 stride-2 conv, cin % 16)."""
        if self.kind != "conv" or self.stride != 2 or self.launches[0].ntaps != 9 or self.cin % 16:
            return None
        w = self.launches[0].view[0]   # the stored (cout, cin, 3, 3) weight
        if self._registry is not None:   # a training step's weights change under the registry, which has no job for this packing
            return pack_conv2d_s2_split(w)
        if self._wsplit_s2 is None:
            self._wsplit_s2 = pack_conv2d_s2_split(w)
        return self._wsplit_s2

    def sk_args(self):
        """Host-side argument block of sessd_conv2d_sk (tile_cfg 30): the launches' weights re-packed in the kernel's LDS image
        (one launch each) + tap tables; None if the layer is not eligible (cin % 16, more than four launches)."""
        if self._sk is None:
            n = len(self.launches)
            if self.cin % 16 or n > 4:
                return None
            ncg = (self.cout + 127) // 128
            wpk, dy, dx = [], (ctypes.c_int * (9 * n))(), (ctypes.c_int * (9 * n))()
            for c, la in enumerate(self.launches):
                w, so, sc, taps = la.view
                nt = len(taps)
                out = torch.empty((ncg, self.cin // 16, nt, 2048), dtype=torch.float32, device=w.device)
                check(lib.sessd_conv2d_sk_pack(w.data_ptr(), int(so), int(sc), (ctypes.c_int * nt)(*[int(t) for t in taps]), nt,
                                               self.cout, self.cin, out.data_ptr(), _stream()), "conv2d_sk_pack")
                wpk.append(out)
                for t in range(nt):
                    dy[9 * c + t], dx[9 * c + t] = int(la.dy[t]), int(la.dx[t])
            self._sk = dict(wpk=wpk, wptr=(ctypes.c_void_p * n)(*[t.data_ptr() for t in wpk]),
                            ntaps=(ctypes.c_int * n)(*[la.ntaps for la in self.launches]), dy=dy, dx=dx,
                            py=(ctypes.c_int * n)(*[la.py for la in self.launches]),
                            px=(ctypes.c_int * n)(*[la.px for la in self.launches]), n=n)
        return self._sk


def _pack_taps_view(w, out_stride, in_stride, tap_offsets, cout, cin):
    """One launch (sessd_conv2d_pack_taps): [cin/2][ntaps][2][cout_pad32] with out[kp][t][h][o] = w.flat[o * out_stride +
    (2 kp + h) * in_stride + tap_offsets[t]] -- a transposed / flipped / tap-selected view of the stored weight, no intermediate."""
    _req(w, torch.float32, "weight")
    nt = len(tap_offsets)
    cp = (cout + 31) // 32 * 32
    out = torch.empty((cin // 2, nt, 2, cp), dtype=torch.float32, device=w.device)
    check(lib.sessd_conv2d_pack_taps(w.data_ptr(), int(out_stride), int(in_stride), (ctypes.c_int * nt)(*[int(t) for t in tap_offsets]),
                                     nt, cout, cin, out.data_ptr(), _stream()), "conv2d_pack_taps")
    _repack_note("dense", w=w, out=out, so=int(out_stride), sc=int(in_stride), taps=[int(t) for t in tap_offsets], cout=int(cout),
                 cin=int(cin), kind=0, flip=0, layout=0)
    return out


def _conv_view(w, adjoint):
    """(cout, cin, out_stride, in_stride, flip) of a Conv2d weight (Cout, Cin, k, k) used as it is, or as the stride-1 ADJOINT layer
    (correlation with the flipped kernel, channels swapped: the data-gradient pass)."""
    co, ci, kh, kw = w.shape
    kk = kh * kw
    return (ci, co, kk, ci * kk, True) if adjoint else (co, ci, ci * kk, kk, False)


def pack_conv2d(weight, stride=1, padding=None, adjoint=False):
    """nn.Conv2d weight (Cout,Cin,k,k), k in {1,3}; padding k//2 (the only form SSFA / Head use). adjoint (stride 1 only): pack the
    layer whose forward is this layer's data gradient -- flipped taps, channels swapped -- straight from the same weight tensor."""
    w = weight.detach().to(torch.float32).contiguous()
    kh, kw = w.shape[2], w.shape[3]
    assert kh == kw and kh in (1, 3) and not (adjoint and stride != 1)
    co, ci, so, sc, flip = _conv_view(w, adjoint)
    assert ci % 2 == 0
    pad = kh // 2 if padding is None else padding
    assert pad == kh // 2
    kk = kh * kw
    dy = [ky - pad for ky in range(kh) for kx in range(kw)]
    dx = [kx - pad for ky in range(kh) for kx in range(kw)]
    taps = [(kk - 1 - t) if flip else t for t in range(kk)]
    la = Launch(torch.tensor(dy, dtype=torch.int32), torch.tensor(dx, dtype=torch.int32), stride, 1, 0, 0, (w, so, sc, taps))
    # nothing is packed here: the launch's weight and the Winograd packings (tile_cfg 20 - 25) are made when first asked for
    return PackedConv([la], ci, co, "conv", stride, w3=(w, bool(adjoint)) if kh == 3 and stride == 1 else None)


def _winograd_pack(weight, layout, adjoint):
    w = weight.detach().to(torch.float32).contiguous()
    _req(w, torch.float32, "weight")
    assert w.shape[2] == 3 and w.shape[3] == 3
    co, ci, so, sc, flip = _conv_view(w, adjoint)
    if layout == 0:
        out = torch.empty((ci // 2, 4, 2, (co + 31) // 32 * 32, 4), dtype=torch.float32, device=w.device)
    elif layout == 3:   # shape 2 (register-resident output transform): [cout group of 128][k-step][wave 4][parity][cout % 32][xi 16]
        out = torch.empty(((co + 127) // 128, ci // 2, 4, 2, 32, 16), dtype=torch.float32, device=w.device)
    elif layout == 4:   # shape 3 (bf16 matrix cores): three bf16 planes [cout group of 128][wave 8][step][plane 3][lane 64][8 channels]
        out = torch.empty(((co + 127) // 128, 8, ci // 2, 3, 64, 8), dtype=torch.bfloat16, device=w.device)
    else:
        nw, c = ((8, 128), (4, 64))[layout - 1]
        out = torch.empty(((co + c - 1) // c, ci // 2, nw, 2, 32, c // 32, 16 // nw), dtype=torch.float32, device=w.device)
    check(lib.sessd_conv3x3_winograd_pack(w.data_ptr(), so, sc, 1 if flip else 0, co, ci, layout, out.data_ptr(), _stream()),
          "conv3x3_winograd_pack")
    _repack_note("dense", w=w, out=out, so=int(so), sc=int(sc), taps=[], cout=int(co), cin=int(ci), kind=1, flip=1 if flip else 0,
                 layout=int(layout))
    return out


def winograd_u(weight):
    """U = G g G^T of a 3x3 conv weight (Cout,Cin,3,3) -> (Cout, Cin, 16) float32, xi = 4 * row + col (host-side reference of the
    device packer, used by the tests)."""
    w = weight.detach().to(torch.float64)
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64, device=w.device)
    return torch.einsum("ia,ocab,jb->ocij", G, w, G).to(torch.float32).reshape(co, ci, 16)


def pack_winograd_sk(weight, shape=0, adjoint=False):
    """U for sessd_conv3x3_winograd_sk: [ceil(Cout/C)][Cin/2][wave NW][channel parity 2][cout%32][(cout/32)%(C/32)][xi%(16/NW)]
    with xi = (16/NW) * wave + xi%(16/NW) and (NW, C) = (8, 128) for shape 0, (4, 64) for shape 1 -- the 8 A operands of a lane
    and k-step are 32 contiguous bytes. Shape 3: U split into three bfloat16 planes (u = u0 + u1 + u2 exactly), [ceil(Cout/128)]
    [wave 8][step = (cin/16) * 8 + xi%2 * 4 + (cout/32)%4][plane 3][lane = (cin/8)%2 * 32 + cout%32][cin%8], xi = 2 wave + xi%2.
    One launch (sessd_conv3x3_winograd_pack)."""
    return _winograd_pack(weight, 1 + shape, adjoint)


_SK_WS = {}
_SK_WS_RETIRED = []


def _sk_workspace(workspace, need, kind, workgroups, device):
    """The stream-K workspace of a conv2d() launch that takes `need` bytes: the caller's, refused before anything is launched if
    it is too small; without one the buffer of the per-(device, stream and capture, kernel kind, workgroups) cache, grown to need."""
    if workspace is not None:
        if workspace.numel() < need:
            raise ValueError("conv2d: stream-K workspace too small (%d < %d bytes)" % (workspace.numel(), need))
        return workspace
    key = (device.index, _cache_scope(), kind, workgroups)
    workspace = _SK_WS.get(key)
    if workspace is None or workspace.numel() < need:
        if workspace is not None:
            _SK_WS_RETIRED.append(workspace)  # a captured graph may still point at it: never hand its memory back
        workspace = _SK_WS[key] = torch.zeros(need, dtype=torch.uint8, device=device)
    return workspace


def winograd_sk_workspace(batch, h, w, cout, device, workgroups=0, shape=0):
    """Zeroed workspace of sessd_conv3x3_winograd_sk (partial-unit scratch + counters)."""
    with torch.cuda.device(device):
        n = int(lib.sessd_conv3x3_winograd_sk_workspace_bytes(batch, h, w, cout, shape, workgroups))
    if n == 0:
        raise ValueError("winograd_sk_workspace: bad arguments")
    return torch.zeros(n, dtype=torch.uint8, device=device)


def conv2d_sk_workspace(batch, tile_h, tile_w, cout, nclass, device, workgroups=0):
    """Zeroed workspace of sessd_conv2d_sk (partial-unit scratch + counters)."""
    with torch.cuda.device(device):
        n = int(lib.sessd_conv2d_sk_workspace_bytes(batch, tile_h, tile_w, cout, nclass, workgroups))
    if n == 0:
        raise ValueError("conv2d_sk_workspace: bad arguments")
    return torch.zeros(n, dtype=torch.uint8, device=device)


# The three argument groups every dense launch entry takes as structs (include/sessd_hip_types.h); the entries read them before
# they return, so a temporary is enough.
def _epilogue(scale, shift, relu, residual):
    return ConvEpilogue(_p(scale), _p(shift), _p(residual), 1 if relu else 0)


def _tile_list(tile_list, n_list):
    _req(tile_list, torch.int32, "tile_list"); _req(n_list, torch.int32, "n_list")
    return TileList(tile_list.data_ptr(), n_list.data_ptr(), tile_list.numel())


def _stream_k(workspace, workgroups, min_rounds=1):
    return StreamK(workspace.data_ptr(), workspace.numel(), int(workgroups), int(min_rounds))


def _winograd_sk(x, nsets, upk, out, cout, epi, tl, sk, shape):
    _req(x, torch.float32, "x")
    B, ci, H, W = x.shape
    check(lib.sessd_conv3x3_winograd_sk(x.data_ptr(), B, int(nsets), ci, H, W, upk.data_ptr(), out.data_ptr(), int(cout), epi, tl, sk,
                                        int(shape), _stream()), "conv3x3_winograd_sk")
    return out


def conv2d_winograd_sk_sets(x, upk_sets, nsets, cout, scale, shift, relu, out, shape, workspace, workgroups=0, residual=None):
    """sessd_conv3x3_winograd_sk with nsets weight sets: x (nsets * B, Cin, H, W), group s of B batch elements convolved with set s.
    upk_sets = the sets' pack_winograd_sk packings concatenated, scale / shift (nsets, cout) or None; out like x with cout channels."""
    return _winograd_sk(x, nsets, upk_sets, out, cout, _epilogue(scale, shift, relu, residual), None, _stream_k(workspace, workgroups), shape)


def conv2d_winograd_sk_active(x, upk, cout, scale, shift, relu, out, shape, workspace, tile_list, n_list, workgroups=0, residual=None,
                              min_rounds=2):
    """sessd_conv3x3_winograd_sk with a tile list: the stream-K Winograd layer over the listed 2x2-output tiles only (entries image *
    (H/2 * W/2) + tile, count on the device: bev_tile_activity); the other tiles of `out` are left alone."""
    return _winograd_sk(x, 1, upk, out, cout, _epilogue(scale, shift, relu, residual), _tile_list(tile_list, n_list),
                        _stream_k(workspace, workgroups, min_rounds), shape)


def _conv2d_sk(x, pc, epi, out, tl, sk, what):
    """sessd_conv2d_sk (tile_cfg 30) on the layer's argument block pc.sk_args(), over the whole map (tl None) or a tile list"""
    _req(x, torch.float32, "x")
    a = pc.sk_args()
    if a is None:
        raise ValueError("%s (LDS-tiled stream-K) needs cin % 16 == 0" % what)
    B, ci, H, W = x.shape
    la = pc.launches[0]
    check(lib.sessd_conv2d_sk(x.data_ptr(), B, ci, H, W, a["n"], _addr(a["wptr"]), _addr(a["ntaps"]), _addr(a["dy"]), _addr(a["dx"]),
                              la.in_mul, *pc.tile_hw(H, W), out.data_ptr(), pc.cout, *pc.out_hw(H, W), la.out_mul, _addr(a["py"]),
                              _addr(a["px"]), epi, tl, sk, _stream()), "conv2d_sk")
    return out


def conv2d_sk_active(x, pc, scale, shift, relu, out, workspace, tile_list, n_list, workgroups=0, residual=None, min_rounds=4):
    """sessd_conv2d_sk with a tile list: the LDS-tiled stream-K layer (tile_cfg 30: stride-2 / 1x1 conv, or the four classes of a
    transposed conv) over the listed 2x2 tiles of its tile space only (entries image * (th/2 * tw/2) + tile, count on the device); the
    other output pixels of `out` are left alone."""
    return _conv2d_sk(x, pc, _epilogue(scale, shift, relu, residual), out, _tile_list(tile_list, n_list),
                      _stream_k(workspace, workgroups, min_rounds), "conv2d_sk_active")


def _conv2d_mfma(x, pc, la, epi, out, tl, tile_cfg):
    """sessd_conv2d_mfma: launch `la` of the layer on the direct kernel, over the whole map (tl None) or a tile list"""
    B, ci, H, W = x.shape
    check(lib.sessd_conv2d_mfma(x.data_ptr(), B, ci, H, W, la.wpk.data_ptr(), la.ntaps, la.dy.data_ptr(), la.dx.data_ptr(), la.in_mul,
                                *pc.tile_hw(H, W), out.data_ptr(), pc.cout, *pc.out_hw(H, W), la.out_mul, la.py, la.px, epi, tl,
                                int(tile_cfg), _stream()), "conv2d_mfma")
    return out


def conv2d_mfma_active(x, pc, scale, shift, relu, out, tile_list, n_list, tile_cfg=11, residual=None):
    """sessd_conv2d_mfma with a tile list: a 1x1 layer on the direct kernel (tile_cfg 3 / 4 / 11 / 12) over the listed 2x2 tiles only;
    the computed pixels carry the bits of the whole-map launch."""
    _req(x, torch.float32, "x")
    assert pc.kind == "conv" and pc.stride == 1 and len(pc.launches) == 1 and pc.launches[0].ntaps == 1 and x.shape[1] % 8 == 0
    return _conv2d_mfma(x, pc, pc.launches[0], _epilogue(scale, shift, relu, residual), out, _tile_list(tile_list, n_list), tile_cfg)


def _pair_args(x, pc_a, pc_b, weights, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, residual_a, residual_b, tile_list, n_list):
    """what the launches of a transposed-conv pair take but for their tile_cfg: the input, the two layers' `weights` (None: the four
    classes' packings and the tap tables they share), the outputs, their epilogues and the tile list (None: the whole map)"""
    _req(x, torch.float32, "x")
    B, ci, H, W = x.shape
    assert pc_a.kind == pc_b.kind == "deconv" and pc_a.cin == pc_b.cin == ci and pc_a.cout == pc_b.cout
    if weights is None:
        weights = (_addr(pc_a.wpk4), _addr(pc_b.wpk4), pc_a.ntaps4.data_ptr(), pc_a.dy4.data_ptr(), pc_a.dx4.data_ptr())
    return (x.data_ptr(), B, ci, H, W, *weights, out_a.data_ptr(), out_b.data_ptr(), pc_a.cout, _epilogue(scale_a, shift_a, relu, residual_a),
            _epilogue(scale_b, shift_b, relu, residual_b), None if tile_list is None else _tile_list(tile_list, n_list))


def deconv2d_s2_pair(x, pc_a, pc_b, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, residual_a=None, residual_b=None, tile_cfg=4):
    """Two ConvTranspose2d(3, 2, 1, 1) layers of one shape on the SAME input in one launch (sessd_deconv2d_s2_mfma_pair); the same
    bits as two conv2d() calls with that tile_cfg (3, 4, 11 or 12)."""
    return deconv2d_s2_pair_active(x, pc_a, pc_b, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, None, None, residual_a, residual_b,
                                   tile_cfg)


def deconv2d_s2_pair_active(x, pc_a, pc_b, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, tile_list, n_list, residual_a=None,
                            residual_b=None, tile_cfg=11):
    """sessd_deconv2d_s2_mfma_pair with a tile list: deconv2d_s2_pair over the listed 2x2 tiles of the INPUT map only (a listed tile = a
    4x4 block of both outputs); the other output pixels are left alone."""
    args = _pair_args(x, pc_a, pc_b, None, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, residual_a, residual_b, tile_list, n_list)
    check(lib.sessd_deconv2d_s2_mfma_pair(*args, int(tile_cfg), _stream()), "deconv2d_s2_mfma_pair")
    return out_a, out_b


class TileActivity:
    """Buffers + launches of sessd_bev_tile_activity / sessd_fill_inactive_tiles for a chain of 3x3 layers over (batch, ., H, W) maps.
    steps: 0 = a 3x3 stride-1 layer (takes the next slot), 1 = a 3x3 stride-2 layer computed everywhere (the map halves), 2 = a
    stride-2 layer that takes a slot itself (the 2x2 tiles of its OUTPUT that hold a non-constant pixel), 3 = a stride-2 transposed
    conv on the current map whose output also receives, as a residual, a map of the last layer slot before the halving (takes a
    slot of 2x2 tiles of its INPUT = 4x4 blocks of its output; dims = the input map), 4 = no layer: the map becomes that transposed
    conv's OUTPUT (twice the resolution), so that a following 0 is a 3x3 layer over it (conv_0 / conv_1);
    an int n means n stride-1 layers. Per slot s: dims[s] = (h, w) of the layer, tile_mask[s] (batch, H/2, 2) int64 -- bit tx of a
    row's 128 bits = tile (ty, tx) is computed; rows beyond h/2 unused --, tile_list[s] (batch * H/2 * W/2,) int32, n_list[s]."""

    def __init__(self, batch, H, W, steps, device):
        steps = [0] * steps if isinstance(steps, int) else [int(v) for v in steps]
        self.batch, self.H, self.W, self.steps = int(batch), int(H), int(W), steps
        self.dims, h, w = [], H, W
        for k in steps:
            if k in (0, 3):
                self.dims.append((h, w))
            elif k == 4:   # the map becomes the output of the transposed conv (step 3) in front: twice the resolution, no slot
                h, w = 2 * h, 2 * w
            else:
                h, w = h // 2, w // 2
                if k == 2:
                    self.dims.append((h, w))
        self.n_slots = self.n_layers = len(self.dims)
        self._steps = (ctypes.c_int32 * len(steps))(*steps)
        tiles = (H // 2) * (W // 2)
        self.tile_mask = torch.zeros((self.n_slots, batch, H // 2, 2), dtype=torch.int64, device=device)
        self.tile_list = torch.zeros((self.n_slots, batch * tiles), dtype=torch.int32, device=device)
        self.n_list = torch.zeros(self.n_slots, dtype=torch.int32, device=device)
        self.ws = torch.zeros(max(256, int(lib.sessd_bev_tile_activity_workspace_bytes(batch, self.n_slots))), dtype=torch.uint8, device=device)
        self._jobs = None

    def run(self, indices, n_dev, n_cap):
        _req(indices, torch.int32, "indices"); _req(n_dev, torch.int32, "n_dev")
        check(lib.sessd_bev_tile_activity(indices.data_ptr(), n_dev.data_ptr(), int(n_cap), self.batch, self.H, self.W, self._steps,
                                          len(self.steps), self.tile_mask.data_ptr(), self.tile_list.data_ptr(), self.n_list.data_ptr(),
                                          self.tile_list.shape[1], self.ws.data_ptr(), self.ws.numel(), _stream()), "bev_tile_activity")

    def mask_bool(self, slot):
        """(batch, h/2, w/2) bool of the slot's computed tiles (tests / reports)"""
        import numpy as np
        h, w = self.dims[slot]
        m = self.tile_mask[slot].cpu().numpy().view("uint64")[:, :h // 2]
        tx = np.arange(w // 2)
        return torch.from_numpy(((m[:, :, tx >> 6] >> (tx & 63).astype("uint64")) & np.uint64(1)).astype(bool))

    def fill(self, outs, values, layers=None, tiles=None, near=None, near_kind=None):
        """outs[i] (batch, cout, h, w) <- values[i][cout] in the tiles slot layers[i] (default i) does not compute (one launch of up
        to 12 jobs; several outputs may share a slot: a 1x1 layer is computed where its input was). tiles[i] = 4: the output of a
        transposed conv over the slot's 2x2 INPUT tiles -- 4x4-pixel tiles, values[i] (4, cout) per output parity class; tiles[i] = 6:
        2x2-pixel tiles with such a (4, cout) table (a 3x3 layer behind the transposed convs).
        near[i] = slot of the list-driven reader of outs[i], or None: only the tiles that reader can reach are filled.
        near_kind[i]: 0 (default) a 3x3 stride-1 layer on the same tile grid; on a grid twice as coarse: 1 = the reader touches
        the map inside its listed tiles only, 2 = a 3x3 stride-2 layer over 2x2 tiles of its output."""
        from ._lib import FillTilesJob
        layers = list(range(len(outs))) if layers is None else list(layers)
        tiles = [2] * len(outs) if tiles is None else list(tiles)
        near = [None] * len(outs) if near is None else list(near)
        near_kind = [0] * len(outs) if near_kind is None else list(near_kind)
        key = tuple((o.data_ptr(), v.data_ptr(), l, t, n, k) for o, v, l, t, n, k in zip(outs, values, layers, tiles, near, near_kind))
        if self._jobs is None or self._jobs[0] != key:
            arr = (FillTilesJob * len(outs))()
            for i, (o, v, l, t) in enumerate(zip(outs, values, layers, tiles)):
                _req(o, torch.float32, "out"); _req(v, torch.float32, "value")
                up = 2 if t == 4 else 1
                assert tuple(o.shape[2:]) == (up * self.dims[l][0], up * self.dims[l][1]) and o.shape[0] == self.batch
                assert v.numel() == (4 if t in (4, 6) else 1) * o.shape[1]   # (4, 6: one value per output parity class)
                arr[i].out, arr[i].value, arr[i].tile_mask, arr[i].cout = o.data_ptr(), v.data_ptr(), self.tile_mask[l].data_ptr(), o.shape[1]
                arr[i].h, arr[i].w, arr[i].mask_th, arr[i].tile = o.shape[2], o.shape[3], self.H // 2, t
                if near[i] is not None:
                    k = int(near_kind[i])
                    dn, dl = self.dims[near[i]], self.dims[l]
                    assert t in (2, 6) and k in (0, 1, 2) and (dn == dl if k == 0 else (2 * dn[0], 2 * dn[1]) == tuple(dl))
                    arr[i].near_mask, arr[i].near_kind = self.tile_mask[near[i]].data_ptr(), k
            self._jobs = (key, arr)
        arr = self._jobs[1]
        check(lib.sessd_fill_inactive_tiles(arr, len(outs), self.batch, _stream()), "fill_inactive_tiles")


def pack_winograd(weight, adjoint=False):
    """U = G g G^T of a 3x3 conv weight (Cout,Cin,3,3) for sessd_conv3x3_winograd, packed
    [Cin/2][xi/4][channel parity][Cout_pad][xi%4]. One launch (sessd_conv3x3_winograd_pack)."""
    return _winograd_pack(weight, 0, adjoint)


def pack_deconv2d_s2(weight):
    """nn.ConvTranspose2d(Cin,Cout,3,stride=2,padding=1,output_padding=1) weight (Cin,Cout,3,3):
    four output-parity classes; out(2y+py, 2x+px) = sum over taps of in(y+ey, x+ex) W[:, :, ky, kx]
    with (k, e) = (1, 0) for even parity and (0, +1), (2, 0) for odd parity (oy = 2*iy - 1 + ky)."""
    w = weight.detach().to(torch.float32)
    ci, co, kh, kw = w.shape
    assert kh == 3 and kw == 3 and ci % 2 == 0
    sel = {0: [(1, 0)], 1: [(0, 1), (2, 0)]}
    launches = []
    w = w.contiguous()
    for py in (0, 1):
        for px in (0, 1):
            taps = [(ky, ey, kx, ex) for (ky, ey) in sel[py] for (kx, ex) in sel[px]]
            # (ci, co, 3, 3) weight: output channel o has element stride 9, input channel c stride co * 9, tap (ky, kx) offset 3 ky + kx
            offs = [3 * ky + kx for (ky, ey, kx, ex) in taps]
            launches.append(Launch(torch.tensor([t[1] for t in taps], dtype=torch.int32), torch.tensor([t[3] for t in taps], dtype=torch.int32),
                                   1, 2, py, px, (w, 9, co * 9, offs)))
    return PackedConv(launches, ci, co, "deconv", 2, wt=w)   # (packs the four classes now)


# taps (ky, kx) of a ConvTranspose2d(3, 2, 1, 1) weight in the order dense_deconv_split.hip uses them: grouped by the input pixel
# (y + ey, x + ex) they multiply -- e = (0,0): W11 W12 W21 W22, (0,1): W10 W20, (1,0): W01 W02, (1,1): W00
DECONV_SPLIT_TAPS = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 0), (2, 0), (0, 1), (0, 2), (0, 0))


def pack_deconv2d_s2_split(weight):
    """nn.ConvTranspose2d(Cin, Cout, 3, 2, 1, 1) weight (Cin, Cout, 3, 3), Cin % 16 == 0, for sessd_deconv2d_s2_pair_split_active:
    w = w0 + w1 + w2 EXACTLY with three bfloat16 terms (each rounded to nearest from the f32 residual of the one before), stored
    [ceil(Cout/128)][Cin/16][tap 9: DECONV_SPLIT_TAPS][plane 3][(cout/32)%4][lane = (cin/8)%2 * 32 + cout%32][cin%8] -- a wave's
    A fragment of a (k-step, tap, plane) is 16 contiguous bytes per lane. Couts beyond Cout are zero. Once per model (plain
    torch, on the weight's device)."""
    w = weight.detach().to(torch.float32)
    ci, co, kh, kw = w.shape
    if kh != 3 or kw != 3 or ci % 16:
        raise ValueError("pack_deconv2d_s2_split: a (Cin, Cout, 3, 3) weight with Cin % 16 == 0")
    ng = (co + 127) // 128
    wt = torch.zeros((9, ci, ng * 128), dtype=torch.float32, device=w.device)
    for t, (ky, kx) in enumerate(DECONV_SPLIT_TAPS):
        wt[t, :, :co] = w[:, :, ky, kx]
    planes = []
    for _ in range(3):
        p = wt.to(torch.bfloat16)
        planes.append(p)
        wt = wt - p.to(torch.float32)   # exact: the residual of a round-to-nearest bf16 fits f32
    pl = torch.stack(planes).view(3, 9, ci // 16, 2, 8, ng, 4, 32)   # plane, tap, k-step, cin half, cin % 8, group, cout block, cout % 32
    return pl.permute(5, 2, 1, 0, 6, 3, 7, 4).contiguous().view(ng, ci // 16, 9, 3, 4, 64, 8)


def deconv2d_s2_pair_split_active(x, pc_a, pc_b, scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, tile_list, n_list, residual_a=None,
                                  residual_b=None):
    """sessd_deconv2d_s2_pair_split_active: deconv2d_s2_pair_active on the bf16 matrix cores (three-way split operands, f32
    accuracy) -- the listed 2x2 tiles of the INPUT map give 4x4 blocks of both outputs, the other output pixels are left alone."""
    wa, wb = pc_a.wsplit(), pc_b.wsplit()
    if wa is None or wb is None:
        raise ValueError("deconv2d_s2_pair_split_active needs cin % 16 == 0")
    args = _pair_args(x, pc_a, pc_b, (wa.data_ptr(), wb.data_ptr()), scale_a, shift_a, scale_b, shift_b, relu, out_a, out_b, residual_a,
                      residual_b, tile_list, n_list)
    check(lib.sessd_deconv2d_s2_pair_split_active(*args, _stream()), "deconv2d_s2_pair_split_active")
    return out_a, out_b


def pack_conv2d_s2_split(weight):
    """nn.Conv2d(Cin, Cout, 3, stride 2, padding 1) weight (Cout, Cin, 3, 3), Cin % 16 == 0, for sessd_conv2d_s2_split_active:
    w = w0 + w1 + w2 EXACTLY with three bfloat16 terms (each rounded to nearest from the f32 residual of the one before), stored
    [ceil(Cout/128)][Cin/16][tap 9 = 3 ky + kx][plane 3][(cout/32)%4][lane = (cin/8)%2 * 32 + cout%32][cin%8] -- a wave's A
    fragment of a (k-step, tap, plane) is 16 contiguous bytes per lane. Couts beyond Cout are zero. Once per model (plain torch,
    on the weight's device)."""
    w = weight.detach().to(torch.float32)
    if w.dim() != 4 or w.shape[2] != 3 or w.shape[3] != 3 or w.shape[1] % 16:
        raise ValueError("pack_conv2d_s2_split: a (Cout, Cin, 3, 3) weight with Cin % 16 == 0")
    co, ci = w.shape[0], w.shape[1]
    ng = (co + 127) // 128
    wt = torch.zeros((9, ci, ng * 128), dtype=torch.float32, device=w.device)
    wt[:, :, :co] = w.permute(2, 3, 1, 0).reshape(9, ci, co)
    planes = []
    for _ in range(3):
        p = wt.to(torch.bfloat16)
        planes.append(p)
        wt = wt - p.to(torch.float32)   # exact: the residual of a round-to-nearest bf16 fits f32
    pl = torch.stack(planes).view(3, 9, ci // 16, 2, 8, ng, 4, 32)   # plane, tap, k-step, cin half, cin % 8, group, cout block, cout % 32
    return pl.permute(5, 2, 1, 0, 6, 3, 7, 4).contiguous().view(ng, ci // 16, 9, 3, 4, 64, 8)


def conv2d_s2_split_active(x, pc, scale, shift, relu, out, tile_list, n_list, residual=None):
    """sessd_conv2d_s2_split_active: a Conv2d(3, stride 2, padding 1) layer on the bf16 matrix cores (three-way split operands, f32
    accuracy) over the listed 2x2 tiles of its OUTPUT map (entries image * (ho/2 * wo/2) + tile, count on the device); the other
    output pixels of `out` are left alone."""
    _req(x, torch.float32, "x"); _req(out, torch.float32, "out")
    tl = _tile_list(tile_list, n_list)
    ws = pc.wsplit_s2()
    if ws is None:
        raise ValueError("conv2d_s2_split_active needs a 3x3 stride-2 conv with cin % 16 == 0")
    B, ci, H, W = x.shape
    ho, wo = pc.out_hw(H, W)
    if ci != pc.cin or tuple(out.shape) != (B, pc.cout, ho, wo):
        raise ValueError("conv2d_s2_split_active: x (B, cin, H, W) and out (B, cout, ceil(H/2), ceil(W/2))")
    check(lib.sessd_conv2d_s2_split_active(x.data_ptr(), B, ci, H, W, ws.data_ptr(), out.data_ptr(), pc.cout, ho, wo,
                                           _epilogue(scale, shift, relu, residual), tl, _stream()), "conv2d_s2_split_active")
    return out


def pack_deconv2d_ks(weight, s):
    """nn.ConvTranspose2d(Cin, Cout, s, stride=s, bias=False) weight (Cin, Cout, s, s), s >= 2 (the RPN's up-samplers): kernel size
    = stride, so every output pixel has ONE input pixel and one tap -- out(s y + py, s x + px) = W[:, :, py, px]^T in(y, x): s * s
    output-parity launches of one tap each (dy = dx = 0, out_mul = s), packed straight from the stored tensor."""
    w = weight.detach().to(torch.float32).contiguous()
    ci, co, kh, kw = w.shape
    s = int(s)
    assert s >= 2 and kh == s and kw == s and ci % 2 == 0
    zero = torch.zeros(1, dtype=torch.int32)
    launches = []
    for py in range(s):
        for px in range(s):
            # output channel o has element stride s * s, input channel c stride co * s * s, tap (py, px) offset py * s + px
            launches.append(Launch(zero, zero, 1, s, py, px, (w, s * s, co * s * s, [py * s + px])))
    pc = PackedConv(launches, ci, co, "deconv_ks", s)
    for la in launches:
        la.wpk   # packed now, as pack_deconv2d_s2 does
    return pc


class PackedDeconvKs:
    """A kernel-size = stride transposed conv packed for sessd_deconv_ks_slice (pack_deconv_ks_slice)."""

    def __init__(self, wpk, cin, cout, s):
        self.wpk, self.cin, self.cout, self.stride, self.kind = wpk, cin, cout, s, "deconv_ks_slice"


def pack_deconv_ks_slice(weight, s):
    """nn.ConvTranspose2d(Cin, Cout, s, stride=s, bias=False) weight (Cin, Cout, s, s), s in {1, 2, 4}, Cin even, Cout % 32 == 0,
    for the ONE-launch form sessd_deconv_ks_slice (csrc/deconv_ks.hip). Layout, floats:
        [py][Cout / 32][Cin / 2][px][Cin parity][32 couts]     out[py][cb][kp][px][h][i] = W[2 kp + h][32 cb + i][py][px]
    -- what a wave (one py, some cout blocks, all px) reads per k-step are adjacent 256-byte rows. A snapshot of the tensor as it
    is now (a torch permute on the device, once per model): the engine that uses it is built from an eval-mode model and re-built
    after a parameter write, so nothing is registered with the repack machinery."""
    w = weight.detach().to(torch.float32).contiguous()
    _req(w, torch.float32, "weight")
    ci, co, kh, kw = w.shape
    s = int(s)
    if s not in (1, 2, 4) or kh != s or kw != s:
        raise ValueError("pack_deconv_ks_slice: kernel size = stride in {1, 2, 4} expected, got kernel %dx%d, s = %d" % (kh, kw, s))
    if ci % 2 or co % 32:
        raise ValueError("pack_deconv_ks_slice: even cin and cout %% 32 == 0 expected, got %d -> %d" % (ci, co))
    wpk = w.view(ci // 2, 2, co // 32, 32, s, s).permute(4, 2, 0, 5, 1, 3).contiguous()   # [kp, h, cb, i, py, px] -> [py, cb, kp, px, h, i]
    return PackedDeconvKs(wpk, ci, co, s)


def deconv_ks_slice(x, packed, scale, shift, relu, out, c_off):
    """x (B, Cin, H, W) -> channels [c_off, c_off + Cout) of out (B, C_total, s*H, s*W), one launch (sessd_deconv_ks_slice):
    ConvTranspose2d(Cin, Cout, s, stride=s) + folded BatchNorm (scale, shift: (Cout) or None) + ReLU. The rest of `out` is not
    touched. Returns out."""
    _req(x, torch.float32, "x")
    _req(out, torch.float32, "out")
    if scale is not None:
        _req(scale, torch.float32, "scale")
    if shift is not None:
        _req(shift, torch.float32, "shift")
    if x.dim() != 4 or out.dim() != 4:
        raise ValueError("deconv_ks_slice: x (B, Cin, H, W) and out (B, C_total, s*H, s*W) expected")
    B, ci, H, W = x.shape
    s = packed.stride
    if ci != packed.cin or out.shape[0] != B or out.shape[2] != s * H or out.shape[3] != s * W:
        raise ValueError("deconv_ks_slice: x %s with cin %d, s = %d does not match out %s" % (tuple(x.shape), packed.cin, s, tuple(out.shape)))
    if any(t is not None and t.numel() != packed.cout for t in (scale, shift)):
        raise ValueError("deconv_ks_slice: scale / shift of %d elements expected" % packed.cout)
    check(lib.sessd_deconv_ks_slice(x.data_ptr(), B, ci, H, W, packed.wpk.data_ptr(), s, out.data_ptr(), packed.cout,
                                    int(out.shape[1]), int(c_off), _p(scale), _p(shift), 1 if relu else 0, _stream()),
          "deconv_ks_slice")
    return out


def _deconv_ks_dims(weight, s, what):
    """(cin, cout) of a ConvTranspose2d(cin, cout, s, stride=s) weight inside the domain of csrc/deconv_ks*.hip, else ValueError"""
    s = int(s)
    if weight.dim() != 4 or s not in (1, 2, 4) or tuple(weight.shape[2:]) != (s, s):
        raise ValueError("%s: a (cin, cout, s, s) weight with s in {1, 2, 4} expected, got %s, s = %d" % (what, tuple(weight.shape), s))
    ci, co = int(weight.shape[0]), int(weight.shape[1])
    if ci < 2 or ci % 2 or co < 32 or co % 32:
        raise ValueError("%s: even cin and cout %% 32 == 0 expected, got %d -> %d" % (what, ci, co))
    return ci, co


def pack_deconv_ks_dgrad(weight, s):
    """nn.ConvTranspose2d(Cin, Cout, s, stride=s) weight (Cin, Cout, s, s) for sessd_deconv_ks_dgrad (csrc/deconv_ks_grad.hip), floats:
        [py][Cout / 2][Cout parity][Cin][px]     out[py][op][h][i][px] = W[i][2 op + h][py][px]
    One torch permute on the device, a snapshot of the tensor as it is now."""
    w = weight.detach().to(torch.float32).contiguous()
    _req(w, torch.float32, "weight")
    ci, co = _deconv_ks_dims(w, s, "pack_deconv_ks_dgrad")
    s = int(s)
    return w.view(ci, co // 2, 2, s, s).permute(3, 1, 2, 0, 4).contiguous()   # [i, op, h, py, px] -> [py, op, h, i, px]


def deconv_ks_dgrad(grad_out, weight, s):
    """Data gradient of ConvTranspose2d(Cin, Cout, s, stride=s): grad_out (B, Cout, s*H, s*W), weight the stored (Cin, Cout, s, s)
    tensor -> (B, Cin, H, W), one launch (sessd_deconv_ks_dgrad) behind the permute of pack_deconv_ks_dgrad."""
    _req(grad_out, torch.float32, "grad_out")
    ci, co = _deconv_ks_dims(weight, s, "deconv_ks_dgrad")
    s = int(s)
    if grad_out.dim() != 4 or grad_out.shape[1] != co or grad_out.shape[2] % s or grad_out.shape[3] % s:
        raise ValueError("deconv_ks_dgrad: grad_out %s does not match the weight %s, s = %d" % (tuple(grad_out.shape), tuple(weight.shape), s))
    B, H, W = int(grad_out.shape[0]), int(grad_out.shape[2]) // s, int(grad_out.shape[3]) // s
    wpk = pack_deconv_ks_dgrad(weight, s)
    gin = torch.empty((B, ci, H, W), dtype=torch.float32, device=grad_out.device)
    check(lib.sessd_deconv_ks_dgrad(grad_out.data_ptr(), B, ci, H, W, wpk.data_ptr(), s, co, gin.data_ptr(), _stream()), "deconv_ks_dgrad")
    return gin


def deconv_ks_wgrad(x, grad_out, s):
    """Weight gradient of ConvTranspose2d(Cin, Cout, s, stride=s), in the stored layout (Cin, Cout, s, s): x (B, Cin, H, W), grad_out
    (B, Cout, s*H, s*W). Two launches (sessd_deconv_ks_wgrad): chunk partials in a cached workspace, then their ordered sum."""
    _req(x, torch.float32, "x")
    _req(grad_out, torch.float32, "grad_out")
    s = int(s)
    if x.dim() != 4 or grad_out.dim() != 4:
        raise ValueError("deconv_ks_wgrad: x (B, Cin, H, W) and grad_out (B, Cout, s*H, s*W) expected")
    B, ci, H, W = (int(v) for v in x.shape)
    co = int(grad_out.shape[1])
    if tuple(grad_out.shape) != (B, co, s * H, s * W):
        raise ValueError("deconv_ks_wgrad: x %s, s = %d does not match grad_out %s" % (tuple(x.shape), s, tuple(grad_out.shape)))
    gw = torch.empty((ci, co, s, s), dtype=torch.float32, device=x.device)
    _deconv_ks_dims(gw, s, "deconv_ks_wgrad")
    if B * H * W == 0:
        return gw.zero_()
    ws = workspace(int(lib.sessd_deconv_ks_wgrad_workspace_bytes(B, ci, H, W, co, s)), x.device, "deconv_ks_wgrad")
    check(lib.sessd_deconv_ks_wgrad(x.data_ptr(), grad_out.data_ptr(), B, ci, H, W, co, s, gw.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream()), "deconv_ks_wgrad")
    return gw


class DeconvKsFunction(torch.autograd.Function):
    """Differentiable ConvTranspose2d(Cin, Cout, s, stride=s, bias=False), s in {1, 2, 4}, on the HIP kernels: apply(x, weight, s).
    forward: sessd_deconv_ks_slice into its own (B, Cout, s*H, s*W) tensor (no scale, no shift, no ReLU);
    backward: sessd_deconv_ks_dgrad and sessd_deconv_ks_wgrad, each only if its gradient is asked for.
    The forward's packed weight is made by pack_deconv_ks_slice on EVERY call (a permute of at most 2 MB), and so is the data
    gradient's copy: the re-pack registry has no job for either layout and is left alone here."""

    @staticmethod
    def forward(ctx, x, weight, s):
        x = x.float().contiguous()
        _req(x, torch.float32, "x")
        s = int(s)
        packed = pack_deconv_ks_slice(weight, s)
        if x.dim() != 4 or x.shape[1] != packed.cin:
            raise ValueError("DeconvKsFunction: x %s does not match the weight %s" % (tuple(x.shape), tuple(weight.shape)))
        B, _, H, W = x.shape
        out = torch.empty((B, packed.cout, s * H, s * W), dtype=torch.float32, device=x.device)
        ctx.save_for_backward(x, weight)
        ctx.s = s
        return deconv_ks_slice(x, packed, None, None, False, out, 0)

    @staticmethod
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        g = grad.float().contiguous()   # torch.cat's backward hands out a channel slice of the wider map
        gx = deconv_ks_dgrad(g, weight, ctx.s) if ctx.needs_input_grad[0] else None
        gw = deconv_ks_wgrad(x, g, ctx.s) if ctx.needs_input_grad[1] else None
        return gx, gw, None


def _device_f32(x):
    """a float32 (B, C, H, W) tensor on the device"""
    return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def _device_param(t):
    """a float32 parameter on the device, or none"""
    return t is None or (t.is_cuda and t.dtype == torch.float32)


def deconv_ks_covers(m, x):
    """True where DeconvKsFunction runs module m on x: an nn.ConvTranspose2d with kernel = stride in {1, 2, 4} (both axes), no
    padding / output_padding / dilation / groups / bias, even cin, cout % 32 == 0, and a float32 (B, cin, H, W) device tensor."""
    if not isinstance(m, torch.nn.ConvTranspose2d) or not _device_f32(x):
        return False
    s = m.stride[0]
    return (tuple(m.kernel_size) == tuple(m.stride) == (s, s) and s in (1, 2, 4) and tuple(m.padding) == (0, 0)
            and tuple(m.output_padding) == (0, 0) and tuple(m.dilation) == (1, 1) and m.groups == 1 and m.bias is None
            and m.in_channels >= 2 and m.in_channels % 2 == 0 and m.out_channels >= 32 and m.out_channels % 32 == 0
            and x.shape[1] == m.in_channels and _device_param(m.weight))


def conv2d_train_covers(m, x, padded=False, any_width=False):
    """True only where ops.conv2d_module(x, m) runs forward AND backward on the HIP kernels (Conv2dFunction has no such check of its
    own: outside this domain it raises, or asserts, somewhere on the way). m: an nn.Conv2d with k in {1, 3} and stride in {1, 2}
    (k = 1: stride 1) on both axes, padding k // 2 -- or, with padded=True, the unpadded 3x3 conv behind an nn.ZeroPad2d(1), which is
    the same layer (x is then the map in FRONT of the pad) -- no dilation, no groups, zero padding mode; x a float32
    (B, cin, H, W) device tensor. The conditions, each
    read off the code that would refuse:
      pack_conv2d (forward and, stride 1, the adjoint layer): cin and cout even;
      stride 2: even H and W -- the data gradient is the ConvTranspose2d(3, 2, 1, 1) of pack_deconv2d_s2, whose output is twice
        its input, and sessd_conv2d_wgrad asks for win == 2 * wout;
      sessd_conv2d_wgrad: wout % 8 == 0, and the whole input and grad_out below 2 GiB (out_fits of sessd_conv2d_mfma asks less).
    any_width=True asks for conv2d_module(x, m, any_width=True), whose weight gradient is sessd_conv2d_wgrad_any_width: the
    wout % 8 condition falls away, every other one stays.
    A bias is covered: its gradient (ops.channel_sum) falls back by itself."""
    if not isinstance(m, torch.nn.Conv2d) or isinstance(m, torch.nn.ConvTranspose2d) or not _device_f32(x):
        return False
    k, s = m.kernel_size[0], m.stride[0]
    if tuple(m.kernel_size) != (k, k) or tuple(m.stride) != (s, s) or k not in (1, 3) or s not in (1, 2) or (k == 1 and s != 1):
        return False
    pad = (0, 0) if (padded and k == 3) else (k // 2, k // 2)
    if padded and k != 3:
        return False
    if (m.padding if isinstance(m.padding, str) else tuple(m.padding)) != pad:
        return False
    if tuple(m.dilation) != (1, 1) or m.groups != 1 or m.padding_mode != "zeros":
        return False
    if not _device_param(m.weight) or not _device_param(m.bias):
        return False
    B, ci, H, W = (int(v) for v in x.shape)
    co = m.out_channels
    if ci != m.in_channels or ci % 2 or co % 2 or B < 1 or H < 1 or W < 1:
        return False
    if s == 2 and (H % 2 or W % 2):
        return False
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    if Wo % 8 and not any_width:
        return False
    return B * ci * H * W * 4 < 0x7FFFFFFF and B * co * Ho * Wo * 4 < 0x7FFFFFFF


# conv2d's kernel families. Each takes the layer as conv2d does, with `out` allocated, and epi = _epilogue(...).
def _conv2d_winograd_sk(x, pc, epi, out, shape, workspace, workgroups):
    B, ci, H, W = x.shape
    upk = pc.upk_sk(shape)
    if upk is None or (H & 1) or (W & 1):
        raise ValueError("tile_cfg 22/23/24/25 (stream-K Winograd) needs a 3x3 stride-1 conv with cin % 16 (22, 24, 25) / 8 (23) == 0 "
                         "and even H, W")
    need = int(lib.sessd_conv3x3_winograd_sk_workspace_bytes(B, H, W, pc.cout, shape, workgroups))
    workspace = _sk_workspace(workspace, need, shape, workgroups, x.device)
    _winograd_sk(x, 1, upk, out, pc.cout, epi, None, _stream_k(workspace, workgroups), shape)


def _conv2d_sk_whole(x, pc, epi, out, workspace, workgroups):
    if pc.sk_args() is None:
        raise ValueError("tile_cfg 30 (LDS-tiled stream-K) needs cin % 16 == 0")
    need = int(lib.sessd_conv2d_sk_workspace_bytes(x.shape[0], *pc.tile_hw(*x.shape[2:]), pc.cout, pc.sk_args()["n"], workgroups))
    workspace = _sk_workspace(workspace, need, "csk", workgroups, x.device)
    _conv2d_sk(x, pc, epi, out, None, _stream_k(workspace, workgroups), "tile_cfg 30")


def _conv2d_winograd(x, pc, epi, out, variant):
    B, ci, H, W = x.shape
    if pc.upk is None or (H & 1) or (W & 1):
        raise ValueError("tile_cfg 20/21 (Winograd) needs a 3x3 stride-1 conv with cin % 8 == 0 and even H, W")
    check(lib.sessd_conv3x3_winograd(x.data_ptr(), B, ci, H, W, pc.upk.data_ptr(), out.data_ptr(), pc.cout, epi, variant, _stream()),
          "conv3x3_winograd")


def _deconv2d_s2_merged(x, pc, epi, out, tile_cfg):
    B, ci, H, W = x.shape
    cfg = tile_cfg if tile_cfg is not None else default_tile_cfg(pc.cout, H * W, 4)
    check(lib.sessd_deconv2d_s2_mfma(x.data_ptr(), B, ci, H, W, _addr(pc.wpk4), pc.ntaps4.data_ptr(), pc.dy4.data_ptr(), pc.dx4.data_ptr(),
                                     out.data_ptr(), pc.cout, epi, cfg, _stream()), "deconv2d_s2_mfma")


def _conv2d_direct(x, pc, epi, out, tile_cfg):
    th, tw = pc.tile_hw(*x.shape[2:])
    for la in pc.launches:
        _conv2d_mfma(x, pc, la, epi, out, None, tile_cfg if tile_cfg is not None else default_tile_cfg(pc.cout, th * tw, la.ntaps))


def conv2d(x, pc, scale=None, shift=None, relu=True, residual=None, out=None, tile_cfg=None, workspace=None, workgroups=0):
    """x (B,Cin,H,W) NCHW float32 on the device. Returns (B,Cout,Ho,Wo): the layer + folded BatchNorm (scale, shift) + ReLU +
    residual. The selectable tile_cfg values, all of them:
      0 - 8, 11, 12, 13 (every layer kind): wave / workgroup tilings of the direct kernel, sessd_conv2d_mfma, one launch per entry of
        pc.launches (dispatch_tile in csrc/dense_conv.hip has the shapes; 11 / 12 / 13 = 4 / 3 / 2 with operands fetched two steps ahead).
        A "deconv" with cin % 8 == 0 runs its four parity classes as ONE launch, sessd_deconv2d_s2_mfma, which refuses 13 and also
        takes 40 / 41 / 42: both px classes of a row parity in every wave (csrc/dense_deconv_pair.hip).
      30 ("conv", "deconv"; cin % 16 == 0): LDS-tiled stream-K, sessd_conv2d_sk (csrc/dense_conv_sk.hip), meant for what is not 3x3 stride 1.
      3x3 stride-1 "conv" only -- 10: activation-stationary LDS variant of the direct kernel, cin % 16 == 0; 20 / 21: Winograd
        F(2x2,3x3), sessd_conv3x3_winograd, cin % 8 == 0 / 21: operands two rounds ahead, cin % 32 == 0; 22 / 23 / 24 / 25: its stream-K
        shapes 0 - 3, sessd_conv3x3_winograd_sk (csrc/dense_wino_sk.hip): 8 waves x 128 couts / 4 x 64 / 4 x 128 with the output
        transform in registers / shape 0 on the bf16 matrix cores, cin % 16 == 0 (23: % 8). All of 20 - 25 need even H, W.
      A "deconv_ks" runs on the direct kernel only: anything from 20 up is refused.
    None: default_tile_cfg, or 20 for a 3x3 stride-1 layer on an even map of >= 4096 pixels while USE_WINOGRAD.
    The stream-K families (22 - 25, 30) take a zeroed `workspace` (winograd_sk_workspace / conv2d_sk_workspace, one per concurrently
    running stream; too small a one is a ValueError) -- without one a per-(device, stream) cache is used -- and `workgroups`."""
    _req(x, torch.float32, "x")
    B, ci, H, W = x.shape
    assert ci == pc.cin
    if pc.kind == "deconv_ks" and tile_cfg is not None and tile_cfg >= 20:
        raise ValueError("a kernel-size = stride transposed conv runs on the sessd_conv2d_mfma tilings only")
    if out is None:
        out = torch.empty((B, pc.cout, *pc.out_hw(H, W)), dtype=torch.float32, device=x.device)
    epi = _epilogue(scale, shift, relu, residual)
    if tile_cfg in (22, 23, 24, 25):
        _conv2d_winograd_sk(x, pc, epi, out, tile_cfg - 22, workspace, workgroups)
    elif tile_cfg == 30:
        _conv2d_sk_whole(x, pc, epi, out, workspace, workgroups)
    elif tile_cfg in (20, 21):
        _conv2d_winograd(x, pc, epi, out, tile_cfg - 20)
    elif pc.kind == "deconv" and ci % 8 == 0:
        _deconv2d_s2_merged(x, pc, epi, out, tile_cfg)
    elif tile_cfg is None and USE_WINOGRAD and pc.is_3x3_s1 and not (H & 1) and not (W & 1) and H * W >= 4096 and ci % 8 == 0:
        # The first-generation kernel: every tile block is computed by one workgroup from start to end, so a frame's bits do not
        # depend on its batch slot or on the batch size. The stream-K kernel (tile_cfg 22 / 23, 20 % faster) is deterministic
        # for a fixed (shape, batch, workgroup count) only -- a unit cut between two workgroups adds two partial sums -- and is
        # chosen explicitly: engine.autotune(), the training path.
        _conv2d_winograd(x, pc, epi, out, 0)
    else:
        _conv2d_direct(x, pc, epi, out, tile_cfg)
    return out


# tile_cfg families of the 3x3 stride-1 convs: 20/21 first-generation Winograd F(2x2,3x3), 22/23 its stream-K form
WINOGRAD_CFGS = (20, 21, 22, 23, 24)
WINOGRAD_SK_CFGS = (22, 23, 24)   # 24: third generation, output transform in registers (same cuts and bits as 22)


def winograd_mult_ratio(tile_cfg):
    """Matrix-core multiplies a 3x3 kernel executes per multiply of direct convolution: F(2x2,3x3) 16/36, direct 1."""
    return 16.0 / 36.0 if tile_cfg in WINOGRAD_CFGS else 1.0


# 3x3 stride-1 convolutions on large maps default to the fused Winograd F(2x2,3x3) kernel (1.4x the direct kernel on
# MI355X; float32 Winograd rounding ~1e-6 of the output scale). Set to False for the exact fmaf-chain direct kernel.
USE_WINOGRAD = True


def assign_targets(anchors, gt_boxes, gt_classes=None, matched_threshold=0.6, unmatched_threshold=0.45):
    """Anchor target assignment of create_target_np (target_ops_v3.py:11-137) on the device: anchors (N,7), gt_boxes (M,7).
    Returns dict(labels (N,) int32, bbox_targets (N,7), bbox_outside_weights (N,), gt_id (N,) int32)."""
    _req(anchors, torch.float32, "anchors")
    n, m = anchors.shape[0], gt_boxes.shape[0]
    dev = anchors.device
    g = gt_boxes.to(device=dev, dtype=torch.float32).contiguous() if m else torch.zeros((1, 7), dtype=torch.float32, device=dev)
    c = None if gt_classes is None or m == 0 else gt_classes.to(device=dev, dtype=torch.int32).contiguous()
    out = dict(labels=torch.empty((n,), dtype=torch.int32, device=dev), bbox_targets=torch.empty((n, 7), dtype=torch.float32, device=dev),
               bbox_outside_weights=torch.empty((n,), dtype=torch.float32, device=dev), gt_id=torch.empty((n,), dtype=torch.int32, device=dev))
    ws = workspace(lib.sessd_assign_targets_workspace_bytes(n), dev, "assign")
    check(lib.sessd_assign_targets(anchors.data_ptr(), n, g.data_ptr(), _p(c), m, float(matched_threshold), float(unmatched_threshold),
                                   out["labels"].data_ptr(), out["bbox_targets"].data_ptr(), out["bbox_outside_weights"].data_ptr(),
                                   out["gt_id"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "assign_targets")
    return out


ASSIGN_MAX_TASKS = 4   # sessd_assign_targets_batch: tasks per call
ASSIGN_MAX_GT = 128    # and ground-truth rows per frame


class AssignTargets:
    """Anchor target assignment for all frames and all tasks of a batch as ONE device op (sessd_assign_targets_batch: one clear
    and two launches, the ground-truth counts read on the device, nothing read back). Per (frame, task) the result is that of
    assign_targets() on the frame's live rows of the task's class with the task's thresholds; labels are 1 on the positives.
    tasks: list of dict(anchors (A, 7) or (B, A, 7) float32 on `device`, class_id, matched_threshold, unmatched_threshold);
    class_id <= 0 takes every live row. Outputs and workspace are allocated here, once: usable inside a captured iteration.
    `labels`, `reg_targets` and `anchors` of the result are what MultiGroupHead.loss_supervised / loss_supervised_device take."""

    _OUT = ("labels", "reg_targets", "reg_weights", "gt_id")

    def __init__(self, batch, num_anchors, tasks, device, gt_capacity=128, labels_i64=False):
        from ._lib import AssignBatchCfg
        self.B, self.A, self.T, self.G = int(batch), int(num_anchors), len(tasks), int(gt_capacity)
        self.dev = torch.device(device)
        if not 1 <= self.T <= ASSIGN_MAX_TASKS:
            raise ValueError("AssignTargets takes 1 to %d tasks, got %d" % (ASSIGN_MAX_TASKS, self.T))
        if not 1 <= self.G <= ASSIGN_MAX_GT:
            raise ValueError("AssignTargets holds 1 to %d ground-truth rows per frame, got gt_capacity = %d" % (ASSIGN_MAX_GT, self.G))
        if self.dev.type != "cuda":
            raise ValueError("AssignTargets needs the HIP device: there is no CPU fallback")
        per_frame = {t["anchors"].dim() == 3 for t in tasks}
        if len(per_frame) != 1:
            raise ValueError("the tasks' anchors must all be (A, 7) or all be (B, A, 7)")
        self.per_frame = per_frame.pop()
        want = (self.B, self.A, 7) if self.per_frame else (self.A, 7)
        self.tasks = []
        for t, d in enumerate(tasks):
            a = d["anchors"]
            if not a.is_cuda or a.dtype != torch.float32 or tuple(a.shape) != want:
                raise ValueError("task %d: anchors must be a float32 device tensor of shape %s, got %s %s %s"
                                 % (t, want, a.device, a.dtype, tuple(a.shape)))
            self.tasks.append(dict(anchors=a.contiguous(), class_id=int(d["class_id"]), matched=float(d["matched_threshold"]),
                                   unmatched=float(d["unmatched_threshold"])))
        c = AssignBatchCfg(self.B, self.A, self.T, self.G, 1 if labels_i64 else 0, 1 if self.per_frame else 0)
        self.cfg, self._cfg_p = c, ctypes.addressof(c)
        need = int(lib.sessd_assign_targets_batch_workspace_bytes(self._cfg_p))
        if need == 0:
            raise ValueError("sessd_assign_targets_batch does not cover this shape (batch and anchors >= 1, batch x tasks <= 65535, "
                             "batch x tasks x anchors x 7 < 2^31)")
        self.label_dtype = torch.int64 if labels_i64 else torch.int32
        z = lambda shape, dt: [torch.zeros(shape, dtype=dt, device=self.dev) for _ in range(self.T)]
        self.ws = torch.zeros(need, dtype=torch.uint8, device=self.dev)
        self.out = dict(labels=z((self.B, self.A), self.label_dtype), reg_targets=z((self.B, self.A, 7), torch.float32),
                        reg_weights=z((self.B, self.A), torch.float32), gt_id=z((self.B, self.A), torch.int32))
        # (B, A, 7) per task as the head loss reads them: made once and contiguous, so that no call (or replay) copies them
        self.anchors = [d["anchors"] if self.per_frame else d["anchors"].unsqueeze(0).repeat(self.B, 1, 1) for d in self.tasks]

    def _check(self, v, name, dtype, shape):
        if not v.is_cuda or v.dtype != dtype or tuple(v.shape) != shape or not v.is_contiguous():
            raise ValueError("%s must be a contiguous %s device tensor of shape %s, got %s %s %s"
                             % (name, dtype, shape, v.device, v.dtype, tuple(v.shape)))

    def run(self, gt_boxes, gt_classes=None, gt_count=None, out=None):
        """gt_boxes (B, G, 7) float32, gt_classes (B, G) int32 or None (every live row belongs to every task), gt_count (B,)
        int32 DEVICE tensor or None (all G rows live). out: dict with any of labels / reg_targets / reg_weights / gt_id, each
        a list of T tensors (or None entries) written in place of this object's own; a key given as False is not computed
        (reg_weights, gt_id). Returns dict(labels, reg_targets, reg_weights, gt_id, anchors), each a list of T tensors."""
        from ._lib import AssignTask
        B, A, T, G = self.B, self.A, self.T, self.G
        self._check(gt_boxes, "gt_boxes", torch.float32, (B, G, 7))
        if gt_classes is not None:
            self._check(gt_classes, "gt_classes", torch.int32, (B, G))
        if gt_count is not None:
            self._check(gt_count, "gt_count", torch.int32, (B,))
        shapes = dict(labels=((B, A), self.label_dtype), reg_targets=((B, A, 7), torch.float32), reg_weights=((B, A), torch.float32),
                      gt_id=((B, A), torch.int32))
        res = {}
        for k in self._OUT:
            given = None if out is None else out.get(k)
            if given is False:
                if k in ("labels", "reg_targets"):
                    raise ValueError("%s is always written" % k)
                res[k] = [None] * T
                continue
            if given is None:
                res[k] = list(self.out[k])
                continue
            if len(given) != T:
                raise ValueError("out[%r] must list %d tensors, got %d" % (k, T, len(given)))
            res[k] = [self.out[k][t] if v is None else v for t, v in enumerate(given)]
            for t, v in enumerate(res[k]):
                self._check(v, "out[%r][%d]" % (k, t), shapes[k][1], shapes[k][0])
        arr = (AssignTask * T)()
        for t, d in enumerate(self.tasks):
            arr[t].anchors, arr[t].class_id, arr[t].matched, arr[t].unmatched = d["anchors"].data_ptr(), d["class_id"], d["matched"], d["unmatched"]
            arr[t].labels, arr[t].reg_targets = res["labels"][t].data_ptr(), res["reg_targets"][t].data_ptr()
            arr[t].reg_weights, arr[t].gt_id = _p(res["reg_weights"][t]) or None, _p(res["gt_id"][t]) or None
        check(lib.sessd_assign_targets_batch(self._cfg_p, ctypes.addressof(arr), gt_boxes.data_ptr(), _p(gt_classes) or None,
                                             _p(gt_count) or None, self.ws.data_ptr(), self.ws.numel(), _stream()), "assign_targets_batch")
        res["anchors"] = list(self.anchors)
        return res


class OdiouFunction(torch.autograd.Function):
    """ODIoU loss of odious.py:837-900 on the device: loss = 2 * sum(weights * term) / batch_size, differentiable with
    respect to the predicted boxes (the kernel returns the per-pair gradient with the value)."""

    @staticmethod
    def forward(ctx, gboxes, qboxes, weights, batch_size):
        g = gboxes.detach().float().contiguous()
        q = qboxes.detach().float().contiguous()
        _req(g, torch.float32, "gboxes")
        n = q.shape[0]
        term = torch.empty((n,), dtype=torch.float32, device=q.device)
        grad = torch.empty((n, 7), dtype=torch.float32, device=q.device)
        check(lib.sessd_odiou3d(g.data_ptr(), q.data_ptr(), n, term.data_ptr(), grad.data_ptr(), _stream()), "odiou3d")
        w = weights.detach().float()
        ctx.save_for_backward(grad, w)
        ctx.scale = 2.0 / float(batch_size)
        ctx.terms = term
        return (term * w).sum() * ctx.scale

    @staticmethod
    def backward(ctx, gl):
        grad, w = ctx.saved_tensors
        return None, grad * (w * (ctx.scale * gl)).unsqueeze(1), None, None


def odiou_3d_loss(gboxes, qboxes, weights, batch_size):
    """Drop-in for `odiou_3D()(gboxes, qboxes, weights, batch_size)` (odious.py:845); boxes (N,7) [x,y,z,w,l,h,r]."""
    return OdiouFunction.apply(gboxes, qboxes, weights, batch_size)


HEAD_LOSS_RECORD = {  # names of the floats of sessd_head_loss's record (include/sessd_hip.h)
    "total": 0, "loss": 1, "cls_loss_reduced": 2, "loc_loss_reduced": 3, "dir_loss_reduced": 4, "iou_pred_loss": 5, "ious_loss": 6,
    "consistency_loss": 7, "cls_pos_loss": 8, "cls_neg_loss": 9, "loc_loss_elem": slice(10, 17), "num_pos": 17, "num_neg": 18,
    "consistency_box": 19, "consistency_score": 20, "consistency_iou": 21, "matched_boxes": 22,
    "loss_ema": 24, "cls_loss_reduced_ema": 26, "loc_loss_reduced_ema": 27, "dir_loss_reduced_ema": 28, "iou_pred_loss_ema": 29,
    "cls_pos_loss_ema": 32, "cls_neg_loss_ema": 33, "loc_loss_elem_ema": slice(34, 41), "num_pos_ema": 41, "num_neg_ema": 42,
    "overflow": 48, "positives": 49, "positives_ema": 50, "candidates": 51, "candidates_ema": 52}


class HeadLoss:
    """The SE-SSD loss of MultiGroupHead.loss / consistency_loss / get_model_ema_loss (mg_head_sessd.py:573-890) as ONE device
    op in capacity form (csrc/head_loss.hip: six launches, every count on the device, nothing read back): value, log record and
    the gradient with respect to the student's four head outputs. Static buffers (allocated here, once): usable inside a
    captured iteration. One object per (batch, anchors) shape and device."""

    def __init__(self, batch, num_anchors, device, labels_i64, cfg, pos_capacity=None, cons_capacity=2048):
        from ._lib import HeadLossCfg
        self.B, self.A, self.dev = int(batch), int(num_anchors), device
        c = HeadLossCfg()
        c.batch, c.num_anchors, c.labels_i64 = self.B, self.A, 1 if labels_i64 else 0
        c.pos_capacity = int(pos_capacity or 1024 * self.B)
        c.cons_capacity = int(cons_capacity)
        for k in ("pos_cls_weight", "neg_cls_weight", "focal_alpha", "focal_gamma", "smooth_l1_sigma", "cls_loss_weight",
                  "loc_loss_weight", "dir_loss_weight", "direction_offset", "score_thresh", "match_iou_thresh"):
            setattr(c, k, float(cfg[k]))
        for i, v in enumerate(cfg["center_range"]):
            c.center_range[i] = float(v)
        self.cfg = c
        import ctypes as C
        self._cfg_p = C.addressof(c)
        need = int(lib.sessd_head_loss_workspace_bytes(self._cfg_p))
        if need == 0:
            raise ValueError("sessd_head_loss does not cover this configuration")
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=device)
        self.ws = torch.zeros(need, dtype=torch.uint8, device=device)
        self.g_box, self.g_cls, self.g_dir, self.g_iou = f(self.B, self.A, 7), f(self.B, self.A), f(self.B, self.A, 2), f(self.B, self.A)
        self.record = f(64)

    def run(self, stu, tea, anchors0, transformation, cons_weight):
        """stu / tea: dict(box, cls, dir, iou, labels, reg_targets, anchors) of contiguous device tensors (shapes of
        sessd_head_loss_net_t); anchors0 (A,7); transformation (B,5) float32; cons_weight: device float32 scalar tensor.
        Returns the record tensor (64 floats, device); the gradients are in self.g_*."""
        from ._lib import HeadLossNet
        import ctypes as C
        nets = []
        for d in (stu, tea):
            n = HeadLossNet()
            for k in ("box", "cls", "dir", "iou", "reg_targets", "anchors"):
                t = d[k]
                _req(t, torch.float32, k)
                setattr(n, k, t.data_ptr())
            lab = d["labels"]
            want = torch.int64 if self.cfg.labels_i64 else torch.int32
            if lab.dtype != want or not lab.is_contiguous() or not lab.is_cuda:
                raise ValueError("labels must be contiguous %s device tensors" % want)
            if lab.numel() != self.B * self.A or d["box"].numel() != self.B * self.A * 7 or d["cls"].numel() != self.B * self.A \
                    or d["dir"].numel() != self.B * self.A * 2 or d["iou"].numel() != self.B * self.A \
                    or d["reg_targets"].numel() != self.B * self.A * 7 or d["anchors"].numel() != self.B * self.A * 7:
                raise ValueError("head-loss tensors do not have the (batch %d, anchors %d) shape" % (self.B, self.A))
            n.labels = lab.data_ptr()
            nets.append(n)
        _req(anchors0, torch.float32, "anchors0")
        _req(transformation, torch.float32, "transformation")
        _req(cons_weight, torch.float32, "cons_weight")
        if anchors0.numel() != self.A * 7 or transformation.numel() != self.B * 5:
            raise ValueError("anchors0 must be (A,7), transformation (B,5)")
        check(lib.sessd_head_loss(self._cfg_p, C.addressof(nets[0]), C.addressof(nets[1]), anchors0.data_ptr(), transformation.data_ptr(),
                                  cons_weight.data_ptr(), self.g_box.data_ptr(), self.g_cls.data_ptr(), self.g_dir.data_ptr(),
                                  self.g_iou.data_ptr(), self.record.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _stream()),
              "head_loss")
        return self.record


class HeadLossFunction(torch.autograd.Function):
    """loss = HeadLoss record[0] as a differentiable scalar of the student's head outputs. unit_grad=True: backward returns the
    kernel's gradients as they are (valid when the scalar itself is what `.backward()` is called on -- the training step; no
    extra launches); otherwise they are scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, box, cls, dirp, iou, runner, stu, tea, anchors0, transformation, cons_weight, unit_grad):
        stu = dict(stu, box=box.detach(), cls=cls.detach(), dir=dirp.detach(), iou=iou.detach())
        rec = runner.run(stu, tea, anchors0, transformation, cons_weight)
        ctx.runner, ctx.unit, ctx.shapes = runner, bool(unit_grad), (box.shape, cls.shape, dirp.shape, iou.shape)
        ctx.mark_non_differentiable(rec)
        return rec[0].clone(), rec

    @staticmethod
    def backward(ctx, g, _g_rec):
        r = ctx.runner
        gs = [t.view(sh) for t, sh in zip((r.g_box, r.g_cls, r.g_dir, r.g_iou), ctx.shapes)]
        if not ctx.unit:
            gs = [t * g for t in gs]
        return (*gs, None, None, None, None, None, None, None)


SUPERVISED_LOSS_ROW = 32   # floats of one row of sessd_supervised_loss's record: one row per task, then the row of their sum
SUPERVISED_LOSS_RECORD = {  # names of the floats of a task's row (include/sessd_hip.h); "total" is [0] of the last row
    "loss": 0, "cls_loss_reduced": 1, "loc_loss_reduced": 2, "dir_loss_reduced": 3, "cls_pos_loss": 4, "cls_neg_loss": 5,
    "loc_loss_elem": slice(6, 13), "num_pos": 13, "num_neg": 14, "positives": 15, "total": 0}


class SupervisedLoss:
    """The plain supervised multi-task head loss of MultiGroupHead.loss (mg_head.py:559-652: sigmoid focal classification,
    smooth-L1 localisation on the sin-encoded yaw, softmax direction loss on the positives, NormByNumPositives) as ONE device op
    (csrc/supervised_loss.hip: three launches for all tasks, nothing read back): value, log record and the gradient with respect
    to every task's box / cls / dir outputs. Static buffers (allocated here, once): usable inside a captured iteration. One
    object per (batch, anchors, tasks) shape and device. cfg: dict of the float fields of sessd_supervised_loss_cfg_t."""

    def __init__(self, batch, num_anchors, num_tasks, device, labels_i64, cfg):
        from ._lib import SupervisedLossCfg
        self.B, self.A, self.T, self.dev = int(batch), int(num_anchors), int(num_tasks), device
        c = SupervisedLossCfg()
        c.batch, c.num_anchors, c.num_tasks, c.labels_i64 = self.B, self.A, self.T, 1 if labels_i64 else 0
        for k in ("pos_cls_weight", "neg_cls_weight", "focal_alpha", "focal_gamma", "smooth_l1_sigma", "cls_loss_weight",
                  "loc_loss_weight", "dir_loss_weight", "direction_offset"):
            setattr(c, k, float(cfg[k]))
        self.cfg = c
        self._cfg_p = ctypes.addressof(c)
        need = int(lib.sessd_supervised_loss_workspace_bytes(self._cfg_p))
        if need == 0:
            raise ValueError("sessd_supervised_loss does not cover this configuration (1 to %d tasks, batch and anchors >= 1)" % MAX_TASKS)
        if torch.device(device).type != "cuda":
            raise ValueError("SupervisedLoss needs the HIP device: there is no CPU fallback")
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=device)
        self.ws = torch.zeros(need, dtype=torch.uint8, device=device)
        self.g_box = [f(self.B, self.A, 7) for _ in range(self.T)]
        self.g_cls = [f(self.B, self.A) for _ in range(self.T)]
        self.g_dir = [f(self.B, self.A, 2) for _ in range(self.T)]
        self.record = f(self.T + 1, SUPERVISED_LOSS_ROW)

    def run(self, tasks):
        """tasks: list of T dict(box, cls, dir, labels, reg_targets, anchors) of contiguous device tensors with B * A * (7, 1, 2,
        1, 7, 7) elements. Returns the record tensor ((T + 1, 32), device); the gradients are in self.g_box / g_cls / g_dir."""
        from ._lib import SupervisedTask
        if len(tasks) != self.T:
            raise ValueError("expected %d tasks, got %d" % (self.T, len(tasks)))
        n = self.B * self.A
        arr = (SupervisedTask * self.T)()
        want_lab = torch.int64 if self.cfg.labels_i64 else torch.int32
        for t, d in enumerate(tasks):
            for k, per, dtype in (("box", 7, torch.float32), ("cls", 1, torch.float32), ("dir", 2, torch.float32), ("labels", 1, want_lab),
                                  ("reg_targets", 7, torch.float32), ("anchors", 7, torch.float32)):
                v = d[k]
                if not v.is_cuda or v.dtype != dtype or not v.is_contiguous() or v.numel() != n * per:
                    raise ValueError("task %d: %s must be a contiguous %s device tensor of %d x %d x %d elements, got %s %s %s"
                                     % (t, k, dtype, self.B, self.A, per, v.device, v.dtype, tuple(v.shape)))
                setattr(arr[t], k, v.data_ptr())
            if d["dir"].data_ptr() % 8:
                raise ValueError("task %d: dir must be 8-byte aligned" % t)
            arr[t].grad_box, arr[t].grad_cls, arr[t].grad_dir = self.g_box[t].data_ptr(), self.g_cls[t].data_ptr(), self.g_dir[t].data_ptr()
        check(lib.sessd_supervised_loss(self._cfg_p, ctypes.addressof(arr), self.record.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                        _stream()), "supervised_loss")
        return self.record


class SupervisedLossFunction(torch.autograd.Function):
    """total = the sum of the tasks' loss (SupervisedLoss record[T, 0]) as a differentiable scalar of the 3 * T head outputs
    (box, cls, dir of task 0, then of task 1, ...). Returns (total, record). unit_grad=True: backward returns the kernel's
    gradient buffers as they are (valid when the scalar itself is what `.backward()` is called on; no extra launches);
    otherwise they are scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, runner, targets, unit_grad, *outs):
        if len(outs) != 3 * runner.T or len(targets) != runner.T:
            raise ValueError("expected box, cls, dir of %d tasks" % runner.T)
        tasks = [dict(targets[t], box=outs[3 * t].detach(), cls=outs[3 * t + 1].detach(), dir=outs[3 * t + 2].detach())
                 for t in range(runner.T)]
        rec = runner.run(tasks)
        ctx.runner, ctx.unit, ctx.shapes = runner, bool(unit_grad), [o.shape for o in outs]
        ctx.mark_non_differentiable(rec)
        return rec[runner.T, 0].clone(), rec

    @staticmethod
    def backward(ctx, g, _g_rec):
        r = ctx.runner
        gs = []
        for t in range(r.T):
            gs += [r.g_box[t], r.g_cls[t], r.g_dir[t]]
        gs = [v.view(sh) for v, sh in zip(gs, ctx.shapes)]
        if not ctx.unit:
            gs = [v * g for v in gs]
        return (None, None, None, *gs)


class _SumAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        if not x.is_cuda:
            raise ValueError("sum_all / mean_all: the tensor must be on the HIP device")
        xc = x.float().contiguous()
        out = torch.empty((), dtype=torch.float32, device=xc.device)
        ws = torch.empty(int(lib.sessd_grad_clip_workspace_bytes()), dtype=torch.uint8, device=xc.device)
        check(lib.sessd_sum_f32(xc.data_ptr(), xc.numel(), float(scale), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()), "sum_f32")
        ctx.shape, ctx.scale = x.shape, float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.scale).expand(ctx.shape), None


def channel_sum(x):
    """(B, C, H, W) float32 on the device -> (C,) sums over images and pixels (a conv's bias gradient) on sessd_nchw_channel_sum;
    torch's own reduction where the kernel's layout assumptions (H * W % 4 == 0, C <= 1024) do not hold."""
    B, C, H, W = x.shape
    if (H * W) % 4 or not x.is_cuda or C > BN2D_MAX_CHANNELS:
        return x.sum((0, 2, 3))
    xc = x.float().contiguous()
    out = torch.empty((C,), dtype=torch.float32, device=x.device)
    ws = zeroed_workspace(lib.sessd_bn2d_relu_train_workspace_bytes(C), x.device, "bn2d")
    check(lib.sessd_nchw_channel_sum(xc.data_ptr(), B, C, H * W, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nchw_channel_sum")
    return out


def sum_all(x):
    """Sum of all elements as a 0-dim tensor (differentiable): sessd_sum_f32, deterministic, safe inside a captured graph --
    unlike torch's x.sum() / x.mean() of a large tensor, whose semaphore memset breaks on graph replay on this stack."""
    return _SumAll.apply(x, 1.0)


def mean_all(x):
    """Mean of all elements as a 0-dim tensor (differentiable); see sum_all."""
    return _SumAll.apply(x, 1.0 / max(1, x.numel()))


USE_WINOGRAD_WGRAD = os.environ.get("SESSD_WINOGRAD_WGRAD", "1") != "0"   # 3x3 stride-1 weight gradients in the Winograd domain


def conv2d_wgrad(inp, grad_out, ksize, stride, winograd=None, any_width=False):
    """Weight gradient (Cout, Cin, k, k) of Conv2d(k, stride, padding k//2): inp (B,Cin,H,W), grad_out (B,Cout,Ho,Wo).
    For ConvTranspose2d(3, s2, p1, op1) pass (inp=its grad_out, grad_out=its input) and get its (Cin, Cout, 3, 3) gradient.
    winograd: None = the Winograd-domain kernel where it covers the layer and the map is large enough to fill the chip
    (USE_WINOGRAD / USE_WINOGRAD_WGRAD), True = that kernel (ValueError outside its shapes), False = the direct kernel.
    any_width: the direct kernel through sessd_conv2d_wgrad_any_width, which takes any Wo >= 1 (Wo % 8 == 0: the same launches and
    bits); False keeps sessd_conv2d_wgrad and its refusal of Wo % 8 != 0. The Winograd choice does not look at it."""
    _req(inp, torch.float32, "inp")
    _req(grad_out, torch.float32, "grad_out")
    B, ci, hi, wi = inp.shape
    B2, co, ho, wo = grad_out.shape
    assert B == B2
    gw = torch.empty((co, ci, ksize, ksize), dtype=torch.float32, device=inp.device)
    asked = winograd is True   # the caller's own True; the automatic choice below is a bool, too, and must fall through to the direct kernel
    if winograd is None:
        winograd = USE_WINOGRAD and USE_WINOGRAD_WGRAD and hi * wi >= 4096
    if winograd and ksize == 3 and stride == 1:
        need = int(lib.sessd_conv3x3_wgrad_winograd_workspace_bytes(B, ci, co, hi, wi))
        if not need and asked:
            raise ValueError("conv2d_wgrad: the Winograd-domain kernel needs cin, cout % 64 == 0, even H, W, W >= 16")
        if need:   # the shape is one the Winograd-domain kernel covers (16 of the 36 products per tile)
            ws = workspace(need, inp.device, "wwgrad")
            check(lib.sessd_conv3x3_wgrad_winograd(inp.data_ptr(), B, ci, hi, wi, grad_out.data_ptr(), co, gw.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), _stream()), "conv3x3_wgrad_winograd")
            return gw
    ws = torch.empty(int(lib.sessd_conv2d_wgrad_workspace_bytes(co, ci, ksize)), dtype=torch.uint8, device=inp.device)
    entry = lib.sessd_conv2d_wgrad_any_width if any_width else lib.sessd_conv2d_wgrad
    check(entry(inp.data_ptr(), B, ci, hi, wi, grad_out.data_ptr(), co, ho, wo, ksize, stride, gw.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream()), "conv2d_wgrad_any_width" if any_width else "conv2d_wgrad")
    return gw


def _train_cfg(pc, x):
    """tile_cfg of the training path: the stream-K Winograd kernel for the 3x3 stride-1 layers it covers, else the default."""
    ok = (USE_WINOGRAD and pc.is_3x3_s1 and pc.cin % 16 == 0 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
          and x.shape[2] * x.shape[3] >= 4096)
    return 22 if ok else None


class Conv2dFunction(torch.autograd.Function):
    """Differentiable Conv2d(k in {1,3}, stride in {1,2}, padding k//2) / ConvTranspose2d(3, s2, p1, op1) on the HIP kernels.
    forward: sessd_conv2d_mfma / sessd_conv3x3_winograd / sessd_deconv2d_s2_mfma (no BatchNorm fold, no ReLU);
    backward: dx = the adjoint layer through the same kernels with re-packed weights, dW = sessd_conv2d_wgrad."""

    @staticmethod
    def forward(ctx, x, weight, bias, transposed, stride):
        x = x.float().contiguous()
        pc = packed_conv2d(weight, stride, transposed=bool(transposed))
        ctx.save_for_backward(x, weight)
        ctx.cfg = (bool(transposed), int(stride), bias is not None)
        return conv2d(x, pc, None, None if bias is None else bias.detach().float().contiguous(), False, tile_cfg=_train_cfg(pc, x))

    @staticmethod
    def backward(ctx, grad):
        return Conv2dFunction._backward(ctx, grad, False)

    @staticmethod
    def _backward(ctx, grad, any_width):
        x, weight = ctx.saved_tensors
        transposed, stride, has_bias = ctx.cfg
        g = grad.float().contiguous()
        w = weight   # (the packers detach; a parameter keeps its identity for the re-pack registry)
        k = w.shape[-1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if transposed:      # adjoint of a stride-2 transposed conv = the stride-2 conv with the same weight tensor
                gx = conv2d(g, packed_conv2d(w, 2), None, None, False)
            elif stride == 2:   # adjoint of the stride-2 conv = the transposed conv with the same weight tensor
                gx = conv2d(g, packed_conv2d(w, 2, transposed=True), None, None, False)
            else:               # stride 1: correlation with the flipped kernel, channels swapped
                pcd = packed_conv2d(w, 1, adjoint=True)
                gx = conv2d(g, pcd, None, None, False, tile_cfg=_train_cfg(pcd, g))
        if ctx.needs_input_grad[1]:
            gw = conv2d_wgrad(g, x, 3, 2, any_width=any_width) if transposed else conv2d_wgrad(x, g, k, stride, any_width=any_width)
        if has_bias and ctx.needs_input_grad[2]:
            gb = channel_sum(g)
        return gx, gw, gb, None, None


class Conv2dFunctionAnyWidth(Conv2dFunction):
    """Conv2dFunction with the weight gradient of sessd_conv2d_wgrad_any_width: maps of any width (conv2d_train_covers(...,
    any_width=True)). A class of its own, so that Conv2dFunction's arguments and its autograd node's name stay what they are."""

    @staticmethod
    def backward(ctx, grad):
        return Conv2dFunction._backward(ctx, grad, True)


def conv2d_module(x, m, any_width=False):
    """Apply an nn.Conv2d / nn.ConvTranspose2d of the SSFA neck through Conv2dFunction (autograd-capable HIP path);
    any_width=True: through Conv2dFunctionAnyWidth."""
    transposed = isinstance(m, torch.nn.ConvTranspose2d)
    fn = Conv2dFunctionAnyWidth if any_width else Conv2dFunction
    return fn.apply(x, m.weight, m.bias, transposed, int(m.stride[0]))


def default_tile_cfg(cout, npix, ntaps):
    # measured on MI355X at batch 1 (engine.autotune() refines per layer): 32c x 32p wave tiles fill the 1024 SIMDs
    # best; pixel-major workgroups (cfg 4) for the 3x3 / 1x1 layers, cout-major (cfg 3) for the merged deconv
    if ntaps == 4 and cout > 32:
        return 3
    return 4


def ssfa_fuse(x0, x1, w0, w1, s0, t0, s1, t1, out=None):
    _req(x0, torch.float32, "x0")
    _req(x1, torch.float32, "x1")
    B, C, H, W = x0.shape
    if out is None:
        out = torch.empty_like(x0)
    check(lib.sessd_ssfa_fuse(x0.data_ptr(), x1.data_ptr(), w0.data_ptr(), w1.data_ptr(), float(s0), float(t0),
                              float(s1), float(t1), B, C, H * W, out.data_ptr(), _stream()), "ssfa_fuse")
    return out


class SsfaFuseTrainFunction(torch.autograd.Function):
    """The SSFA attention tail in train mode on csrc/ssfa_train.hip: (x0, x1) -> x0 * a0 + x1 * a1 with
    a = softmax(BN_0(conv1x1_0(x0)), BN_1(conv1x1_1(x1))), batch-statistics BatchNorm2d(1); running statistics updated in place."""

    @staticmethod
    def forward(ctx, x0, x1, w0, w1, g0, b0, g1, b1, rm0, rv0, rm1, rv1, eps, momentum):
        x0, x1 = x0.float().contiguous(), x1.float().contiguous()
        _req(x0, torch.float32, "x0")
        B, C, H, W = x0.shape
        dev = x0.device
        w0f, w1f = w0.detach().float().reshape(-1).contiguous(), w1.detach().float().reshape(-1).contiguous()
        gb = [t.detach().float().contiguous() for t in (g0, b0, g1, b1)]
        out = torch.empty_like(x0)
        smap = torch.empty((2, B * H * W), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        ws = zeroed_workspace(lib.sessd_ssfa_fuse_train_workspace_bytes(B, C, H * W), dev, "ssfa_train")
        check(lib.sessd_ssfa_fuse_train_fwd(x0.data_ptr(), x1.data_ptr(), B, C, H * W, w0f.data_ptr(), w1f.data_ptr(), gb[0].data_ptr(),
                                            gb[1].data_ptr(), gb[2].data_ptr(), gb[3].data_ptr(), float(eps), float(momentum), _p(rm0),
                                            _p(rv0), _p(rm1), _p(rv1), out.data_ptr(), smap.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _stream()), "ssfa_fuse_train_fwd")
        ctx.save_for_backward(x0, x1, w0f, w1f, *gb, smap, stats)
        ctx.wshape = (tuple(w0.shape), tuple(w1.shape))
        return out

    @staticmethod
    def backward(ctx, grad):
        x0, x1, w0f, w1f, g0, b0, g1, b1, smap, stats = ctx.saved_tensors
        g = grad.float().contiguous()
        B, C, H, W = x0.shape
        dev = x0.device
        dx0, dx1 = torch.empty_like(x0), torch.empty_like(x1)
        dw0, dw1 = torch.empty(C, device=dev), torch.empty(C, device=dev)
        dgam, dbet = torch.empty(2, device=dev), torch.empty(2, device=dev)
        dz = torch.empty(B * H * W, device=dev)
        ws = zeroed_workspace(lib.sessd_ssfa_fuse_train_workspace_bytes(B, C, H * W), dev, "ssfa_train")
        check(lib.sessd_ssfa_fuse_train_bwd(g.data_ptr(), x0.data_ptr(), x1.data_ptr(), B, C, H * W, w0f.data_ptr(), w1f.data_ptr(),
                                            g0.data_ptr(), b0.data_ptr(), g1.data_ptr(), b1.data_ptr(), smap.data_ptr(), stats.data_ptr(),
                                            dz.data_ptr(), dx0.data_ptr(), dx1.data_ptr(), dw0.data_ptr(), dw1.data_ptr(), dgam.data_ptr(),
                                            dbet.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ssfa_fuse_train_bwd")
        return (dx0, dx1, dw0.reshape(ctx.wshape[0]), dw1.reshape(ctx.wshape[1]), dgam[0:1], dbet[0:1], dgam[1:2], dbet[1:2],
                None, None, None, None, None, None)


def ssfa_fuse_train(x0, x1, conv0, bn0, conv1, bn1):
    """rpn_v1.py:225-235 in train mode: conv0 / conv1 = the Conv2d(C, 1, 1, bias=False) of w_0 / w_1, bn0 / bn1 their
    BatchNorm2d(1) (train mode, affine; running statistics and batch counters updated like the torch modules do)."""
    if not ssfa_fuse_train_covers(x0, conv0, bn0, conv1, bn1):
        raise ValueError("ssfa_fuse_train: layer configuration outside the kernel's (see ssfa_fuse_train_covers)")
    mom = _bn_momentum(bn0)
    _bn_momentum(bn1)
    return SsfaFuseTrainFunction.apply(x0, x1, conv0.weight, conv1.weight, bn0.weight, bn0.bias, bn1.weight, bn1.bias,
                                       bn0.running_mean, bn0.running_var, bn1.running_mean, bn1.running_var, bn0.eps, mom)


def ssfa_fuse_train_covers(x, conv0, bn0, conv1, bn1):
    """What csrc/ssfa_train.hip implements: bias-free 1x1 convs to ONE channel, plain affine BatchNorm2d(1) layers in train mode
    with a shared eps / fixed momentum, channels % 4 == 0 (<= 1024), H * W % 4 == 0."""
    nn = torch.nn
    convs_ok = all(type(c) is nn.Conv2d and c.bias is None and c.kernel_size == (1, 1) and c.out_channels == 1 and c.groups == 1
                   and c.stride == (1, 1) and c.padding == (0, 0) for c in (conv0, conv1))
    bns_ok = all(type(b) is nn.BatchNorm2d and b.training and b.weight is not None and b.momentum is not None and b.num_features == 1
                 for b in (bn0, bn1))
    if not (convs_ok and bns_ok) or sync_bn_active():   # SyncBN: the tail's two BatchNorm2d(1) take the split (all-reduce) passes
        return False
    same = bn0.eps == bn1.eps and bn0.momentum == bn1.momentum and (bn0.running_mean is None) == (bn1.running_mean is None)
    C = x.shape[1]
    return bool(same and x.is_cuda and C % 4 == 0 and C <= 1024 and conv0.in_channels == C and conv1.in_channels == C
                and (x.shape[2] * x.shape[3]) % 4 == 0)


class SplitNhwcFunction(torch.autograd.Function):
    """planar (B, C, H, W) -> the parts of `sizes` channels each as contiguous NHWC tensors (B, H, W, size): what
    `[p.permute(0, 2, 3, 1).contiguous() for p in torch.split(y, sizes, 1)]` gives, in one launch each way."""

    @staticmethod
    def forward(ctx, y, *sizes):
        import ctypes
        y = y.float().contiguous()
        _req(y, torch.float32, "y")
        B, C, H, W = y.shape
        assert sum(sizes) == C and 1 <= len(sizes) <= 4
        outs = [torch.empty((B, H, W, int(n)), dtype=torch.float32, device=y.device) for n in sizes]
        n = len(sizes)
        check(lib.sessd_nchw_split_nhwc(y.data_ptr(), B, C, H * W, n, (ctypes.c_int * n)(*[int(v) for v in sizes]),
                                        (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), _stream()), "nchw_split_nhwc")
        ctx.meta = (tuple(int(v) for v in sizes), tuple(y.shape))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        import ctypes
        sizes, shape = ctx.meta
        B, C, H, W = shape
        gs = [None if g is None else g.float().contiguous() for g in grads]
        dev = next(g.device for g in gs if g is not None)
        gy = torch.empty(shape, dtype=torch.float32, device=dev)
        n = len(sizes)
        check(lib.sessd_nhwc_merge_nchw((ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in gs]), n,
                                        (ctypes.c_int * n)(*sizes), B, C, H * W, gy.data_ptr(), _stream()), "nhwc_merge_nchw")
        return (gy,) + (None,) * n


def split_nhwc(y, sizes):
    return SplitNhwcFunction.apply(y, *[int(v) for v in sizes])


MAX_TASKS = 4        # multi-task inference: tasks per head (sessd_ssfa_fuse_head_tasks / sessd_predict)
TASK_HEAD_CH = 22    # planar head channels of one task: [box 14 | cls 2 | dir 4 | iou 2], one class, two rotations per location


def check_num_tasks(num_tasks):
    """The limit of the multi-task inference path, as a ValueError that names it."""
    if not 1 <= int(num_tasks) <= MAX_TASKS:
        raise ValueError("multi-task inference supports 1 to %d tasks, got %d" % (MAX_TASKS, int(num_tasks)))
    return int(num_tasks)


def ssfa_fuse_head(x0, x1, w0, w1, s0, t0, s1, t1, head_w, head_b, head_out=None, out=None, score_thresh=0.0, keys=None,
                   key_count=None, num_tasks=1):
    """ssfa_fuse + the 1x1 heads in one launch: head_w (22, C) row-major, head_b (22) or None -> head_out (B, 22, H*W) planar.
    `out` (B, C, H, W): optional buffer that receives the SSFA output (not written when None).
    keys (B, 2*H*W) int64 + key_count (B,) int32 (zeroed by the caller): the launch also appends predict's score-filter keys
    (sessd_ssfa_fuse_head_keys) -- the inputs predict() takes instead of running its own score filter.
    num_tasks = T > 1 (sessd_ssfa_fuse_head_tasks): head_w (T*22, C), head_b (T*22) or None -> head_out (B, T*22, H*W) =
    (B, T, 22, H*W), task t's planes bit-equal to the single-task call with task t's weights; keys (B, T, 2*H*W) and key_count
    (B*T,) per (frame, task)."""
    _req(x0, torch.float32, "x0")
    _req(x1, torch.float32, "x1")
    _req(head_w, torch.float32, "head_w")
    B, C, H, W = x0.shape
    nout = head_w.shape[0]
    T = check_num_tasks(num_tasks)
    if T > 1 and (nout != T * TASK_HEAD_CH or (head_b is not None and head_b.numel() != nout)):
        raise ValueError("multi-task head weights must be (num_tasks * 22, C) with a (num_tasks * 22) bias: %d channels for %d tasks"
                         % (nout, T))
    if head_out is None:
        head_out = torch.empty((B, nout, H * W), dtype=torch.float32, device=x0.device)
    if keys is not None:
        assert key_count is not None and keys.dtype == torch.int64 and key_count.dtype == torch.int32 and keys.is_contiguous()
        assert keys.numel() >= B * T * 2 * H * W and key_count.numel() >= B * T
    if T == 1:
        check(lib.sessd_ssfa_fuse_head_keys(x0.data_ptr(), x1.data_ptr(), w0.data_ptr(), w1.data_ptr(), float(s0), float(t0), float(s1),
                                            float(t1), B, C, H * W, _p(out), head_w.data_ptr(), _p(head_b), nout, head_out.data_ptr(),
                                            float(score_thresh), _p(keys), 2 * H * W if keys is not None else 0, _p(key_count),
                                            _stream()), "ssfa_fuse_head_keys")
        return head_out
    assert head_out.numel() >= B * nout * H * W and head_out.is_contiguous() and head_w.is_contiguous()
    check(lib.sessd_ssfa_fuse_head_tasks(x0.data_ptr(), x1.data_ptr(), w0.data_ptr(), w1.data_ptr(), float(s0), float(t0), float(s1),
                                         float(t1), B, C, H * W, _p(out), head_w.data_ptr(), _p(head_b), T, head_out.data_ptr(),
                                         float(score_thresh), _p(keys), 2 * H * W if keys is not None else 0, _p(key_count),
                                         _stream()), "ssfa_fuse_head_tasks")
    return head_out


def rpn_up_head(x, up_w, up_scale, up_shift, head_w, head_b, head_out=None, out=None, score_thresh=0.0, keys=None, key_count=None,
                num_tasks=1):
    """The tail of the three-class config's RPN neck + the 1x1 heads in one launch (sessd_rpn_up_head_tasks): x (B, 128, H, W) =
    the last 3x3 layer's output; up_w (128, 128) [cin][cout] = the ConvTranspose2d(128, 128, 1, stride=1) weight as stored,
    up_scale / up_shift (128) its folded BatchNorm (ReLU follows): u = relu(up_scale * (up_w^T x) + up_shift) on the f32 matrix
    cores, kept in LDS. head_w (T*22, 128), head_b (T*22) or None -> head_out (B, T*22, H*W) = (B, T, 22, H*W) planar; `out`
    (B, 128, H, W): optional buffer that receives u. keys (B, T, 2*H*W) int64 + key_count (B*T,) int32 (zeroed by the caller):
    predict's score-filter keys per (frame, task), as ssfa_fuse_head writes them."""
    for t, name in ((x, "x"), (up_w, "up_w"), (up_scale, "up_scale"), (up_shift, "up_shift"), (head_w, "head_w")):
        _req(t, torch.float32, name)
    B, C, H, W = x.shape
    nout = head_w.shape[0]
    T = check_num_tasks(num_tasks)
    if C != 128 or up_w.numel() != C * C or up_scale.numel() != C or up_shift.numel() != C or head_w.shape[1] != C:
        raise ValueError("rpn_up_head takes 128 channels in and out (x (B, 128, H, W), up_w (128, 128), up_scale / up_shift (128), "
                         "head_w (T*22, 128)): got %d channels, up_w %s" % (C, tuple(up_w.shape)))
    if nout != T * TASK_HEAD_CH or (head_b is not None and head_b.numel() != nout):
        raise ValueError("head weights must be (num_tasks * 22, C) with a (num_tasks * 22) bias: %d channels for %d tasks" % (nout, T))
    if head_out is None:
        head_out = torch.empty((B, nout, H * W), dtype=torch.float32, device=x.device)
    if keys is not None:
        assert key_count is not None and keys.dtype == torch.int64 and key_count.dtype == torch.int32 and keys.is_contiguous()
        assert keys.numel() >= B * T * 2 * H * W and key_count.numel() >= B * T
    assert head_out.numel() >= B * nout * H * W and head_out.is_contiguous()
    assert out is None or (out.numel() >= B * C * H * W and out.is_contiguous())
    check(lib.sessd_rpn_up_head_tasks(x.data_ptr(), up_w.data_ptr(), up_scale.data_ptr(), up_shift.data_ptr(), B, C, H * W, _p(out),
                                      head_w.data_ptr(), _p(head_b), T, head_out.data_ptr(), float(score_thresh), _p(keys),
                                      2 * H * W if keys is not None else 0, _p(key_count), _stream()), "rpn_up_head_tasks")
    return head_out


def fill_multi(segments):
    """[(tensor, 32-bit pattern), ...] (<= 4, 16-byte aligned, sizes multiples of 4 bytes) cleared in ONE launch."""
    import ctypes
    n = len(segments)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in segments])
    vals = (ctypes.c_uint32 * n)(*[int(v) & 0xFFFFFFFF for _, v in segments])
    cnts = (ctypes.c_size_t * n)(*[t.numel() * t.element_size() // 4 for t, _ in segments])
    check(lib.sessd_fill_u32_multi(n, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(vals, ctypes.c_void_p),
                                   ctypes.cast(cnts, ctypes.c_void_p), _stream()), "fill_u32_multi")


# ------------------------------------------------------------------ predict / post-processing
NMS_TYPES = ("rotate_nms", "rotate_weighted_nms")
DI_MAX_CANDIDATES = 1024   # sessd_predict with DI-NMS: one thread per candidate in the selection workgroup
# the literals get_task_detections passes to rotate_weighted_nms (mg_head_sessd.py:1012-1017)
DI_DEFAULTS = dict(nms_cnt_thresh=2.6, nms_sigma_dist_interval=(0, 20, 40, 60), nms_sigma_square=(0.0009, 0.009, 0.1, 1),
                   suppressed_thresh=0.3, centerness_pow=2)


def nms_settings(nms_cfg, pre_max=None):
    """(nms_type, di) of a test_cfg["nms"] mapping: nms_type absent = "rotate_nms" (di None); "rotate_weighted_nms" = DI-NMS with
    DI_DEFAULTS overridden by the keys the mapping carries. Raises ValueError for an unknown nms_type, for pre_max above the
    1024 candidates DI-NMS handles and for malformed intervals -- before anything touches the device."""
    get = nms_cfg.get if hasattr(nms_cfg, "get") else (lambda k, d=None: getattr(nms_cfg, k, d))
    nms_type = get("nms_type", None)
    nms_type = "rotate_nms" if nms_type is None else nms_type
    if nms_type not in NMS_TYPES:
        raise ValueError("nms_type must be one of %s, got %r" % (NMS_TYPES, nms_type))
    if nms_type == "rotate_nms":
        return nms_type, None
    di = {k: (get(k, None) if get(k, None) is not None else d) for k, d in DI_DEFAULTS.items()}
    check_di(di, pre_max)
    return nms_type, di


def check_di(di, pre_max=None):
    """DI-NMS settings -> the sessd_di_cfg_t of the call (ValueError for what the kernels do not cover)."""
    from ._lib import DiCfg
    unknown = set(di) - set(DI_DEFAULTS)
    if unknown:
        raise ValueError("unknown DI-NMS settings %s (known: %s)" % (sorted(unknown), sorted(DI_DEFAULTS)))
    d = dict(DI_DEFAULTS)
    d.update(di)
    if pre_max is not None and int(pre_max) > DI_MAX_CANDIDATES:
        raise ValueError("rotate_weighted_nms handles at most %d candidates per (frame, task) (one thread each in the selection "
                         "workgroup): nms_pre_max_size = %d" % (DI_MAX_CANDIDATES, int(pre_max)))
    iv, sg = [float(v) for v in d["nms_sigma_dist_interval"]], [float(v) for v in d["nms_sigma_square"]]
    if not 1 <= len(iv) <= 8 or len(sg) < len(iv) - 1:
        raise ValueError("DI-NMS takes 1 to 8 distance bounds and one sigma square per interval, got %d and %d" % (len(iv), len(sg)))
    c = DiCfg()
    c.cnt_thresh, c.suppressed_thresh, c.centerness_pow = float(d["nms_cnt_thresh"]), float(d["suppressed_thresh"]), float(d["centerness_pow"])
    c.n_interval = len(iv)
    for k, v in enumerate(iv):
        c.interval[k] = v
    for k, v in enumerate(sg[:8]):
        c.sigma_sq[k] = v
    return c


def _predict_layout(B, T, post_max, multi, di):
    """(name, shape, dtype) of predict's outputs. multi: the layout of num_tasks = T > 1 and of DI-NMS, task_count included. di:
    DI-NMS adds where the selection stopped at post_max with candidates left, the kept candidates' ranks in the top-k order before
    the filters (the reference's `selected`) and their number."""
    f32, i32 = torch.float32, torch.int32
    rows = [("box", (B, T * post_max, 7), f32), ("score", (B, T * post_max), f32), ("label", (B, T * post_max), i32), ("count", (B,), i32)]
    if multi:
        rows.append(("task_count", (B, T), i32))
    if di:
        rows += [("di_truncated", (B, T), i32), ("di_keep", (B, T, post_max), i32), ("di_keep_count", (B, T), i32)]
    return rows


class Predict:
    """The predict stage of one shape and one set of settings: validated once, its sessd_predict_args_t filled once, launched many
    times. B frames, T = num_tasks, P = H * W pixels; anchors (A,7) / (B,A,7) for T = 1, (T,A,7) / (B,T,A,7) for any T, A = 2 * P;
    frustum (B,1,6,4,3) float64 or None; the settings as predict() documents them.
    out: preallocated outputs, used as they are (box, score, label, count; task_count, di_truncated, di_keep + di_keep_count where
    present); None = a fresh dict in predict()'s layout for (T, nms_type). sticky: one int32 that DI-NMS ORs its truncation flag
    into. workspace: an owned uint8 tensor of at least `need` bytes; None = the cached workspace(need, device, "predict") of the
    stream and capture scope each launch runs in.
    The object keeps every tensor alive whose address the struct holds; head, keys and records are bound per launch()."""

    def __init__(self, B, T, P, anchors, frustum=None, score_thresh=0.3, pre_max=1000, post_max=100, nms_thresh=0.01,
                 post_center_range=(0, -40.0, -5.0, 70.4, 40.0, 5.0), direction_offset=0.0, nms_type="rotate_nms", di=None,
                 device=None, out=None, workspace=None, sticky=None):
        from ._lib import PredictArgs
        if nms_type not in NMS_TYPES:
            raise ValueError("nms_type must be one of %s, got %r" % (NMS_TYPES, nms_type))
        self.di_cfg = check_di({} if di is None else di, pre_max) if nms_type == "rotate_weighted_nms" else None
        _req(anchors, torch.float32, "anchors")
        B, T, P, post_max = int(B), check_num_tasks(T), int(P), int(post_max)
        self.B, self.T, self.P, self.post_max = B, T, P, post_max
        if T == 1 and anchors.dim() in (2, 3):  # (A,7) / (B,A,7) -> (1,A,7) / (B,1,A,7)
            anchors = anchors.unsqueeze(-3)
        assert anchors.dim() in (3, 4) and tuple(anchors.shape[-3:]) == (T, 2 * P, 7), "anchors: (T, 2*P, 7) or (B, T, 2*P, 7)"
        assert anchors.dim() == 3 or anchors.shape[0] == B
        if frustum is not None:
            _req(frustum, torch.float64, "frustum")
            assert frustum.numel() == B * 72
        self.dev = dev = anchors.device if device is None else device
        multi = T > 1 or self.di_cfg is not None
        if out is None:
            out = {name: torch.empty(shape, dtype=dt, device=dev)
                   for name, shape, dt in _predict_layout(B, T, post_max, multi, self.di_cfg is not None)}
        assert out["box"].numel() >= B * T * post_max * 7 and out["score"].numel() >= B * T * post_max
        self.anchors, self.frustum, self.out, self.sticky, self.ws = anchors, frustum, out, sticky, workspace
        self.need = int(lib.sessd_predict_workspace_bytes(B, T, 2 * P, int(pre_max), post_max, 0 if self.di_cfg is None else 1))
        assert workspace is None or workspace.numel() >= self.need
        a = self.args = PredictArgs()
        a.batch, a.num_tasks, a.num_pixels = B, T, P
        a.anchors, a.anchors_per_frame, a.frustum = anchors.data_ptr(), 2 * P if anchors.dim() == 4 else 0, _p(frustum)
        a.score_thresh, a.pre_max_size, a.post_max_size, a.nms_iou_thresh = float(score_thresh), int(pre_max), post_max, float(nms_thresh)
        a.post_center_range[:] = [float(v) for v in post_center_range]
        a.direction_offset = float(direction_offset)
        a.out_box, a.out_score, a.out_label, a.out_count = [out[k].data_ptr() for k in ("box", "score", "label", "count")]
        a.out_task_count = _p(out.get("task_count")) if multi else 0
        if self.di_cfg is not None:
            assert out["di_truncated"].numel() >= B * T and out["di_truncated"].dtype == torch.int32
            a.di = ctypes.pointer(self.di_cfg)
            a.di_truncated, a.di_truncated_sticky = out["di_truncated"].data_ptr(), _p(sticky)
            a.di_keep, a.di_keep_count = _p(out.get("di_keep")), _p(out.get("di_keep_count"))

    def launch(self, head, keys=None, records=None, stream=None):
        """One call of sessd_predict on head (B, T*22, P). keys = (keys, key_count): the score-filter keys the head launch already
        produced; records = (records (F, T*post, 9), counts (F,), cursor (1,)): the ring the call's last launch appends the frames'
        detection records to. None = absent: both bindings are set on EVERY launch, so none survives from an earlier one."""
        B, T, P, a = self.B, self.T, self.P, self.args
        _req(head, torch.float32, "head")
        if tuple(head.shape) != (B, T * TASK_HEAD_CH, P):
            raise ValueError("predict takes 22 planar head channels per task (one class, two rotations per location): head (%d, %d, %d), "
                             "got %s for %d tasks" % (B, T * TASK_HEAD_CH, P, tuple(head.shape), T))
        k, kc = keys if keys is not None else (None, None)
        if k is not None:
            assert kc is not None and k.numel() >= B * T * 2 * P and kc.numel() >= B * T
        rec, rcnt, rcur = records if records is not None else (None, None, None)
        if rec is not None:
            assert rec.shape[1] == T * self.post_max and rec.shape[2] == 9, "records: (frames, num_tasks * post_max, 9)"
        a.head, a.ext_keys, a.ext_key_count = head.data_ptr(), _p(k), _p(kc)
        a.records, a.record_counts, a.cursor = _p(rec), _p(rcnt), _p(rcur)
        a.capacity_frames = int(rec.shape[0]) if rec is not None else 0
        ws = self.ws if self.ws is not None else workspace(self.need, self.dev, "predict")
        check(lib.sessd_predict(ctypes.byref(a), ws.data_ptr(), ws.numel(), _stream() if stream is None else stream), "predict")
        return self.out


def predict(head, anchors, frustum=None, score_thresh=0.3, pre_max=1000, post_max=100, nms_thresh=0.01,
            post_center_range=(0, -40.0, -5.0, 70.4, 40.0, 5.0), direction_offset=0.0, out=None, keys=None, key_count=None,
            records=None, num_tasks=1, nms_type="rotate_nms", di=None, sticky=None):
    """head (B,22,P) planar float32; anchors (A,7) or (B,A,7); frustum (B,1,6,4,3) float64 or None.
    Returns dict(box (B,post,7), score (B,post), label (B,post) int32, count (B,) int32), all on the device.
    keys / key_count: the score-filter keys already produced by ssfa_fuse_head(keys=...) (sessd_predict skips its own filter);
    records = (records (F,post,9) float32, counts (F,) int32, cursor (1,) int32): the call's last launch also appends the
    frames' detection records to that ring.
    num_tasks = T > 1: head (B,T*22,P) = (B,T,22,P); anchors (T,A,7) shared by the frames or (B,T,A,7);
    every task runs its own score filter, top-k, NMS and post_max. Returns box (B,T*post,7), score / label (B,T*post), count (B,)
    -- task 0's detections in NMS order, then task 1's, ...; label = task index -- and task_count (B,T); records (F,T*post,9).
    nms_type = "rotate_weighted_nms" (any T): DI-NMS instead of the greedy rotated NMS, per (frame, task), with
    the settings `di` (keys of DI_DEFAULTS; None = the reference's literals); pre_max <= 1024; nms_thresh is not read (as in the
    reference). The selection stops at post_max kept boxes: the result also carries di_truncated (B,T) int32, 1 where candidates
    were left (sticky: one int32 that 1 is ORed into in that case), and di_keep (B,T,post) / di_keep_count (B,T): the kept
    candidates' ranks in the top-k order before the filters. Returns the layout of num_tasks = T (task_count included) for every T.
    One Predict built and launched once: a caller with a fixed shape keeps the Predict instead."""
    B, _, P = head.shape
    if out is not None and nms_type == "rotate_weighted_nms":  # a caller's dict receives the DI entries it lacks
        for name, shape, dt in _predict_layout(B, check_num_tasks(num_tasks), post_max, True, True):
            if name.startswith("di_") and name not in out:
                out[name] = torch.empty(shape, dtype=dt, device=head.device)
    stage = Predict(B, num_tasks, P, anchors, frustum, score_thresh, pre_max, post_max, nms_thresh, post_center_range, direction_offset,
                    nms_type, di, head.device, out, sticky=sticky)
    return stage.launch(head, None if keys is None else (keys, key_count), records)


def rotate_nms_corners_sorted(corners, thresh, post_max):
    """corners (N,4,2) sorted by descending score -> (keep int32[post_max], num int32[1]) on the device
    (rotate_non_max_suppression_cpu of nms_cpu.h:72-168)."""
    _req(corners, torch.float32, "corners")
    n = corners.shape[0]
    keep = torch.empty((post_max,), dtype=torch.int32, device=corners.device)
    num = torch.zeros((1,), dtype=torch.int32, device=corners.device)
    ws = workspace(lib.sessd_rotate_nms_workspace_bytes(n), corners.device, "rnms")
    check(lib.sessd_rotate_nms_corners_sorted(corners.data_ptr(), n, float(thresh), int(post_max), keep.data_ptr(),
                                              num.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "rotate_nms_corners_sorted")
    return keep, num


def rotate_nms_sorted(dets, thresh, post_max):
    """dets (N,5) [x,y,w,l,r] sorted by descending score -> (keep int32[post_max], num int32[1]) on the device."""
    _req(dets, torch.float32, "dets")
    n = dets.shape[0]
    keep = torch.empty((post_max,), dtype=torch.int32, device=dets.device)
    num = torch.zeros((1,), dtype=torch.int32, device=dets.device)
    ws = workspace(lib.sessd_rotate_nms_workspace_bytes(n), dets.device, "rnms")
    check(lib.sessd_rotate_nms_sorted(dets.data_ptr(), n, float(thresh), int(post_max), keep.data_ptr(), num.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream()), "rotate_nms_sorted")
    return keep, num
