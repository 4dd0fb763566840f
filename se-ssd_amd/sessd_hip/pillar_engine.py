"""Whole-frame inference engine of the PointPillars config: voxelize -> pillar feature net + scatter -> three-block RPN with
one-launch up-samplers -> head -> predict on one HIP stream.

The same lifecycle as engine.InferenceEngine -- every buffer allocated in the constructor, every data-dependent count on the
device, nothing in `enqueue()` synchronises, so a frame is some thirty back-to-back launches that `capture()` records in a hipGraph and
`replay()` re-issues -- but none of its sparse or tile-list state: this engine is built FROM the det3d-mirror PointPillars
(PillarFeatureNet / PointPillarsScatter / RPN / MultiGroupHead), reads its parameters, folds eval-mode BatchNorm and packs the
weights with the packers the modules use, so that every block output is bit for bit the module path's.

What the frame does NOT do that the module path does: allocate, clear the canvas in a call of its own allocation, and
torch.cat the up-samplers' outputs -- each up-sampler is ONE launch of sessd_deconv_ks_slice that writes its own channels of the
(B, sum us_num_filters, H', W') neck map. `fused_upsamplers = False` (set before capture()) selects the module path's lowering
instead (ops.pack_deconv2d_ks: s * s one-tap launches into a scratch map, + a copy into the slice): for A/B runs and for the
bit-equality test against the module path.

The front end (clouds -> canvas) has two forms, `front_end=`: "tensor" = sessd_voxelize_frames, which writes the (N, T, 4) pillar
tensor, then sessd_pillar_features, which reads its live slots; "fused" = sessd_pillar_frames, the same insert / count / assign
launches followed by ONE wave-per-pillar launch that reads the voxelizer's index lists and the staged cloud itself -- the same bits
on the canvas, no pillar tensor. DEFAULT_FRONT_END is what scripts/pillar_engine_probe.py measured faster.

For runner.HostFedPipeline / runner.pillar_engines_on_cu_sets the engine has InferenceEngine's runner surface: attach_records()
(a device ring the frame's last launch appends its detections to), num_tasks, nms_truncated, cu_budget, err_text.

Not here: multi-task heads, tile lists, training."""
import numpy as np
import torch
from torch import nn

from ._lib import lib, check
from . import ops
from .engine import FrameEngine, fold_bn, _round_up

UP_STRIDES = (1, 2, 4)   # sessd_deconv_ks_slice
FRONT_ENDS = ("fused", "tensor")
DEFAULT_FRONT_END = "fused"


def _block_layers(block, i):
    """[(conv, bn)] of an RPN block: ZeroPad2d(1) + (3x3 conv, BN, ReLU) x (1 + n); ValueError names what is not that."""
    mods = list(block._modules.values())
    what = "RPN block %d must be ZeroPad2d(1) + (3x3 conv, BatchNorm2d, ReLU) x (1 + n)" % i
    if not mods or not isinstance(mods[0], nn.ZeroPad2d) or tuple(mods[0].padding) != (1, 1, 1, 1) or (len(mods) - 1) % 3 or len(mods) < 4:
        raise ValueError("%s, got %d modules starting with %s" % (what, len(mods), type(mods[0]).__name__ if mods else None))
    layers = []
    for k in range(1, len(mods), 3):
        conv, bn, act = mods[k], mods[k + 1], mods[k + 2]
        first = k == 1
        if (not isinstance(conv, nn.Conv2d) or tuple(conv.kernel_size) != (3, 3) or conv.bias is not None
                or not isinstance(bn, nn.BatchNorm2d) or not isinstance(act, nn.ReLU)
                or tuple(conv.padding) != ((0, 0) if first else (1, 1))):
            raise ValueError("%s: layer %d is (%s, %s, %s)" % (what, (k - 1) // 3, type(conv).__name__, type(bn).__name__, type(act).__name__))
        if conv.stride[0] != conv.stride[1] or (first and conv.stride[0] not in (1, 2)) or (not first and conv.stride[0] != 1):
            raise ValueError("RPN block stride must be 1 or 2 (first layer of the block; 1 for the others), got %s in block %d"
                             % (tuple(conv.stride), i))
        if conv.in_channels % 2 or conv.out_channels % 2:
            raise ValueError("RPN block channel counts must be even, got %d -> %d in block %d" % (conv.in_channels, conv.out_channels, i))
        layers.append((conv, bn))
    return layers


def check_pillar_model(model, canvas_hw=None):
    """The limits of PillarEngine, on the modules alone (no device; a CPU model will do): ValueError that names the limit.
    canvas_hw = (ny, nx): also checks that the up-samplers' outputs share one spatial size on that canvas. Returns
    dict(blocks=[[(conv, bn), ...]], ups=[(deconv, bn, stride)], head=Head)."""
    from det3d.models.readers.pillar_encoder import PillarFeatureNet, PointPillarsScatter
    from det3d.models.necks.rpn_v1 import RPN
    if model.training:
        raise ValueError("PillarEngine needs the model in eval mode (model.training is True): BatchNorm is folded from the running statistics")
    reader = getattr(model, "reader", None)
    if not isinstance(reader, PillarFeatureNet):
        raise ValueError("PillarEngine: the reader must be a PillarFeatureNet, got %s" % type(reader).__name__)
    if len(reader.pfn_layers) != 1:
        raise ValueError("PillarEngine: the reader must have ONE PFN layer, got %d" % len(reader.pfn_layers))
    pfn = reader.pfn_layers[0]
    if pfn.units != ops.PILLAR_CHANNELS or not isinstance(pfn.norm, nn.BatchNorm1d):
        raise ValueError("PillarEngine: the PFN layer must have %d filters and a BatchNorm1d, got %d filters and %s"
                         % (ops.PILLAR_CHANNELS, pfn.units, type(pfn.norm).__name__))
    if not isinstance(getattr(model, "backbone", None), PointPillarsScatter):
        raise ValueError("PillarEngine: the backbone must be a PointPillarsScatter, got %s" % type(getattr(model, "backbone", None)).__name__)
    neck = getattr(model, "neck", None)
    if not isinstance(neck, RPN):
        raise ValueError("PillarEngine: the neck must be an RPN, got %s" % type(neck).__name__)
    if neck._upsample_start_idx != 0 or len(neck.deblocks) != len(neck.blocks):
        raise ValueError("PillarEngine: the up-samplers must start at block 0 (_upsample_start_idx == 0: one up-sampler per block), "
                         "got %d blocks and us_layer_strides of %d" % (len(neck.blocks), len(neck._upsample_strides)))
    blocks = [_block_layers(b, i) for i, b in enumerate(neck.blocks)]
    if blocks[0][0][0].in_channels != ops.PILLAR_CHANNELS:
        raise ValueError("PillarEngine: the neck must take the %d canvas channels, got %d" % (ops.PILLAR_CHANNELS, blocks[0][0][0].in_channels))
    ups = []
    for i, de in enumerate(neck.deblocks):
        mods = list(de._modules.values())
        stride = neck._upsample_strides[i]
        up = mods[0]
        if int(stride) != stride or int(stride) not in UP_STRIDES or not isinstance(up, nn.ConvTranspose2d):
            raise ValueError("PillarEngine: every up-sampler stride must be an integer in %s (a ConvTranspose2d), got %r for up-sampler %d"
                             % (UP_STRIDES, stride, i))
        s = int(stride)
        if (tuple(up.kernel_size) != (s, s) or tuple(up.stride) != (s, s) or up.bias is not None or len(mods) != 3
                or not isinstance(mods[1], nn.BatchNorm2d) or not isinstance(mods[2], nn.ReLU)):
            raise ValueError("PillarEngine: up-sampler %d must be ConvTranspose2d(k = stride, bias=False) + BatchNorm2d + ReLU" % i)
        if up.in_channels != blocks[i][-1][0].out_channels or up.in_channels % 2 or up.out_channels % 32:
            raise ValueError("PillarEngine: up-sampler %d needs even input channels and output channels %% 32 == 0, got %d -> %d"
                             % (i, up.in_channels, up.out_channels))
        ups.append((up, mods[1], s))
    if canvas_hw is not None:
        h, w = int(canvas_hw[0]), int(canvas_hw[1])
        sizes = []
        for layers, (_, _, s) in zip(blocks, ups):
            st = layers[0][0].stride[0]
            h, w = (h + st - 1) // st, (w + st - 1) // st
            sizes.append((s * h, s * w))
        if len(set(sizes)) != 1:
            raise ValueError("PillarEngine: the up-sampler outputs must share one spatial size, got %s on a %d x %d canvas"
                             % (sizes, int(canvas_hw[0]), int(canvas_hw[1])))
    head = getattr(model, "bbox_head", None)
    tasks = list(getattr(head, "tasks", []))
    if len(tasks) != 1:
        raise ValueError("PillarEngine: the head must have ONE task, got %d (multi-task heads are not part of this engine)" % len(tasks))
    t = tasks[0]
    convs = [t.conv_box, t.conv_cls] + ([t.conv_dir] if t.use_dir else []) + [t.conv_iou]
    ch = sum(c.out_channels for c in convs)
    if list(head.num_classes) != [1] or not t.use_dir or ch != ops.TASK_HEAD_CH:
        raise ValueError("PillarEngine: the head's task must have one class and two rotations per location (%d planar channels), got "
                         "num_classes %s and %d channels" % (ops.TASK_HEAD_CH, list(head.num_classes), ch))
    if convs[0].in_channels != sum(u[0].out_channels for u in ups):
        raise ValueError("PillarEngine: the head must take the %d concatenated up-sampler channels, got %d"
                         % (sum(u[0].out_channels for u in ups), convs[0].in_channels))
    return dict(blocks=blocks, ups=ups, head=t)


class PillarEngine(FrameEngine):
    num_tasks = 1   # one head task (check_pillar_model): a frame's record holds post_max rows

    def __init__(self, model, voxel_generator_cfg, test_cfg, batch_size=1, max_points=32768, anchors=None, device=None,
                 front_end=None):
        """model: the mirror's PointPillars, eval mode, on the device. voxel_generator_cfg: range, voxel_size, max_points_in_voxel,
        max_voxel_num (configs.VOXEL_GENERATOR_POINTPILLARS). max_points: capacity of a frame's cloud. anchors: (A, 7) or
        (B, A, 7), A = 2 * H' * W'; None = the anchors of the head's class (configs.KITTI_3CLASS_ANCHORS) over the voxel range.
        front_end: "fused" | "tensor" (module docstring); None = DEFAULT_FRONT_END."""
        nms = test_cfg["nms"] if isinstance(test_cfg, dict) else test_cfg.nms
        self.pre_max, self.post_max = int(nms["nms_pre_max_size"]), int(nms["nms_post_max_size"])
        self.nms_thresh = float(nms["nms_iou_threshold"])
        self.nms_type, self.di = ops.nms_settings(nms, self.pre_max)   # checked before anything touches the device
        vg = voxel_generator_cfg
        self.vrange = torch.tensor([float(v) for v in vg["range"]], dtype=torch.float32)
        self.vsize = torch.tensor([float(v) for v in vg["voxel_size"]], dtype=torch.float32)
        self.grid = torch.round((self.vrange[3:] - self.vrange[:3]) / self.vsize).to(torch.int32)   # x, y, z
        nx, ny = int(self.grid[0]), int(self.grid[1])
        parts = check_pillar_model(model, (ny, nx))
        self.front_end = DEFAULT_FRONT_END if front_end is None else front_end
        if self.front_end not in FRONT_ENDS:
            raise ValueError("PillarEngine: front_end must be one of %s, got %r" % (FRONT_ENDS, front_end))
        self.dev = dev = next(model.parameters()).device if device is None else device
        if dev.type != "cuda":
            raise ValueError("PillarEngine needs the model on the HIP device: there is no CPU fallback")
        B = self.B = int(batch_size)
        self.T, self.max_voxels = int(vg["max_points_in_voxel"]), int(vg["max_voxel_num"])
        self.P_cap = _round_up(max_points, 256)
        self.nx, self.ny = nx, ny
        f32, i32 = torch.float32, torch.int32
        E = lambda *s, dt=f32: torch.empty(s, dtype=dt, device=dev)
        F = lambda t: t.detach().to(dev).float().contiguous()
        # ---- reader
        reader = model.reader
        pfn = reader.pfn_layers[0]
        self.pfn_w = F(pfn.linear.weight)
        self.pfn_scale, self.pfn_shift = [F(t) for t in fold_bn(pfn.norm)]
        self.with_distance = bool(reader._with_distance)
        self.reader_geom = (float(reader.vx), float(reader.vy), float(reader.x_offset), float(reader.y_offset))
        # ---- voxelizer: sized as ops.voxelize_frames does (hash over all staged points, its own workspace)
        self.points = torch.full((B, self.P_cap, 4), -1.0e6, dtype=f32, device=dev)   # padded rows fall out of range
        self.hash = ops.VoxelHash(self.P_cap * B, dev)
        cap = self.cap = B * self.max_voxels
        self.coors, self.nump = E(cap, 4, dt=i32), E(cap, dt=i32)
        # the (N, T, 4) pillar tensor and the mean rows: the tensor front end's alone
        self.voxels, self.mean = (E(cap, self.T, 4), E(cap, 4)) if self.front_end == "tensor" else (None, None)
        self.prefix = torch.zeros((B + 1,), dtype=i32, device=dev)   # prefix[0] stays 0; [1 .. B] written by every frame
        self.vox_ws = torch.empty(int(lib.sessd_voxelize_frames_workspace_bytes(self.hash.capacity, B, self.P_cap, self.T, self.max_voxels)),
                                  dtype=torch.uint8, device=dev)
        # a pillar outside the canvas: STICKY across frames (the kernel only ever sets it); results() reports and re-arms it
        self.err = torch.zeros((1,), dtype=i32, device=dev)
        self.err_text = "a pillar's cell lies outside the %d x %d canvas: voxel range and canvas do not match" % (ny, nx)
        self.canvas = torch.zeros((B, ops.PILLAR_CHANNELS, ny, nx), dtype=f32, device=dev)
        # ---- neck: the packers and default tile_cfg choices of RPN.forward / _run_block
        self.blocks, self.ups = [], []
        h, w, c_off = ny, nx, 0
        c_total = sum(u[0].out_channels for u in parts["ups"])
        for layers, (up, ubn, s) in zip(parts["blocks"], parts["ups"]):
            blk = []
            for conv, bn in layers:
                st = conv.stride[0]
                h, w = (h + st - 1) // st, (w + st - 1) // st
                sc, sh = fold_bn(bn)
                blk.append(dict(pc=ops.pack_conv2d(F(conv.weight), st), scale=F(sc), shift=F(sh), out=E(B, conv.out_channels, h, w)))
            self.blocks.append(blk)
            sc, sh = fold_bn(ubn)
            wt = F(up.weight)
            parent = ops.pack_conv2d(wt.transpose(0, 1).contiguous(), 1) if s == 1 else ops.pack_deconv2d_ks(wt, s)
            self.ups.append(dict(s=s, c_off=c_off, cout=up.out_channels, scale=F(sc), shift=F(sh), fused=ops.pack_deconv_ks_slice(wt, s),
                                 parent=parent, scratch=E(B, up.out_channels, s * h, s * w), x=blk[-1]["out"]))
            c_off += up.out_channels
            self.H, self.W = s * h, s * w
        H, W = self.H, self.W
        self.neck = E(B, c_total, H, W)
        # `fused_upsamplers`: True = sessd_deconv_ks_slice for every up-sampler; False = the module path's lowering + a copy
        # (bit for bit the module path); a per-layer tuple of bools is accepted, too. Set before capture().
        self.fused_upsamplers = True
        # ---- head: the task's four 1x1 convs as one packed conv (Head.planar)
        t = parts["head"]
        convs = [t.conv_box, t.conv_cls, t.conv_dir, t.conv_iou]
        self.head_pc = ops.pack_conv2d(torch.cat([F(c.weight) for c in convs], 0))
        self.head_b = torch.cat([F(c.bias) for c in convs], 0).contiguous()
        self.head = E(B, ops.TASK_HEAD_CH, H * W)
        # every weight packing made now, not by the first frame (PackedConv packs on demand)
        for pc in [L["pc"] for blk in self.blocks for L in blk] + [u["parent"] for u in self.ups] + [self.head_pc]:
            for la in pc.launches:
                la.wpk             # sessd_conv2d_mfma's fragment order
            pc.upk                 # the Winograd form ops.conv2d picks by default for a large 3x3 stride-1 layer (None if not one)
        # ---- predict, as MultiGroupHead.predict passes it: the head's own score threshold and centre range
        mh = model.bbox_head
        self.score_thresh = float(mh.thresh)
        self.post_range = [float(v) for v in mh.post_center_range]
        self.dir_offset = float(getattr(mh, "direction_offset", 0.0))
        if anchors is None:
            anchors = self._default_anchors(mh)
        anchors = anchors.detach().float() if torch.is_tensor(anchors) else torch.from_numpy(np.asarray(anchors, dtype=np.float32))
        if anchors.dim() not in (2, 3) or anchors.shape[-2] != 2 * H * W or anchors.shape[-1] != 7 or (anchors.dim() == 3 and anchors.shape[0] != B):
            raise ValueError("anchors must be (A, 7) or (B, A, 7) with A = 2 * %d * %d, got %s" % (H, W, tuple(anchors.shape)))
        self.anchors = anchors.to(dev).contiguous()
        post = self.post_max
        self.out = dict(box=torch.zeros((B, post, 7), dtype=f32, device=dev), score=torch.zeros((B, post), dtype=f32, device=dev),
                        label=torch.zeros((B, post), dtype=i32, device=dev), count=torch.zeros((B,), dtype=i32, device=dev))
        if self.nms_type == "rotate_weighted_nms":   # the layout ops.predict returns for DI-NMS (one task)
            self.out.update(task_count=torch.zeros((B, 1), dtype=i32, device=dev), di_truncated=torch.zeros((B, 1), dtype=i32, device=dev),
                            di_keep=torch.zeros((B, 1, post), dtype=i32, device=dev), di_keep_count=torch.zeros((B, 1), dtype=i32, device=dev))
        # the STICKY OR of DI-NMS's di_truncated over all frames so far (outside every per-frame clear, like self.err; nothing raises)
        self.nms_truncated = torch.zeros((1,), dtype=i32, device=dev)
        self.pred_ws = torch.empty(int(lib.sessd_predict_workspace_bytes(B, 1, 2 * H * W, self.pre_max, post, 0 if self.di is None else 1)),
                                   dtype=torch.uint8, device=dev)
        self.predict = ops.Predict(B, 1, H * W, self.anchors, None, self.score_thresh, self.pre_max, post, self.nms_thresh, self.post_range,
                                   self.dir_offset, self.nms_type, self.di, dev, out=self.out, workspace=self.pred_ws,
                                   sticky=self.nms_truncated)
        # compute units this engine's stream may use (0 = the whole chip): sizes the persistent launches of ops.conv2d
        self.cu_budget = 0
        self.graph = None
        self._marks = None

    def _wgs(self):
        """persistent workgroups of a stream-K launch of ops.conv2d (InferenceEngine._wgs): 0 = the library's choice for the whole chip"""
        return max(8, int(self.cu_budget) & ~7) if self.cu_budget else 0

    def _default_anchors(self, head):
        from . import configs
        from .anchors import create_task_anchors
        known = {t["class_names"][0]: a for t, a in zip(configs.KITTI_3CLASS_TASKS, configs.KITTI_3CLASS_ANCHORS)}
        name = head.class_names[0][0]
        if name not in known:
            raise ValueError("no anchor sizes known for class %r (known: %s): pass anchors=" % (name, sorted(known)))
        r = [float(v) for v in self.vrange]
        return create_task_anchors((self.H, self.W), [known[name]], (r[0], r[1], r[3], r[4]))[0]

    # ------------------------------------------------------------------ the frame
    def set_points(self, points_list):
        """Copy a batch of (P, 4) float32 DEVICE point clouds into the static input buffer (async; tail rows out of range)."""
        if len(points_list) != self.B:
            raise ValueError("set_points takes %d clouds, got %d" % (self.B, len(points_list)))
        s = torch.cuda.current_stream().cuda_stream
        for b, p in enumerate(points_list):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.dim() != 2 or p.shape[1] != 4 or not p.is_cuda:
                raise ValueError("points must be contiguous (P, 4) float32 device tensors")
            if p.shape[0] > self.P_cap:
                raise ValueError("frame has %d points, engine capacity is %d" % (p.shape[0], self.P_cap))
            check(lib.sessd_stage_points(p.data_ptr(), p.shape[0], self.points[b].data_ptr(), self.P_cap, s), "stage_points")

    def _mark(self, name):
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((name, ev))

    def _fused(self, i):
        f = self.fused_upsamplers
        return bool(f[i]) if isinstance(f, (tuple, list)) else bool(f)

    def enqueue(self):
        """One batch on the current stream: no host synchronisation, every count on the device, every buffer static."""
        s = torch.cuda.current_stream().cuda_stream
        self._enqueue_front(s)
        return self._enqueue_rest(s)

    def _enqueue_front(self, s):
        """staged clouds -> canvas (scripts/pillar_front_end_probe.py times this part alone)"""
        B = self.B
        vx, vy, xo, yo = self.reader_geom
        self.hash.clear()
        if self.front_end == "fused":
            # ---- 1 / 2. hash clear, canvas clear, then clouds -> canvas in five launches (no pillar tensor, no feature rows)
            check(lib.sessd_fill_u32(self.canvas.data_ptr(), 0, self.canvas.numel(), s), "fill_u32")
            self._mark("canvas_clear")
            check(lib.sessd_pillar_frames(self.points.data_ptr(), B, self.P_cap, 4, self.vrange.data_ptr(), self.vsize.data_ptr(),
                                          self.grid.data_ptr(), self.T, self.max_voxels, self.hash.keys.data_ptr(),
                                          self.hash.vals.data_ptr(), self.hash.capacity, vx, vy, xo, yo, self.pfn_w.data_ptr(),
                                          self.pfn_scale.data_ptr(), self.pfn_shift.data_ptr(), ops.PILLAR_CHANNELS,
                                          1 if self.with_distance else 0, self.ny, self.nx, self.canvas.data_ptr(),
                                          self.coors.data_ptr(), self.prefix.data_ptr(), self.nump.data_ptr(), 0, self.err.data_ptr(),
                                          self.vox_ws.data_ptr(), self.vox_ws.numel(), s), "pillar_frames")
            self._mark("front_end")
        else:
            # ---- 1. voxelize: hash clear + the four launches of all frames (the per-cell lists are cleared inside)
            check(lib.sessd_voxelize_frames(self.points.data_ptr(), B, self.P_cap, 4, self.vrange.data_ptr(), self.vsize.data_ptr(),
                                            self.grid.data_ptr(), self.T, self.max_voxels, self.hash.keys.data_ptr(),
                                            self.hash.vals.data_ptr(), self.hash.capacity, self.voxels.data_ptr(), self.coors.data_ptr(), 4,
                                            self.nump.data_ptr(), self.mean.data_ptr(), self.prefix.data_ptr(), self.vox_ws.data_ptr(),
                                            self.vox_ws.numel(), s), "voxelize_frames")
            self._mark("voxelize")
            # ---- 2. canvas clear, then pillar features with the canvas written in the SAME launch (no feature rows kept)
            check(lib.sessd_fill_u32(self.canvas.data_ptr(), 0, self.canvas.numel(), s), "fill_u32")
            self._mark("canvas_clear")
            check(lib.sessd_pillar_features(self.voxels.data_ptr(), self.nump.data_ptr(), self.coors.data_ptr(),
                                            self.prefix[B:].data_ptr(), self.cap, self.T, 4, vx, vy, xo, yo, self.pfn_w.data_ptr(),
                                            self.pfn_scale.data_ptr(), self.pfn_shift.data_ptr(), ops.PILLAR_CHANNELS,
                                            1 if self.with_distance else 0, B, self.ny, self.nx, 0, self.canvas.data_ptr(),
                                            self.err.data_ptr(), s), "pillar_features")
            self._mark("pillar")

    def _enqueue_rest(self, s):
        B = self.B
        # ---- 3 / 4. the RPN blocks, each followed by its up-sampler into its channels of the neck map
        x = self.canvas
        wgs = self._wgs()
        for i, (blk, u) in enumerate(zip(self.blocks, self.ups)):
            for L in blk:
                x = ops.conv2d(x, L["pc"], L["scale"], L["shift"], True, None, out=L["out"], workgroups=wgs)
            self._mark("blk%d" % i)
            if self._fused(i):
                ops.deconv_ks_slice(x, u["fused"], u["scale"], u["shift"], True, self.neck, u["c_off"])
            else:
                ops.conv2d(x, u["parent"], u["scale"], u["shift"], True, None, out=u["scratch"], workgroups=wgs)
                self.neck[:, u["c_off"]:u["c_off"] + u["cout"]].copy_(u["scratch"])
            self._mark("up%d" % i)
        # ---- 5. head
        ops.conv2d(self.neck, self.head_pc, None, self.head_b, False, None, out=self.head.view(B, ops.TASK_HEAD_CH, self.H, self.W),
                   workgroups=wgs)
        self._mark("head")
        # ---- 6. predict
        self.predict.launch(self.head, records=self._record_ring(), stream=s)
        self._mark("predict")
        return self.out

    def stage_times(self, reps=10):
        """Eager per-stage device time in ms of the staged batch (HIP events on the current stream, launch gaps of eager mode
        included): voxelize (with its hash and list clears), canvas_clear, pillar -- front_end "fused": canvas_clear (with the hash
        clear), front_end (the five launches of sessd_pillar_frames) -- then blk<i>, up<i>, head, predict."""
        acc = {}
        for _ in range(2):
            self.enqueue()
        for _ in range(reps):
            self._marks = []
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
            self.enqueue()
            marks, self._marks = self._marks, None
            torch.cuda.synchronize()
            prev = e0
            for name, ev in marks:
                acc[name] = acc.get(name, 0.0) + prev.elapsed_time(ev) / reps
                prev = ev
        return acc

    # ------------------------------------------------------------------ hipGraph
    def capture(self, warmup=2):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.enqueue()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        ops.new_capture_epoch()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.enqueue()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()
        return self.out
