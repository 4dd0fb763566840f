"""Whole-frame inference engine: voxelize -> SpMiddleFHD -> SSFA (or the SECOND-style RPN neck of the three-class config) -> heads
-> predict on one HIP stream.

All device buffers are allocated once for fixed capacities, every data-dependent count stays on the
device, and nothing in `enqueue()` synchronises or allocates -- so a frame is ~60 back-to-back kernel
launches that can be captured in a hipGraph (`capture()` / `replay()`), removing the Python and
launch overhead that otherwise dominates a ~1 ms frame.

The engine is built FROM the det3d-mirror modules (VoxelNet / SpMiddleFHD / SSFA / MultiGroupHead):
it reads their parameters (reference state_dict layout), folds eval-mode BatchNorm into per-channel
(scale, shift) and packs the weights into the MFMA fragment layouts of the kernels.
"""
import math
import os
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from ._lib import lib, check
from . import ops


def _round_up(v, m):
    return (int(v) + m - 1) // m * m


def fold_bn(bn):
    """eval-mode BatchNorm -> y = x*scale + shift (running statistics; eps from the module)."""
    w = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(bn.running_mean)
    b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(bn.running_mean)
    scale = w / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = b - bn.running_mean.detach().float() * scale
    return scale.contiguous(), shift.contiguous()


# (kind, cin, cout, ksize, stride, padding, indice_key) -- det3d/models/backbones/scn.py:106-148
# Stream-K Winograd shape 3 (8 waves x 128 couts on the bf16 matrix cores, f32 operands split three ways; csrc/dense_wino_sk.hip)
# among the autotune's candidates and in the default list configuration. SESSD_WINO_SPLIT=0 leaves it out (A/B runs in one tree).
WINO_SPLIT = os.environ.get("SESSD_WINO_SPLIT", "1") != "0"
WINO_LIST_SHAPES = (0, 1, 3) if WINO_SPLIT else (0, 1)
# The transposed pair over its tile list on the bf16 matrix cores (three-way split operands; csrc/dense_deconv_split.hip): the pair
# configuration PAIR_SPLIT_CFG beside the direct kernel's tile_cfg 3 / 4 / 11 / 12, among the autotune's candidates.
# SESSD_DECONV_SPLIT=0 leaves it out (A/B runs in one tree).
DECONV_SPLIT = os.environ.get("SESSD_DECONV_SPLIT", "1") != "0"
PAIR_SPLIT_CFG = 45
# The stride-2 list layer b1.0 on the bf16 matrix cores (three-way split operands; csrc/dense_conv_s2_split.hip): the active
# configuration (S2_SPLIT_CFG, 0) beside the LDS-tiled stream-K kernel's (30, min_rounds), among the autotune's candidates.
# SESSD_CONV_S2_SPLIT=0 leaves it out (A/B runs in one tree).
CONV_S2_SPLIT = os.environ.get("SESSD_CONV_S2_SPLIT", "1") != "0"
S2_SPLIT_CFG = 46

SPMIDDLE_LAYERS = [
    ("subm", 4, 16, 3, 1, 0, "subm0"), ("subm", 16, 16, 3, 1, 0, "subm0"),
    ("conv", 16, 32, 3, 2, 1, None),
    ("subm", 32, 32, 3, 1, 0, "subm1"), ("subm", 32, 32, 3, 1, 0, "subm1"),
    ("conv", 32, 64, 3, 2, 1, None),
    ("subm", 64, 64, 3, 1, 0, "subm2"), ("subm", 64, 64, 3, 1, 0, "subm2"), ("subm", 64, 64, 3, 1, 0, "subm2"),
    ("conv", 64, 64, 3, 2, [0, 1, 1], None),
    ("subm", 64, 64, 3, 1, 0, "subm3"), ("subm", 64, 64, 3, 1, 0, "subm3"), ("subm", 64, 64, 3, 1, 0, "subm3"),
    ("conv", 64, 64, (3, 1, 1), (2, 1, 1), 0, None),
]


def _t3(v):
    return [int(v)] * 3 if isinstance(v, int) else [int(x) for x in v]


class ListLayer(NamedTuple):
    """One row of an engine's table of list layers (`InferenceEngine.lists`: id -> row): a dense layer, or two that share a tile
    list, that can run over the tiles sessd_bev_tile_activity lists instead of the whole map.
    kind: "wino" = a 3x3 stride-1 layer on the stream-K Winograd list kernel, configuration (shape, min_rounds);
          "direct" = a stride-2 or 1x1 layer: (30, min_rounds) on the LDS-tiled stream-K kernel, (tile_cfg 3 / 4 / 11 / 12, 0) on the
                     direct kernel (1x1 only), (S2_SPLIT_CFG, 0) on the split bf16 kernel (3x3 stride 2 only);
          "pair" = the two transposed convs as one launch over 2x2 tiles of their input: (tile_cfg, 0) or (PAIR_SPLIT_CFG, 0);
          "branches" = conv_0 and conv_1 over one list, a Winograd list launch each: (shape, min_rounds).
    layer / x_in / x_out are pairs where the row holds two layers ("pair": one input, two outputs; "branches": two of each)."""
    name: str
    layer: Any
    x_in: Any
    x_out: Any
    mask: int              # slot of the row's tile mask / list (sessd_bev_tile_activity)
    kind: str
    near: Optional[int]    # id of the map's ONE reader where that is a 3x3 stride-1 layer on the same tile grid, else None


# Outputs whose readers run on a grid twice as coarse, or on the map's own list (coarse_fill): name -> (the readers, which must all
# run over lists; the reader whose list bounds what the fill has to reach, None = nothing needs the constant; near kind).
#   x0 (b0.2's output): read by b1.0 (3x3 stride 2, a list on the grid of ITS output: kind 2) and by trans_0 (1x1 over x0's own
#      list: computed tiles only);
#   tr0 (trans_0's output): read by the transposed pair as a residual inside its listed 4x4-pixel blocks (kind 1);
#   x1 (b1.2's output): read by trans_1 alone -- when that runs over x1's own list, NOTHING needs the constant (job dropped)
COARSE_READERS = {"b0.2": (("b1.0", "trans_0"), "b1.0", 2), "trans_0": (("deconv_0+deconv_1",), "deconv_0+deconv_1", 1),
                  "b1.2": (("trans_1",), None, 0)}


def fill_reach(table, ids, near_fill=True, coarse_fill=True):
    """The jobs of sessd_fill_inactive_tiles for the list layers `ids` of `table` (id -> ListLayer; names, kinds, masks and near
    ids are all it reads): a list of (id, part, mask slot, tile size, near slot or None, near kind), part = which of a row's two
    outputs (None: it has one). Which tiles of a map need the layer's constant depends on who reads it (near_fill): a map whose
    readers all run over tile lists gets it only where they can reach --
      a map with a `near` reader that runs over its list: 3x3 tiles around that list (kind 0);
      the maps of COARSE_READERS (coarse_fill): see there;
    everything a full-map launch reads (trans_1's and the pair's outputs, and any of the above whose reader stayed on the full
    map) is filled everywhere. Tile sizes: 2 = the layer's 2x2-output tiles; one constant per output parity class behind the
    transposed pair (4: 4x4 blocks) and behind conv_0 / conv_1 (6: 2x2 tiles)."""
    ids = list(ids)
    by_name = {table[l].name: l for l in ids}
    jobs = []
    for l in ids:
        row = table[l]
        if row.kind in ("pair", "branches"):
            jobs += [(l, part, row.mask, 4 if row.kind == "pair" else 6, None, 0) for part in (0, 1)]
            continue
        nr, kind = None, 0
        if near_fill:
            readers, bound, ckind = COARSE_READERS.get(row.name, ((), None, 0))
            if row.near is not None and row.near in ids and table[row.near].kind == "wino":
                nr = table[row.near].mask
            elif coarse_fill and readers and all(r in by_name for r in readers):
                if bound is None:
                    continue
                nr, kind = table[by_name[bound]].mask, ckind
        jobs.append((l, None, row.mask, 2, nr, kind))
    return jobs


class SparsePlan:
    """Packed weights + folded BN of a stack of sparse conv layers (generic over the layer table)."""

    def __init__(self, convs, bns, layers, device):
        self.layers = []
        for (kind, cin, cout, ks, st, pd, key), conv, bn in zip(layers, convs, bns):
            w = conv.weight.detach().to(device=device, dtype=torch.float32).contiguous()
            assert tuple(w.shape[-2:]) == (cin, cout), (w.shape, cin, cout)
            scale, shift = fold_bn(bn)
            self.layers.append(dict(kind=kind, cin=cin, cout=cout, ks=_t3(ks), st=_t3(st), pd=_t3(pd), key=key,
                                    wpk=ops.sparse_pack_weight(w), scale=scale.to(device), shift=shift.to(device)))


def active_tile_constants(neck):
    """What the SSFA layers in front of conv_0 / conv_1 (rpn_v1.py:135-199, 224) compute where their input is CONSTANT, float64 on
    the host over the folded weights: c_0 = 0 (the BEV map away from the sparse sites), c_{l+1}[co] = relu(scale * sum_ci c_l[ci] *
    sum_k W[co][ci][k] + shift) -- the stride-2 layer that opens block 1 included: away from the top / left border its window of a
    constant map is constant. Entries 0-2 = bottom_up_block_0, 3-5 = bottom_up_block_1, 6 / 7 = trans_0 / trans_1 (1x1 layers over
    the constants of block 0 / block 1), 8 = (deconv_block_0 + the residual trans_0 map, deconv_block_1): (4, cout) each, one
    constant per output parity class (py, px) -- out(2y+py, 2x+px) sums the taps ky in K(py), kx in K(px), K(0) = {1},
    K(1) = {0, 2}; 9 = (conv_0, conv_1) over those parity-class constants: (4, cout) each again.
    tests/test_active_rule_cpu.py holds them to the modules applied to constant maps."""
    b0, b1 = neck.bottom_up_block_0, neck.bottom_up_block_1
    def step(seq, ci, bi, c):
        s_, t_ = fold_bn(seq[bi])
        return torch.relu(s_.double().cpu() * (seq[ci].weight.detach().double().cpu().sum((2, 3)) @ c) + t_.double().cpu())
    def dstep(seq, c):
        s_, t_ = fold_bn(seq[1])
        w = seq[0].weight.detach().double().cpu()   # (cin, cout, 3, 3)
        K = {0: [1], 1: [0, 2]}
        rows = []
        for py in (0, 1):
            for px in (0, 1):
                ws = sum(w[:, :, ky, kx] for ky in K[py] for kx in K[px])   # (cin, cout)
                rows.append(torch.relu(s_.double().cpu() * (c @ ws) + t_.double().cpu()))
        return torch.stack(rows)
    c = torch.zeros(b0[1].weight.shape[1], dtype=torch.float64)
    chain = []
    for seq, ci, bi in ((b0, 1, 2), (b0, 4, 5), (b0, 7, 8), (b1, 0, 1), (b1, 3, 4), (b1, 6, 7)):
        c = step(seq, ci, bi, c)
        chain.append(c)
    chain += [step(neck.trans_0, 0, 1, chain[2]), step(neck.trans_1, 0, 1, chain[5])]
    chain.append((dstep(neck.deconv_block_0, chain[7]) + chain[6][None], dstep(neck.deconv_block_1, chain[7])))
    def pstep(seq, cpar):
        """a 3x3 stride-1 conv + BN + ReLU over a map that holds cpar[(py * 2 + px)] at pixels of parity (py, px): the output pixel
        of parity (py, px) sees tap (ky, kx) on a pixel of parity ((py + ky - 1) & 1, (px + kx - 1) & 1) -- again one constant per
        parity class (entry 9: conv_0 / conv_1 behind the transposed convs, rpn_v1.py:200-210, 226-227)"""
        s_, t_ = fold_bn(seq[1])
        w = seq[0].weight.detach().double().cpu()   # (cout, cin, 3, 3)
        rows = []
        for py in (0, 1):
            for px in (0, 1):
                acc = sum(w[:, :, ky, kx] @ cpar[((py + ky - 1) & 1) * 2 + ((px + kx - 1) & 1)] for ky in range(3) for kx in range(3))
                rows.append(torch.relu(s_.double().cpu() * acc + t_.double().cpu()))
        return torch.stack(rows)
    chain.append((pstep(neck.conv_0, chain[8][0]), pstep(neck.conv_1, chain[8][1])))
    return chain


def pack_task_heads(head_tasks):
    """The 1x1 heads of T tasks as ONE conv: per task [conv_box 14 | conv_cls 2 | conv_dir 4 | conv_iou 2] = 22 channels, the
    tasks one after the other -> weight (T * 22, C, 1, 1), bias (T * 22). The limits of the multi-task inference path are
    checked here: 1 to 4 tasks, one class per task, two rotations per location."""
    import torch.nn as nn
    if isinstance(head_tasks, nn.Module) and not isinstance(head_tasks, nn.ModuleList):
        head_tasks = [head_tasks]
    ops.check_num_tasks(len(head_tasks))
    ws, bs = [], []
    for t, h in enumerate(head_tasks):
        convs = [h.conv_box, h.conv_cls, h.conv_dir, h.conv_iou]
        if [c.out_channels for c in convs] != [14, 2, 4, 2]:
            raise ValueError("multi-task inference supports one class per task and two rotations per location (head channels "
                             "14 box + 2 cls + 4 dir + 2 iou); task %d has %s" % (t, [c.out_channels for c in convs]))
        ws += [c.weight for c in convs]
        bs += [c.bias for c in convs]
    return torch.cat(ws, 0), torch.cat(bs, 0)


class DensePlan:
    """SSFA neck + head lowered to conv launches (det3d/models/necks/rpn_v1.py:135-235, mg_head_sessd.py:202-230)."""

    def __init__(self, neck, head_tasks, device):
        def cbr(seq, ci, bi, deconv=False):
            conv, bn = seq[ci], seq[bi]
            w = conv.weight.detach().to(device)
            pc = ops.pack_deconv2d_s2(w) if deconv else ops.pack_conv2d(w, conv.stride[0])
            s, t = fold_bn(bn)
            return pc, s.to(device), t.to(device)

        b0, b1 = neck.bottom_up_block_0, neck.bottom_up_block_1
        self.b0 = [cbr(b0, 1, 2), cbr(b0, 4, 5), cbr(b0, 7, 8)]  # index 0 is ZeroPad2d(1) + unpadded conv == pad 1
        # What the layers in front of conv_0 / conv_1 compute where their input is CONSTANT (the BEV map is zero outside the sparse
        # sites): active_tile_constants() above; the engine writes them into the tiles it does not compute (csrc/dense_active.hip).
        chain = active_tile_constants(neck)
        self.act_const = [v.float().to(device).contiguous() for v in chain[:8]]
        self.act_const.append((chain[8][0].float().to(device).contiguous(), chain[8][1].float().to(device).contiguous()))
        self.act_const.append((chain[9][0].float().to(device).contiguous(), chain[9][1].float().to(device).contiguous()))
        self.b1 = [cbr(b1, 0, 1), cbr(b1, 3, 4), cbr(b1, 6, 7)]
        self.trans_0 = cbr(neck.trans_0, 0, 1)
        self.trans_1 = cbr(neck.trans_1, 0, 1)
        self.deconv_0 = cbr(neck.deconv_block_0, 0, 1, True)
        self.deconv_1 = cbr(neck.deconv_block_1, 0, 1, True)
        self.conv_0 = cbr(neck.conv_0, 0, 1)
        self.conv_1 = cbr(neck.conv_1, 0, 1)
        self.w0 = neck.w_0[0].weight.detach().to(device).reshape(-1).float().contiguous()
        self.w1 = neck.w_1[0].weight.detach().to(device).reshape(-1).float().contiguous()
        s0, t0 = fold_bn(neck.w_0[1])
        s1, t1 = fold_bn(neck.w_1[1])
        self.wbn = (float(s0), float(t0), float(s1), float(t1))  # host scalars, read once at plan time
        # per task the four 1x1 heads fused into one 22-channel conv [box 14 | cls 2 | dir 4 | iou 2]; the tasks one after the
        # other (task-major channels): (T * 22, C)
        hw, hb = pack_task_heads(head_tasks)
        hw, hb = hw.detach().to(device), hb.detach().to(device).float().contiguous()
        self.num_tasks = hw.shape[0] // ops.TASK_HEAD_CH
        self.head = (ops.pack_conv2d(hw), None, hb)
        self.head_w = hw.reshape(hw.shape[0], -1).float().contiguous()  # row-major (T * 22, C): the fused SSFA-tail + heads launch
        self.head_b = hb

    # the program of sessd_bev_tile_activity behind the list layers: masks 0 - 5 = the two blocks (2 = a stride-2 step), 6 = the
    # transposed pair over trans_1's map, 7 = conv_0 / conv_1 over the pair's output (steps 3, 4)
    ACTIVITY_STEPS = (0, 0, 0, 2, 0, 0, 3, 4, 0)

    def list_layers(self, bev, t, h):
        """id -> ListLayer over the engine's buffers (bev, full-resolution t, half-resolution h). Ids 0 - 5: bottom_up_block_0 /
        bottom_up_block_1; 6 / 7: the 1x1 trans layers over the lists of x0 / x1; 8: the two transposed convs as one launch over
        2x2 tiles of their input; 9: conv_0 and conv_1 (rpn_v1.py:200-210) over the 2x2 tiles of the transposed convs' OUTPUT that
        can differ from their per-parity-class constants (two launches, one list)."""
        rows = [("b0.0", self.b0[0], bev, t["a"], 0, "wino", 1), ("b0.1", self.b0[1], t["a"], t["b"], 1, "wino", 2),
                ("b0.2", self.b0[2], t["b"], t["x0"], 2, "wino", None), ("b1.0", self.b1[0], t["x0"], h["a"], 3, "direct", 4),
                ("b1.1", self.b1[1], h["a"], h["b"], 4, "wino", 5), ("b1.2", self.b1[2], h["b"], h["x1"], 5, "wino", None),
                ("trans_0", self.trans_0, t["x0"], t["tr0"], 2, "direct", None),
                ("trans_1", self.trans_1, h["x1"], h["tr1"], 5, "direct", None),
                ("deconv_0+deconv_1", (self.deconv_0, self.deconv_1), h["tr1"], (t["mid0"], t["mid1"]), 6, "pair", None),
                ("conv_0+conv_1", (self.conv_0, self.conv_1), (t["mid0"], t["mid1"]), (t["o0"], t["o1"]), 7, "branches", None)]
        return {l: ListLayer(*row) for l, row in enumerate(rows)}

    def default_active_cfg(self):
        """what autotune() ends in on MI355X; with WINO_SPLIT the 8-wave list layers on the bf16 matrix cores (shape 3)"""
        s8 = 3 if WINO_SPLIT else 0
        return {0: (1, 4), 1: (s8, 1), 2: (1, 2), 3: (30, 4), 4: (1, 2), 5: (s8, 1), 6: (11, 0), 7: (30, 8), 8: (4, 0), 9: (s8, 8)}


def _const_step(conv, bn, c):
    """relu(scale * (sum_k W[co][ci][k]) @ c + shift): what a conv + BN + ReLU layer computes on the constant map c, float64"""
    s_, t_ = fold_bn(bn)
    return torch.relu(s_.double().cpu() * (conv.weight.detach().double().cpu().sum((2, 3)) @ c) + t_.double().cpu())


def rpn_tile_constants(neck):
    """The `step` recurrence of active_tile_constants over the 3x3 stride-1 layers of the RPN neck's one block (rpn_v1.py:84-99),
    starting from 0 (the BEV map away from the sparse sites): entry l = what layer l computes where its input is constant, away
    from the border. tests/test_rpn_mirror_cpu.py holds them to the modules applied to constant maps."""
    blk = neck.blocks[0]
    c = torch.zeros(blk[1].weight.shape[1], dtype=torch.float64)
    chain = []
    for ci in range(1, len(blk), 3):
        c = _const_step(blk[ci], blk[ci + 1], c)
        chain.append(c)
    return chain


def check_rpn_neck(neck):
    """The RPN necks the engine lowers, as ValueErrors that name the limit (nothing here touches the device): what the three-class
    config uses -- ONE block of ZeroPad2d(1) + unpadded 3x3 conv, then layer_nums[0] padded 3x3 convs, all stride 1, 128 -> 128,
    each + BatchNorm2d + ReLU, and ONE stride-1 up-sampler ConvTranspose2d(128, 128, 1, stride=1) + BatchNorm2d + ReLU."""
    import torch.nn as nn
    if len(neck.blocks) != 1 or len(neck.deblocks) != 1:
        raise ValueError("the engine lowers an RPN neck of ONE block with ONE up-sampler (layer_nums=[n], us_layer_strides=[1]); "
                         "this one has %d blocks and %d up-samplers (multi-block SECOND necks are not supported)"
                         % (len(neck.blocks), len(neck.deblocks)))
    blk, de = list(neck.blocks[0]._modules.values()), list(neck.deblocks[0]._modules.values())
    convs = [m for m in blk if isinstance(m, nn.Conv2d)]
    for m in convs:
        if tuple(m.stride) != (1, 1) or tuple(m.kernel_size) != (3, 3):
            raise ValueError("the engine lowers an RPN block of 3x3 stride-1 convs (ds_layer_strides=[1]); this one has kernel %s "
                             "stride %s" % (tuple(m.kernel_size), tuple(m.stride)))
        if m.in_channels != 128 or m.out_channels != 128:
            raise ValueError("the engine lowers an RPN block of 128 filters on a 128-channel BEV map (ds_num_filters=[128], "
                             "num_input_features=128); this one has a %d -> %d conv" % (m.in_channels, m.out_channels))
    ok = len(blk) == 1 + 3 * len(convs) and isinstance(blk[0], nn.ZeroPad2d) and tuple(blk[0].padding) == (1, 1, 1, 1)
    for i, m in enumerate(convs):
        ok = ok and blk[1 + 3 * i] is m and isinstance(blk[2 + 3 * i], nn.BatchNorm2d) and isinstance(blk[3 + 3 * i], nn.ReLU)
        ok = ok and tuple(m.padding) == ((0, 0) if i == 0 else (1, 1)) and m.bias is None
    if not ok or not convs:
        raise ValueError("the engine lowers an RPN block of the form ZeroPad2d(1), (Conv2d 3x3, BatchNorm2d, ReLU) x (1 + n)")
    up = de[0]
    if not (len(de) == 3 and isinstance(up, nn.ConvTranspose2d) and tuple(up.kernel_size) == (1, 1) and tuple(up.stride) == (1, 1)
            and isinstance(de[1], nn.BatchNorm2d) and isinstance(de[2], nn.ReLU) and up.bias is None):
        raise ValueError("the engine lowers an RPN up-sampler of stride 1: ConvTranspose2d(128, 128, 1, stride=1) + BatchNorm2d + "
                         "ReLU (us_layer_strides=[1]); this one is %r" % (up,))
    if up.in_channels != 128 or up.out_channels != 128:
        raise ValueError("the engine lowers an RPN up-sampler of 128 -> 128 channels (us_num_filters=[128]); this one is %d -> %d"
                         % (up.in_channels, up.out_channels))


class RpnPlan:
    """The RPN neck of the three-class config + heads lowered to launches (det3d/models/necks/rpn_v1.py:23-116 with
    layer_nums=[n], strides 1, 128 filters; mg_head_sessd.py:202-230): `layers` = the 1 + n 3x3 stride-1 layers (index 0 is
    ZeroPad2d(1) + unpadded conv == pad 1), `up` = the stride-1 up-sampler as a 1x1 conv with the weight transposed (the
    two-launch form), `up_w` = its weight as stored, [cin][cout] (the fused tail + heads launch)."""
    form = "rpn"

    def __init__(self, neck, head_tasks, device):
        check_rpn_neck(neck)
        blk, de = neck.blocks[0], neck.deblocks[0]

        def cbr(conv, bn, w=None):
            s, t = fold_bn(bn)
            return ops.pack_conv2d((conv.weight.detach() if w is None else w).to(device), 1), s.to(device), t.to(device)

        self.layers = [cbr(blk[ci], blk[ci + 1]) for ci in range(1, len(blk), 3)]
        self.act_const = [v.float().to(device).contiguous() for v in rpn_tile_constants(neck)]
        wt = de[0].weight.detach().float()   # (cin, cout, 1, 1): y[o] = sum_i x[i] * W[i][o]
        self.up = cbr(de[0], de[1], w=wt.transpose(0, 1).contiguous())
        self.up_w = wt.reshape(wt.shape[0], wt.shape[1]).to(device).contiguous()
        hw, hb = pack_task_heads(head_tasks)
        if hw.shape[1] != 128:
            raise ValueError("the heads behind an RPN neck read its 128 channels (in_channels=128), got %d" % hw.shape[1])
        hw, hb = hw.detach().to(device), hb.detach().to(device).float().contiguous()
        self.num_tasks = hw.shape[0] // ops.TASK_HEAD_CH
        self.head = (ops.pack_conv2d(hw), None, hb)
        self.head_w = hw.reshape(hw.shape[0], -1).float().contiguous()  # row-major (T * 22, C): the fused tail + heads launch
        self.head_b = hb

    @property
    def ACTIVITY_STEPS(self):
        """layer i = mask slot i, all stride 1"""
        return (0,) * len(self.layers)

    def list_layers(self, bev, t, h):
        """id -> ListLayer, one row per layer of the block, all on the Winograd list launches, where every layer has a map of its
        own (t["l0"] ...: an engine with a tile-activity program); outputs 0 .. n-2 have one reader each, the next layer on the same
        grid, the last one is read by the tail launch over the whole map (filled everywhere)."""
        nl = len(self.layers)
        if "l%d" % (nl - 1) not in t:
            return {}
        bufs = [bev] + [t["l%d" % i] for i in range(nl)]
        return {i: ListLayer("blk0.%d" % i, self.layers[i], bufs[i], bufs[i + 1], i, "wino", i + 1 if i < nl - 1 else None)
                for i in range(nl)}

    def default_active_cfg(self):
        """what autotune() chose on MI355X for the full-size three-class engine (DESIGN.md section 3,
        profiles/rpn_tail_and_lists.json): the four-wave shape, stream-K shares of >= 4 rounds for the first (shortest) list and
        whole units for the next three; the eight-wave shape (bf16 split where built) on whole units for the last two"""
        s8 = 3 if WINO_SPLIT else 0
        tuned = [(1, 4), (1, -1), (1, -1), (1, -1), (s8, -1), (s8, -1)]
        return {i: tuned[min(i, 5)] for i in range(len(self.layers))}


class FrameEngine:
    """What the whole-frame engines share around their predict stage: the device ring of detection records and the synchronising
    read-back. A subclass has B, dev, num_tasks, post_max (a frame's record holds num_tasks * post_max rows), out, graph, the
    sticky device flag err and its message err_text."""
    records = record_counts = record_cursor = None

    def attach_records(self, capacity_frames):
        """Keep every frame's detections on the device as a fixed-size record (capacity_frames, num_tasks * post_max, 9) [box 7 |
        score | label] + counts, appended by the frame's own last launch (also inside a captured graph, hence before capture())."""
        if self.graph is not None or getattr(self, "graph_front", None) is not None:
            raise RuntimeError("attach_records must precede capture(): the ring's address is baked into the graph")
        cap = max(int(capacity_frames), self.B)
        self.records = torch.zeros((cap, self.num_tasks * self.post_max, 9), dtype=torch.float32, device=self.dev)
        self.record_counts = torch.zeros((cap,), dtype=torch.int32, device=self.dev)
        self.record_cursor = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        return self.records, self.record_counts

    def _record_ring(self):
        """launch()'s `records` of the frame: the attached ring, or None"""
        return None if self.records is None else (self.records, self.record_counts, self.record_cursor)

    def results(self):
        """The one synchronising read-back: list of dict(box3d_lidar, scores, label_preds) numpy per frame; raises err_text (once,
        then re-armed) when the sticky device flag is set."""
        cnt = self.out["count"].cpu().numpy()
        if int(self.err.item()) != 0:
            self.err.zero_()
            raise RuntimeError(self.err_text)
        res = []
        for b in range(self.B):
            n = int(cnt[b])
            res.append(dict(box3d_lidar=self.out["box"][b, :n].cpu().numpy(), scores=self.out["score"][b, :n].cpu().numpy(),
                            label_preds=self.out["label"][b, :n].cpu().numpy().astype(np.int64)))
        return res


class InferenceEngine(FrameEngine):
    err_text = "sparse level capacity overflow: raise `growth` or max_voxels"

    def __init__(self, model, voxel_range, voxel_size, max_points_per_voxel, max_voxels, test_cfg, batch_size=1,
                 max_points_per_frame=32768, device=None, growth=(1.5, 1.0, 0.75, 0.75), anchors=None,
                 use_frustum=False, allow_winograd=True, sort_sites=False, sort_tiles=False, active_tiles=True):
        """growth[i]: capacity of sparse level i+1 relative to level i (observed ratios on KITTI-like scans are
        ~1.05-1.25, 0.5, 0.4, 0.85; the worst case is 8 / 8 / 8 / 2). Exceeding a capacity raises in results().
        sort_sites: renumber the voxels by grid row between the voxelizer and the first sparse conv
        (sessd_sparse_renumber_sites; validated on hardware in round 2, tests/test_site_renumber_gpu.py); the detections do
        not depend on it."""
        # the post-processor (test_cfg["nms"]["nms_type"]: the greedy rotated NMS, or DI-NMS = "rotate_weighted_nms"), checked
        # before anything touches the device
        nms = test_cfg["nms"] if isinstance(test_cfg, dict) else test_cfg.nms
        self.nms_type, self.di = ops.nms_settings(nms, int(nms["nms_pre_max_size"]))
        # the neck's form: "ssfa" (DensePlan) or "rpn" (RpnPlan: the SECOND-style neck of the three-class config, whose limits are
        # checked here, too)
        self.form = "rpn" if type(model.neck).__name__ == "RPN" else "ssfa"
        if self.form == "rpn":
            check_rpn_neck(model.neck)
        self.dev = torch.device("cuda:0") if device is None else device
        dev = self.dev
        self.B = int(batch_size)
        self.max_voxels = int(max_voxels)
        self.max_points = int(max_points_per_voxel)
        self.P_cap = _round_up(max_points_per_frame, 256)
        self.vrange = torch.tensor(voxel_range, dtype=torch.float32)
        self.vsize = torch.tensor(voxel_size, dtype=torch.float32)
        self.grid = torch.round((self.vrange[3:] - self.vrange[:3]) / self.vsize).to(torch.int32)  # x,y,z
        gx, gy, gz = [int(v) for v in self.grid]
        self.sparse_shape = [gz + 1, gy, gx]  # scn.py:179
        convs = [m for m in model.backbone.middle_conv if hasattr(m, "indice_key")]
        bns = [m for m in model.backbone.middle_conv if isinstance(m, torch.nn.BatchNorm1d)]
        self.sp = SparsePlan(convs, bns, SPMIDDLE_LAYERS, dev)
        self.dn = (RpnPlan if self.form == "rpn" else DensePlan)(model.neck, model.bbox_head.tasks, dev)
        T = self.num_tasks = self.dn.num_tasks  # (frame, task) goes through predict as the virtual frame b * T + t
        nms = test_cfg["nms"] if isinstance(test_cfg, dict) else test_cfg.nms
        self.score_thresh = float(test_cfg["score_threshold"])
        self.pre_max = int(nms["nms_pre_max_size"])
        self.post_max = int(nms["nms_post_max_size"])
        self.nms_thresh = float(nms["nms_iou_threshold"])
        self.post_range = torch.tensor([float(v) for v in test_cfg["post_center_limit_range"]], dtype=torch.float32)
        self.dir_offset = float(getattr(model.bbox_head, "direction_offset", 0.0))
        self.use_frustum = use_frustum
        self.allow_winograd = allow_winograd
        B = self.B
        # ---------------- level geometry and capacities
        self.levels = []  # dict(shape, cap)
        shape = list(self.sparse_shape)
        cap = _round_up(B * self.max_voxels, 64)
        self.levels.append(dict(shape=shape, hash_dims=[gz, gy, gx], cap=cap))
        if isinstance(growth, (int, float)):
            growth = (growth,) * 4
        gi = 0
        for (kind, cin, cout, ks, st, pd, key) in SPMIDDLE_LAYERS:
            if kind == "conv":
                ks3, st3, pd3 = _t3(ks), _t3(st), _t3(pd)
                shape = [(d + 2 * p - k) // s + 1 for d, k, s, p in zip(shape, ks3, st3, pd3)]
                cells = B * shape[0] * shape[1] * shape[2]
                cap = _round_up(min(int(growth[gi] * cap), cells), 64)
                gi += 1
                self.levels.append(dict(shape=shape, hash_dims=shape, cap=cap))
        self.bev_c = 64 * self.levels[-1]["shape"][0]
        self.H, self.W = self.levels[-1]["shape"][1], self.levels[-1]["shape"][2]
        H, W = self.H, self.W
        f32, i32 = torch.float32, torch.int32
        E = lambda *s, dt=f32: torch.empty(s, dtype=dt, device=dev)
        # ---------------- static buffers
        self.points = torch.full((B, self.P_cap, 4), -1.0e6, dtype=f32, device=dev)  # padded rows fall out of range
        cap0 = self.levels[0]["cap"]
        self.voxels = E(cap0, self.max_points, 4)
        self.coors = E(cap0, 4, dt=i32)
        self.nump = E(cap0, dt=i32)
        self.vfeat = E(cap0, 4)
        # ---- sites and rulebooks of the whole strided chain (csrc/sparse_sites.hip): levels 1.. numbered in (b,z,y,x) order
        steps = [(lay[3], lay[4], lay[5]) for lay in SPMIDDLE_LAYERS if lay[0] == "conv"]
        jobs, li = [], 0
        self._job_of = {}  # layer index -> job index
        for idx, (kind, cin, cout, ks, st, pd, key) in enumerate(SPMIDDLE_LAYERS):
            if kind == "subm":
                if ("subm", li) not in self._job_of:
                    self._job_of[("subm", li)] = len(jobs)
                    jobs.append((li, li, ks, 1, [k // 2 for k in _t3(ks)]))
                self._job_of[idx] = self._job_of[("subm", li)]
            else:
                self._job_of[idx] = len(jobs)
                jobs.append((li, li + 1, ks, st, pd))
                li += 1
        chain_bytes = ops.SparseChain.workspace_bytes(self.sparse_shape, steps, [L["cap"] for L in self.levels[1:]], B)
        # control words + the chain's occupancy maps, cleared to 0 by the frame's one clear launch: prefix[B+1] | (unused) |
        # key_count[B * T] (candidates per (frame, task) of the score filter that runs inside the head launch) | maps
        n_ctrl = (B + 2 + B * T + 63) // 64 * 64
        self.zero_arena = torch.zeros((n_ctrl + (chain_bytes + 3) // 4,), dtype=i32, device=dev)
        self.ctrl = self.zero_arena[:n_ctrl]
        self.prefix = self.ctrl[:B + 1]
        # overflow flag of the sparse levels: OUTSIDE the per-frame clear arena, so that it is STICKY across frames (kernels only
        # ever OR into it) -- a pipeline that reads it once per fetch / per job still sees an overflow of any earlier frame
        # (round-3 advisor finding: inside the arena the next frame's clear erased it). results() / the pipeline clear it when
        # they raise.
        self.err = torch.zeros((1,), dtype=i32, device=dev)
        self.key_count = self.ctrl[B + 2:B + 2 + B * T]
        self.chain = ops.SparseChain(self.sparse_shape, steps, [L["cap"] for L in self.levels[1:]], B, jobs, dev,
                                     workspace_tensor=self.zero_arena[n_ctrl:].view(torch.uint8))
        # offset-pattern tiles (sort_tiles=True): the chain also sorts the sites of every 256-row group by neighbour pattern (one
        # more launch); a sparse layer then walks those tiles when sparse_sorted[layer] says so (autotune times both: same bits
        # either way). MEASURED ON MI355X AND OFF BY DEFAULT: useful MFMA rows 57 -> 73 % (batch 1) / 63 -> 80 % (dense scene), yet
        # the autotune kept the plain tiles for EVERY layer at both scales -- the position -> row byte table adds a dependent load
        # to each tile's prologue and epilogue and the 16 sites of a tile gather from scattered rows -- and the sort launch cost
        # 0.09 ms of the dense-scene batch (profiles/r4_offset_pattern_tiles.txt)
        self.chain.sort_tiles = bool(sort_tiles)
        self.chain.bind_tables(cap0)
        # ---- one contiguous arena for everything that must read 0x7F7F7F7F at the start of a frame (hash tables,
        # per-cell point lists, first-touch words): cleared by ONE fill instead of ~17 small ones
        cap0h = int(lib.sessd_hash_capacity(self.P_cap * B))
        # all frames of a batch are voxelized by ONE set of four launches (sessd_voxelize_frames; round 3: four per frame)
        vox_bytes = int(lib.sessd_voxelize_frames_workspace_bytes(cap0h, B, self.P_cap, self.max_points, self.max_voxels))
        plan, off = [], 0

        def take(nbytes):
            nonlocal off
            o = off
            off = (off + int(nbytes) + 255) // 256 * 256
            return (o, int(nbytes))

        p_k0, p_v0, p_vox = take(cap0h * 4), take(cap0h * 4), take(vox_bytes)
        self.arena = torch.empty(off, dtype=torch.uint8, device=dev)
        view_i32 = lambda pr: self.arena[pr[0]:pr[0] + pr[1]].view(torch.int32)
        self.hash0 = ops.VoxelHash(self.P_cap * B, dev, view_i32(p_k0), view_i32(p_v0))
        self.vox_ws = self.arena[p_vox[0]:p_vox[0] + p_vox[1]]
        for li, L in enumerate(self.levels):
            c = L["cap"]
            L["feat_a"] = E(c, 64)
            L["feat_b"] = E(c, 64)
            if li == 0:
                L["indices"], L["n"] = self.coors, None  # n = prefix[B]
                L["hash"] = ops.SiteHash(self.hash0.capacity, L["hash_dims"], dev, self.hash0.keys, self.hash0.vals)
            else:
                L["indices"], L["n"] = self.chain.indices[li - 1], self.chain.n_dev[li - 1]
        self.bev = torch.zeros((B, self.bev_c, H, W), dtype=f32, device=dev)
        # an RPN engine: one buffer per layer of the block ("l0" ... : a layer in active-tile mode writes its listed tiles only, the
        # rest of ITS map holds its constant from the head of the stage; without a tile-activity program the layers ping-pong
        # between "l0" and "l1"), "out" = the up-sampler's output (the two-launch form, or keep_ssfa); no branches, no
        # half-resolution maps
        tiles_ok = bool(active_tiles) and H <= 256 and W <= 192 and H % 4 == 0 and W % 8 == 0
        if self.form == "rpn":
            nl = len(self.dn.layers)
            if nl > 8:
                tiles_ok = False   # sessd_bev_tile_activity takes at most eight slots
            self.t = {k: E(B, 128, H, W) for k in ["l%d" % i for i in range(nl if tiles_ok else min(nl, 2))] + ["out"]}
            self._rpn_bufs = [self.bev] + [self.t["l%d" % (i if tiles_ok else i & 1)] for i in range(nl)]
        else:
            self.t = {k: E(B, 128, H, W) for k in ("a", "b", "x0", "tr0", "out")}
        # the two branches after the transposed convs are one shape: adjacent buffers, so that conv_0 / conv_1 can be one launch
        if self.form == "ssfa":
            self.t["mid"], self.t["o"] = E(2 * B, 128, H, W), E(2 * B, 128, H, W)
            for k, src in (("mid0", "mid"), ("mid1", "mid"), ("o0", "o"), ("o1", "o")):
                self.t[k] = self.t[src][:B] if k.endswith("0") else self.t[src][B:]
        self.merge_branch_convs = True  # conv_0 + conv_1 as one stream-K Winograd launch when both were tuned to the same shape
        self.h = {k: E(B, 256, H // 2, W // 2) for k in ("a", "b", "x1", "tr1")} if self.form == "ssfa" else {}
        self.head = E(B, T * 22, H * W)
        if anchors is None:
            if T > 1:
                raise ValueError("a %d-task head needs its anchors: pass anchors=(T, H*W*2, 7), one set per task in task order "
                                 "(sessd_hip.anchors.create_task_anchors), here H, W = %d, %d" % (T, H, W))
            from .anchors import create_anchors_3d_range
            anchors = create_anchors_3d_range((1, H, W)).reshape(-1, 7)
        if T > 1:
            if isinstance(anchors, (list, tuple)):
                anchors = torch.stack([torch.as_tensor(a, dtype=f32).reshape(-1, 7) for a in anchors])
            anchors = torch.as_tensor(anchors, dtype=f32)
            if tuple(anchors.shape) != (T, 2 * H * W, 7):
                raise ValueError("anchors of a %d-task head: (%d, %d, 7), one set per task in task order, got %s"
                                 % (T, T, 2 * H * W, tuple(anchors.shape)))
        self.anchors = torch.as_tensor(anchors, dtype=f32).to(dev).contiguous()
        self.frustum = torch.zeros((B, 1, 6, 4, 3), dtype=torch.float64, device=dev) if use_frustum else None
        # T tasks: each keeps up to post_max rows; a frame's rows are task 0's, then task 1's, ... (label = task)
        self.out = dict(box=E(B, T * self.post_max, 7), score=E(B, T * self.post_max), label=E(B, T * self.post_max, dt=i32),
                        count=torch.zeros((B,), dtype=i32, device=dev))
        if T > 1:
            self.out["task_count"] = torch.zeros((B, T), dtype=i32, device=dev)
        self.pred_ws = torch.empty(int(lib.sessd_predict_workspace_bytes(B, T, 2 * H * W, self.pre_max, self.post_max,
                                                                         0 if self.di is None else 1)), dtype=torch.uint8, device=dev)
        # DI-NMS keeps at most post_max boxes per (frame, task) (the reference's wrapper has no cap): di_truncated (B, T) says where
        # the selection stopped with candidates left, nms_truncated is the STICKY OR over all frames so far (outside every per-frame
        # clear, like self.err; nothing raises on it)
        self.nms_truncated = torch.zeros((1,), dtype=i32, device=dev)
        if self.di is not None:
            self.out["di_truncated"] = torch.zeros((B, T), dtype=i32, device=dev)
        # (a11-a14) top-k + decode, suppression mask, greedy walk + filters (+ the frame's record): 3 launches with the head's keys;
        # DI-NMS: overlap rows and selection + filters in place of mask and walk; T > 1: the same over B * T virtual frames + the merge
        self.predict = ops.Predict(B, T, H * W, self.anchors, self.frustum, self.score_thresh, self.pre_max, self.post_max,
                                   self.nms_thresh, self.post_range, self.dir_offset, self.nms_type, self.di, dev, out=self.out,
                                   workspace=self.pred_ws, sticky=self.nms_truncated)
        self.keys = torch.empty((B * T, 2 * H * W), dtype=torch.int64, device=dev)  # score-filter keys written by the head launch
        self.fuse_predict = True  # score filter inside the head launch; NMS walk + filters + record in one launch
        self.batched_voxelizer = True  # the frames of a batch in four launches (False: four per frame, as round 3)
        # The neighbour table of the voxels (level 0, hash lookups) and the two submanifold convs that use it depend on the
        # voxelizer only, not on the site chain of the deeper levels: with fork_front they run on a second stream (a parallel
        # branch of the captured graph) beside mark / gather / count / scan / emit and the remaining tables. MEASURED SLOWER on
        # MI355X / ROCm 7.2 and therefore off: 1042 against 1067 frames/s one frame at a time, 1032 against 1310 with two frames in
        # flight -- the cross-stream edges of a two-branch hipGraph cost more than the ~19 us of launches they take off the
        # critical path, and with two engines the four streams serialise against each other.
        self.fork_front = False
        self.side_stream = torch.cuda.Stream(device=dev)
        # Active-tile mode of bottom_up_block_0, bottom_up_block_1 and the two 1x1 trans layers (round 4): the BEV map is zero
        # outside the last sparse level's sites, so these layers are computed only in the 2x2-output tiles whose input patch is
        # not constant (14 / 26 / 36 % of the tiles of block 0, 46 / 54 / 68 % of block 1's on a 20 k-point scan; a 1x1 layer is
        # computed where its input was) and the rest is filled with the layer's constant.
        # self.lists: id -> ListLayer, the table everything below reads (the plan's list_layers()); the masks are the slots of the
        # plan's ACTIVITY_STEPS program.
        self.active_tiles = bool(active_tiles)
        self.active_cfg = {}   # id -> (number, min_rounds) as ListLayer.kind reads it, chosen by autotune(); empty = dense launches
        self.ta = ops.TileActivity(B, H, W, list(self.dn.ACTIVITY_STEPS), dev) if tiles_ok else None
        self.lists = self.dn.list_layers(self.bev, self.t, self.h)
        self._list_id = {row.name: l for l, row in self.lists.items()}
        self._kind_id = {kind: next((l for l, row in self.lists.items() if row.kind == kind), -1) for kind in ("pair", "branches")}
        # the table as bench.py and the tests read it (nothing in the engine does): the rows (positional reads), mask slots, the
        # "direct" ids, the id of the pair / of the branches (-1: none), the near readers, the default configuration
        self.ACTIVE_SLOTS = self.lists
        self.ACTIVE_MASK = {l: row.mask for l, row in self.lists.items()}
        self.ACTIVE_SK = tuple(l for l, row in self.lists.items() if row.kind == "direct")
        self.ACTIVE_PAIR, self.ACTIVE_CONV = self._kind_id["pair"], self._kind_id["branches"]
        self.NEAR_READER = {l: row.near for l, row in self.lists.items() if row.near is not None}
        self.DEFAULT_ACTIVE_CFG = {l: c for l, c in self.dn.default_active_cfg().items() if l in self.lists}
        self.allow_active_conv = True   # autotune() may put conv_0 / conv_1 on their tile list (bench.py --no-active-conv: A/B)
        self.near_fill = True   # fill only the tiles a list-driven reader can reach where that reader is the map's only one
        self.coarse_fill = True  # ... also where the readers run on a grid twice as coarse (x0, tr0) or on the map's own list (x1): round 5
        # minimum share lengths autotune() tries for a Winograd list launch: > 0 rounds of a stream-K share (units may be cut, partial
        # sums through memory), < 0 WHOLE units per workgroup (round 5: nothing cut, as many workgroups as units -- slower alone on
        # a short list, but it leaves the other CUs to the second frame in flight)
        self.list_share_candidates = (1, 4, 8, 16, -1, -2)
        # EXPERIMENT, measured slower on MI355X / ROCm 7.2 and therefore off (1154 against 1163 frames/s one frame at a time, 1132
        # against ~1550 with two frames in flight): the activity + fill launches as a side branch beside the sparse convs (see enqueue)
        self.fork_active = False
        self.sort_sites = bool(sort_sites)
        if self.sort_sites:
            self.coors_s, self.vfeat_s = E(cap0, 4, dt=i32), E(cap0, 4)
            self.levels[0]["indices"] = self.coors_s
            self._hash0_dims = torch.tensor(self.levels[0]["hash_dims"], dtype=torch.int32)
            self.renum_ws = torch.empty(int(lib.sessd_sparse_renumber_workspace_bytes(B, self._hash0_dims.data_ptr())),
                                        dtype=torch.uint8, device=dev)
        self._ks = {}
        self._npts = [0] * B
        self.graph = None
        self._marks = None
        self.tile_cfg = {}
        self.sk_ws = None  # workspace of the stream-K launches, tile_cfg 22 / 23 / 30 (autotune allocates it)
        # SSFA fusion tail + the 1x1 heads in one launch (the SSFA output stays in registers); an RPN engine: the stride-1 up-sampler
        # + the heads in one launch (ops.rpn_up_head, its output stays in LDS). False: the two-launch form through ops.conv2d and
        # predict's own score filter
        # MEASURED for the RPN form on the full-size three-class engine: the fused launch 61 us against
        # 21.5 + 16.5 us for the two launches, 619 against 600 us per replayed frame -- so an RPN engine defaults to the two-launch
        # form and the fused kernel stays selectable (fuse_head = True)
        self.fuse_head = self.form != "rpn"
        self.keep_ssfa = False  # with fuse_head: also write the neck's output to self.t["out"] (tests compare it with the oracle)
        self.allow_streamk = True  # autotune may choose the stream-K kernels (Winograd: tile_cfg 22 / 23; LDS-tiled direct: 30)
        self.allow_offset_split = True  # autotune may choose the offset-split sparse conv (see sessd_sparse_conv)
        self.sk_workgroups = 0  # persistent workgroups of those launches (0 = one or two per CU; fewer leaves CUs to a second stream)
        # compute units this engine's stream may use (0 = the whole chip): with several frames in flight on CU-masked streams
        # (ops.cu_masked_stream, bench.py --cu-split) the persistent launches are sized for the engine's own CUs
        self.cu_budget = 0
        self.tune_report = {}
        self._tuning = None
        self._kmarks = None
        self.sparse_split = {}
        self.sparse_sorted = {}   # layer -> walk the offset-pattern tiles (default True when the chain builds them)
        self._tuning_sparse = None

    # ------------------------------------------------------------------ helpers
    def _i3(self, v):
        key = tuple(_t3(v))
        t = self._ks.get(key)
        if t is None:
            t = torch.tensor(key, dtype=torch.int32)
            self._ks[key] = t
        return t

    def _wgs(self, shape):
        """persistent workgroups of a stream-K launch: shape 0 / 1 = the Winograd shapes (one / two workgroups per CU), 2 = the
        LDS-tiled kernel (one per CU); 0 = the library's default for the whole chip"""
        if self.sk_workgroups:
            return self.sk_workgroups
        if not self.cu_budget:
            return 0
        return max(8, ((2 if shape == 1 else 1) * int(self.cu_budget)) & ~7)

    def _wgs_cfg(self, cfg):
        return self._wgs(1 if cfg == 23 else (2 if cfg == 30 else 0))

    def set_points(self, points_list, frustum=None):
        """Copy a batch of (P,4) float32 DEVICE point clouds into the static input buffer (async D2D)."""
        assert len(points_list) == self.B
        for b, p in enumerate(points_list):
            n = p.shape[0]
            if n > self.P_cap:
                raise ValueError("frame has %d points, engine capacity is %d" % (n, self.P_cap))
            if p.dtype != torch.float32 or not p.is_contiguous() or p.shape[1] != 4 or not p.is_cuda:
                raise ValueError("points must be contiguous (P,4) float32 device tensors")
            check(lib.sessd_stage_points(p.data_ptr(), n, self.points[b].data_ptr(), self.P_cap,
                                         torch.cuda.current_stream().cuda_stream), "stage_points")
        if frustum is not None and self.frustum is not None:
            self.frustum.copy_(frustum.reshape(self.frustum.shape), non_blocking=True)

    def _n(self, li):
        L = self.levels[li]
        return self.prefix.data_ptr() + 4 * self.B if li == 0 else L["n"].data_ptr()

    def _sconv(self, lay, in_feat, nbr, tm, out_li, out_feat, s, dense=False, idx=None):
        Lo = self.levels[out_li]
        kv = lay["ks"][0] * lay["ks"][1] * lay["ks"][2]
        dd = self._i3(Lo["shape"]).data_ptr() if dense else 0
        perm = 0
        if self.chain.sort_tiles and self.sparse_sorted.get(idx, True):
            j = self._job_of[idx]
            if self.chain.nbr[j] is nbr:   # the layer runs on the chain's own table: its sorted tiles
                tm, perm = self.chain.tile_mask_sorted[j], self.chain.perm[j].data_ptr()
        check(lib.sessd_sparse_conv_sorted(in_feat.data_ptr(), lay["cin"], nbr.data_ptr(), tm.data_ptr(), kv, self._n(out_li),
                                           Lo["cap"], lay["wpk"].data_ptr(), lay["scale"].data_ptr(), lay["shift"].data_ptr(), 1,
                                           0 if dense else out_feat.data_ptr(), lay["cout"],
                                           Lo["indices"].data_ptr() if dense else 0, self.bev.data_ptr() if dense else 0, dd,
                                           self.sparse_split.get(idx, 0), perm, s), "sparse_conv_sorted")
        if self._tuning_sparse is not None and not dense:
            self._tuning_sparse.append((idx, lay, in_feat, nbr, tm, out_li, out_feat))

    def _need_sk_ws(self, nbytes):
        """The engine's stream-K workspace holds at least nbytes: a fresh zeroed buffer if it did not (it never shrinks)."""
        if self.sk_ws is None or self.sk_ws.numel() < nbytes:
            self.sk_ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)

    def _branch_sets(self, shape):
        """conv_0 / conv_1 as two weight sets of one launch: packed U back to back, BatchNorm constants stacked (made once)."""
        key = "_sets%d" % shape
        if not hasattr(self, key):
            d = self.dn
            (p0, s0, t0), (p1, s1, t1) = d.conv_0, d.conv_1
            u0, u1 = p0.upk_sk(shape), p1.upk_sk(shape)
            ok = u0 is not None and u1 is not None and p0.cout == p1.cout == 128 and p0.cin == p1.cin and s0 is not None and s1 is not None
            need = int(lib.sessd_conv3x3_winograd_sk_workspace_bytes(2 * self.B, self.H, self.W, 128, shape, 0)) if ok else 0
            if ok and self.sk_ws is not None:
                self._need_sk_ws(need)
            setattr(self, key, dict(upk=torch.cat([u0.reshape(-1), u1.reshape(-1)]), scale=torch.stack([s0, s1]).contiguous(),
                                    shift=torch.stack([t0, t1]).contiguous()) if ok else None)
        return getattr(self, key)

    def _fill_jobs(self, ids):
        """(outs, values, mask slots, tile sizes, near slots, near kinds) of sessd_fill_inactive_tiles for the active layer ids:
        fill_reach()'s jobs with their buffers and constants."""
        jobs = fill_reach(self.lists, ids, self.near_fill, self.coarse_fill)
        pick = lambda v, part: v if part is None else v[part]
        outs = [pick(self.lists[l].x_out, part) for l, part, *_ in jobs]
        vals = [pick(self.dn.act_const[l], part) for l, part, *_ in jobs]
        slots, tiles, near, kinds = ([j[i] for j in jobs] for i in (2, 3, 4, 5))
        return outs, vals, slots, tiles, near, kinds

    def _lists_on(self):
        return self.ta is not None and self._tuning is None and self.sk_ws is not None

    def _active_layers(self):
        """ids (self.lists) of the layers that run in active-tile mode in this configuration"""
        return sorted(self.active_cfg) if self._lists_on() else []

    def _bracket(self, name, fn):
        """fn(), between two HIP events kept under `name` when a frame collects per-launch times (dense_layer_times)"""
        if self._kmarks is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self._kmarks.append((name, e0, e1))
        return r

    def _time(self, fn, reps):
        """ms per fn() on the current stream: two warm-up calls, then `reps` calls between two HIP events; synchronises"""
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # ------------------------------------------------------------------ the list layers: what a configuration means, per kind
    def _list_parts(self, l):
        """[(layer, input, output)] of row l: one per launch of a "wino" / "branches" row"""
        row = self.lists[l]
        return list(zip(row.layer, row.x_in, row.x_out)) if row.kind == "branches" else [(row.layer, row.x_in, row.x_out)]

    def _list_cfg_error(self, l, cfg):
        """None, or why list layer l cannot run under cfg = (number, min_rounds): a missing packing is an error, not a fall-back"""
        if l not in self.lists:
            return "an %s engine's list layers are %s, got %r" % (self.form.upper(), sorted(self.lists), l)
        row, shape = self.lists[l], cfg[0]
        if row.kind == "pair" and shape == PAIR_SPLIT_CFG and any(pc.wsplit() is None for pc, _, _ in row.layer):
            return "active-tile layer %s: no split weight planes (cin %% 16)" % row.name
        if shape == S2_SPLIT_CFG and (row.kind != "direct" or row.layer[0].wsplit_s2() is None):
            return "active-tile layer %s: no split weight planes of a 3x3 stride-2 conv (cin %% 16)" % row.name
        if row.kind == "direct" and shape == 30 and row.layer[0].sk_args() is None:
            return "active-tile layer %s: no LDS-tiled stream-K packing (cin %% 16)" % row.name
        if row.kind in ("wino", "branches") and (shape not in (0, 1, 2, 3) or any(pc.upk_sk(shape) is None for (pc, _, _), _, _ in self._list_parts(l))):
            return "active-tile layer %s: no stream-K Winograd packing for shape %d" % (row.name, shape)
        return None

    def _list_candidates(self, l):
        """The configurations autotune() times for list layer l, in the order it tries them (a tie goes to the first)."""
        row = self.lists[l]
        if row.kind in ("wino", "branches"):
            shares = self.list_share_candidates if row.kind == "wino" else (4, 8, 16, -1)
            for shape in WINO_LIST_SHAPES:
                if all(pc.upk_sk(shape) is not None for (pc, _, _), _, _ in self._list_parts(l)):
                    for mr in shares:
                        yield (shape, mr)
            return
        direct = [(cfg, 0) for cfg in (3, 4, 11, 12)]
        if row.kind == "pair":
            yield from direct
            if DECONV_SPLIT and all(pc.wsplit() is not None for pc, _, _ in row.layer):
                yield (PAIR_SPLIT_CFG, 0)
            return
        pc = row.layer[0]
        if pc.launches[0].ntaps == 1 and pc.cin % 8 == 0:
            yield from direct
        if pc.sk_args() is not None:
            for mr in (1, 4, 8, 16):
                yield (30, mr)
        if CONV_S2_SPLIT and pc.wsplit_s2() is not None:   # the 3x3 stride-2 layer: whole units on the bf16 matrix cores
            yield (S2_SPLIT_CFG, 0)

    def _list_ws_bytes(self, l, cfg):
        """stream-K workspace the launch of _list_call(l, cfg) needs (0: it uses none)"""
        row, shape = self.lists[l], cfg[0]
        if row.kind == "pair" or (row.kind == "direct" and shape != 30):
            return 0
        (pc, _, _), x_in, _ = self._list_parts(l)[0]
        if row.kind == "direct":
            return int(lib.sessd_conv2d_sk_workspace_bytes(self.B, *pc.tile_hw(*x_in.shape[2:]), pc.cout, len(pc.launches), 0))
        return int(lib.sessd_conv3x3_winograd_sk_workspace_bytes(self.B, x_in.shape[2], x_in.shape[3], pc.cout, shape, 0))

    def _list_call(self, l, cfg):
        """A callable that issues the launch (the two launches of "branches") of list layer l under cfg = (number, min_rounds) over
        the listed tiles only: the others hold the layer's constant from the fill at the head of the stage."""
        err = self._list_cfg_error(l, cfg)
        if err is not None:
            raise ValueError(err)
        row, (shape, mr) = self.lists[l], cfg
        lst = lambda: (self.ta.tile_list[row.mask], self.ta.n_list[row.mask:row.mask + 1])
        if row.kind in ("wino", "branches"):
            parts = self._list_parts(l)
            def call():
                for (pc, scale, shift), x, out in parts:
                    ops.conv2d_winograd_sk_active(x, pc.upk_sk(shape), pc.cout, scale, shift, True, out, shape, self.sk_ws, *lst(),
                                                  workgroups=self._wgs(shape), min_rounds=mr)
            return call
        if row.kind == "pair":   # both transposed convs; trans_0's map is deconv_0's residual
            (pa, sa, ta), (pb, sb, tb) = row.layer
            args = (row.x_in, pa, pb, sa, ta, sb, tb, True, row.x_out[0], row.x_out[1])
            if shape == PAIR_SPLIT_CFG:
                return lambda: ops.deconv2d_s2_pair_split_active(*args, *lst(), residual_a=self.t["tr0"])
            return lambda: ops.deconv2d_s2_pair_active(*args, *lst(), residual_a=self.t["tr0"], tile_cfg=shape)
        pc, scale, shift = row.layer
        if shape == S2_SPLIT_CFG:   # the 3x3 stride-2 layer on the split bf16 list kernel
            return lambda: ops.conv2d_s2_split_active(row.x_in, pc, scale, shift, True, row.x_out, *lst())
        if shape == 30:
            return lambda: ops.conv2d_sk_active(row.x_in, pc, scale, shift, True, row.x_out, self.sk_ws, *lst(), workgroups=self._wgs(2),
                                                min_rounds=mr)
        return lambda: ops.conv2d_mfma_active(row.x_in, pc, scale, shift, True, row.x_out, *lst(), tile_cfg=shape)   # a 1x1 layer

    def _full_map_pair(self):
        """Both transposed convs read tr1: ONE launch over their 2 x 4 parity classes (same bits as two launches) where both were
        tuned to a direct tile_cfg; None = the two layers' own launches."""
        cd = self.tile_cfg.get("deconv_0")
        if not (self.merge_branch_convs and cd in (3, 4, 11, 12) and self.tile_cfg.get("deconv_1") in (3, 4, 11, 12) and self._tuning is None):
            return None
        d, t = self.dn, self.t
        (pa, sa, ta), (pb, sb, tb) = d.deconv_0, d.deconv_1
        return lambda: ops.deconv2d_s2_pair(self.h["tr1"], pa, pb, sa, ta, sb, tb, True, t["mid0"], t["mid1"], residual_a=t["tr0"], tile_cfg=cd)

    def _full_map_branches(self):
        """conv_0 + conv_1 as ONE two-set stream-K Winograd launch where both were tuned to the same stream-K shape; None = the two
        layers' own launches."""
        c01 = self.tile_cfg.get("conv_0")
        if not (self.merge_branch_convs and c01 in (22, 23, 24, 25) and self.tile_cfg.get("conv_1") == c01 and self._tuning is None
                and self.sk_ws is not None and self._branch_sets(c01 - 22) is not None):
            return None
        sets, t = self._branch_sets(c01 - 22), self.t
        return lambda: ops.conv2d_winograd_sk_sets(t["mid"], sets["upk"], 2, 128, sets["scale"], sets["shift"], True, t["o"], c01 - 22,
                                                   self.sk_ws, self._wgs(c01 - 22))

    def _conv(self, x, layer, out, relu=True, residual=None, name=None):
        l = self._list_id.get(name)
        if l in self.active_cfg and self._lists_on():   # over its tile list (x, out = the row's buffers)
            self._bracket(name, self._list_call(l, self.active_cfg[l]))
            return out
        pc, scale, shift = layer
        if self._tuning is not None:
            self._tuning.append((name, x, layer, out, relu, residual))
        cfg = self.tile_cfg.get(name)   # per-launch HIP events inside a whole eager frame: dense_layer_times
        return self._bracket(name, lambda: ops.conv2d(x, pc, scale, shift, relu, residual, out, cfg, workspace=self.sk_ws,
                                                      workgroups=self._wgs_cfg(cfg)))

    def adopt_tuning(self, other):
        """Take another engine's tuned configuration (per-layer tilings, sparse variants, stream-K workgroup count) with a
        stream-K workspace of this engine's own: engines that run concurrently must not share one."""
        self.tile_cfg = dict(other.tile_cfg)
        self.active_cfg = dict(other.active_cfg) if self.ta is not None else {}
        self.sparse_split = dict(other.sparse_split)
        self.sparse_sorted = dict(other.sparse_sorted)
        self.sk_workgroups = other.sk_workgroups
        self.cu_budget = other.cu_budget
        self.merge_branch_convs = other.merge_branch_convs
        self.sk_ws = torch.zeros_like(other.sk_ws) if other.sk_ws is not None else None

    def force_active_tiles(self, active_cfg=None):
        """The configuration autotune() ends in on MI355X, WITHOUT timing anything: the neck's 3x3 stride-1 layers on the stream-K
        Winograd kernels, the stride-2 / 1x1 layers on the LDS-tiled stream-K kernel, and every layer of self.lists over its
        tile list with the given (kernel, minimum share) choices (default: the plan's default_active_cfg(), all of them). Allocates
        the stream-K workspace. Used by __graft_entry__.smoke() and the tests, so that what the driver smokes is the kind of
        configuration bench.py times."""
        if self.ta is None:
            raise RuntimeError("this engine has no tile-activity program (active_tiles=False or an unsupported BEV size)")
        B, wino_ws = self.B, lib.sessd_conv3x3_winograd_sk_workspace_bytes
        if self.form == "rpn":
            # its 3x3 layers on the stream-K Winograd kernel (8 waves x 128 couts, exact f32) where they run as full-map launches
            self.tile_cfg.update({"blk0.%d" % i: 22 for i in range(len(self.dn.layers))})
            self._need_sk_ws(max(int(wino_ws(B, self.H, self.W, 128, sh, 0)) for sh in (0, 1)))
        else:
            self.tile_cfg.update({"b0.0": 22, "b0.1": 22, "b0.2": 23, "b1.0": 30, "b1.1": 23, "b1.2": 22, "trans_0": 30, "trans_1": 30,
                                  "conv_0": 22, "conv_1": 22})
            self._need_sk_ws(max([int(wino_ws(2 * B, self.H, self.W, 256, sh, 0)) for sh in (0, 1)] +
                                 [int(lib.sessd_conv2d_sk_workspace_bytes(B, self.H, self.W, 256, 1, 0))]))
        cfg = dict(self.dn.default_active_cfg() if active_cfg is None else active_cfg)
        for l, c in cfg.items():
            err = self._list_cfg_error(l, c)
            if err is not None:
                raise ValueError(err)
        self.active_cfg = cfg
        return self.active_cfg

    def autotune(self, candidates=(1, 2, 3, 4, 6, 11, 12), reps=5):
        """Pick the wave/workgroup tiling of every dense conv launch by timing it on this device (one-off, ~0.1 s).
        Needs one representative frame already staged with set_points()."""
        self._tuning, self._tuning_sparse = [], []
        self.enqueue()
        torch.cuda.synchronize()
        todo, self._tuning = self._tuning, None
        todo_sp, self._tuning_sparse = self._tuning_sparse, None
        st = torch.cuda.current_stream().cuda_stream
        for idx, lay, in_feat, nbr, tm, out_li, out_feat in todo_sp:
            # sparse_split[idx] = cout_split + 256 * depth + 65536 * offset_split (sessd_sparse_conv's `tuning`). cout split and
            # depth do not change the results; the offset split (allow_offset_split; four waves per tile, for levels with fewer
            # tiles than SIMDs) has one summation order of its own (last-bit differences)
            best = (None, 1e30)
            cands = [(a, b, c) for c in ((0, 1) if self.allow_offset_split else (0,)) for a in (1, 2, 4) for b in (2, 3, 4)]
            cands += [(a, 2, 2) for a in (1, 2, 4)]  # mode 2: W[k] shared through LDS by the four tiles of a workgroup (same bits)
            # modes 16 / 32: two / four tiles per wave, the next tile's neighbour rows fetched under the current tile's MFMAs (same
            # bits); only where a level has several tiles per wave slot (the dense-scene batch)
            if self.levels[out_li]["cap"] >= 65536 or getattr(self, "sparse_mt_candidates", False):
                cands += [(a, b, c) for c in (16, 32) for a in (1, 2, 4) for b in (2, 3)]
            for split, depth, ks in cands:
                if (lay["cout"] // 16) % split or (ks == 1 and depth == 4):
                    continue
                for srt in ((True, False) if self.chain.sort_tiles else (False,)):
                    self.sparse_split[idx] = split + 256 * depth + 65536 * ks
                    self.sparse_sorted[idx] = srt
                    t = self._time(lambda: self._sconv(lay, in_feat, nbr, tm, out_li, out_feat, st, idx=idx), reps)
                    if t < best[1]:
                        best = (split + 256 * depth + 65536 * ks + (1 << 24 if srt else 0), t)
            self.sparse_split[idx] = best[0] & 0xFFFFFF
            self.sparse_sorted[idx] = bool(best[0] >> 24)
            self.tune_report["sparse%d" % idx] = best
        # A/B hook (round 6: levers that lose a per-launch timing are re-measured in the THROUGHPUT regime, where the partner frame
        # fills a launch's stalls and frames/s follows executed work): force_sparse = {layer: (tuning or None, sorted or None)}
        for idx, (tun, srt) in getattr(self, "force_sparse", {}).items():
            if tun is not None:
                self.sparse_split[idx] = int(tun)
            if srt is not None and self.chain.sort_tiles:
                self.sparse_sorted[idx] = bool(srt)
        for name, x, layer, out, relu, residual in todo:
            pc, scale, shift = layer
            best = (None, 1e30)
            cands = list(candidates)
            if pc.is_3x3_s1 and pc.cin % 16 == 0:
                cands.append(10)  # activation-stationary LDS variant
                if pc.upk is not None and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and self.allow_winograd:
                    cands.append(20)  # fused Winograd F(2x2,3x3)
                    if pc.cin % 32 == 0:
                        cands.append(21)  # same, operands fetched two rounds ahead
                    # stream-K Winograd (all couts of a unit in one workgroup, equal shares of rounds per CU): 8 waves x 128
                    # couts / 4 waves x 64 couts. One workspace per engine: its launches are serialised on the engine's stream.
                    # (tile_cfg 24, the third generation with the output transform in registers, is selectable but not a candidate:
                    # measured 81 / 96 us against 63 / 66 us for 22 / 23 on the two SSFA shapes, profiles/r4_wino_rk_probe.json)
                    for cfg, shape in ((22, 0), (23, 1)) + (((25, 3),) if WINO_SPLIT else ()) if self.allow_streamk else ():
                        if pc.upk_sk(shape) is not None:
                            self._need_sk_ws(int(lib.sessd_conv3x3_winograd_sk_workspace_bytes(x.shape[0], x.shape[2], x.shape[3], pc.cout, shape, 0)))
                            cands.append(cfg)
            # LDS-tiled stream-K implicit GEMM (csrc/dense_conv_sk.hip) for what is not 3x3 stride 1: the stride-2 conv, the 1x1
            # convs, the transposed convs (four parity classes in one launch). Shares the engine's stream-K workspace.
            if self.allow_streamk and pc.cout > 32 and not pc.is_3x3_s1 and pc.sk_args() is not None:
                self._need_sk_ws(int(lib.sessd_conv2d_sk_workspace_bytes(x.shape[0], *pc.tile_hw(*x.shape[2:]), pc.cout, len(pc.launches), 0)))
                cands.append(30)
            if pc.kind == "deconv":
                cands += [40, 41, 42]  # both px classes of a row parity in every wave: whole-line stores, shared input loads (same bits)
            for cfg in cands:
                if pc.cout <= 32 and cfg != 4:
                    continue
                if cfg == 13 and pc.kind != "conv":
                    continue
                t = self._time(lambda: ops.conv2d(x, pc, scale, shift, relu, residual, out, cfg, workspace=self.sk_ws,
                                                  workgroups=self._wgs_cfg(cfg)), reps)
                if t < best[1]:
                    best = (cfg, t)
            self.tile_cfg[name] = best[0]
            self.tune_report[name] = best
        self._autotune_active_tiles(reps)
        self.enqueue()  # leave every buffer consistent with the chosen configuration
        torch.cuda.synchronize()
        return self.tune_report

    def _autotune_active_tiles(self, reps):
        """The SSFA layers in front of conv_0 / conv_1 in active-tile mode (csrc/dense_active.hip) where that is faster on the staged
        frame: per layer the kernel (Winograd stream-K shape / LDS-tiled stream-K / direct tile_cfg) and the minimum share length
        against its full-map launch; then each layer whose output needs the constant over the whole map against its own share of
        the fill launch; then the whole set against the cost of the activity + fill launches."""
        self.active_cfg = {}
        if self.ta is None or not self.allow_streamk or not self.allow_winograd:
            return
        L4 = self.levels[-1]
        self.ta.run(L4["indices"], L4["n"], L4["cap"])
        pick, gain, dense = {}, 0.0, {}
        full_map = {"pair": self._full_map_pair, "branches": self._full_map_branches}
        for l, row in self.lists.items():
            if row.kind == "branches" and not self.allow_active_conv:
                continue
            # what enqueue() runs otherwise: the merged launch of two layers (timed here), or each layer's own (timed by autotune())
            full = full_map[row.kind]() if row.kind in full_map else None
            dense[l] = self._time(full, reps) if full is not None else sum(self.tune_report.get(n, (None, 0.0))[1] for n in row.name.split("+"))
            best = (None, 1e30)
            for cfg in self._list_candidates(l):
                need = self._list_ws_bytes(l, cfg)
                if need:
                    self._need_sk_ws(need)
                tt = self._time(self._list_call(l, cfg), reps)
                if tt < best[1]:
                    best = (cfg, tt)
            if best[0] is not None and best[1] < dense[l]:
                pick[l] = best
                gain += dense[l] - best[1]
        def overhead(ids):
            fj = self._fill_jobs(ids)
            return self._time(lambda: (self.ta.run(L4["indices"], L4["n"], L4["cap"]), self.ta.fill(fj[0], fj[1], layers=fj[2], tiles=fj[3], near=fj[4], near_kind=fj[5])),
                              4 * reps)   # (differences of a few microseconds are decided on these)
        sl = sorted(pick)
        over = overhead(sl) if pick else 0.0
        # the layers whose outputs are read by full-map launches need the constant EVERYWHERE outside their lists (trans_0 / trans_1:
        # 0.4 - 0.7 of an 18 / 9 MB map, the transposed pair: two 18 MB maps): each must pay for its own share of the fill launch
        for l in (self._kind_id["branches"], self._kind_id["pair"], 7, 6):
            if l in pick and len(pick) > 1:
                rest = [q for q in sl if q != l]
                over_wo = overhead(rest)
                g = dense[l] - pick[l][1]
                if over - over_wo >= g:
                    del pick[l]
                    sl, over, gain = rest, over_wo, gain - g
        if pick and gain > over:
            self.active_cfg = {l: pick[l][0] for l in pick}
        # (choice, gain ms per frame over the dense launches, ms of the activity + fill launches, per-layer ms): a tuple like the others
        self.tune_report["active_tiles"] = ({self.lists[l].name: v for l, v in self.active_cfg.items()}, gain - over, over,
                                            {self.lists[l].name: pick[l][1] for l in pick})

    def set_list_shares(self, mode):
        """After autotune(): 'whole' = every Winograd list layer on whole-unit shares (min_rounds -1), 'cut' = on stream-K shares
        (the best positive candidate is not re-timed: 4 rounds), anything else leaves the autotune's choice. For A/B runs of
        the two-frames-in-flight rate, which autotune()'s per-launch timing cannot see."""
        for l, (shape, mr) in list(self.active_cfg.items()):
            if self.lists[l].kind != "wino":   # (the conv_0 / conv_1 lists are long: their share rule is the autotune's)
                continue
            if mode == "whole":
                self.active_cfg[l] = (shape, -1)
            elif mode == "cut" and mr < 0:
                self.active_cfg[l] = (shape, 4)

    def active_tile_fractions(self):
        """name -> share of the 2x2-output tiles the layer computed in the LAST enqueued batch (layers in active-tile mode only)"""
        act = self._active_layers()
        if not act:
            return {}
        n = self.ta.n_list.cpu().numpy()
        rows = [self.lists[l] for l in act]
        return {r.name: float(n[r.mask]) / (self.B * (self.ta.dims[r.mask][0] // 2) * (self.ta.dims[r.mask][1] // 2)) for r in rows}

    # ------------------------------------------------------------------ the frame
    def enqueue(self, part=None):
        """Enqueue one batch on the current stream. No host synchronisation, no allocation. part = "front": voxelizer, site chain,
        sparse convs, tile lists and fill only; "back": the dense convs, the SSFA tail + heads and predict of a frame whose front has
        run (capture(split=True) keeps them as two graphs: EXPERIMENT bench.py --dense-token); None: the whole frame."""
        s = torch.cuda.current_stream().cuda_stream
        B = self.B
        for l in self._active_layers():   # a configuration set by hand: refused before anything is launched
            err = self._list_cfg_error(l, self.active_cfg[l])
            if err is not None:
                raise ValueError(err)
        if part == "back":
            return self._enqueue_body(s, "back")
        if self.cu_budget and (self.fork_front or self.fork_active):
            # the side branches run on a plain stream of the engine's own: on the whole chip, outside the CU set the engine's stream is
            # confined to (and its launches are sized for). Both options were measured slower anyway (see __init__).
            raise RuntimeError("fork_front / fork_active put part of the frame on an unmasked side stream: not available to an engine "
                               "that runs on a CU set (cu_budget = %d)" % self.cu_budget)
        # ---- voxelize (a1-a3)
        # every clear of the frame in ONE launch: control words + occupancy maps (0), hash tables and per-cell lists (empty marker),
        # the dense BEV map the last sparse layer scatters into (0; round 2 cleared it between two sparse convs, on the critical path)
        ops.fill_multi([(self.zero_arena, 0), (self.arena, 0x7F7F7F7F), (self.bev, 0)])
        lib.sessd_set_external_clear(1)  # the arena fill above replaces the per-call scratch clears
        try:
            return self._enqueue_body(s, part)
        finally:
            lib.sessd_set_external_clear(0)

    def _enqueue_body(self, s, part=None):
        B = self.B
        forked_active = False
        if part != "back":   # ---- the FRONT of a frame: voxelizer, site chain, the 14 sparse convs (+ the tile lists and the fill below)
            if self.batched_voxelizer:
                check(lib.sessd_voxelize_frames(self.points.data_ptr(), B, self.P_cap, 4, self.vrange.data_ptr(), self.vsize.data_ptr(),
                                                self.grid.data_ptr(), self.max_points, self.max_voxels, self.hash0.keys.data_ptr(),
                                                self.hash0.vals.data_ptr(), self.hash0.capacity, self.voxels.data_ptr(),
                                                self.coors.data_ptr(), 4, self.nump.data_ptr(), self.vfeat.data_ptr(),
                                                self.prefix.data_ptr(), self.vox_ws.data_ptr(), self.vox_ws.numel(), s), "voxelize_frames")
            else:
                for b in range(B):
                    check(lib.sessd_voxelize_frame(self.points[b].data_ptr(), self.P_cap, 4, self.vrange.data_ptr(),
                                                   self.vsize.data_ptr(), self.grid.data_ptr(), self.max_points, self.max_voxels,
                                                   b, self.hash0.keys.data_ptr(), self.hash0.vals.data_ptr(), self.hash0.capacity,
                                                   self.voxels.data_ptr(), self.coors.data_ptr(), 4, self.nump.data_ptr(),
                                                   self.vfeat.data_ptr(), self.prefix.data_ptr(), self.vox_ws.data_ptr(),
                                                   self.vox_ws.numel(), s), "voxelize_frame")
            feat = self.vfeat
            if self.sort_sites:
                check(lib.sessd_sparse_renumber_sites(self.coors.data_ptr(), self._n(0), self.levels[0]["cap"], B,
                                                      self._hash0_dims.data_ptr(), self.vfeat.data_ptr(), 4,
                                                      self.hash0.keys.data_ptr(), self.hash0.vals.data_ptr(), self.hash0.capacity,
                                                      self.coors_s.data_ptr(), self.vfeat_s.data_ptr(), self.renum_ws.data_ptr(),
                                                      self.renum_ws.numel(), s), "sparse_renumber_sites")
                feat = self.vfeat_s
            self._mark("voxelize")
            # ---- SpMiddleFHD (a4-a8): every level's sites and every rulebook first (4 launches), then the 14 convolutions
            L0 = self.levels[0]
            n_layers = len(self.sp.layers)
            # layers that only need level-0 tables (the leading submanifold convs) and the jobs they use
            lead = 0
            while lead < n_layers and self.sp.layers[lead]["kind"] == "subm":
                lead += 1
            lead_jobs = 1 + max([self._job_of[i] for i in range(lead)] + [-1])
            fork = self.fork_front and lead > 0 and self._tuning_sparse is None and self._marks is None
            forked_active = False

            def run_layers(lo, hi, feat, li, st):
                for idx in range(lo, hi):
                    lay = self.sp.layers[idx]
                    last = idx == n_layers - 1
                    j = self._job_of[idx]
                    nbr, tm = self.chain.nbr[j], self.chain.tile_mask[j]
                    if lay["kind"] == "subm":
                        L = self.levels[li]
                        out = L["feat_a"] if feat is not L["feat_a"] else L["feat_b"]
                        self._sconv(lay, feat, nbr, tm, li, out, st, idx=idx)
                        feat = out
                    else:
                        Lo = self.levels[li + 1]
                        if last:
                            self._sconv(lay, feat, nbr, tm, li + 1, None, st, dense=True, idx=idx)
                        else:
                            self._sconv(lay, feat, nbr, tm, li + 1, Lo["feat_a"], st, idx=idx)
                            feat = Lo["feat_a"]
                        li += 1
                return feat, li

            if fork:
                main = torch.cuda.current_stream()
                side = self.side_stream
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    s2 = side.cuda_stream
                    self.chain.run_rulebooks(L0["indices"], self._n(0), L0["cap"], L0["hash"], 0, lead_jobs, stream=s2)
                    feat, li = run_layers(0, lead, feat, 0, s2)
                self.chain.run_sites(L0["indices"], self._n(0), L0["cap"], self.err, clear=False, stream=s)
                self.chain.run_rulebooks(L0["indices"], self._n(0), L0["cap"], L0["hash"], lead_jobs, len(self.chain.jobs), stream=s)
                main.wait_stream(side)
                feat, li = run_layers(lead, n_layers, feat, li, s)
            else:
                self.chain.run(L0["indices"], self._n(0), L0["cap"], L0["hash"], self.err, clear=False, stream=s)
                # EXPERIMENT (off, measured slower): the tile lists and the fill depend on the last level's SITES only -- as a side branch
                # beside the 14 sparse convs (which leave most of the chip idle) instead of in front of the dense stage
                forked_active = self.fork_active and self._marks is None and self._kmarks is None and bool(self._active_layers())
                if forked_active:
                    main, side = torch.cuda.current_stream(), self.side_stream
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        L4 = self.levels[-1]
                        self.ta.run(L4["indices"], L4["n"], L4["cap"])
                        fj = self._fill_jobs(self._active_layers())
                        self.ta.fill(fj[0], fj[1], layers=fj[2], tiles=fj[3], near=fj[4], near_kind=fj[5])
                feat, li = run_layers(0, n_layers, feat, 0, s)
                if forked_active:
                    main.wait_stream(side)
        if part != "back":
            self._mark("spmiddle")
        # ---- SSFA (a9) rpn_v1.py:220-235
        t, h, d = self.t, self.h, self.dn
        act = self._active_layers()
        if act and not forked_active and part != "back":
            def lists_and_fill():
                L4 = self.levels[-1]
                self.ta.run(L4["indices"], L4["n"], L4["cap"])
                fj = self._fill_jobs(act)
                self.ta.fill(fj[0], fj[1], layers=fj[2], tiles=fj[3], near=fj[4], near_kind=fj[5])
            self._bracket("tile_activity+fill", lists_and_fill)
        if part == "front":
            return self.out
        if self.form == "rpn":
            return self._enqueue_predict(s, self._enqueue_rpn_neck())
        x = self._conv(self.bev, d.b0[0], t["a"], name="b0.0")
        x = self._conv(x, d.b0[1], t["b"], name="b0.1")
        x0 = self._conv(x, d.b0[2], t["x0"], name="b0.2")
        y = self._conv(x0, d.b1[0], h["a"], name="b1.0")
        y = self._conv(y, d.b1[1], h["b"], name="b1.1")
        x1 = self._conv(y, d.b1[2], h["x1"], name="b1.2")
        tr0 = self._conv(x0, d.trans_0, t["tr0"], name="trans_0")
        tr1 = self._conv(x1, d.trans_1, h["tr1"], name="trans_1")
        # the two transposed convs, then conv_0 / conv_1: over their tile list, else as one merged full-map launch, else one by one
        def two_layers(kind, full_map):
            l = self._kind_id[kind]
            call = self._list_call(l, self.active_cfg[l]) if l in act else full_map()
            if call is not None:
                self._bracket(self.lists[l].name, call)
            return call is not None
        mid0, mid1, o0, o1 = t["mid0"], t["mid1"], t["o0"], t["o1"]
        if not two_layers("pair", self._full_map_pair):
            self._conv(tr1, d.deconv_0, mid0, residual=tr0, name="deconv_0")
            self._conv(tr1, d.deconv_1, mid1, name="deconv_1")
        if not two_layers("branches", self._full_map_branches):
            self._conv(mid0, d.conv_0, o0, name="conv_0")
            self._conv(mid1, d.conv_1, o1, name="conv_1")
        # ---- SSFA tail + heads (a10): one launch; the two-launch form stays for channel counts the fused kernel does not take
        fused_keys = self.fuse_head and d.head_w.shape[1] in (64, 128) and self._tuning is None
        if fused_keys:
            self._bracket("ssfa_tail+head", lambda: ops.ssfa_fuse_head(
                o0, o1, d.w0, d.w1, *d.wbn, d.head_w, d.head_b, head_out=self.head, out=t["out"] if self.keep_ssfa else None,
                score_thresh=self.score_thresh, keys=self.keys if self.fuse_predict else None,
                key_count=self.key_count if self.fuse_predict else None, num_tasks=self.num_tasks))
        else:
            ops.ssfa_fuse(o0, o1, d.w0, d.w1, *d.wbn, out=t["out"])
            self._conv(t["out"], d.head, self.head.view(self.B, self.num_tasks * 22, self.H, self.W), relu=False, name="head")
        self._mark("ssfa_head")
        return self._enqueue_predict(s, fused_keys)

    def _enqueue_rpn_neck(self):
        """The RPN neck (rpn_v1.py:107-116) + heads: the block's 3x3 layers, then the up-sampler + the heads of every task (+ the
        score-filter keys) in one launch, or as two ops.conv2d launches. Returns whether the launch wrote the keys."""
        d, t = self.dn, self.t
        x = self.bev
        for i, layer in enumerate(d.layers):
            x = self._conv(x, layer, self._rpn_bufs[i + 1], name="blk0.%d" % i)
        fused_keys = self.fuse_head and self._tuning is None
        if fused_keys:
            self._bracket("rpn_tail+head", lambda: ops.rpn_up_head(
                x, d.up_w, d.up[1], d.up[2], d.head_w, d.head_b, head_out=self.head, out=t["out"] if self.keep_ssfa else None,
                score_thresh=self.score_thresh, keys=self.keys if self.fuse_predict else None,
                key_count=self.key_count if self.fuse_predict else None, num_tasks=self.num_tasks))
        else:
            self._conv(x, d.up, t["out"], name="up")
            self._conv(t["out"], d.head, self.head.view(self.B, self.num_tasks * 22, self.H, self.W), relu=False, name="head")
        self._mark("ssfa_head")
        return fused_keys

    def _enqueue_predict(self, s, fused_keys):
        use_keys = fused_keys and self.fuse_predict
        self.predict.launch(self.head, (self.keys, self.key_count) if use_keys else None, self._record_ring(), s)
        self._mark("predict")
        return self.out

    def _mark(self, name):
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((name, ev))

    def stage_times(self, reps=10):
        """Eager (no graph) per-stage GPU time in ms of the staged batch, HIP events on the current stream:
        dict(clear, voxelize, spmiddle, ssfa_head, predict). Informational; launch gaps of eager mode included."""
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

    def spmiddle_algorithmic_bytes(self):
        """per sparse layer (N_in*Cin + N_out*Cout)*4 + K*Cin*Cout*4 + (N_in + N_out)*16 bytes (features in
        and out once, weights once, indices once) with the live site counts of the last batch, plus the dense BEV
        write. Synchronises."""
        ns = [int(self.prefix[self.B].item())] + [int(L["n"].item()) for L in self.levels[1:]]
        total, li = 0, 0
        for lay in self.sp.layers:
            kv = lay["ks"][0] * lay["ks"][1] * lay["ks"][2]
            n_in = ns[li]
            if lay["kind"] != "subm":
                li += 1
            n_out = ns[li]
            total += (n_in * lay["cin"] + n_out * lay["cout"]) * 4 + kv * lay["cin"] * lay["cout"] * 4 + (n_in + n_out) * 16
        total -= ns[-1] * self.sp.layers[-1]["cout"] * 4  # the last layer writes the dense map instead of a feature table
        total += self.bev.numel() * 4
        return total, ns

    def dense_layer_times(self, reps=10):
        """In-frame duration (ms) of every dense conv launch: whole frames are enqueued eagerly with a HIP event before and after
        each launch on the launching stream (the launches are 10-80 us long and the host runs ahead of the device, so the events
        bracket the kernel, in the cache / clock state the frame really gives it). dict name -> mean ms."""
        acc = {}
        for _ in range(2):
            self.enqueue()
        for _ in range(reps):
            self._kmarks = []
            self.enqueue()
            marks, self._kmarks = self._kmarks, None
            torch.cuda.synchronize()
            for name, e0, e1 in marks:
                acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1) / reps
        return acc

    def spmiddle_mfma_report(self, reps=10):
        """Per sparse conv layer of the staged batch: HIP-event time of the launch alone, rulebook pairs (useful work) and active
        (16-site tile, offset) steps (executed work: every step multiplies 16 rows whatever the number of pairs in it).
        Returns dict(layers=[...], conv_ms, useful_gflop, executed_gflop, executed_tflops, executed_frac_of_f32_mfma_peak)."""
        self._tuning_sparse = []
        self.enqueue()
        torch.cuda.synchronize()
        todo, self._tuning_sparse = self._tuning_sparse, None
        ns = [int(self.prefix[self.B].item())] + [int(L["n"].item()) for L in self.levels[1:]]
        st = torch.cuda.current_stream().cuda_stream
        rows, tot_ms, tot_use, tot_exe = [], 0.0, 0.0, 0.0
        # the dense-output layer is not in the tuning list: time it with its own arguments
        last_idx = len(self.sp.layers) - 1
        jl = self._job_of[last_idx]
        todo = list(todo) + [(last_idx, self.sp.layers[last_idx], None, self.chain.nbr[jl], self.chain.tile_mask[jl], len(self.levels) - 1, None)]
        feat_last = None
        for idx, lay, in_feat, nbr, tm, out_li, out_feat in todo:
            n = ns[out_li]
            kv = lay["ks"][0] * lay["ks"][1] * lay["ks"][2]
            pairs = int((nbr[:kv, :n] >= 0).sum().item())
            srt = bool(self.chain.sort_tiles and self.sparse_sorted.get(idx, True))
            # the tiles the launch really walks: offset-pattern tiles (all masks beyond the live groups are zero) or 16 consecutive rows
            masks = self.chain.tile_mask_sorted[self._job_of[idx]] if srt else tm[:(n + 15) // 16]
            steps = int(sum(int(((masks >> k) & 1).sum().item()) for k in range(kv)))
            if in_feat is None:  # last layer: input = output of the previous one
                in_feat, dense = feat_last, True
            else:
                dense = False
            ms = self._time(lambda: self._sconv(lay, in_feat, nbr, tm, out_li, out_feat, st, dense=dense, idx=idx), reps)
            use, exe = 2.0 * pairs * lay["cin"] * lay["cout"] / 1e9, 2.0 * steps * 16 * lay["cin"] * lay["cout"] / 1e9
            rows.append(dict(layer=idx, kind=lay["kind"], cin=lay["cin"], cout=lay["cout"], sites=n, pairs=pairs, tile_steps=steps,
                             sorted_tiles=srt,
                             ms=round(ms, 5), useful_gflop=round(use, 4), executed_gflop=round(exe, 4),
                             executed_tflops=round(exe / ms, 2) if ms > 0 else 0.0))
            tot_ms, tot_use, tot_exe = tot_ms + ms, tot_use + use, tot_exe + exe
            feat_last = out_feat if out_feat is not None else feat_last
        self.enqueue()  # leave the buffers consistent
        torch.cuda.synchronize()
        return dict(layers=rows, conv_ms=round(tot_ms, 5), useful_gflop=round(tot_use, 3), executed_gflop=round(tot_exe, 3),
                    executed_tflops=round(tot_exe / tot_ms, 2), executed_frac_of_f32_mfma_peak=round(tot_exe / tot_ms / 157.3, 4),
                    useful_row_fraction=round(tot_use / tot_exe, 4))

    # ------------------------------------------------------------------ hipGraph
    def capture(self, warmup=2, split=False):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.enqueue()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        ops.new_capture_epoch()
        if split:
            # EXPERIMENT (bench.py --dense-token): the frame as TWO graphs, so that the caller can order the dense stages of the engines
            # that share a CU set (replay_front(); wait for the set's token; replay_back())
            gf = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf):
                self.enqueue("front")
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, pool=gf.pool()):
                self.enqueue("back")
            self.graph, self.graph_front, self.graph_back = None, gf, gb
            return gf, gb
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.enqueue()
        self.graph = g
        return g

    def replay(self):
        if self.graph is None and getattr(self, "graph_front", None) is not None:
            self.graph_front.replay()
            self.graph_back.replay()
            return self.out
        self.graph.replay()
        return self.out
