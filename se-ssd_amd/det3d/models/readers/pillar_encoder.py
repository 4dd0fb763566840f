"""mirrors det3d/models/readers/pillar_encoder.py: PFNLayer (:17-57), PillarFeatureNet (:60-153) and PointPillarsScatter
(:156-208). Same constructor arguments, defaults and state_dict keys (`pfn_layers.0.linear.weight`, `pfn_layers.0.norm.*`).

Device path: ONE PFN layer in eval mode on a device tensor runs ops.pillar_features (sessd_pillar_features), the scatter runs
ops.pillar_scatter. In train mode the same layer runs ops.pillar_features_train (batch statistics from float64 totals over the
live points, the eval kernel with them, a backward by recomputation: `fused_train`), and a scatter whose features carry a gradient
runs ops.pillar_scatter_train. More than one layer, a point tensor that carries a gradient or a CPU tensor run the torch
formulation below (`_forward_torch`), written for this project: the padding slots are masked before anything is computed from
them, the per-pillar constants are broadcast, BatchNorm is one functional call over the flattened slots, the scatter is one
indexed store. tests/test_pillars_mirror_cpu.py holds it to the reference's classes run from source.

Two things of this fork that both paths keep:
  * the reader's `voxel_size` / `pc_range` defaults (0.2 m pillars from x = 0, y = -40) are what the reference computes the centre
    columns with -- the PointPillars config passes neither, although its voxel generator makes 0.16 m pillars;
  * the centre columns are -(coor * v + offset), per-pillar constants: the line that would have made them an offset from the
    point is commented out (:126-133)."""
import torch
from torch import nn
from torch.nn import functional as F

from sessd_hip import ops
from sessd_hip.engine import fold_bn

from ..registry import BACKBONES, READERS
from ..utils import build_norm_layer


class PFNLayer(nn.Module):
    """Linear(no bias) -> BatchNorm1d over the channel -> ReLU -> max over the slots of a pillar. The last layer returns the
    (N, 1, units) maximum; an earlier one appends it to every slot's own features, (N, T, 2 * units)."""

    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__()
        self.name = "PFNLayer"
        self.last_vfe = last_layer
        self.units = out_channels if last_layer else out_channels // 2
        self.norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01) if norm_cfg is None else norm_cfg
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = build_norm_layer(self.norm_cfg, self.units)[1]

    def forward(self, inputs):
        n, t, _ = inputs.shape
        y = self.linear(inputs.reshape(n * t, -1))           # every slot is a row: BatchNorm1d normalises per channel over rows
        y = F.relu(self.norm(y)).reshape(n, t, self.units)
        top = y.amax(dim=1, keepdim=True)
        return top if self.last_vfe else torch.cat([y, top.expand(n, t, self.units)], dim=2)


@READERS.register_module
class PillarFeatureNet(nn.Module):
    fused_train = True   # train mode on the device: ops.pillar_features_train (False: the torch formulation), cf. RPN.fused_bn_train

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None):
        super().__init__()
        self.name = "PillarFeatureNet"
        assert len(num_filters) > 0
        self._with_distance = with_distance
        widths = [num_input_features + (6 if with_distance else 5)] + list(num_filters)   # + centred xyz, centre xy (, |xyz|)
        self.pfn_layers = nn.ModuleList(PFNLayer(cin, cout, norm_cfg=norm_cfg, last_layer=i == len(widths) - 2)
                                        for i, (cin, cout) in enumerate(zip(widths[:-1], widths[1:])))
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset = self.vx / 2 + pc_range[0]
        self.y_offset = self.vy / 2 + pc_range[1]

    def on_device_path(self, features):
        """One PFN layer of the kernel's width, eval mode, a 4-value point on the device, no gradient wanted: what
        sessd_pillar_features covers."""
        pfn = self.pfn_layers[0]
        return (len(self.pfn_layers) == 1 and not self.training and features.is_cuda and not features.requires_grad
                and features.shape[-1] == 4 and pfn.units == ops.PILLAR_CHANNELS and isinstance(pfn.norm, nn.BatchNorm1d))

    def on_device_train_path(self, features):
        """The same layer in train mode: what ops.pillar_features_train covers (a plain BatchNorm1d whose batch holds at least two
        slots; the points carry no gradient)."""
        pfn = self.pfn_layers[0]
        return (self.fused_train and len(self.pfn_layers) == 1 and self.training and features.is_cuda
                and not features.requires_grad and features.dim() == 3 and features.shape[-1] == 4
                and pfn.units == ops.PILLAR_CHANNELS and type(pfn.norm) is nn.BatchNorm1d
                and features.shape[0] * features.shape[1] >= 2)

    def forward(self, features, num_voxels, coors, num_voxels_dev=None):
        """features (N, T, 4), num_voxels (N,) points per pillar, coors (N, 4) [b, z, y, x] -> (N, C). The reference's trailing
        `.squeeze()` collapses N = 1 to (C,); this returns (N, C) always. num_voxels_dev (device int32[1]): capacity form -- only
        the rows below it are pillars; the rest enter neither the features (zero rows) nor the batch statistics nor a gradient.
        The kernels read the count on the device; the torch formulation cannot, so capacity form needs the device path."""
        pfn = self.pfn_layers[0]
        if self.on_device_train_path(features):
            return ops.pillar_features_train(features.float().contiguous(), num_voxels.int().contiguous(), coors.int().contiguous(),
                                             pfn.linear.weight, pfn.norm, self.vx, self.vy, self.x_offset, self.y_offset,
                                             with_distance=self._with_distance, num_voxels_dev=num_voxels_dev)
        if not self.on_device_path(features):
            if num_voxels_dev is not None:
                raise ValueError("PillarFeatureNet: capacity form (num_voxels_dev) needs the device path -- one PFN layer of %d "
                                 "channels on a device tensor; the torch formulation would count the padded rows" % ops.PILLAR_CHANNELS)
            return self._forward_torch(features, num_voxels, coors)
        scale, shift = fold_bn(pfn.norm)
        # (with a count, pillar_features leaves the rows beyond it unwritten: they are the scatter's to skip)
        return ops.pillar_features(features.float().contiguous(), num_voxels.int().contiguous(), coors.int().contiguous(),
                                   pfn.linear.weight.detach().float().contiguous(), scale, shift, self.vx, self.vy,
                                   self.x_offset, self.y_offset, with_distance=self._with_distance, num_voxels_dev=num_voxels_dev)

    def _forward_torch(self, features, num_voxels, coors):
        """The same in torch ops, any device, any number of PFN layers, train or eval mode."""
        n, t, _ = features.shape
        live = (torch.arange(t, device=features.device)[None, :] < num_voxels.reshape(-1, 1)).unsqueeze(-1)   # (N, T, 1)
        pts = features * live                      # the padding slots hold zeros already: stated, not assumed
        xyz = pts[..., :3]
        mean = xyz.sum(dim=1, keepdim=True) / num_voxels.reshape(-1, 1, 1).to(pts.dtype)
        # per-pillar constants of this fork: minus the pillar's centre, whatever the point
        centre = torch.stack([coors[:, 3].to(pts.dtype) * self.vx + self.x_offset,
                              coors[:, 2].to(pts.dtype) * self.vy + self.y_offset], dim=-1)
        cols = [pts, xyz - mean, -centre[:, None, :].expand(n, t, 2)]
        if self._with_distance:
            cols.append(xyz.norm(dim=-1, keepdim=True))
        x = torch.cat(cols, dim=-1) * live         # every decoration column of a padding slot is zero, too
        for pfn in self.pfn_layers:
            x = pfn(x)
        return x.reshape(n, -1)


@BACKBONES.register_module
class PointPillarsScatter(nn.Module):
    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", **kwargs):
        super().__init__()
        self.name = "PointPillarsScatter"
        self.nchannels = num_input_features

    def forward(self, voxel_features, coords, batch_size, input_shape, num_voxels_dev=None):
        """voxel_features (N, C), coords (N, 4) [b, z, y, x], input_shape [nx, ny, ...] -> (batch_size, C, ny, nx).
        num_voxels_dev (device int32[1]): capacity form -- rows at or beyond it reach neither the canvas nor a gradient."""
        self.nx, self.ny = int(input_shape[0]), int(input_shape[1])
        kw = {} if num_voxels_dev is None else dict(num_voxels_dev=num_voxels_dev)
        if voxel_features.is_cuda and voxel_features.shape[1] == ops.PILLAR_CHANNELS and voxel_features.requires_grad:
            return ops.pillar_scatter_train(voxel_features.float().contiguous(), coords.int().contiguous(), int(batch_size), self.ny,
                                            self.nx, **kw)
        if (voxel_features.is_cuda and voxel_features.shape[1] == ops.PILLAR_CHANNELS and not voxel_features.requires_grad
                and (not self.training or num_voxels_dev is not None)):
            return ops.pillar_scatter(voxel_features.float().contiguous(), coords.int().contiguous(), int(batch_size), self.ny,
                                      self.nx, **kw)
        if num_voxels_dev is not None:
            raise ValueError("PointPillarsScatter: capacity form (num_voxels_dev) needs the device path (%d-channel device features)"
                             % ops.PILLAR_CHANNELS)
        return self._forward_torch(voxel_features, coords, int(batch_size))

    def _forward_torch(self, voxel_features, coords, batch_size):
        """One indexed store into a (B, ny * nx, C) canvas (differentiable w.r.t. the features), then channels first."""
        c = coords.long()
        canvas = voxel_features.new_zeros((batch_size, self.ny * self.nx, voxel_features.shape[1]))
        canvas[c[:, 0], c[:, 2] * self.nx + c[:, 3]] = voxel_features
        return canvas.permute(0, 2, 1).reshape(batch_size, voxel_features.shape[1], self.ny, self.nx).contiguous()
