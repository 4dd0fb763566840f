"""TEST INFRASTRUCTURE ONLY -- the PointPillars front end and the multi-block SECOND-style RPN neck in plain torch ops, in any float
dtype, on state dicts with the reference's key names; plus the seeded inputs that tests/golden/make_golden_pillars.py ran the
REFERENCE's own classes on (tests/golden/pillars_ref.npz). tests/test_pillars_mirror_cpu.py holds these functions (float32) to
that golden output; the GPU tests use them in float64 as the yardstick of the kernels.

  pillar_features  PillarFeatureNet.forward with ONE PFNLayer in eval mode (det3d/models/readers/pillar_encoder.py:114-153) on
                   an explicit weight (C, K) and folded BatchNorm1d (scale, shift): columns [x, y, z, r, x - mx, y - my, z - mz,
                   fcx, fcy (, |xyz|)], fcx = -(coor_x * vx + x_offset), fcy = -(coor_y * vy + y_offset) per pillar (the fork's
                   centre columns, :126-133), slots >= num_points zeroed in all K columns, max over ALL T slots. The padding
                   slots are masked BEFORE anything reads them (the reference multiplies by 0 and relies on a zero-filled
                   tensor; the GPU tests fill them with NaN).
  reader_forward   the same from a state dict (pfn_layers.0.linear.weight, pfn_layers.0.norm.*), with the reader's defaults
  scatter          PointPillarsScatter.forward (:173-208)
  rpn_forward      RPN.forward (det3d/models/necks/rpn_v1.py:107-116) for any number of blocks / up-samplers of integer stride"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3  # norm_cfg = dict(type="BN1d" / "BN", eps=1e-3, momentum=0.01)
VOXEL_SIZE = (0.2, 0.2, 4)               # PillarFeatureNet's defaults (pillar_encoder.py:67-68): the config does not pass them
PC_RANGE = (0, -40, -3, 70.4, 40, 1)


def pillar_input(seed, N=48, T=8, B=2, ny=8, nx=12):
    """N pillars in distinct cells of B (ny, nx) canvases, frames interleaved, corners (0, 0) and (ny - 1, nx - 1) taken;
    num_points mixed in {1, .., T} with 1, T - 1 and T present; padding slots zero (as a voxelizer leaves them)."""
    rng = np.random.RandomState(seed)
    cells = rng.permutation(B * ny * nx)[:N]
    cells[0], cells[1] = 0, B * ny * nx - 1
    cells = np.unique(cells)
    cells = cells[rng.permutation(len(cells))]
    N = len(cells)
    coors = np.stack([cells // (ny * nx), np.zeros(N, np.int64), (cells // nx) % ny, cells % nx], 1).astype(np.int32)
    num = rng.randint(1, T + 1, size=N).astype(np.int32)
    num[:3] = [1, max(T - 1, 1), T]
    vox = (rng.rand(N, T, 4) * np.array([70.4, 80.0, 4.0, 1.0]) + np.array([0.0, -40.0, -3.0, 0.0])).astype(np.float32)
    for i in range(N):
        vox[i, num[i]:] = 0
    return vox, num, coors


def rpn_input(seed, B=2, C=64, H=16, W=24):
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(B, C, H, W, generator=g)
    return torch.relu(x) * (torch.rand(B, 1, H, W, generator=g) > 0.4)  # a canvas: non-negative, empty cells


def fold_bn(sd, p, dtype):
    scale = sd[p + ".weight"].to(dtype) / torch.sqrt(sd[p + ".running_var"].to(dtype) + EPS)
    return scale, sd[p + ".bias"].to(dtype) - sd[p + ".running_mean"].to(dtype) * scale


def pillar_columns(voxels, num_points, coors, vx, vy, x_offset, y_offset, with_distance, dtype):
    """(N, T, K) decorated and masked columns, and the (N, T) mask of the live slots."""
    v = torch.as_tensor(voxels).to(dtype)
    n = torch.as_tensor(num_points).to(torch.int64)
    c = torch.as_tensor(coors)
    N, T, _ = v.shape
    live = torch.arange(T).view(1, -1) < n.view(-1, 1)
    v = torch.where(live.unsqueeze(-1), v, torch.zeros((), dtype=dtype))
    mean = v[:, :, :3].sum(dim=1, keepdim=True) / n.to(dtype).view(-1, 1, 1)
    cols = [v, v[:, :, :3] - mean,
            (-(c[:, 3].to(dtype) * vx + x_offset)).view(-1, 1, 1).expand(N, T, 1),
            (-(c[:, 2].to(dtype) * vy + y_offset)).view(-1, 1, 1).expand(N, T, 1)]
    if with_distance:
        cols.append(torch.norm(v[:, :, :3], 2, 2, keepdim=True))
    f = torch.cat(cols, dim=-1)
    return torch.where(live.unsqueeze(-1), f, torch.zeros((), dtype=dtype)), live


def pillar_features(voxels, num_points, coors, weight, scale, shift, vx, vy, x_offset, y_offset, with_distance=False,
                    dtype=torch.float32):
    f, _ = pillar_columns(voxels, num_points, coors, vx, vy, x_offset, y_offset, with_distance, dtype)
    y = F.linear(f, torch.as_tensor(weight).to(dtype)) * torch.as_tensor(scale).to(dtype) + torch.as_tensor(shift).to(dtype)
    return torch.relu(y).max(dim=1)[0]


def reader_forward(voxels, num_points, coors, sd, prefix="reader.", with_distance=False, voxel_size=VOXEL_SIZE, pc_range=PC_RANGE,
                   dtype=torch.float32):
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    assert not any(k.startswith("pfn_layers.1.") for k in sd), "one PFN layer"
    scale, shift = fold_bn(sd, "pfn_layers.0.norm", dtype)
    vx, vy = voxel_size[0], voxel_size[1]
    return pillar_features(voxels, num_points, coors, sd["pfn_layers.0.linear.weight"], scale, shift, vx, vy,
                           vx / 2 + pc_range[0], vy / 2 + pc_range[1], with_distance, dtype)


def scatter(feat, coors, batch, ny, nx):
    c = torch.as_tensor(coors).long()
    canvas = torch.zeros(batch, feat.shape[1], ny * nx, dtype=feat.dtype)
    for b in range(batch):
        m = c[:, 0] == b
        canvas[b][:, c[m, 2] * nx + c[m, 3]] = feat[m].t()
    return canvas.view(batch, feat.shape[1], ny, nx)


def _bn_relu(x, sd, p):
    return torch.relu(F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS))


def rpn_forward(x, sd, ds_strides, us_strides, prefix="neck."):
    """x (B, C, H, W) -> the concatenated up-sampled maps; sd: reference-keyed state dict of x's dtype. Block i:
    blocks.i.{1,2} = ZeroPad2d(1) + unpadded 3x3 of stride ds_strides[i] (== F.conv2d padding 1), blocks.i.{4,5}, ... 3x3 padding 1,
    each + BatchNorm (running statistics) + ReLU; deblocks.k.{0,1} = ConvTranspose2d(k = stride = us_strides[k]) + BN + ReLU."""
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    start = len(ds_strides) - len(us_strides)
    ups = []
    for i, s in enumerate(ds_strides):
        x = _bn_relu(F.conv2d(x, sd["blocks.%d.1.weight" % i], None, stride=s, padding=1), sd, "blocks.%d.2" % i)
        ci = 4
        while "blocks.%d.%d.weight" % (i, ci) in sd:
            x = _bn_relu(F.conv2d(x, sd["blocks.%d.%d.weight" % (i, ci)], None, stride=1, padding=1), sd, "blocks.%d.%d" % (i, ci + 1))
            ci += 3
        if i - start >= 0:
            k = i - start
            ups.append(_bn_relu(F.conv_transpose2d(x, sd["deblocks.%d.0.weight" % k], None, stride=us_strides[k]), sd,
                                "deblocks.%d.1" % k))
    return torch.cat(ups, dim=1)


RPN3_ARGS = dict(layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[1, 2, 4],
                 us_num_filters=[128, 128, 128], num_input_features=64, norm_cfg=None)


def load_golden(golden_dir):
    """tests/golden/pillars_ref.npz with its seeded weights and canvas regenerated (and checked against the stored sums)."""
    import ast
    import os
    import sys
    sys.path.insert(0, golden_dir)
    import forward_cases as FC
    g = np.load(os.path.join(golden_dir, "pillars_ref.npz"))
    out = dict(voxels=g["voxels"], num_points=g["num_points"], coors=g["coors"], scatter=torch.from_numpy(g["scatter"]))
    vox, num, coors = pillar_input(int(g["pillar_seed"][0]))
    assert np.array_equal(vox, out["voxels"]) and np.array_equal(num, out["num_points"]) and np.array_equal(coors, out["coors"])
    for tag in ("plain", "dist", "rpn3"):
        p = tag if tag == "rpn3" else "pfn_" + tag
        shapes = {k: ast.literal_eval(s) for k, s in zip(g[p + "_keys"].tolist(), g[p + "_shapes"].tolist())}
        seed = int(g["rpn3_seeds"][0]) if tag == "rpn3" else int(g[p + "_seed"][0])
        sd = FC.seeded_state_dict(shapes, seed=seed)
        # the generators have not drifted from what the reference ran on
        assert np.allclose([float(sd[k].double().sum()) for k in sorted(shapes)], g[p + "_weight_check"], rtol=1e-12, atol=1e-9)
        out[tag] = dict(shapes=shapes, sd=sd, out=torch.from_numpy(g["rpn3_eval"] if tag == "rpn3" else g[p]))
        if tag != "rpn3":
            out[tag]["shift_signs"] = g[p + "_shift_signs"]
    x = rpn_input(int(g["rpn3_seeds"][1]))
    assert np.allclose([float(x.double().sum()), float(x.abs().max())], g["rpn3_input_check"], rtol=1e-12)
    out["rpn3"]["x"] = x
    return out
