"""Generates tests/golden/pillars_ref.npz by running the REFERENCE's PointPillars front end and RPN neck from source on the CPU
(build container only; nothing of the reference is copied into the repository, only input / output vectors and check sums are
stored):

  pfn_*      det3d/models/readers/pillar_encoder.py   PillarFeatureNet.__init__ + forward  :60-153  (eval mode), with_distance
             False (pfn_plain) and True (pfn_dist), the reader's default voxel_size / pc_range as the PointPillars config leaves them
  scatter    det3d/models/readers/pillar_encoder.py   PointPillarsScatter.forward          :156-208 on pfn_plain, B = 2, nx = 12, ny = 8
  rpn3_*     det3d/models/necks/rpn_v1.py             RPN.__init__ + forward               :23-116  (eval mode) with the neck
             arguments of examples/point_pillars/configs/original_pp_mghead_syncbn_kitti.py:52-62 (three blocks, up-samplers of
             stride 1 / 2 / 4) on a (2, 64, 16, 24) canvas

The loader and the stubs are those of tests/golden/make_golden_rpn.py. Weights are forward_cases.seeded_state_dict(shapes, seed);
the pillars and the canvas come from tests/pillars_ref.py (pillar_input / rpn_input); the pillars are stored, check sums of the
weights and of the canvas are stored. The seeded BatchNorm1d must fold to shifts of both signs (a negative shift is what tells
relu(shift) from shift in the padding rule): checked here and stored.

    python tests/golden/make_golden_pillars.py
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_forward as MF  # noqa: E402  (puts the repository on sys.path; REF, forward_cases)
import forward_cases as FC  # noqa: E402
import pillars_ref as PR  # noqa: E402

PFN_SEEDS = dict(plain=41, dist=42)
PILLAR_SEED, RPN_WEIGHT_SEED, RPN_INPUT_SEED = 9, 43, 10
B, NY, NX, T = 2, 8, 12, 8
RPN_ARGS = dict(layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[1, 2, 4],
                us_num_filters=[128, 128, 128], num_input_features=64)


def main():
    assert os.path.isdir(MF.REF)
    warnings.filterwarnings("ignore")
    from oracle import capi
    import make_golden_head_loss as HL
    HL.install(capi)
    mod, load_as = HL.mod, HL.load_as

    class _Logger:
        def info(self, *a, **k):
            pass

    class _Reg:
        @staticmethod
        def register_module(obj):
            return obj

    for n in ("matplotlib", "matplotlib.pyplot", "torchvision", "torchvision.models", "det3d.ops.syncbn", "det3d.utils.dist"):
        mod(n)
    sys.modules["torchvision.models"].resnet = types.ModuleType("resnet")
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["det3d.ops.syncbn"].DistributedSyncBN = torch.nn.BatchNorm2d
    sys.modules["det3d.utils.dist"].dist_common = types.SimpleNamespace(get_world_size=lambda: 1)
    mod("det3d.torchie.cnn", constant_init=None, kaiming_init=None, xavier_init=None)
    mod("det3d.torchie.trainer", load_checkpoint=None)
    misc = load_as("det3d/models/utils/misc.py", "refpkg.models.utils.misc")
    norm = load_as("det3d/models/utils/norm.py", "refpkg.models.utils.norm")
    mod("refpkg.models.utils", build_norm_layer=norm.build_norm_layer)
    mod("det3d.models.utils", Empty=misc.Empty, GroupNorm=misc.GroupNorm, Sequential=misc.Sequential,
        change_default_args=misc.change_default_args, get_paddings_indicator=misc.get_paddings_indicator)
    mod("refpkg.models.registry", NECKS=_Reg(), HEADS=_Reg(), LOSSES=_Reg(), READERS=_Reg(), BACKBONES=_Reg())
    mod("refpkg.models").builder = mod("refpkg.models.builder")
    mod("refpkg.models.necks")
    mod("refpkg.models.readers")
    rpn = load_as("det3d/models/necks/rpn_v1.py", "refpkg.models.necks.rpn_v1")
    pe = load_as("det3d/models/readers/pillar_encoder.py", "refpkg.models.readers.pillar_encoder")

    out = {}
    vox, num, coors = PR.pillar_input(PILLAR_SEED, T=T, B=B, ny=NY, nx=NX)
    out["voxels"], out["num_points"], out["coors"] = vox, num, coors
    out["pillar_seed"] = np.array([PILLAR_SEED])
    for tag, dist in (("plain", False), ("dist", True)):
        net = pe.PillarFeatureNet(num_filters=[64], with_distance=dist, norm_cfg=None)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        sd = FC.seeded_state_dict(shapes, seed=PFN_SEEDS[tag])
        net.load_state_dict(sd)
        net.eval()
        with torch.no_grad():
            feat = net(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(coors))
        out["pfn_%s" % tag] = feat.numpy()
        out["pfn_%s_keys" % tag] = np.array(sorted(shapes))
        out["pfn_%s_shapes" % tag] = np.array([str(shapes[k]) for k in sorted(shapes)])
        out["pfn_%s_weight_check" % tag] = np.array([float(sd[k].double().sum()) for k in sorted(shapes)])
        out["pfn_%s_seed" % tag] = np.array([PFN_SEEDS[tag]])
        _, shift = PR.fold_bn(sd, "pfn_layers.0.norm", torch.float64)
        signs = np.array([int((shift < 0).sum()), int((shift > 0).sum())])
        assert signs.min() >= 8, signs   # folded shifts of both signs
        out["pfn_%s_shift_signs" % tag] = signs
        print("PillarFeatureNet(with_distance=%s) from source:" % dist, feat.shape, "max %.4f" % float(feat.max()),
              "shift signs (-, +)", signs.tolist())
        if not dist:
            sc = pe.PointPillarsScatter(num_input_features=64)
            with torch.no_grad():
                canvas = sc(feat, torch.from_numpy(coors), B, [NX, NY, 1])
            assert tuple(canvas.shape) == (B, 64, NY, NX)
            out["scatter"] = canvas.numpy()

    neck = rpn.RPN(norm_cfg=None, logger=_Logger(), **RPN_ARGS)
    shapes = {k: tuple(v.shape) for k, v in neck.state_dict().items()}
    sd = FC.seeded_state_dict(shapes, seed=RPN_WEIGHT_SEED)
    neck.load_state_dict(sd)
    x = PR.rpn_input(RPN_INPUT_SEED)
    neck.eval()
    with torch.no_grad():
        out["rpn3_eval"] = neck(x).numpy()
    out["rpn3_keys"] = np.array(sorted(shapes))
    out["rpn3_shapes"] = np.array([str(shapes[k]) for k in sorted(shapes)])
    out["rpn3_weight_check"] = np.array([float(sd[k].double().sum()) for k in sorted(shapes)])
    out["rpn3_input_check"] = np.array([float(x.double().sum()), float(x.abs().max())])
    out["rpn3_seeds"] = np.array([RPN_WEIGHT_SEED, RPN_INPUT_SEED])
    print("RPN (3 blocks) from source:", out["rpn3_eval"].shape, "params", sum(int(np.prod(s)) for s in shapes.values()),
          "max |out| %.4f" % float(np.abs(out["rpn3_eval"]).max()))
    path = os.path.join(HERE, "pillars_ref.npz")
    np.savez_compressed(path, **out)
    print("pillars golden written:", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
