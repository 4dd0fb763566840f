"""Generates tests/golden/rpn_ref.npz by running the REFERENCE's RPN neck from source on the CPU (build container only; nothing
of the reference is copied into the repository, only input / output vectors are stored):

  rpn_*   det3d/models/necks/rpn_v1.py   RPN.__init__ + forward  :23-116   (eval mode)

with the constructor arguments of examples/second/configs/kitti_all_vfev3_spmiddlefhd_rpn1_mghead_syncbn.py:74-84 (one block of
1 + 5 3x3 layers, one stride-1 up-sampler, 128 filters). The loader and the stubs are those tests/golden/make_golden_forward.py
uses for SSFA from the same file (make_golden_head_loss.install / mod / load_as; matplotlib, torchvision, syncbn, registries and
checkpoint helpers are inert stand-ins). Weights are forward_cases.seeded_state_dict(shapes, seed), the input is
forward_cases.ssfa_input(seed, B=2, H=16, W=12); check sums of both are stored.

    python tests/golden/make_golden_rpn.py
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_forward as MF  # noqa: E402  (puts the repository on sys.path; REF, forward_cases)
import forward_cases as FC  # noqa: E402

WEIGHT_SEED, INPUT_SEED = 31, 8


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
    mod("refpkg.models.registry", NECKS=_Reg(), HEADS=_Reg(), LOSSES=_Reg(), READERS=_Reg())
    mod("refpkg.models.necks")
    rpn = load_as("det3d/models/necks/rpn_v1.py", "refpkg.models.necks.rpn_v1")
    neck = rpn.RPN(layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1], us_num_filters=[128],
                   num_input_features=128, norm_cfg=None, logger=_Logger())
    shapes = {k: tuple(v.shape) for k, v in neck.state_dict().items()}
    sd = FC.seeded_state_dict(shapes, seed=WEIGHT_SEED)
    neck.load_state_dict(sd)
    x = FC.ssfa_input(INPUT_SEED, B=2, H=16, W=12)
    neck.eval()
    out = {}
    with torch.no_grad():
        out["rpn_eval"] = neck(x).numpy()
    out["rpn_keys"] = np.array(sorted(shapes))
    out["rpn_shapes"] = np.array([str(shapes[k]) for k in sorted(shapes)])
    out["rpn_weight_check"] = np.array([float(sd[k].double().sum()) for k in sorted(shapes)])
    out["rpn_input_check"] = np.array([float(x.double().sum()), float(x.abs().max())])
    out["rpn_seeds"] = np.array([WEIGHT_SEED, INPUT_SEED])
    print("RPN from source:", out["rpn_eval"].shape, "params", sum(int(np.prod(s)) for s in shapes.values()),
          "max |out| %.4f" % float(np.abs(out["rpn_eval"]).max()))
    path = os.path.join(HERE, "rpn_ref.npz")
    np.savez_compressed(path, **out)
    print("rpn golden written:", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
