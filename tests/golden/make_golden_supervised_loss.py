"""Generates tests/golden/supervised_loss_ref.npz by running the REFERENCE's plain supervised head loss from source on the CPU:
    det3d/models/bbox_heads/mg_head.py   MultiGroupHead.loss :559-652 with create_loss :155-193, prepare_loss_weights :514-557,
                                         get_direction_target :57-71, _get_pos_neg_loss :42-54, add_sin_difference :34-39
together with the reference's own losses.py (focal :364-418, smooth-L1 :146-203, softmax :489-531). This is the loss of the
reference's three-class SECOND config and of its PointPillars config (mg_head_sessd.py's needs a teacher).
What cannot run here is substituted, and only that: the stubs of make_golden_head_loss.install (registries, builders, logging /
checkpoint helpers, numba, `.cuda()`), an inert matplotlib.pyplot, and `MultiGroupHead.__init__` is bypassed (it builds conv layers);
the attributes loss() reads are set from the constructor arguments the configs pass.
Two cases from tests/supervised_loss_ref.make_case:  a: B = 2, T = 3, A = 600, task 1's sample 1 without a positive, 30 ignored
labels per sample;  b: B = 3, T = 1, A = 257. Stored: the inputs, every returned term per task, the gradients of sum(loss) with
respect to box / cls / dir. Nothing from the reference is copied into the repository; only input / output vectors are stored.
Run in the build container only:  python tests/golden/make_golden_supervised_loss.py"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = dict(a=dict(seed=11, B=2, T=3, A=600, empty=((1, 1),)), b=dict(seed=12, B=3, T=1, A=257))


def main():
    import make_golden_head_loss as HL
    import supervised_loss_ref as SR
    assert os.path.isdir(HL.REF)
    warnings.filterwarnings("ignore")
    from oracle import capi
    HL.mod("matplotlib"); HL.mod("matplotlib.pyplot")
    _, ll, _, _, build_loss = HL.install(capi)
    head = HL.load_as("det3d/models/bbox_heads/mg_head.py", "refpkg.models.bbox_heads.mg_head")
    cfg = SR.CFG
    out = {}
    for name, kw in CASES.items():
        c = SR.make_case(**kw)
        T, B, A = c["labels"].shape
        h = object.__new__(head.MultiGroupHead)
        torch.nn.Module.__init__(h)
        h.num_classes = [1] * T
        h.box_n_dim = 7
        h.encode_rad_error_by_sin = True
        h.encode_background_as_zeros = True
        h.bev_only = False
        h.use_direction_classifier = True
        h.direction_offset = cfg["direction_offset"]
        h.loss_norm = dict(type="NormByNumPositives", pos_cls_weight=cfg["pos_cls_weight"], neg_cls_weight=cfg["neg_cls_weight"])
        h.loss_cls = build_loss(dict(type="SigmoidFocalLoss", alpha=cfg["focal_alpha"], gamma=cfg["focal_gamma"],
                                     loss_weight=cfg["cls_loss_weight"]))
        h.loss_reg = build_loss(dict(type="WeightedSmoothL1Loss", sigma=cfg["smooth_l1_sigma"], code_weights=[1.0] * 7, codewise=True,
                                     loss_weight=cfg["loc_loss_weight"]))
        h.loss_aux = build_loss(dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier",
                                     loss_weight=cfg["dir_loss_weight"]))
        F = torch.from_numpy
        example = dict(voxels=None, num_points=None, coordinates=None, anchors=[F(c["anchors"][t]) for t in range(T)],
                       labels=[F(c["labels"][t]) for t in range(T)], reg_targets=[F(c["reg_targets"][t]) for t in range(T)])
        leaves = [{k: F(c[k][t]).clone().requires_grad_(True) for k in ("box", "cls", "dir")} for t in range(T)]
        preds = [dict(box_preds=l["box"], cls_preds=l["cls"], dir_cls_preds=l["dir"]) for l in leaves]
        ret = h.loss(example, preds)
        sum(ret["loss"]).backward()
        for k, v in c.items():
            out["%s_%s" % (name, k)] = v
        for k in SR.VALUE_KEYS:
            out["%s_ret_%s" % (name, k)] = np.array([float(v.detach()) for v in ret[k]], np.float64)
        out[name + "_ret_loc_loss_elem"] = np.array([[float(e) for e in v] for v in ret["loc_loss_elem"]], np.float64)
        for k in ("num_pos", "num_neg"):
            out["%s_ret_%s" % (name, k)] = np.array([int(v) for v in ret[k]], np.int64)
        for k in ("box", "cls", "dir"):
            out["%s_grad_%s" % (name, k)] = np.stack([l[k].grad.numpy() for l in leaves])
        print(name, {k: out["%s_ret_%s" % (name, k)].tolist() for k in ("loss", "num_pos", "num_neg")})
    np.savez_compressed(os.path.join(HERE, "supervised_loss_ref.npz"), **out)


if __name__ == "__main__":
    main()
