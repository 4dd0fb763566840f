"""TEST INFRASTRUCTURE ONLY -- the plain supervised multi-task head loss (sigmoid focal classification, smooth-L1 localisation on the
sin-encoded yaw, softmax direction loss on the positives, NormByNumPositives; one class per task) restated in plain torch float64
from the formulas, with autograd for the gradients, and the generator of the synthetic cases the golden file and the tests share.
It is the yardstick of the device op sessd_supervised_loss and is itself held to the reference run stored in
tests/golden/supervised_loss_ref.npz (tests/test_supervised_loss_cpu.py). Nothing of the product is imported here."""
import numpy as np
import torch

CFG = dict(pos_cls_weight=1.0, neg_cls_weight=1.0, focal_alpha=0.25, focal_gamma=2.0, smooth_l1_sigma=3.0, cls_loss_weight=1.0,
           loc_loss_weight=2.0, dir_loss_weight=0.2, direction_offset=0.0)
VALUE_KEYS = ("loss", "cls_loss_reduced", "loc_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss")
DIR_MARGIN = 1e-3   # |reg_target yaw + anchor yaw - offset| of every positive stays above it: the direction target is no rounding decision


def make_case(seed, B, T, A, n_pos=14, n_ignore=30, empty=(), direction_offset=0.0, anchors=None):
    """Synthetic head outputs / targets of T tasks, B samples, A anchors: n_pos positives per sample with small regression targets
    and predictions near them, n_ignore labels -1, logits around -3 (negatives) / 1.5 (positives). `empty`: (task, sample) pairs
    without a positive; `anchors`: (A, 7) anchors to use for every task and sample instead of random ones. Arrays are
    (T, B, A[, k]); labels int64."""
    rng = np.random.RandomState(seed)
    given = anchors
    n_pos, n_ignore = min(n_pos, A), min(n_ignore, max(A - n_pos, 0))
    anchors = np.zeros((T, B, A, 7), np.float32)
    anchors[..., 0] = rng.uniform(0, 70, (T, B, A)); anchors[..., 1] = rng.uniform(-40, 40, (T, B, A)); anchors[..., 2] = -1.0
    anchors[..., 3:6] = [1.6, 3.9, 1.56]
    anchors[..., 6] = rng.choice([0.0, 1.57], (T, B, A))
    if given is not None:
        anchors[:] = np.asarray(given, np.float32).reshape(1, 1, A, 7)
    labels = np.zeros((T, B, A), np.int64)
    for t in range(T):
        for b in range(B):
            order = rng.permutation(A)
            labels[t, b, order[n_pos:n_pos + n_ignore]] = -1
            if (t, b) not in empty:
                labels[t, b, order[:n_pos]] = 1
    pos = labels > 0
    n = int(pos.sum())
    reg_targets = np.zeros((T, B, A, 7), np.float32)
    reg_targets[pos] = rng.normal(0, 0.15, (n, 7)).astype(np.float32)
    yaw = reg_targets[..., 6] + anchors[..., 6] - np.float32(direction_offset)
    near = pos & (np.abs(yaw) < 4 * DIR_MARGIN)
    reg_targets[..., 6][near] += np.float32(0.05)
    box = rng.normal(0, 0.05, (T, B, A, 7)).astype(np.float32)
    box[pos] = reg_targets[pos] + rng.normal(0, 0.08, (n, 7)).astype(np.float32)
    cls = rng.normal(-3.0, 1.0, (T, B, A)).astype(np.float32)
    cls[pos] = rng.normal(1.5, 0.7, n).astype(np.float32)
    dirp = rng.normal(0, 1, (T, B, A, 2)).astype(np.float32)
    c = dict(anchors=anchors, labels=labels, reg_targets=reg_targets, box=box, cls=cls, dir=dirp)
    check_margin(c, direction_offset)
    return c


def check_margin(c, direction_offset=0.0):
    pos = c["labels"] > 0
    yaw = (c["reg_targets"][..., 6].astype(np.float64) + c["anchors"][..., 6].astype(np.float64) - direction_offset)[pos]
    assert yaw.size == 0 or np.abs(yaw).min() >= DIR_MARGIN


def reference(c, cfg=CFG, dtype=torch.float64):
    """The loss of every task and the gradients of their sum, in `dtype`. Returns dict: each of VALUE_KEYS -> (T,) numpy,
    loc_loss_elem (T, 7), num_pos / num_neg (T,) of sample 0, positives (T,) of the batch, total, grad_box / grad_cls / grad_dir
    (T, B, A[, k])."""
    T, B, A = c["labels"].shape
    F = lambda k: torch.tensor(np.asarray(c[k]), dtype=dtype)
    box, cls, dirp = (F(k).requires_grad_(True) for k in ("box", "cls", "dir"))
    tg, anc = F("reg_targets"), F("anchors")
    labels = torch.as_tensor(np.asarray(c["labels"]))
    pos, neg = (labels > 0), (labels == 0)
    posf, negf = pos.to(dtype), neg.to(dtype)
    norm = posf.sum(-1, keepdim=True).clamp(min=1.0)                      # positives of the sample, at least 1
    cls_w = (negf * cfg["neg_cls_weight"] + posf * cfg["pos_cls_weight"]) / norm
    reg_w = posf / norm
    # sigmoid focal loss, target 1 on the positives
    ce = cls.clamp(min=0) - cls * posf + torch.log1p(torch.exp(-cls.abs()))
    one_minus_pt = torch.where(pos, torch.sigmoid(-cls), torch.sigmoid(cls))
    mod = one_minus_pt ** cfg["focal_gamma"] if cfg["focal_gamma"] else torch.ones_like(cls)
    alpha_t = posf * cfg["focal_alpha"] + (1 - posf) * (1 - cfg["focal_alpha"])
    focal = mod * alpha_t * ce * cls_w                                    # (T, B, A)
    # smooth L1 with the transition at 1 / sigma^2 (<=), yaw as sin(p - t) = sin p cos t - cos p sin t
    s2 = cfg["smooth_l1_sigma"] ** 2
    d = torch.cat([box[..., :6] - tg[..., :6],
                   torch.sin(box[..., 6:]) * torch.cos(tg[..., 6:]) - torch.cos(box[..., 6:]) * torch.sin(tg[..., 6:])], -1)
    loc = torch.where(d.abs() <= 1.0 / s2, 0.5 * s2 * d * d, d.abs() - 0.5 / s2) * reg_w.unsqueeze(-1)   # (T, B, A, 7)
    # direction: softmax cross entropy against (target yaw + anchor yaw - offset) > 0, on the positives
    dir_t = ((tg[..., 6] + anc[..., 6]) - cfg["direction_offset"] > 0).long()
    dce = torch.logsumexp(dirp, -1) - dirp.gather(-1, dir_t.unsqueeze(-1)).squeeze(-1)
    dir_l = dce * reg_w
    S = lambda v: v.reshape(T, -1).sum(1) / B
    cls_red, loc_red, dir_red = cfg["cls_loss_weight"] * S(focal), cfg["loc_loss_weight"] * S(loc), S(dir_l)
    loss = loc_red + cls_red + cfg["dir_loss_weight"] * dir_red
    loss.sum().backward()
    N = lambda v: v.detach().double().numpy()
    return dict(loss=N(loss), cls_loss_reduced=N(cls_red), loc_loss_reduced=N(loc_red), dir_loss_reduced=N(dir_red),
                cls_pos_loss=N(S(focal * posf) / cfg["pos_cls_weight"]), cls_neg_loss=N(S(focal * negf) / cfg["neg_cls_weight"]),
                loc_loss_elem=N(loc.sum((1, 2)) / B), num_pos=pos[:, 0].sum(1).numpy(), num_neg=neg[:, 0].sum(1).numpy(),
                positives=pos.reshape(T, -1).sum(1).numpy(), total=float(loss.detach().sum()), grad_box=N(box.grad), grad_cls=N(cls.grad),
                grad_dir=N(dirp.grad))


def value_close(got, want, rel):
    """|got - want| <= rel * max(1e-3, |want|): the project's form of a relative bound with a floor."""
    got = got.detach() if torch.is_tensor(got) else got
    return abs(float(got) - float(want)) <= rel * max(1e-3, abs(float(want)))


def grad_close(got, want, rel, tiny=1e-30):
    """(ok, message). Largest error <= rel of the largest entry of `want`, and the same support: an entry that is exactly zero in
    `want` is exactly zero in `got`, and an entry of `want` that float32 can hold (|w| >= tiny; below that a float32 result may
    underflow to zero) is non-zero in `got`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    zero_kept = bool(np.all(got[want == 0] == 0))
    live_kept = bool(np.all(got[np.abs(want) >= tiny] != 0))
    return err <= rel * top and zero_kept and live_kept, "max err %.3e, bound %.3e, zeros kept %s, non-zeros kept %s" % (
        err, rel * top, zero_kept, live_kept)


def golden_case(g, name):
    """(case, want) of one case of tests/golden/supervised_loss_ref.npz: the inputs as make_case returns them and the reference
    run's terms (each indexed [task]) with the gradients grad_box / grad_cls / grad_dir (indexed [task])."""
    c = {k: g["%s_%s" % (name, k)] for k in ("anchors", "labels", "reg_targets", "box", "cls", "dir")}
    want = {k: g["%s_ret_%s" % (name, k)] for k in VALUE_KEYS + ("loc_loss_elem", "num_pos", "num_neg")}
    want.update({"grad_" + k: g["%s_grad_%s" % (name, k)] for k in ("box", "cls", "dir")})
    return c, want


def example_and_preds(c, device, labels_dtype=torch.int64):
    """(example, leaves, preds) of a case on `device`: example as the head's loss methods read it, leaves[t] = dict(box, cls, dir)
    of tensors that require a gradient, preds[t] the head-output dict over them."""
    T = c["labels"].shape[0]
    F = lambda k, t: torch.from_numpy(np.ascontiguousarray(c[k][t])).to(device)
    example = dict(anchors=[F("anchors", t) for t in range(T)], labels=[F("labels", t).to(labels_dtype) for t in range(T)],
                   reg_targets=[F("reg_targets", t) for t in range(T)])
    leaves = [{k: F(k, t).clone().requires_grad_(True) for k in ("box", "cls", "dir")} for t in range(T)]
    preds = [dict(box_preds=l["box"], cls_preds=l["cls"], dir_cls_preds=l["dir"]) for l in leaves]
    return example, leaves, preds


def hold(label, ret, grads, want, value_rel, grad_rel):
    """Every term of every task of `ret` (a dict indexed [key][task], loc_loss_elem [task][i]) within value_rel of `want`, the
    counts equal, and grads[k][task] within grad_rel of want['grad_' + k][task] with the same support. Prints every figure, then
    asserts them all."""
    T = len(want["loss"])
    bad = []
    for t in range(T):
        pairs = [(k, ret[k][t], want[k][t]) for k in VALUE_KEYS] + \
                [("loc_loss_elem[%d]" % i, ret["loc_loss_elem"][t][i], want["loc_loss_elem"][t][i]) for i in range(7)]
        for k, a, b in pairs:
            ok = value_close(a, b, value_rel)
            a = a.detach() if torch.is_tensor(a) else a
            print("%s task %d %-18s got %.8g want %.8g %s" % (label, t, k, float(a), float(b), "" if ok else "MISS"))
            if not ok:
                bad.append((t, k, float(a), float(b)))
        for k in ("num_pos", "num_neg"):
            if int(ret[k][t]) != int(want[k][t]):
                bad.append((t, k, int(ret[k][t]), int(want[k][t])))
        for k in ("box", "cls", "dir"):
            got = grads[k][t]
            got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
            ok, msg = grad_close(got.reshape(want["grad_" + k][t].shape), want["grad_" + k][t], grad_rel)
            print("%s task %d grad_%s %s %s" % (label, t, k, msg, "" if ok else "MISS"))
            if not ok:
                bad.append((t, "grad_" + k, msg))
    assert not bad, (label, bad)
