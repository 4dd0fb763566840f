"""Generates tests/golden/assign_multi_ref.npz by running the REFERENCE's target assignment from source on CPU, per task, as
det3d/core/anchor/target_assigner.py:68-136 (assign_v2) wires it: create_target_np (target_ops_v3.py:11-137) on the task's
anchors, the ground truth rows named like the task's class, class ids all 1, the task's thresholds, NearestIouSimilarity and
second_box_encode. Anchors: oracle.postprocess.create_anchors_3d_range, pinned to the reference's generator elsewhere (as in
make_golden_assign.py; the reference's own fails on a tuple from np.meshgrid under the numpy installed here).
Two configs (sizes, z, rotations and thresholds are those of sessd_hip.configs.ASSIGNER_3CLASS / ASSIGNER_POINTPILLARS, which
tests hold equal to the reference's config files), each on a crop of its map that keeps the config's anchor stride:
    c3  three-class SECOND config: feature map (1, 40, 44) of the (1, 200, 176) one, 0.4 m, A = 3520 per task
    pp  PointPillars config:       feature map (1, 37, 29) of the (1, 248, 216) one, ~0.32 m, A = 2146 (no multiple of 256)
Stored per config and frame: the ground truth and its class codes (index into `names`), and per task the labels as int8, the
positives' indices, the targets at the positives and positive_gt_id; everywhere else the targets are zero (asserted here).
Stubs and loader: make_golden.py, as make_golden_assign.py. Run in the build container only:
    python tests/golden/make_golden_assign_multi.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))
sys.path.insert(0, HERE)

NAMES = ["Car", "Pedestrian", "Cyclist", "Van"]
SIZES = {"Car": (1.6, 3.9, 1.56), "Pedestrian": (0.6, 0.8, 1.73), "Cyclist": (0.6, 1.76, 1.73), "Van": (1.9, 5.0, 2.2)}
FRAMES = "abcdefgh"


def crop(gen, full_map, fmap):
    """the generator's anchor range cut to `fmap` cells of the `full_map` grid, starting at x = range start and centred in y"""
    r = np.array(gen["anchor_ranges"], np.float64)
    sx, sy = (r[3] - r[0]) / full_map[2], (r[4] - r[1]) / full_map[1]
    return [float(r[0]), float(-sy * fmap[1] / 2), float(r[2]), float(r[0] + sx * fmap[2]), float(sy * fmap[1] / 2), float(r[5])]


def frames(rng, extent):
    """name -> (boxes (M, 7), class codes (M,)): the edge cases the batched kernel has to hold, inside the crop `extent`"""
    x0, y0, x1, y1 = extent

    def boxes(names):
        m = len(names)
        b = np.zeros((m, 7), np.float32)
        b[:, 0] = rng.uniform(x0 + 1, x1 - 1, m); b[:, 1] = rng.uniform(y0 + 1, y1 - 1, m); b[:, 2] = rng.uniform(-1.4, -0.4, m)
        for i, n in enumerate(names):
            b[i, 3:6] = np.array(SIZES[n]) * rng.uniform(0.85, 1.15, 3)
        b[:, 6] = rng.uniform(-np.pi, np.pi, m)
        return b, np.array([NAMES.index(n) for n in names], np.int8)

    out = {}
    out["a"] = boxes(["Car", "Pedestrian", "Cyclist", "Car", "Pedestrian", "Cyclist", "Car", "Pedestrian", "Car", "Cyclist"])
    out["b"] = boxes(["Car", "Cyclist", "Car", "Cyclist", "Cyclist"])                       # no Pedestrian
    out["c"] = boxes([])                                                                    # empty
    out["d"] = boxes(["Car", "Van", "Pedestrian", "Van", "Cyclist"])                        # rows that belong to no task
    b, c = boxes(["Car", "Pedestrian", "Cyclist", "Car", "Pedestrian", "Cyclist"])         # one box per class overlaps no anchor
    b[3:, :2] = [150.0, 150.0]
    out["e"] = (b, c)
    b, c = boxes(["Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Cyclist"])         # yaw on either side of pi / 4
    b[0::2, 6] = np.float32(np.pi / 4) - np.float32(5e-4)
    b[1::2, 6] = np.float32(np.pi / 4) + np.float32(5e-4)
    out["f"] = (b, c)
    b, c = boxes(["Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Cyclist", "Car"])  # identical pairs: first argmax
    b[1], b[3], b[5] = b[0], b[2], b[4]
    out["g"] = (b, c)
    out["h"] = boxes(["Car", "Pedestrian", "Cyclist"] * 10)                                 # 30 boxes
    return out


def main():
    import make_golden as MG
    assert os.path.isdir(MG.REF)
    from oracle import postprocess as pp
    from sessd_hip import configs   # before the stubs: it imports the mirror's det3d, which the stubs then shadow
    assigners = dict(c3=configs.ASSIGNER_3CLASS, pp=configs.ASSIGNER_POINTPILLARS)
    for k in [k for k in sys.modules if k == "det3d" or k.startswith("det3d.")]:
        del sys.modules[k]
    MG.install_stubs()
    np.bool = bool  # removed alias still used by the reference
    MG.load_ref("det3d/core/bbox/geometry.py", "det3d.core.bbox.geometry")
    bnp = MG.load_ref("det3d/core/bbox/box_np_ops.py", "det3d.core.bbox.box_np_ops")
    sys.modules["det3d.core.bbox"].box_np_ops = bnp
    ops = MG.load_ref("det3d/core/anchor/target_ops_v3.py", "ref_target_ops")

    def similarity(a, g):  # NearestIouSimilarity._compare on [x, y, w, l, r] (target_assigner.py:79-82)
        return bnp.iou_jit(bnp.rbbox2d_to_near_bbox(a[:, [0, 1, 3, 4, -1]]), bnp.rbbox2d_to_near_bbox(g[:, [0, 1, 3, 4, -1]]), eps=0.0)

    def encode(boxes, anc):
        return bnp.second_box_encode(boxes, anc, False, False)

    out = dict(names=np.array(NAMES))
    for key, assigner, full_map, fmap, seed in (("c3", assigners["c3"], (1, 200, 176), (1, 40, 44), 3),
                                                ("pp", assigners["pp"], (1, 248, 216), (1, 37, 29), 4)):
        gens = assigner["target_assigner"]["anchor_generators"]
        out[key + "_feature_map"] = np.array(fmap, np.int32)
        out[key + "_task_names"] = np.array([g["class_name"] for g in gens])
        out[key + "_thresholds"] = np.array([[g["matched_threshold"], g["unmatched_threshold"]] for g in gens], np.float32)
        anchors = []
        for t, g in enumerate(gens):
            rng_t = crop(g, full_map, fmap)
            a = pp.create_anchors_3d_range(fmap, rng_t, g["sizes"], g["rotations"]).reshape(-1, 7).astype(np.float32)
            anchors.append(a)
            out["%s_range%d" % (key, t)] = np.array(rng_t, np.float64)
            out["%s_sizes%d" % (key, t)] = np.array(g["sizes"], np.float64)
            out["%s_rotations%d" % (key, t)] = np.array(g["rotations"], np.float64)
            out["%s_anchors_checksum%d" % (key, t)] = a.astype(np.float64).sum(0)
        r0 = out[key + "_range0"]
        N = anchors[0].shape[0]
        for f, (gt, codes) in frames(np.random.RandomState(seed), (r0[0], r0[1], r0[3], r0[4])).items():
            out["%s_%s_gt" % (key, f)] = gt
            out["%s_%s_codes" % (key, f)] = codes
            gt_names = np.array(NAMES)[codes] if len(codes) else np.zeros(0, "<U10")
            for t, g in enumerate(gens):
                mask = np.array([c == g["class_name"] for c in gt_names], dtype=np.bool_)   # assign_v2 :90
                tg = ops.create_target_np(anchors[t], gt[mask], similarity, encode, prune_anchor_fn=None,
                                          gt_classes=np.ones(int(mask.sum()), np.int32),
                                          matched_threshold=np.full(N, g["matched_threshold"], np.float32),
                                          unmatched_threshold=np.full(N, g["unmatched_threshold"], np.float32),
                                          positive_fraction=None, rpn_batch_size=512, norm_by_num_examples=False, box_code_size=7)
                pos = np.nonzero(tg["labels"] > 0)[0]
                assert np.all(tg["bbox_targets"][tg["labels"] <= 0] == 0) and set(np.unique(tg["labels"])) <= {-1, 0, 1}
                assert np.array_equal(tg["bbox_outside_weights"], (tg["labels"] > 0).astype(np.float32))
                p = "%s_%s_t%d_" % (key, f, t)
                out[p + "labels"] = tg["labels"].astype(np.int8)
                out[p + "pos"] = pos.astype(np.int32)
                out[p + "targets_pos"] = tg["bbox_targets"][pos].astype(np.float32)
                out[p + "gt_id"] = np.asarray(tg["positive_gt_id"], np.int32)
                print(key, f, g["class_name"], "gt", int(mask.sum()), "pos", len(pos), "neg", int((tg["labels"] == 0).sum()),
                      "ignore", int((tg["labels"] < 0).sum()))
    np.savez_compressed(os.path.join(HERE, "assign_multi_ref.npz"), **out)


if __name__ == "__main__":
    main()
