"""Pin the CPU oracle (oracle/*.c) to the reference's own outputs (tests/golden/*.npz, produced by
tests/golden/make_golden.py from the reference sources / the compiled reference iou3d_cpu.cpp)."""
import os

import numpy as np
import pytest

import oracle
from sessd_hip import synth


@pytest.mark.parametrize("case", ["frame", "cap", "edge", "dup", "mp35", "empty"])
def test_voxelizer_oracle_bit_exact(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "voxelize_ref.npz"))
    mp, mv = g[case + "_cfg"]
    v, c, n = oracle.points_to_voxel(g[case + "_pts"], synth.KITTI_VOXEL, synth.KITTI_RANGE, int(mp), int(mv))
    assert v.shape == g[case + "_voxels"].shape
    assert np.array_equal(c, g[case + "_coors"])
    assert np.array_equal(n, g[case + "_num"])
    assert np.array_equal(v.view(np.uint32), g[case + "_voxels"].view(np.uint32))


def test_iou3d_oracle_vs_compiled_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "iou3d_ref.npz"))
    assert np.array_equal(oracle.boxes_overlap_bev(g["a5"], g["b5"]), g["overlap"])
    assert np.array_equal(oracle.boxes_iou_bev(g["a5"], g["b5"]), g["iou_bev"])
    assert np.array_equal(oracle.boxes_iou3d(g["a7"], g["b7"], gpu_variant=False), g["iou3d_cpu"])
    assert np.array_equal(oracle.boxes_overlap_bev(g["literal"], g["literal"]), g["lit_overlap"])
    # analytic anchors of the algorithm itself
    lit = g["lit_iou"]
    assert abs(lit[0, 1] - 1.0 / 7.0) < 1e-6      # unit-offset 2x2 squares
    assert abs(lit[0, 2] - 0.70710678) < 1e-5     # 45 degree copy
    assert lit[0, 3] == 0.0                        # disjoint
    assert abs(lit[0, 4] - 1.0) < 1e-6             # identical
    assert (g["overlap"] > 0).sum() > 50           # the fixture really exercises overlapping pairs


def test_live_reference_agrees_when_present(golden_dir):
    """The restatement is bit-equal to the compiled reference on the seed-99 clustered boxes: live where oracle/_ref exists (built
    from the reference sources), and always against that reference's stored output (iou_bev_live_ref.npz, make_golden_iou_live.py)."""
    a = synth.boxes7_to_bev5(synth.clustered_boxes7(200, seed=99))
    if oracle.ref_lib() is not None:
        assert np.array_equal(oracle.boxes_iou_bev(a, a), oracle.ref_boxes_iou_bev(a, a))
    g = np.load(os.path.join(golden_dir, "iou_bev_live_ref.npz"))
    assert np.array_equal(oracle.boxes_iou_bev(g["boxes"], g["boxes"]), g["iou_bev"])
    assert (g["iou_bev"] > 0).sum() > 2 * len(a)   # the clustered boxes overlap beyond the diagonal


def test_nms_helpers_vs_reference_numpy(golden_dir):
    g = np.load(os.path.join(golden_dir, "nms_helpers_ref.npz"))
    c = oracle.box2d_corners(g["dets"])
    assert np.allclose(c, g["corners"], atol=2e-6, rtol=0)
    su = np.concatenate([c.min(1), c.max(1)], 1)
    assert np.allclose(su, g["standup"], atol=2e-6, rtol=0)


def test_quad_iou_agrees_with_iou3d_reference_algorithm():
    """Polygon clipping (oracle, f64) and the reference iou3d algorithm (f32) must agree to ~1e-5."""
    b = synth.clustered_boxes7(120, seed=4)
    d = b[:, [0, 1, 3, 4, 6]]
    c = oracle.box2d_corners(d)
    ref = oracle.boxes_iou_bev(synth.boxes7_to_bev5(b), synth.boxes7_to_bev5(b))
    worst = 0.0
    for i in range(0, 120, 3):
        for j in range(120):
            # NOTE the two conventions rotate in opposite senses for the same angle value:
            # iou3d rotates corners by +angle (x' = x cos + y sin ...) exactly like rotation_2d.
            worst = max(worst, abs(oracle.quad_iou(c[i], c[j]) - float(ref[i, j])))
    assert worst < 5e-5, worst


def test_postprocess_oracle_vs_reference_helpers(golden_dir):
    """anchors, frustum surfaces, frustum test and box decode of oracle/postprocess.py vs the reference's own functions."""
    from oracle import postprocess as pp
    g = np.load(os.path.join(golden_dir, "nms_helpers_ref.npz"))
    anchors = pp.create_anchors_3d_range().reshape(-1, 7)
    assert np.array_equal(anchors[g["anchors_sample_idx"]], g["anchors_sample"])
    assert np.allclose(anchors.sum(0), g["anchors_sum"], rtol=1e-6)
    cal = synth.kitti_calib()
    fr = pp.get_valid_frustum(cal["rect"], cal["Trv2c"], cal["P2"], cal["image_shape"])
    assert fr.shape == (1, 6, 4, 3) and np.allclose(fr, g["frustum"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(pp.points_in_frustum(g["frustum_pts"], g["frustum"]), g["frustum_inside"].reshape(-1))
    d = np.load(os.path.join(golden_dir, "decode_ref.npz"))
    dec = pp.second_box_decode(d["enc"], d["anchors"])
    assert np.allclose(dec, d["dec"], rtol=2e-6, atol=2e-6)


def test_standup_iou_prefilter_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "nms_helpers_ref.npz"))
    su = g["standup"]
    # the oracle's prefilter (iou_jit eps=0 > 0) decision on every pair
    iw = np.minimum(su[:, None, 2], su[None, :, 2]) - np.maximum(su[:, None, 0], su[None, :, 0])
    ih = np.minimum(su[:, None, 3], su[None, :, 3]) - np.maximum(su[:, None, 1], su[None, :, 1])
    assert np.array_equal((iw > 0) & (ih > 0), g["standup_iou"] > 0)


def test_numba_rotate_iou_oracle_vs_reference_source(golden_dir):
    """oracle/rotate_iou_eval.c vs the reference's numba device functions executed as Python (bit-equal)."""
    g = np.load(os.path.join(golden_dir, "rotate_iou_numba_ref.npz"))
    q = g["boxes"]
    got = np.array([[oracle.rotate_iou_pair(q[i], q[j], -1) for j in range(24)] for i in range(24)], np.float32)
    assert np.array_equal(got, g["iou"])
    for crit, key in ((-1, "eval_m1"), (0, "eval_0"), (1, "eval_1"), (2, "eval_2")):
        e = np.array([[oracle.rotate_iou_pair(q[i], q[j], crit) for j in range(12)] for i in range(12)], np.float32)
        assert np.array_equal(e, g[key])
    # the eval kernel passes the QUERY box first (nms_gpu.py:626-631)
    ev = oracle.rotate_iou_eval(q[:5], q[5:9], 0)
    assert ev[2, 1] == np.float32(oracle.rotate_iou_pair(q[6], q[2], 0))


def test_assign_target_oracle_vs_reference_run(golden_dir):
    """oracle/assign_target.py vs the reference's create_target_np + NearestIouSimilarity + second_box_encode run from source."""
    from oracle import assign_target as oat, postprocess as pp
    g = np.load(os.path.join(golden_dir, "assign_ref.npz"))
    anchors = pp.create_anchors_3d_range().reshape(-1, 7).astype(np.float32)
    assert np.allclose(anchors.sum(0), g["anchors_checksum"], rtol=1e-6)
    for c in "abcd":
        r = oat.assign(anchors, g[c + "_gt"])
        pos = np.nonzero(r["labels"] > 0)[0]
        assert np.array_equal(r["labels"], g[c + "_labels"]) and np.array_equal(pos, g[c + "_pos"])
        assert np.array_equal(r["positive_gt_id"], g[c + "_gt_id"])
        if len(pos):
            assert np.abs(r["bbox_targets"][pos] - g[c + "_targets_pos"]).max() < 1e-6
