"""Generates tests/golden/iou_bev_live_ref.npz: the COMPILED reference iou3d_cpu.cpp (oracle/_ref, built by oracle/build.py where
the reference sources exist) on the seed-99 clustered boxes of tests/test_oracle_golden.py::test_live_reference_agrees_when_present,
so that the test holds the restatement to the reference where oracle/_ref cannot be built.
Run in the build container (needs oracle/_ref): python tests/golden/make_golden_iou_live.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "se-ssd_amd")]
import oracle  # noqa: E402
from sessd_hip import synth  # noqa: E402

assert oracle.ref_lib() is not None, "oracle/_ref not built (needs the reference sources)"
a = synth.boxes7_to_bev5(synth.clustered_boxes7(200, seed=99))
np.savez_compressed(os.path.join(HERE, "iou_bev_live_ref.npz"), boxes=a, iou_bev=oracle.ref_boxes_iou_bev(a, a))
print("wrote iou_bev_live_ref.npz:", os.path.getsize(os.path.join(HERE, "iou_bev_live_ref.npz")), "bytes")
