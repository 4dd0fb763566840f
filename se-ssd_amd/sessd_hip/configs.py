"""The SE-SSD KITTI-car model / test / voxel settings as plain dicts (values of examples/second/configs/config.py:
model :48-90, test_cfg :113-124, voxel_generator :174-180), for tests and the benchmark on machines where the
reference tree (and therefore its config file) is absent. `Config.fromfile(<reference config.py>)` gives the same."""
import logging

from det3d.builder import build_box_coder


# Three-class KITTI variant (one task per class, as MultiGroupHead builds one Head per task): per-task anchor box sizes
# (w, l, h) and anchor centre heights; two rotations per location each.
KITTI_3CLASS_TASKS = [dict(num_class=1, class_names=["Car"]), dict(num_class=1, class_names=["Pedestrian"]),
                      dict(num_class=1, class_names=["Cyclist"])]
KITTI_3CLASS_ANCHORS = [dict(sizes=(1.6, 3.9, 1.56), z=-1.0, rotations=(0, 1.57)),
                        dict(sizes=(0.6, 0.8, 1.73), z=-0.6, rotations=(0, 1.57)),
                        dict(sizes=(0.6, 1.76, 1.73), z=-0.6, rotations=(0, 1.57))]


def kitti_3class_model():
    """kitti_car_model() with tasks = [Car, Pedestrian, Cyclist]; its loss is the supervised one (MultiGroupHead.loss_supervised /
    loss_supervised_device), the SE-SSD loss and TrainStep are single-task."""
    return kitti_car_model(tasks=KITTI_3CLASS_TASKS)


def kitti_3class_rpn_model():
    """The model dict of the reference's three-class config (examples/second/configs/
    kitti_all_vfev3_spmiddlefhd_rpn1_mghead_syncbn.py:62-115): the three one-class tasks on the SECOND-style RPN neck (one block
    of 1 + 5 3x3 layers, one stride-1 up-sampler) instead of SSFA. Anchors: kitti_3class_anchors(). VoxelNet.forward(example, is_ema=[False, None]) returns its
    supervised loss; sessd_hip.train.SupervisedTrainStep is its iteration."""
    m = kitti_car_model(tasks=KITTI_3CLASS_TASKS)
    m["neck"] = dict(type="RPN", layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1],
                     us_num_filters=[128], num_input_features=128, norm_cfg=None, logger=logging.getLogger("RPN"))
    m["bbox_head"]["in_channels"] = sum([128])
    m["bbox_head"]["weights"] = [1]
    return m


def kitti_3class_anchors(feature_hw=(200, 176), voxel_range=None):
    """(3, H*W*2, 7) anchors of KITTI_3CLASS_ANCHORS over the x / y extent of `voxel_range` (default: the KITTI range)."""
    from .anchors import create_task_anchors
    r = VOXEL_GENERATOR["range"] if voxel_range is None else voxel_range
    return create_task_anchors(feature_hw, KITTI_3CLASS_ANCHORS, (r[0], r[1], r[3], r[4]))


def _anchor_generator(class_name, sizes, z, matched, unmatched):
    return dict(type="anchor_generator_range", sizes=list(sizes), anchor_ranges=[0, -40.0, z, 70.4, 40.0, z], rotations=[0, 1.57],
                matched_threshold=matched, unmatched_threshold=unmatched, class_name=class_name)


_BOX_CODER = dict(type="ground_box3d_coder", n_dim=7, linear_dim=False, encode_angle_vector=False)

# The `assigner` dict (train_cfg.assigner, what the AssignTarget stage takes as cfg) of the reference's three-class config
# (examples/second/configs/kitti_all_vfev3_spmiddlefhd_rpn1_mghead_syncbn.py:19-55,117-122): one anchor generator per task on
# the [1, 200, 176] map, Car at 0.6 / 0.45, Pedestrian and Cyclist at 0.4 / 0.2.
ASSIGNER_3CLASS = dict(
    box_coder=_BOX_CODER,
    target_assigner=dict(type="iou", anchor_generators=[
        _anchor_generator("Car", KITTI_3CLASS_ANCHORS[0]["sizes"], KITTI_3CLASS_ANCHORS[0]["z"], 0.6, 0.45),
        _anchor_generator("Pedestrian", KITTI_3CLASS_ANCHORS[1]["sizes"], KITTI_3CLASS_ANCHORS[1]["z"], 0.4, 0.2),
        _anchor_generator("Cyclist", KITTI_3CLASS_ANCHORS[2]["sizes"], KITTI_3CLASS_ANCHORS[2]["z"], 0.4, 0.2)],
        sample_positive_fraction=-1, sample_size=512, region_similarity_calculator=dict(type="nearest_iou_similarity"),
        pos_area_threshold=-1, tasks=KITTI_3CLASS_TASKS),
    out_size_factor=8, debug=False)

# The same of the PointPillars config (examples/point_pillars/configs/original_pp_mghead_syncbn_kitti.py:17-35,95-99): the car
# generator on the config's own anchor range, and the map its head really has -- the reference's stage hard-codes
# [1, 200, 176], which is not the 248 x 216 output of this neck.
ASSIGNER_POINTPILLARS = dict(
    box_coder=_BOX_CODER,
    target_assigner=dict(type="iou", anchor_generators=[_anchor_generator("Car", (1.6, 3.9, 1.56), -1.0, 0.6, 0.45)],
                         sample_positive_fraction=-1, sample_size=512,
                         region_similarity_calculator=dict(type="nearest_iou_similarity"), pos_area_threshold=-1,
                         tasks=[dict(num_class=1, class_names=["Car"])]),
    out_size_factor=2, feature_map_size=[1, 248, 216])


def kitti_car_model(tasks=None):
    tasks = [dict(num_class=1, class_names=["Car"])] if tasks is None else [dict(t) for t in tasks]
    box_coder = dict(type="ground_box3d_coder", n_dim=7, linear_dim=False, encode_angle_vector=False)
    return dict(
        type="VoxelNet", pretrained=None,
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=4, norm_cfg=None),
        backbone=dict(type="SpMiddleFHD", num_input_features=4, ds_factor=8, norm_cfg=None),
        neck=dict(type="SSFA", layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1],
                  us_num_filters=[128], num_input_features=128, norm_cfg=None, logger=logging.getLogger("RPN")),
        bbox_head=dict(type="MultiGroupHead", mode="3d", in_channels=128, norm_cfg=None, tasks=tasks, weights=[1] * len(tasks),
                       box_coder=build_box_coder(box_coder), encode_background_as_zeros=True,
                       loss_norm=dict(type="NormByNumPositives", pos_cls_weight=1.0, neg_cls_weight=1.0),
                       loss_cls=dict(type="SigmoidFocalLoss", alpha=0.25, gamma=2.0, loss_weight=1.0),
                       use_sigmoid_score=True,
                       loss_bbox=dict(type="WeightedSmoothL1Loss", sigma=3.0, code_weights=[1.0] * 7, codewise=True, loss_weight=2.0),
                       encode_rad_error_by_sin=True,
                       loss_aux=dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier", loss_weight=0.2),
                       direction_offset=0.0))


TEST_CFG = dict(nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=100,
                         nms_iou_threshold=0.01),
                score_threshold=0.3, post_center_limit_range=[0, -40.0, -5.0, 70.4, 40.0, 5.0], max_per_img=100)

# TEST_CFG with the other post-processor of get_task_detections (mg_head_sessd.py:999-1018): DI-NMS. Further keys of "nms" it
# reads, defaults = the reference's literals: nms_cnt_thresh, nms_sigma_dist_interval, nms_sigma_square, suppressed_thresh,
# centerness_pow (sessd_hip.ops.DI_DEFAULTS).
TEST_CFG_DI_NMS = dict(TEST_CFG, nms=dict(TEST_CFG["nms"], nms_type="rotate_weighted_nms"))

VOXEL_GENERATOR = dict(range=[0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel_size=[0.05, 0.05, 0.1], max_points_in_voxel=5,
                       max_voxel_num=20000)


def kitti_pointpillars_model():
    """The model dict of the reference's PointPillars config (examples/point_pillars/configs/original_pp_mghead_syncbn_kitti.py:
    42-93): PillarFeatureNet (one 64-filter PFN layer; voxel_size / pc_range not passed -- the reader's defaults apply) ->
    PointPillarsScatter -> RPN with three blocks and up-samplers of stride 1 / 2 / 4 -> one Car task on 384 channels.
    Through the det3d mirror; inference only unless the model is switched to `supervised = True` (PointPillars.forward_loss)."""
    m = kitti_car_model()
    m["type"] = "PointPillars"
    m["reader"] = dict(type="PillarFeatureNet", num_filters=[64], with_distance=False, norm_cfg=None)
    m["backbone"] = dict(type="PointPillarsScatter", ds_factor=1, norm_cfg=None)
    m["neck"] = dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256],
                     us_layer_strides=[1, 2, 4], us_num_filters=[128, 128, 128], num_input_features=64, norm_cfg=None,
                     logger=logging.getLogger("RPN"))
    m["bbox_head"]["in_channels"] = sum([128, 128, 128])
    m["bbox_head"]["weights"] = [1]
    return m


# test_cfg :104-115 and voxel_generator :166-171 of the same file
TEST_CFG_POINTPILLARS = dict(nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=300,
                                      nms_iou_threshold=0.5),
                             score_threshold=0.05, post_center_limit_range=[0, -40.0, -5.0, 70.4, 40.0, 5.0], max_per_img=100)

VOXEL_GENERATOR_POINTPILLARS = dict(range=[0, -39.68, -3, 69.12, 39.68, 1], voxel_size=[0.16, 0.16, 4.0], max_points_in_voxel=100,
                                    max_voxel_num=12000)


def build_synthetic_detector(device, seed=0, calib_frame_seed=0, max_voxels=16000, num_points=20000, supersample=1,
                             model_cfg=None, voxel_range=None):
    """det3d-mirror VoxelNet with seeded weights, BatchNorm statistics calibrated on one synthetic frame (on `device`) of the
    workload's own density (supersample = 3 for the 200 k-point dense scenes): random weights calibrated on a sparse scan give
    activations (and decoded boxes) of absurd magnitude on a dense one.
    model_cfg: another model dict (kitti_3class_model(), kitti_3class_rpn_model()); voxel_range: a reduced range (the frame is cropped by the voxelizer)."""
    import torch
    from det3d.models import build_detector
    from . import ops, synth
    model = build_detector(kitti_car_model() if model_cfg is None else model_cfg, train_cfg=None, test_cfg=TEST_CFG)
    synth.init_synthetic_weights(model, seed)
    model.to(device)
    pts = torch.from_numpy(synth.make_frame(calib_frame_seed, num_points, supersample=supersample)).to(device)
    vr = VOXEL_GENERATOR["range"] if voxel_range is None else voxel_range
    vs = VOXEL_GENERATOR["voxel_size"]
    r = ops.voxelize_batch([pts], vs, vr, 5, max_voxels)
    m = int(r["prefix"][1].item())
    grid = [int(round((vr[i + 3] - vr[i]) / vs[i])) for i in range(3)]  # [1408, 1600, 40] for the KITTI range
    synth.calibrate_synthetic_model(model, r["mean"][:m].contiguous(), r["coors"][:m].contiguous(), 1, grid)
    return model
