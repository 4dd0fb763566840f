"""PointPillars detector: pillar reader -> scatter to the BEV canvas -> neck -> head (+ predict), the inference surface of
det3d/models/detectors/point_pillars.py:5-54 and single_stage.py:8-19. Same constructor kwargs and the reference's
`forward(example, return_loss=True)` signature: `return_loss=False` returns `bbox_head.predict(...)`, a list of
dict(box3d_lidar, scores, label_preds, metadata); `return_loss=True` raises NotImplementedError (inference only) unless the model
was switched to `supervised = True`: then it returns the supervised loss dict of `bbox_head.loss_supervised` (mg_head.py:559-652),
and `forward_loss` gives the same loss as one scalar, from the device op sessd_supervised_loss where that covers the head."""
from torch import nn

from .. import builder
from ..registry import DETECTORS


@DETECTORS.register_module
class PointPillars(nn.Module):
    def __init__(self, reader, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.reader = builder.build_reader(reader)
        self.backbone = builder.build_backbone(backbone)
        if neck is not None:
            self.neck = builder.build_neck(neck)
        self.bbox_head = builder.build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        # opt-in: the default keeps the inference-only contract (return_loss=True is refused by name); True enables
        # forward(return_loss=True) and forward_loss, which sessd_hip.train.SupervisedTrainStep runs and captures
        self.supervised = False
        self.device_loss = True   # forward_loss: sessd_supervised_loss where it covers (False: the torch formulation)

    @property
    def with_neck(self):
        return getattr(self, "neck", None) is not None

    def extract_feat(self, data):
        n_dev = data.get("num_voxels_dev")
        if n_dev is None:
            input_features = self.reader(data["features"], data["num_voxels"], data["coors"])
            x = self.backbone(input_features, data["coors"], data["batch_size"], data["input_shape"])
        else:   # capacity form: fixed-size tables, the live pillar count on the device (a captured iteration replays on it)
            input_features = self.reader(data["features"], data["num_voxels"], data["coors"], num_voxels_dev=n_dev)
            x = self.backbone(input_features, data["coors"], data["batch_size"], data["input_shape"], num_voxels_dev=n_dev)
        return self.neck(x) if self.with_neck else x

    def forward(self, example, return_loss=True, **kwargs):
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0],
                    num_voxels_dev=example.get("num_voxels_dev"))
        if return_loss and not self.supervised:
            raise NotImplementedError("PointPillars: inference only (return_loss=False); training of this config is not supported")
        preds = self.bbox_head(self.extract_feat(data))
        if return_loss:
            return self.bbox_head.loss_supervised(example, preds)
        return self.bbox_head.predict(example, preds, self.test_cfg)

    def forward_loss(self, example, unit_grad=False):
        """(total, record_or_dict): the supervised loss summed over the tasks as one differentiable scalar. Where
        bbox_head.supervised_loss_covers (and device_loss is on) it is the device op, with its (T + 1, 32) device record
        (bbox_head.supervised_record_to_dict reads it); otherwise the torch formulation with its dict. In train mode the pass
        runs through the fused reader and neck as every forward does. Needs `supervised = True`."""
        if not self.supervised:
            raise NotImplementedError("PointPillars: inference only (return_loss=False); training of this config is not supported "
                                      "unless the model is switched to supervised = True")
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0],
                    num_voxels_dev=example.get("num_voxels_dev"))
        preds = self.bbox_head(self.extract_feat(data))
        if self.device_loss and self.bbox_head.supervised_loss_covers(example, preds):
            return self.bbox_head.loss_supervised_device(example, preds, unit_grad=unit_grad)
        ret = self.bbox_head.loss_supervised(example, preds)
        return sum(ret["loss"]), ret
