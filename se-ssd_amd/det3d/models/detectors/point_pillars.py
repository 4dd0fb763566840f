"""PointPillars detector: pillar reader -> scatter to the BEV canvas -> neck -> head (+ predict), the inference surface of
det3d/models/detectors/point_pillars.py:5-54 and single_stage.py:8-19. Same constructor kwargs and the reference's
`forward(example, return_loss=True)` signature: `return_loss=False` returns `bbox_head.predict(...)`, a list of
dict(box3d_lidar, scores, label_preds, metadata); `return_loss=True` raises NotImplementedError (inference only)."""
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

    @property
    def with_neck(self):
        return getattr(self, "neck", None) is not None

    def extract_feat(self, data):
        input_features = self.reader(data["features"], data["num_voxels"], data["coors"])
        x = self.backbone(input_features, data["coors"], data["batch_size"], data["input_shape"])
        return self.neck(x) if self.with_neck else x

    def forward(self, example, return_loss=True, **kwargs):
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0])
        if return_loss:
            raise NotImplementedError("PointPillars: inference only (return_loss=False); training of this config is not supported")
        preds = self.bbox_head(self.extract_feat(data))
        return self.bbox_head.predict(example, preds, self.test_cfg)
