from .pillar_encoder import PFNLayer, PillarFeatureNet, PointPillarsScatter  # noqa: F401
from .voxel_encoder import VoxelFeatureExtractorV3  # noqa: F401
