from .point_pillars import PointPillars  # noqa: F401
from .voxelnet import VoxelNet  # noqa: F401
