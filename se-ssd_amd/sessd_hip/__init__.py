"""MI355X-native SE-SSD hot path: Python face of libsessd_hip.so (device pointers come from torch)."""
from ._lib import lib, LIB_PATH, SIGNATURES, SessdError, check  # noqa: F401
from . import ops  # noqa: F401
from .pillar_engine import PillarEngine, check_pillar_model  # noqa: F401
from .runner import HostFedPipeline, pillar_engines_on_cu_sets  # noqa: F401
