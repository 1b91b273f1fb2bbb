from .pillar_encoder import PFNLayer, PillarFeatureNet, PointPillarsScatter  # noqa: F401
from .voxel_reader import VoxelMeanFeatureExtractor  # noqa: F401
