from .voxel_downsampling import VoxelDownsampling

__all__ = ["VoxelDownsampling"]
