"""Mirror of reference pytorch_model/pointcloud/voxel_downsampling.py (VoxelDownsampling): the K12 voxel-grid kernels
(`mi_voxel_downsample`).  Same voxel set, order, counts and mask as the reference; the means are the fp64 means rounded
once to float32, not the reference's differences of float32 cumsums (include/mi355x_match.h)."""
import torch
from torch import nn

from ... import ops


class VoxelDownsampling(nn.Module):
    """Voxel downsampling for point cloud data.

    Downsamples a point cloud by averaging points within each voxel grid cell.
    """

    DTYPE = torch.float32

    def __init__(self) -> None:
        super().__init__()

    def forward(self, points: torch.Tensor, leaf_size: torch.Tensor):
        """points: (N, D) float32 on the GPU, D >= 3; leaf_size: scalar tensor (a device tensor is read on the device)
        or number.  Returns output_points (N, D) -- the M voxel means first, then zero rows -- and mask (N,) bool, True
        for the first M rows."""
        return ops.voxel_downsample(points, leaf_size)
