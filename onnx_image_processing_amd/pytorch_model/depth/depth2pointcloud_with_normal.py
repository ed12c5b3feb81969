"""Mirror of reference pytorch_model/depth/depth2pointcloud_with_normal.py (DepthToPointCloudWithNormal): points and
Sobel normals in one launch of the K13 points kernel; the point image is not read back for the normals."""
import torch
from torch import nn

from ... import ops
from .depth2pointcloud import DepthToPointCloud


class DepthToPointCloudWithNormal(nn.Module):
    def __init__(self, scale: float, width: int, height: int, cx: float, cy: float, fx: float, fy: float) -> None:
        super().__init__()
        self.base_model = DepthToPointCloud(scale, width, height, cx, cy, fx, fy)

    def forward(self, depth: torch.Tensor):
        """depth as for DepthToPointCloud -> (points, normals), (H, W, 3) or (B, H, W, 3) each; normals =
        normalize((dx, dy, -1)) with dx / dy the 3x3 Sobel responses of X + Y + Z, zero padding."""
        b = self.base_model
        return ops.depth_to_points(depth, b.u_tab, b.v_tab, b.z_scale, normals=True)
