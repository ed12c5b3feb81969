"""Mirror of reference pytorch_model/depth/depth2pointcloud.py (DepthToPointCloud): the K13 points kernel
(`mi_depth_to_points`).  The reference's (H, W, 3) `uv` buffer has three distinct columns -- one value per image
column, one per image row and one constant -- which are kept as two small tables and a scalar; the products are the
reference's bits."""
import torch
from torch import nn

from ... import ops


def pinhole_tables(scale: float, width: int, height: int, cx: float, cy: float, fx: float, fy: float):
    """(u_tab (width,), v_tab (height,), z_scale): the columns of the reference's `uv`, built on the CPU with the
    reference's own float32 operations in its order (subtract, IEEE divide, multiply by scale)."""
    u = torch.arange(width, dtype=torch.float32)
    v = torch.arange(height, dtype=torch.float32)
    u -= cx
    u /= fx
    v -= cy
    v /= fy
    ones = torch.ones(1, dtype=torch.float32)
    u *= scale
    v *= scale
    ones *= scale
    return u, v, float(ones[0])


class DepthToPointCloud(nn.Module):
    def __init__(self, scale: float, width: int, height: int, cx: float, cy: float, fx: float, fy: float) -> None:
        super().__init__()
        self.scale = float(scale)
        self.width, self.height = int(width), int(height)
        u, v, self.z_scale = pinhole_tables(self.scale, self.width, self.height, cx, cy, fx, fy)
        self.register_buffer("u_tab", u, persistent=False)     # moved with the module, not in the state dict
        self.register_buffer("v_tab", v, persistent=False)

    def forward(self, depth: torch.Tensor):
        """depth: (H, W, 1) float32 on the GPU as in the reference -> (H, W, 3); also (H, W), (B, H, W), (B, H, W, 1)
        (-> (B, H, W, 3)) and uint16 sensor counts."""
        return ops.depth_to_points(depth, self.u_tab, self.v_tab, self.z_scale)
