"""Mirror of reference pytorch_model/depth/depth_align.py (DepthAlignment): the K13 alignment kernels
(`mi_depth_align`).  Same arithmetic per source pixel; where the reference races (duplicate indices of its four
index_put_), raises (targets in column `width` / row `height`) or sends out-of-frame sources to pixel (0, 0), this module
keeps the minimum over all writers, drops the target and writes nothing (include/mi355x_match.h)."""
import torch
from torch import nn

from ... import ops
from .depth2pointcloud import pinhole_tables


class DepthAlignment(nn.Module):
    DTYPE = torch.float32

    def __init__(self, scale: float, width: int, height: int, depth_cx: float, depth_cy: float, depth_fx: float,
                 depth_fy: float, rgb_cx: float, rgb_cy: float, rgb_fx: float, rgb_fy: float, rotation: torch.Tensor,
                 translation: torch.Tensor) -> None:
        super().__init__()
        self.width, self.height = int(width), int(height)
        self.scale = float(scale)
        u, v, self.z_scale = pinhole_tables(self.scale, self.width, self.height, depth_cx, depth_cy, depth_fx, depth_fy)
        self.rgb = (float(rgb_cx), float(rgb_cy), float(rgb_fx), float(rgb_fy))
        self.register_buffer("u_tab", u, persistent=False)
        self.register_buffer("v_tab", v, persistent=False)
        self.register_buffer("rotation", torch.as_tensor(rotation).reshape(3, 3).to(dtype=self.DTYPE).clone(), persistent=False)
        self.register_buffer("translation", torch.as_tensor(translation).reshape(3).to(dtype=self.DTYPE).clone(), persistent=False)

    def forward(self, depth_image: torch.Tensor) -> torch.Tensor:
        """depth_image: (H, W, 1) float32 on the GPU as in the reference -> (H, W, 1); also (H, W), (B, H, W),
        (B, H, W, 1) and uint16; the result has the input's shape."""
        return ops.depth_align(depth_image, self.u_tab, self.v_tab, self.z_scale, *self.rgb, self.rotation, self.translation)
