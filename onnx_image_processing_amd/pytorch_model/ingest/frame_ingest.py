"""The front door of the frames -> matches -> pose chain: what the reference's hosts do to every camera frame on the CPU
(sample/visual_odometry.py:65-92 load_image_from_array: BGR2GRAY, resize to the model's resolution, float32) and to the
camera matrix (:928-941), on the device."""
from __future__ import annotations

import torch
from torch import nn

from ... import ops


class FrameIngest(nn.Module):
    """uint8 colour frames (B, Hs, Ws, C) or (Hs, Ws, C), C in {1, 3, 4}, of any size -> (B, 1, height, width) gray model
    frames: torch.uint8 (for the uint8 forms of the matchers) or torch.float32 holding the same values.  One HIP launch
    (`mi_ingest_frames`), asynchronous on the current stream and capturable; the arithmetic is the header's integer
    restatement of OpenCV's 8-bit path."""

    def __init__(self, height: int, width: int, channel_order: str = "bgr", out_dtype: torch.dtype = torch.uint8):
        super().__init__()
        if int(height) < 1 or int(width) < 1 or max(int(height), int(width)) > ops.INGEST_MAX_DIM:
            raise ValueError(f"height and width must be in 1 .. {ops.INGEST_MAX_DIM}, got ({height}, {width})")
        if channel_order not in ("bgr", "rgb"):
            raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
        if out_dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
        self.height, self.width, self.channel_order, self.out_dtype = int(height), int(width), channel_order, out_dtype

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        return ops.ingest_frames(frames, self.height, self.width, channel_order=self.channel_order, out_dtype=self.out_dtype)


def scale_intrinsics(K, src_size, dst_size) -> torch.Tensor:
    """The camera matrix of frames resized from src_size to dst_size, both (height, width): fx and cx times
    dst_w / src_w, fy and cy times dst_h / src_h (the sample's rule; skew, if any, scales with x).  K: 3x3, a tensor or
    anything torch.as_tensor takes; returned on K's device in K's floating dtype (float32 for integers), ready for
    RelativePoseEstimator."""
    k = torch.as_tensor(K)
    if k.shape != (3, 3):
        raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(k.shape)}")
    (sh, sw), (dh, dw) = src_size, dst_size
    if min(sh, sw, dh, dw) <= 0:
        raise ValueError(f"sizes must be positive (height, width) pairs, got {src_size} -> {dst_size}")
    if not k.is_floating_point():
        k = k.float()
    s = torch.tensor([dw / sw, dh / sh, 1.0], dtype=k.dtype, device=k.device)
    return k * s[:, None]
