"""DirectRgbdRefiner -- DenseRgbdRefiner with the gray frames kept: a photometric (intensity) term is joined to every step of
the point-to-plane ICP, so that texture pins the directions a wall, a floor or a table top leaves free.  K21:
`mi_intensity_maps`, `mi_rgbd_refine`; the algorithm is stated in include/mi355x_match.h.  The reference has no counterpart."""
import math

import torch

from ... import ops
from .dense_rgbd import DenseRgbdRefiner
from .rgbd_pose import RgbdPoseEstimator


class DirectRgbdRefiner(DenseRgbdRefiner):
    """forward(depth1, gray1, depth2, gray2, R0=None, t0=None) -> (R, t, information, rmse, count, rmse_photo, count_photo, ok)
    for depth frames (B, H, W) or (B, 1, H, W), float32 or uint16, ALREADY aligned to the camera of K, and the gray frames
    of the same pixels, (B, H, W) or (B, 1, H, W), uint8 or float32 (FrameIngest's outputs).  X2 = R X1 + t.  information
    (B, 6, 6) is the joint sum J^T J of the final linearisation; rmse / count belong to the point-to-plane term, rmse_photo
    (gray levels) / count_photo to the intensity term; ok is False -- with the pose before the failed step -- where the
    joint system was degenerate (too few correspondences, or a single plane without texture).  (H, W) frames give
    unbatched output.

    The constructor is DenseRgbdRefiner's, and photo_weight: the weight of one gray level in the depth's unit (0 turns the
    term off and gives DenseRgbdRefiner's result); intensity_threshold: residuals above it, in gray levels, are dropped.
    The term is an option, not a replacement: texture seen past an occlusion edge biases it, and on a scene with enough
    geometry (a room with objects) DenseRgbdRefiner alone can be the more accurate."""

    def __init__(self, K: torch.Tensor, depth_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                 schedule=((4, 4), (2, 4), (1, 6)), distance_threshold: float = 0.1, angle_threshold_deg: float = 30.0,
                 normal_max_jump: float = 0.1, min_correspondences: int = 64, photo_weight: float = 0.003,
                 intensity_threshold: float = 30.0) -> None:
        super().__init__(K, depth_scale, min_depth, max_depth, schedule, distance_threshold, angle_threshold_deg, normal_max_jump,
                         min_correspondences)
        if not (photo_weight >= 0 and math.isfinite(photo_weight)):
            raise ValueError(f"photo_weight must be finite and not negative, got {photo_weight}")
        if not (intensity_threshold > 0 and math.isfinite(intensity_threshold)):
            raise ValueError(f"intensity_threshold must be positive and finite, got {intensity_threshold}")
        self.photo_weight = float(photo_weight)
        self.intensity_threshold = float(intensity_threshold)

    @torch.no_grad()
    def forward(self, depth1: torch.Tensor, gray1: torch.Tensor, depth2: torch.Tensor, gray2: torch.Tensor,
                R0: torch.Tensor | None = None, t0: torch.Tensor | None = None):
        single = depth1.dim() == 2
        d1 = RgbdPoseEstimator._frames(depth1, single, "depth1")
        d2 = RgbdPoseEstimator._frames(depth2, single, "depth2")
        g1 = RgbdPoseEstimator._frames(gray1, single, "gray1")
        g2 = RgbdPoseEstimator._frames(gray2, single, "gray2")
        if not d1.is_cuda:
            raise RuntimeError(f"DirectRgbdRefiner: depth must live on the GPU (got device {d1.device}); this package has no CPU path")
        if d1.shape != d2.shape or g1.shape != d1.shape or g2.shape != d1.shape:
            raise RuntimeError(f"depth1, gray1, depth2 and gray2 must have one shape, got {tuple(depth1.shape)}, {tuple(gray1.shape)}, "
                               f"{tuple(depth2.shape)} and {tuple(gray2.shape)}")
        b = int(d1.shape[0])
        r0 = torch.eye(3, device=d1.device).expand(b, 3, 3) if R0 is None else R0.reshape(-1, 3, 3)
        t0 = torch.zeros((b, 3), device=d1.device) if t0 is None else t0.reshape(-1, 3)
        k_inv = self.K_inv.to(d1.device)
        m1 = ops.surfel_maps(d1, k_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump)
        m2 = ops.surfel_maps(d2, k_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump)
        r, t, info, rmse, count, rmse_p, count_p, _, ok = ops.rgbd_refine(
            (*m1, ops.intensity_maps(g1)), (*m2, ops.intensity_maps(g2)), r0, t0, self.camera, self.schedule, self.distance_threshold,
            self.angle_threshold, self.photo_weight, self.intensity_threshold, self.min_correspondences)
        out = (r, t, info, rmse, count, rmse_p, count_p, ok)
        return tuple(x[0] for x in out) if single else out
