"""DenseRgbdRefiner -- the last step of an RGB-D odometry: the pose of RgbdPoseEstimator (or the identity, for a frame with too
few matches) refined against every pixel of the two depth frames by projective point-to-plane ICP, with the 6x6 information
matrix of the result.  K18: `mi_surfel_maps`, `mi_icp_refine`; the algorithm is stated in include/mi355x_match.h.  The
reference has no counterpart."""
import math

import torch
from torch import nn

from ... import ops
from .rgbd_pose import RgbdPoseEstimator


class DenseRgbdRefiner(nn.Module):
    """forward(depth1, depth2, R0=None, t0=None) -> (R, t, information, rmse, count, ok) for depth frames (B, H, W) or
    (B, 1, H, W), float32 or uint16, ALREADY aligned to the camera of K (DepthAlignment).  X2 = R X1 + t, the convention of
    RgbdPoseEstimator, whose (R, t) is the intended R0 / t0 (default: identity).  information (B, 6, 6) is sum J^T J of the
    final linearisation in (rotation, translation) order, rmse the root-mean-square point-to-plane residual over its `count`
    correspondences; ok is False -- with the pose before the failed step -- where the system was degenerate (too few
    correspondences, or a scene such as a single plane that leaves a direction unconstrained).  (H, W) depth gives unbatched
    output.

    K: the 3x3 camera matrix.  depth_scale turns a depth value into the unit of the result; pixels outside [min_depth,
    max_depth] are ignored.  schedule: up to 4 stages of (source stride in {1, 2, 4, 8}, iterations), run as given.  A
    correspondence needs a distance below distance_threshold and normals within angle_threshold_deg; a normal is formed only
    where the four neighbours' depths are within normal_max_jump of the pixel's."""

    def __init__(self, K: torch.Tensor, depth_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                 schedule=((4, 4), (2, 4), (1, 6)), distance_threshold: float = 0.1, angle_threshold_deg: float = 30.0,
                 normal_max_jump: float = 0.1, min_correspondences: int = 64) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        if not depth_scale > 0:
            raise ValueError(f"depth_scale must be positive, got {depth_scale}")
        if not min_depth > 0 or not max_depth >= min_depth:
            raise ValueError(f"need 0 < min_depth <= max_depth, got {min_depth}, {max_depth}")
        try:
            sched = tuple((int(s), int(i)) for s, i in schedule)
        except (TypeError, ValueError):
            raise ValueError(f"schedule must be a sequence of (stride, iterations) pairs, got {schedule!r}") from None
        if not 1 <= len(sched) <= ops.ICP_MAX_STAGES:
            raise ValueError(f"schedule needs 1 .. {ops.ICP_MAX_STAGES} stages, got {len(sched)}")
        if any(s not in ops.ICP_STRIDES or i < 0 for s, i in sched):
            raise ValueError(f"every stage needs a stride in {ops.ICP_STRIDES} and iterations >= 0, got {sched}")
        if sum(i for _, i in sched) > ops.ICP_MAX_ITERATIONS:
            raise ValueError(f"at most {ops.ICP_MAX_ITERATIONS} iterations in all, got {sum(i for _, i in sched)}")
        if not distance_threshold > 0:
            raise ValueError(f"distance_threshold must be positive, got {distance_threshold}")
        if not 0 < angle_threshold_deg <= 180:
            raise ValueError(f"angle_threshold_deg must be in (0, 180], got {angle_threshold_deg}")
        if not normal_max_jump > 0:
            raise ValueError(f"normal_max_jump must be positive, got {normal_max_jump}")
        if min_correspondences < 1:
            raise ValueError(f"min_correspondences must be positive, got {min_correspondences}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.camera = (float(K_f[0, 0]), float(K_f[1, 1]), float(K_f[0, 2]), float(K_f[1, 2]))
        self.depth_scale = float(depth_scale)
        self.min_depth = float(min_depth)
        self.max_depth = float(max_depth)
        self.schedule = sched
        self.distance_threshold = float(distance_threshold)
        self.angle_threshold = math.radians(float(angle_threshold_deg))
        self.normal_max_jump = float(normal_max_jump)
        self.min_correspondences = int(min_correspondences)

    @torch.no_grad()
    def forward(self, depth1: torch.Tensor, depth2: torch.Tensor, R0: torch.Tensor | None = None, t0: torch.Tensor | None = None):
        single = depth1.dim() == 2
        d1 = RgbdPoseEstimator._frames(depth1, single, "depth1")
        d2 = RgbdPoseEstimator._frames(depth2, single, "depth2")
        if not d1.is_cuda:
            raise RuntimeError(f"DenseRgbdRefiner: depth must live on the GPU (got device {d1.device}); this package has no CPU path")
        if d1.shape != d2.shape:
            raise RuntimeError(f"depth1 and depth2 must have one shape, got {tuple(depth1.shape)} and {tuple(depth2.shape)}")
        b = int(d1.shape[0])
        r0 = torch.eye(3, device=d1.device).expand(b, 3, 3) if R0 is None else R0.reshape(-1, 3, 3)
        t0 = torch.zeros((b, 3), device=d1.device) if t0 is None else t0.reshape(-1, 3)
        k_inv = self.K_inv.to(d1.device)
        m1 = ops.surfel_maps(d1, k_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump)
        m2 = ops.surfel_maps(d2, k_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump)
        r, t, info, rmse, count, _, ok = ops.icp_refine(m1, m2, r0, t0, self.camera, self.schedule, self.distance_threshold,
                                                        self.angle_threshold, self.min_correspondences)
        out = (r, t, info, rmse, count, ok)
        return tuple(x[0] for x in out) if single else out
