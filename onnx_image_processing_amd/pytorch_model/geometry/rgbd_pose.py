"""RgbdPoseEstimator -- the metric counterpart of RelativePoseEstimator for cameras that deliver depth (the reference's
camera back ends: RealSense, Orbbec, OAK).  Matched keypoints are lifted through the two aligned depth frames to 3-D and
the rigid motion between the frames is estimated by 3-point RANSAC, so the translation comes out in the depth's units
instead of at unit length.  K17: `mi_lift_keypoints`, `mi_rigid_ransac`; the algorithm is stated in
include/mi355x_match.h.  The reference has no counterpart (its odometry sample sums unit translations)."""
import torch
from torch import nn

from ... import ops


class RgbdPoseEstimator(nn.Module):
    """forward(keypoints1, keypoints2, depth1, depth2, valid=None) -> (R, t, inlier_mask, rmse, ok) for matched keypoints
    (B, N, 2) in pixel (y, x) order, the order MatchExtractionWrapper returns, and the depth frames (B, H, W) or (B, 1, H, W)
    of the two images, float32 or uint16, ALREADY aligned to the camera of K (DepthAlignment); `valid` (B, N) selects the real
    matches of a padded batch.  X2 = R X1 + t with det R = +1 and t in the units of depth * depth_scale (the direction
    convention of RelativePoseEstimator); inlier_mask marks the matches within distance_threshold of that motion, rmse is
    their root-mean-square distance; ok is False -- with R = identity, t = 0, no inliers -- where fewer than 3 matches have
    usable depth in both frames or no sample explains 3 of them.  (N, 2) keypoints with (H, W) or (1, H, W) depth give
    unbatched output.

    K: the 3x3 camera matrix.  depth_scale turns a depth value into the unit of the result (0.001 for millimetre counts and
    metres); matches whose depth falls outside [min_depth, max_depth] in either frame are ignored.  num_hypotheses 3-point
    samples are drawn per pair by the counter-based sampler from `seed`; distance_threshold is the inlier distance in the
    unit of the result; refine_rounds rounds of refit-on-inliers follow the selection."""

    def __init__(self, K: torch.Tensor, depth_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                 num_hypotheses: int = 128, distance_threshold: float = 0.05, refine_rounds: int = 3, seed: int = 0) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        if not depth_scale > 0:
            raise ValueError(f"depth_scale must be positive, got {depth_scale}")
        if not min_depth > 0 or not max_depth >= min_depth:
            raise ValueError(f"need 0 < min_depth <= max_depth, got {min_depth}, {max_depth}")
        if num_hypotheses < 1:
            raise ValueError(f"num_hypotheses must be positive, got {num_hypotheses}")
        if not distance_threshold > 0:
            raise ValueError(f"distance_threshold must be positive, got {distance_threshold}")
        if not 0 <= refine_rounds <= ops.POSE_MAX_REFINE_ROUNDS:
            raise ValueError(f"refine_rounds must be in 0 .. {ops.POSE_MAX_REFINE_ROUNDS}, got {refine_rounds}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.depth_scale = float(depth_scale)
        self.min_depth = float(min_depth)
        self.max_depth = float(max_depth)
        self.num_hypotheses = int(num_hypotheses)
        self.distance_threshold = float(distance_threshold)
        self.refine_rounds = int(refine_rounds)
        self.seed = int(seed)

    @staticmethod
    def _frames(depth: torch.Tensor, single: bool, what: str) -> torch.Tensor:
        d = depth
        if single and d.dim() == 2:
            d = d.unsqueeze(0)
        elif not single and d.dim() == 4 and d.shape[1] == 1:
            d = d[:, 0]
        if d.dim() != 3:
            raise RuntimeError(f"{what} must be (B, H, W) or (B, 1, H, W), got {tuple(depth.shape)}")
        return d

    @torch.no_grad()
    def forward(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, depth1: torch.Tensor, depth2: torch.Tensor,
                valid: torch.Tensor | None = None):
        single = keypoints1.dim() == 2
        k1 = keypoints1.unsqueeze(0) if single else keypoints1
        k2 = keypoints2.unsqueeze(0) if single else keypoints2
        v = valid.unsqueeze(0) if (single and valid is not None) else valid
        if k1.dim() != 3 or k1.shape[-1] != 2 or k1.shape != k2.shape:
            raise RuntimeError(f"keypoints must both be (B, N, 2) or (N, 2), got {tuple(keypoints1.shape)}, {tuple(keypoints2.shape)}")
        d1, d2 = self._frames(depth1, single, "depth1"), self._frames(depth2, single, "depth2")
        k_inv = self.K_inv.to(k1.device)
        x1, v1 = ops.lift_keypoints(k1, d1, k_inv, self.depth_scale, self.min_depth, self.max_depth, v)
        x2, v2 = ops.lift_keypoints(k2, d2, k_inv, self.depth_scale, self.min_depth, self.max_depth, v1)
        r, t, inlier, _, _, rmse, ok = ops.rigid_ransac(x1, x2, v2, self.num_hypotheses, self.distance_threshold,
                                                        self.refine_rounds, self.seed)
        out = (r, t, inlier, rmse, ok)
        return tuple(x[0] for x in out) if single else out
