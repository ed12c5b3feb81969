"""FeatureTracker -- the KLT front end: the keypoints of one frame followed into the next by pyramidal Lucas-Kanade, the
forward-backward test and the refill of lost slots with fresh corners.  K32: `mi_flow_pyramid`, `mi_flow_track`,
`mi_flow_check`, `mi_flow_replenish`; the algorithm is stated in include/mi355x_match_flow.h.  The reference has no
counterpart (its hosts call cv2.calcOpticalFlowPyrLK on the CPU)."""
import torch
from torch import nn

from ... import ops


class FeatureTracker(nn.Module):
    """pyramid(frames) -> the pyramid of gray frames (B, H, W) or (B, 1, H, W), uint8 or float32: build it once per frame and
    keep it for the next pair.
    track(pyr1, pyr2, keypoints1, guess=None) -> (keypoints2 (B, K, 2) pixel (y, x), status (B, K) bool, residual (B, K)): a
    slot keeps its index from frame to frame, a lost one is (-1, -1) with status False.  guess (B, K, 2): a predicted
    displacement (dy, dx).  With fb_threshold > 0 the result is tracked back into frame 1 and a point that does not return
    within fb_threshold pixels is lost: the only test that catches a track which slid onto other texture, since every sample
    is clamped into the frame and the tracker by itself loses almost nothing.  track_full(...) also returns the codes, the
    iteration counts and the forward-backward distance.
    matches(status) -> (match_ij (B, K, 2) int32 with rows (k, k), match_valid (B, K)): the form LandmarkTracks takes per
    frame pair.
    replenish(keypoints, status, candidates, cand_count, height, width) -> (keypoints (B, K, 2), is_new (B, K), counts
    (B, 3)): lost slots refilled from score-descending corners, one per free cell of `cell` pixels."""

    def __init__(self, levels: int = 3, radius: int = 7, max_iterations: int = 30, epsilon: float = 0.01, min_eigen: float = 1e-3,
                 fb_threshold: float = 0.0, cell: int = 16) -> None:
        super().__init__()
        if not 1 <= levels <= ops.FLOW_MAX_LEVELS:
            raise ValueError(f"levels must be in 1 .. {ops.FLOW_MAX_LEVELS}, got {levels}")
        if not 1 <= radius <= ops.FLOW_MAX_RADIUS:
            raise ValueError(f"radius must be in 1 .. {ops.FLOW_MAX_RADIUS}, got {radius}")
        if not 1 <= max_iterations <= ops.FLOW_MAX_ITERATIONS:
            raise ValueError(f"max_iterations must be in 1 .. {ops.FLOW_MAX_ITERATIONS}, got {max_iterations}")
        if not 0 < epsilon < float("inf"):
            raise ValueError(f"epsilon must be positive and finite, got {epsilon}")
        if not 0 <= min_eigen < float("inf"):
            raise ValueError(f"min_eigen must be non-negative and finite, got {min_eigen}")
        if not 0 <= fb_threshold < float("inf"):
            raise ValueError(f"fb_threshold must be non-negative and finite, got {fb_threshold}")
        if cell < 1:
            raise ValueError(f"cell must be positive, got {cell}")
        self.levels, self.radius, self.max_iterations = int(levels), int(radius), int(max_iterations)
        self.epsilon, self.min_eigen, self.fb_threshold, self.cell = float(epsilon), float(min_eigen), float(fb_threshold), int(cell)

    @torch.no_grad()
    def pyramid(self, frames: torch.Tensor) -> ops.FlowPyramid:
        return ops.flow_pyramid(frames, self.levels)

    def _track(self, a, b, kp, guess):
        return ops.flow_track(a, b, kp, guess, self.radius, self.max_iterations, self.epsilon, self.min_eigen)

    @torch.no_grad()
    def track_full(self, pyr1: ops.FlowPyramid, pyr2: ops.FlowPyramid, keypoints1: torch.Tensor, guess: torch.Tensor | None = None):
        """-> (keypoints2, status, residual, code, iterations, fb_distance or None)"""
        kp2, status, code, residual, iterations = self._track(pyr1, pyr2, keypoints1, guess)
        fb = None
        if self.fb_threshold > 0:
            back, status_b = self._track(pyr2, pyr1, kp2, None if guess is None else -guess)[:2]
            status, fb = ops.flow_check(keypoints1, back, status, status_b, self.fb_threshold)
            kp2 = torch.where(status[..., None], kp2, torch.full_like(kp2, -1.0))
            residual = torch.where(status, residual, torch.zeros_like(residual))
        return kp2, status, residual, code, iterations, fb

    def track(self, pyr1: ops.FlowPyramid, pyr2: ops.FlowPyramid, keypoints1: torch.Tensor, guess: torch.Tensor | None = None):
        return self.track_full(pyr1, pyr2, keypoints1, guess)[:3]

    forward = track

    @staticmethod
    def matches(status: torch.Tensor):
        if not status.is_cuda:
            raise RuntimeError(f"status must live on the GPU (got device {status.device}); this package has no CPU path")
        k = status.shape[-1]
        idx = torch.arange(k, dtype=torch.int32, device=status.device)
        return idx[:, None].expand(*status.shape, 2).contiguous(), status != 0

    @torch.no_grad()
    def replenish(self, keypoints: torch.Tensor, status: torch.Tensor, candidates: torch.Tensor, cand_count: torch.Tensor | None,
                  height: int, width: int):
        return ops.flow_replenish(keypoints, status, candidates, cand_count, height, width, self.cell)
