"""StereoMatcher -- a rectified stereo pair to a disparity map and a depth frame: census transform, semi-global aggregation of
the Hamming cost, winner-take-all with a uniqueness test and a left-right check, a parabola sub-pixel step, depth = f b / d.
K33: `mi_stereo_census`, `mi_stereo_aggregate`, `mi_stereo_select`, `mi_stereo_depth`; the algorithm is stated in
include/mi355x_match_stereo.h.  The reference has no module for it (its OAK-D back end turns the camera's own StereoDepth on;
a host with a plain rig calls cv2.StereoSGBM on the CPU)."""
import torch
from torch import nn

from ... import ops
from .disparity_filter import DisparityFilter


class StereoMatcher(nn.Module):
    """forward(left, right) -> (disparity float32, code uint8): gray views (B, H, W) or (B, 1, H, W), uint8 or float32, RECTIFIED
    (a scene point lies on one row of both views, at x_right = x_left - d, d >= 0); the outputs have the shape of `left`.
    disparity is d* plus a sub-pixel offset in [-0.5, 0.5], or -1 on a rejected pixel; code is ops.STEREO_OK,
    ops.STEREO_NOT_UNIQUE or ops.STEREO_LR.  uniqueness = 0 and lr_max_diff < 0 turn the two tests off.
    depth(disparity, fx, baseline, min_disparity=0.5) -> fx * baseline / disparity in the baseline's unit, 0 where the
    disparity is below min_disparity (rejected pixels among them): the frame DepthToPointCloud, TsdfVolume.integrate and the
    RGB-D estimators read.
    speckle_size, speckle_range, median: DisparityFilter's arguments (K35), off by default; with one of them on, forward applies
    the filter to its result and code is ops.FILTER_SPECKLE on a pixel the speckle filter dropped."""

    def __init__(self, max_disparity: int = 128, p1: int = 10, p2: int = 120, paths: int = 8, uniqueness: int = 10,
                 lr_max_diff: int = 1, speckle_size: int = 0, speckle_range: float = 1.0, median: int = 0) -> None:
        super().__init__()
        if max_disparity not in ops.STEREO_DISPARITIES:
            raise ValueError(f"max_disparity must be one of {ops.STEREO_DISPARITIES}, got {max_disparity}")
        if not 0 <= p1 <= p2 <= 255:
            raise ValueError(f"the penalties must satisfy 0 <= p1 <= p2 <= 255, got {p1}, {p2}")
        if paths not in (4, 8):
            raise ValueError(f"paths must be 4 or 8, got {paths}")
        if not 0 <= uniqueness <= 100:
            raise ValueError(f"uniqueness must be in 0 .. 100, got {uniqueness}")
        self.max_disparity, self.p1, self.p2, self.paths = int(max_disparity), int(p1), int(p2), int(paths)
        self.uniqueness, self.lr_max_diff = int(uniqueness), int(lr_max_diff)
        self.filter = DisparityFilter(speckle_size, speckle_range, median)

    @torch.no_grad()
    def volume(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """the aggregated sums S (B, H, W, max_disparity) uint16"""
        return ops.stereo_aggregate(ops.stereo_census(left), ops.stereo_census(right), self.max_disparity, self.paths, self.p1, self.p2)

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor):
        if left.shape != right.shape:
            raise RuntimeError(f"the two views differ in shape: {tuple(left.shape)} and {tuple(right.shape)}")
        disparity, _, code = ops.stereo_select(self.volume(left, right), self.uniqueness, self.lr_max_diff, want_right=self.lr_max_diff >= 0)
        if self.filter.active:
            disparity, code = self.filter(disparity, code)
        return disparity.view(left.shape), code.view(left.shape)

    @torch.no_grad()
    def depth(self, disparity: torch.Tensor, fx: float, baseline: float, min_disparity: float = 0.5) -> torch.Tensor:
        return ops.stereo_depth(disparity, float(fx) * float(baseline), min_disparity)
