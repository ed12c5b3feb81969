"""DisparityFilter -- the two post-filters of a disparity map a cv2.StereoSGBM user has: a k x k median over the valid
disparities, then the speckle filter (components of at most `speckle_size` pixels whose neighbours differ by at most
`speckle_range` are dropped).  K35: `mi_filter_median`, `mi_filter_speckle`; stated in include/mi355x_match_filter.h.  Both are
off by default: on the library's synthetic scenes the median does not lower the bad-pixel count, and the speckle filter earns
its place on textureless surfaces."""
import torch
from torch import nn

from ... import ops


class DisparityFilter(nn.Module):
    """forward(disparity, code=None) -> (disparity, code): float32 disparities (B, H, W) or (B, 1, H, W) as StereoMatcher returns
    them (-1 on a rejected pixel, valid from 0).  median = 0 (off), 3 or 5 runs first; speckle_size > 0 then drops every
    component of at most speckle_size pixels (speckle_size = 0: off) and, where `code` is given, writes ops.FILTER_SPECKLE on the
    valid pixels it dropped (into a copy: the argument is left as it is)."""

    def __init__(self, speckle_size: int = 0, speckle_range: float = 1.0, median: int = 0) -> None:
        super().__init__()
        if int(speckle_size) != speckle_size or speckle_size < 0:
            raise ValueError(f"speckle_size must be an integer >= 0, got {speckle_size}")
        if not (0.0 <= float(speckle_range) < float("inf")):
            raise ValueError(f"speckle_range must be finite and >= 0, got {speckle_range}")
        if median not in (0,) + ops.FILTER_MEDIANS:
            raise ValueError(f"median must be 0 or one of {ops.FILTER_MEDIANS}, got {median}")
        self.speckle_size, self.speckle_range, self.median = int(speckle_size), float(speckle_range), int(median)

    @property
    def active(self) -> bool:
        return self.speckle_size > 0 or self.median > 0

    @torch.no_grad()
    def forward(self, disparity: torch.Tensor, code: torch.Tensor | None = None):
        if code is not None and code.shape != disparity.shape:
            raise RuntimeError(f"disparity and code differ in shape: {tuple(disparity.shape)} and {tuple(code.shape)}")
        if self.median:
            disparity = ops.filter_median(disparity, self.median, 0.0, -1.0)
        if self.speckle_size > 0:
            disparity, removed = ops.filter_speckle(disparity, self.speckle_size, self.speckle_range, 0.0, -1.0, want_removed=True)
            if code is not None:
                code = torch.where(removed != 0, torch.full_like(code, ops.FILTER_SPECKLE), code)
        return disparity, code
