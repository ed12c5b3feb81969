"""Mirror of reference pytorch_model/threshold/otsu.py (OtsuThreshold): the K14 histogram, Otsu search and apply
kernels (`mi_histogram`, `mi_otsu_threshold`, `mi_threshold_apply`).  The reference's two BINS x BINS masks are not
built: an int64 prefix sum over the bins gives the same four sums per bin, and the float32 score follows the
reference's operation order, so `thresh` is the reference's value.  min_val is honoured and out-of-range values are
not counted (include/mi355x_match.h)."""
import torch
from torch import nn

from ... import ops


class OtsuThreshold(nn.Module):
    def __init__(self, min_val: int, max_val: int, dtype=torch.int32, device="cpu") -> None:
        super().__init__()
        self.min_val = int(min_val)
        self.max_val = int(max_val)
        self.BINS = self.max_val - self.min_val + 1
        if self.BINS < 1 or self.BINS > ops.THRESHOLD_MAX_BINS:
            raise ValueError(f"max_val - min_val + 1 = {self.BINS} bins: between 1 and {ops.THRESHOLD_MAX_BINS}")
        if dtype not in (torch.uint8, torch.int32, torch.float32):
            raise ValueError(f"dtype of bin_img must be uint8, int32 or float32, got {dtype}")
        self.dtype = dtype
        self.device = device

    def forward(self, img_HxW: torch.Tensor):
        """img_HxW: (H, W) uint8, uint16, int32 or float32 on the GPU -> (thresh int64 (), bin_img (H, W) in self.dtype);
        (B, H, W) -> (thresh (B,), bin_img (B, H, W)).  No synchronisation."""
        thresh, bin_img = ops.otsu(img_HxW, self.min_val, self.max_val, self.dtype)
        return thresh.to(torch.int64), bin_img
