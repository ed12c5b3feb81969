"""Mirror of reference pytorch_model/threshold/multi_otsu.py (MultiOtsuThreshold): the K14 histogram and combination
search kernels (`mi_histogram`, `mi_multi_otsu_threshold`).  The reference's (n_class, COMBINATIONS, BINS) mask is not
built: every candidate's class sums come from two int64 prefix sums, scored in fp64 in a fixed order; the result is the
argmax with torch.argmax's first-maximum rule in itertools.combinations order (include/mi355x_match.h)."""
import torch
from torch import nn

from ... import ops


class MultiOtsuThreshold(nn.Module):
    DTYPE = torch.float32          # the reference's score type; the search here scores in fp64

    def __init__(self, min_val: int, max_val: int, device="cpu", n_class=3, calc_hist=False) -> None:
        super().__init__()
        self.min_val = int(min_val)
        self.max_val = int(max_val)
        self.BINS = self.max_val - self.min_val
        self.device = device
        self.n_class = int(n_class)
        self.calc_hist = calc_hist
        self.COMBINATIONS = ops.multi_otsu_combinations(self.BINS, self.n_class)      # ValueError outside the limits

    def calc_histogram(self, img_HxW: torch.Tensor) -> torch.Tensor:
        """int64 counts (BINS,) / (B, BINS) of the values min_val .. max_val - 1; anything else is not counted"""
        return ops.histogram(img_HxW, self.min_val, self.BINS)

    def forward(self, input: torch.Tensor):
        """calc_hist=True: an image (H, W) or a batch (B, H, W) on the GPU; otherwise a histogram of counts (BINS,) or
        (B, BINS).  Returns a list of n_class - 1 int64 thresholds, each () or (B,): the inclusive upper bounds of the
        classes.  No synchronisation."""
        if self.calc_hist:
            hist = self.calc_histogram(input)
        else:
            if not input.is_cuda:
                raise RuntimeError(f"hist must live on the GPU (got device {input.device}); this package has no CPU path")
            if input.shape[-1] != self.BINS:
                raise RuntimeError(f"hist must have {self.BINS} bins, got shape {tuple(input.shape)}")
            hist = input if input.dtype == torch.int64 else input.to(torch.int64)
        th = ops.multi_otsu_threshold(hist, self.min_val, self.n_class).to(torch.int64)
        return [th[..., k] for k in range(self.n_class - 1)]
