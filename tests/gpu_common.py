"""Shared by the GPU test files: the device, the marks, array upload, bit views and repeat checks, the event timer, the
module fixture.  Importing this module needs torch but no GPU: nothing here touches the device before a test calls it."""
import os

import numpy as np
import pytest
import torch

from onnx_image_processing_amd.synth import synth_batch, synth_image  # noqa: F401

DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_NEEDS_GPU = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
GPU = [pytest.mark.gpu, _NEEDS_GPU]                 # pytestmark of a test_gpu_*.py
GPU_PERF = [pytest.mark.gpu_perf, _NEEDS_GPU]       # pytestmark of a test_gpu_*_perf.py


def _status_word(state) -> int:
    """The status word of the mi_sinkhorn_dots call behind `state` (ops.sinkhorn_bits(..., return_state=True)): it lives
    inside the call's workspace; 0 = solved."""
    work, addr = state[4]
    torch.cuda.synchronize()
    return int(work.view(torch.int32)[(addr - work.data_ptr()) // 4].item())


def gpu(*arrays):
    """numpy arrays on the device: one array gives a tensor, several a tuple; None stays None.  A read-only array (the
    oracles cache theirs) is copied first, since torch.from_numpy wants a writable one."""
    def one(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)
    out = tuple(None if a is None else one(a) for a in arrays)
    return out[0] if len(out) == 1 else out


def k_inv(K):
    """the inverse of a camera matrix, float32 on the device, as the entries take it"""
    return torch.from_numpy(np.linalg.inv(K)).float().to(DEV)


def up(x, k):
    return (x + k - 1) // k * k


def bits(x):
    """the bytes of a tensor or of a numpy array"""
    return x.contiguous().view(torch.uint8) if isinstance(x, torch.Tensor) else np.ascontiguousarray(x).view(np.uint8)


def same_bits(a, b):
    """two sequences of tensors, pairwise equal byte for byte (NaN included)"""
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def twice(what, run):
    """run() -> tuple of numpy arrays (None entries are skipped); called twice, the results must be equal bit for bit.
    Returns the first."""
    first, second = run(), run()
    for x, y in zip(first, second):
        if x is not None:
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: the call does not repeat bit for bit"
    return first


def time_ms(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return float(np.median(times))


@pytest.fixture(scope="module")
def mods():
    from onnx_image_processing_amd import _native
    from onnx_image_processing_amd.pytorch_model.descriptor.bad import SparseBAD
    from onnx_image_processing_amd.pytorch_model.detector import ShiTomasiScore
    from onnx_image_processing_amd.pytorch_model.feature_detection import (
        MatchExtractionWrapper, ShiTomasiSparseBADSinkhornMatcher)
    from onnx_image_processing_amd.pytorch_model.matching import SinkhornMatcher, SinkhornMatcherWithScores
    from onnx_image_processing_amd.pytorch_model.matching.match_extraction import MutualNearestNeighborMatcher
    from onnx_image_processing_amd.pytorch_model.utils import apply_nms_maxpool, select_topk_keypoints
    from onnx_image_processing_amd.pytorch_model.utils.keypoint_utils import detect_keypoints
    _native.load()     # fail loudly if the HIP library is missing
    return dict(locals())


def _images(g):
    a, b = synth_batch(int(g["seed"]), 1, int(g["h"]), int(g["w"]), noise=int(g["noise"]))
    if int(g["blank"][0]) >= 0:
        y0, y1, x0, x1 = [int(v) for v in g["blank"]]
        b[:, :, y0:y1, x0:x1] = 77.0
    return a, b
