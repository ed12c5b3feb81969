"""K16 frame ingest on the GPU: every case bit-exact against the numpy restatement of the header's arithmetic
(tests/ingest_oracle.py).  Runs unchanged under MI_POISON_EMPTY=1 (every output comes from torch.empty: a byte the kernel
does not write, or a write outside the output, fails the case)."""
import numpy as np
import pytest
import torch

import ingest_oracle as IO
from gpu_common import DEV, GPU, gpu
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_colour_frame

pytestmark = GPU


def _check(frames_np, frames_gpu, h, w, order="bgr"):
    """both output types against the oracle; the float32 output is the uint8 output cast"""
    want = IO.ingest(frames_np, h, w, order)
    got8 = ops.ingest_frames(frames_gpu, h, w, channel_order=order)
    got32 = ops.ingest_frames(frames_gpu, h, w, channel_order=order, out_dtype=torch.float32)
    assert got8.dtype == torch.uint8 and got32.dtype == torch.float32 and got8.shape == got32.shape == want.shape
    g8 = got8.cpu().numpy()
    assert np.array_equal(g8, want), f"{int((g8 != want).sum())} of {want.size} bytes differ, max {int(np.abs(g8.astype(int) - want).max())}"
    assert torch.equal(got32, got8.float())
    return got8


@pytest.mark.parametrize("content", IO.CONTENTS)
@pytest.mark.parametrize("shape", IO.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_shapes_bit_exact(shape, content):
    (hs, ws), (h, w) = shape
    frames = IO.make_frames(content, 3, hs, ws, 3, seed=21)
    _check(frames, gpu(frames), h, w)


# one same-size shape, one downscale with vector stores, one upscale with the scalar-store tail: with 1, 3 and 4 channels
# they reach each of the six kernel instantiations (channels x {same size, resize}) on both store paths
@pytest.mark.parametrize("shape", [((48, 64), (48, 64)), ((48, 61), (48, 61)), ((108, 192), (48, 64)), ((37, 53), (48, 67))],
                         ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_channels_and_orders(channels, order, shape):
    (hs, ws), (h, w) = shape
    frames = IO.make_frames("noise", 3, hs, ws, channels, seed=22)
    got = _check(frames, gpu(frames), h, w, order)
    if channels == 3 and order == "rgb":
        assert not np.array_equal(got.cpu().numpy(), IO.ingest(frames, h, w, "bgr"))       # the order is honoured
    single = ops.ingest_frames(gpu(frames[1]), h, w, channel_order=order)                # a 3-D input is B = 1
    assert single.shape == (1, 1, h, w) and torch.equal(single[0], got[1])


@pytest.mark.parametrize("shape", [((135, 241), (30, 40)), ((37, 53), (37, 53)), ((37, 53), (48, 64))],
                         ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_pitched_crop_view_goes_in_without_a_copy(shape):
    """a (3, Hs, Ws, 3) crop at an odd byte offset inside a larger buffer, odd row and frame pitches: the same result as
    the contiguous copy whatever the buffer's other bytes hold"""
    (hs, ws), (h, w) = shape
    frames = IO.make_frames("noise", 3, hs, ws, 3, seed=23)
    row_pitch = ws * 3 + 13
    frame_pitch = hs * row_pitch + 101
    want = IO.ingest(frames, h, w)
    for fill in (0xFF, 0x00):
        buf = torch.full((7 + 3 * frame_pitch + 64,), fill, dtype=torch.uint8, device=DEV)
        view = torch.as_strided(buf, (3, hs, ws, 3), (frame_pitch, row_pitch, 3, 1), 7)
        view.copy_(gpu(frames))
        assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
        before = buf.clone()
        got = ops.ingest_frames(view, h, w)
        assert np.array_equal(got.cpu().numpy(), want), fill
        assert torch.equal(buf, before)
    # a view the entry cannot take by its strides (channels-first storage) is made contiguous first
    chw = gpu(np.ascontiguousarray(frames.transpose(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert np.array_equal(ops.ingest_frames(chw, h, w).cpu().numpy(), want)


def test_one_real_size():
    frames = IO.make_frames("noise", 2, 1080, 1920, 3, seed=24)
    _check(frames, gpu(frames), 480, 640)


def test_capture_and_replay():
    """a linear torch.cuda.graph around ops.ingest_frames on static buffers, replayed with two different contents"""
    hs, ws, h, w = 108, 192, 48, 64
    first = IO.make_frames("noise", 3, hs, ws, 3, seed=25)
    second = IO.make_frames("checker", 3, hs, ws, 3, seed=26)
    static = gpu(first)
    ops.ingest_frames(static, h, w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ingest_frames(static, h, w, out_dtype=torch.float32)
    for frames in (first, second):
        static.copy_(gpu(frames))
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), IO.ingest(frames, h, w).astype(np.float32))


def test_ingested_frames_match_like_the_oracles():
    """colour frame pairs -> ingest -> mi_match_pairs_u8 with the parameters of the small default golden case (K = 64,
    max_matches 20, threshold 0.01; hard bits, which the single call requires): every output identical to the same call
    on the oracle's ingested frames, and the comparison is not empty against empty"""
    from onnx_image_processing_amd.pytorch_model.feature_detection import (
        MatchExtractionWrapper, ShiTomasiSparseBADSinkhornMatcher)
    from onnx_image_processing_amd.pytorch_model.ingest import FrameIngest
    a = np.stack([synth_colour_frame(2000 + i, 240, 320) for i in range(2)])
    b = np.roll(a, shift=(6, 10), axis=(1, 2))
    ingest = FrameIngest(120, 160)
    a8, b8 = ingest(gpu(a)), ingest(gpu(b))
    ra, rb = IO.ingest(a, 120, 160), IO.ingest(b, 120, 160)
    assert np.array_equal(a8.cpu().numpy(), ra) and np.array_equal(b8.cpu().numpy(), rb)
    fm = ShiTomasiSparseBADSinkhornMatcher(max_keypoints=64, binarize=True, soft_binarize=False).to(DEV)
    wrap = MatchExtractionWrapper(fm, 20, 0.01)
    d = fm.descriptor
    prm = dict(block_size=fm.corner_detector.block_size, nms_radius=fm.nms_radius, max_keypoints=fm.max_keypoints,
               score_threshold=fm.score_threshold, border_margin=fm.border_margin, pair_geom=d.pair_geom, pair_thr=d.pair_thr,
               plan=d._get_plan(), normalize_descriptors=d.normalize_descriptors, epsilon=fm.matcher.epsilon,
               unused_score=fm.matcher.unused_score, sinkhorn_iterations=fm.matcher.iterations,
               max_matches=wrap.match_extractor.max_matches, match_threshold=wrap.match_extractor.threshold)
    got = ops.match_pairs(a8, b8, **prm)
    want = ops.match_pairs(gpu(ra), gpu(rb), **prm)
    for g, r in zip(got, want):
        assert torch.equal(g, r)
    valid = got[5]
    assert int(valid.sum()) >= 2 * 5, int(valid.sum())
    assert int((got[0][:, :, 0] >= 0).sum()) >= 2 * 32                                    # corners were found after the ingest
