"""K16 frame ingest without a GPU: the kernel's per-pixel functions (csrc/ingest_math.h), compiled for the host, against
the numpy oracle bit for bit; the host-side argument checks of mi_ingest_frames (MI_E_* before any launch); the Python
layers' refusal of CPU tensors and bad arguments; the `pytorch_model.ingest` alias; scale_intrinsics; the synthetic colour
frame; and the oracle's own sanity (identity at equal sizes, constants stay constant, < 1 gray level from a float64
bilinear resize)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import ingest_oracle as IO
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_colour_frame

NULL, SHAPE, PARAM = -1, -2, -3
BGR, RGB = 0, 1


# tests/native/ingest_host.cpp: frames ingested on the host by the kernel's own per-pixel functions
ingest_host = helpers.host_program("ingest_host.cpp", hip=True)


def run_host(exe, frames, height, width, channel_order):
    b, hs, ws, c = frames.shape
    head = f"{b} {hs} {ws} {c} {int(channel_order == 'rgb')} {height} {width}\n".encode()
    out = helpers.run_host(exe, [], head + np.ascontiguousarray(frames).tobytes(), binary=True)
    return np.frombuffer(out, np.uint8).reshape(b, 1, height, width)


@pytest.mark.parametrize("content", IO.CONTENTS)
@pytest.mark.parametrize("shape", IO.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_native_arithmetic_is_the_oracles_bit_for_bit(ingest_host, shape, content):
    (hs, ws), (h, w) = shape
    for channels, order in ((3, "bgr"), (3, "rgb"), (4, "bgr"), (1, "bgr")):
        frames = IO.make_frames(content, 2, hs, ws, channels, seed=11)
        got, want = run_host(ingest_host, frames, h, w, order), IO.ingest(frames, h, w, order)
        assert np.array_equal(got, want), (channels, order, int(np.abs(got.astype(int) - want).max()))


def test_native_arithmetic_on_a_real_ratio(ingest_host):
    """a 1080p-wide strip (the tap positions of the real 1920 -> 640 and 1080 -> 480 ratios) and a 16384-wide row (the
    cap: the largest tap position a float32 has to hold)"""
    for (hs, ws), (h, w) in (((27, 1920), (12, 640)), ((2, 16384), (3, 5461))):
        frames = IO.make_frames("noise", 1, hs, ws, 3, seed=12)
        assert np.array_equal(run_host(ingest_host, frames, h, w, "bgr"), IO.ingest(frames, h, w, "bgr"))


def test_argument_checks():
    lib = N.load()
    f = lib.mi_ingest_frames
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255          # a fake aligned "device" pointer: never dereferenced by a refused call

    def call(src=p, batch=2, sh=10, sw=12, c=3, rp=36, fp=360, order=BGR, dst=p, f32=0, h=5, w=6):
        return f(src, batch, sh, sw, c, rp, fp, order, dst, f32, h, w, None)
    assert call(src=None) == NULL and call(dst=None) == NULL
    for kw in (dict(batch=0), dict(sh=0), dict(sw=-1), dict(h=0), dict(w=0)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(c=2), dict(c=0), dict(c=5), dict(order=2), dict(order=-1), dict(rp=35), dict(fp=359),
               dict(batch=16385), dict(sh=16385, fp=36 * 16385), dict(sw=16385, rp=3 * 16385, fp=30 * 16385),
               dict(h=16385), dict(w=16385), dict(rp=(1 << 40) + 1, fp=1 << 50), dict(fp=(1 << 48) + 1)):
        assert call(**kw) == PARAM, kw
    assert call(src=None, batch=0, c=7) == NULL and call(batch=0, c=7) == SHAPE       # NULL before SHAPE before PARAM
    assert lib.mi_abi_version() == 3


def test_ops_and_module_refuse_cpu_tensors_and_bad_arguments():
    from onnx_image_processing_amd.pytorch_model.ingest import FrameIngest
    frames = torch.zeros(2, 10, 12, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_frames(frames, 5, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_frames(frames[0], 5, 6, out_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FrameIngest(5, 6)(frames)
    with pytest.raises(ValueError, match="channel_order"):
        ops.ingest_frames(frames, 5, 6, channel_order="gbr")
    with pytest.raises(ValueError, match="out_dtype"):
        ops.ingest_frames(frames, 5, 6, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="shape"):
        ops.ingest_frames(torch.zeros(2, 10, 12, 2, dtype=torch.uint8), 5, 6)
    with pytest.raises(RuntimeError, match="shape"):
        ops.ingest_frames(torch.zeros(10, 12, dtype=torch.uint8), 5, 6)
    m = FrameIngest(480, 640)
    assert (m.height, m.width, m.channel_order, m.out_dtype) == (480, 640, "bgr", torch.uint8)
    for args, kw in (((0, 640), {}), ((480, -1), {}), ((480, 20000), {}), ((480, 640), dict(channel_order="xyz")),
                     ((480, 640), dict(out_dtype=torch.int32))):
        with pytest.raises(ValueError):
            FrameIngest(*args, **kw)


def test_ingest_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.ingest as real
    from pytorch_model.ingest import FrameIngest, scale_intrinsics
    assert FrameIngest is real.FrameIngest and scale_intrinsics is real.scale_intrinsics
    from pytorch_model.ingest.frame_ingest import FrameIngest as again
    assert again is FrameIngest


def test_scale_intrinsics():
    from onnx_image_processing_amd.pytorch_model.geometry import RelativePoseEstimator
    from onnx_image_processing_amd.pytorch_model.ingest import scale_intrinsics
    K = torch.tensor([[1400.0, 0.0, 960.0], [0.0, 1410.0, 540.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    k = scale_intrinsics(K, (1080, 1920), (480, 640))
    want = torch.tensor([[1400.0 / 3, 0.0, 320.0], [0.0, 1410.0 * 480 / 1080, 240.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    assert k.dtype == torch.float64 and k.shape == (3, 3) and torch.allclose(k, want, rtol=1e-15, atol=0)
    assert torch.equal(scale_intrinsics(K, (480, 640), (480, 640)), K)                 # recomputed at equal sizes: unchanged
    assert torch.equal(K, torch.tensor([[1400.0, 0.0, 960.0], [0.0, 1410.0, 540.0], [0.0, 0.0, 1.0]], dtype=torch.float64))
    ki = scale_intrinsics([[500, 0, 320], [0, 500, 240], [0, 0, 1]], (480, 640), (240, 320))
    assert ki.dtype == torch.float32 and ki.tolist() == [[250.0, 0.0, 160.0], [0.0, 250.0, 120.0], [0.0, 0.0, 1.0]]
    assert RelativePoseEstimator(k).focal == pytest.approx((1400.0 / 3 + 1410.0 * 480 / 1080) / 2, rel=1e-6)
    with pytest.raises(ValueError, match="3x3"):
        scale_intrinsics(torch.eye(4), (480, 640), (240, 320))
    with pytest.raises(ValueError, match="positive"):
        scale_intrinsics(K, (0, 640), (240, 320))


def test_synth_colour_frame():
    a = synth_colour_frame(5, 240, 320)
    assert a.shape == (240, 320, 3) and a.dtype == np.uint8 and np.array_equal(a, synth_colour_frame(5, 240, 320))
    assert not np.array_equal(a, synth_colour_frame(6, 240, 320))
    assert synth_colour_frame(5, 31, 45, 4).shape == (31, 45, 4) and synth_colour_frame(5, 31, 45, 1).shape == (31, 45, 1)
    means = a.reshape(-1, 3).mean(0)
    assert means[2] < means[0] < means[1]                                               # the per-channel gains
    g = IO.ingest(a[None], 120, 160)[0, 0].astype(np.int64)
    assert np.abs(np.diff(g, axis=1)).max() > 60 and g.std() > 30                       # structure survives the ingest
    with pytest.raises(ValueError):
        synth_colour_frame(5, 8, 8, 2)


@pytest.mark.parametrize("content", IO.CONTENTS)
def test_oracle_sanity(content):
    worst = 0.0
    for (hs, ws), (h, w) in IO.SHAPES:
        for channels in (1, 3):
            frames = IO.make_frames(content, 2, hs, ws, channels, seed=13)
            g = IO.gray(frames)
            out = IO.resize_gray(g, h, w)
            if (hs, ws) == (h, w):
                assert np.array_equal(out, g)                                           # the identity at equal sizes
            worst = max(worst, float(np.abs(out - IO.bilinear_f64(g, h, w)).max()))
        for value in (0, 1, 127, 255):
            flat = np.full((1, hs, ws, 3), value, np.uint8)
            assert (IO.ingest(flat, h, w) == value).all()                               # gray of (v, v, v) is v; constants stay
    assert worst < 1.0, worst
    assert IO.gray(np.array([[[[255, 255, 255]]]], np.uint8)).item() == 255
    assert IO.gray(np.array([[[[10, 20, 30]]]], np.uint8), "bgr").item() != IO.gray(np.array([[[[10, 20, 30]]]], np.uint8), "rgb").item()
    s0, s1, w0, w1 = IO.taps(37, 48)
    assert s0[0] == 0 and w1[0] == 0 and s0[-1] == 36 and s1[-1] == 36 and w1[-1] == 0  # clamps on both borders
    assert (w0 + w1 >= 2047).all() and (w0 + w1 <= 2049).all()
