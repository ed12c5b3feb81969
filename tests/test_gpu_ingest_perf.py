"""K16 rate: mi_ingest_frames on 16 colour frames in one call (1080x1920x3 -> 480x640, and 480x640x3 at the model's size)
beats the best of two torch-on-GPU formulations of the same step written here from stock ops -- what a user with frames
in device memory has to do without it: (a) the frame to float32, the integer-weighted channel sum there, F.interpolate
(bilinear, align_corners=False), round and clamp; (b) the gray image in integers first, so that only one channel goes to
float32.  Both are first checked to compute the same thing (within 1 gray level on >= 99 % of the pixels)."""
import numpy as np
import torch
import torch.nn.functional as F

from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_colour_frame

pytestmark = GPU_PERF
FRAMES = 16
WORKLOADS = {"1080x1920x3 -> 480x640": ((1080, 1920), (480, 640)), "480x640x3 -> 480x640": ((480, 640), (480, 640))}
WEIGHTS = (3735.0, 19235.0, 9798.0)


def torch_float_first(frames, h, w, weights):
    """(a): float32 copy of the whole frame, weighted channel sum, bilinear resize, round, clamp"""
    g = torch.floor(((frames.float() * weights).sum(-1) + 16384.0) / 32768.0)
    r = F.interpolate(g[:, None], size=(h, w), mode="bilinear", align_corners=False)
    return r.round().clamp(0, 255).to(torch.uint8)


def torch_gray_first(frames, h, w, weights):
    """(b): gray in int32 (exactly the header's), one channel to float32, bilinear resize, round, clamp"""
    f = frames.to(torch.int32)
    g = (3735 * f[..., 0] + 19235 * f[..., 1] + 9798 * f[..., 2] + 16384) >> 15
    r = F.interpolate(g.float()[:, None], size=(h, w), mode="bilinear", align_corners=False)
    return r.round().clamp(0, 255).to(torch.uint8)


FORMULATIONS = {"float first": torch_float_first, "gray first": torch_gray_first}


def workload(src_size, frames=FRAMES, seed=700):
    """(frames, Hs, Ws, 3) uint8 on the GPU: 4 distinct synthetic colour frames, repeated"""
    distinct = [synth_colour_frame(seed + i, *src_size) for i in range(min(4, frames))]
    return torch.from_numpy(np.stack([distinct[i % len(distinct)] for i in range(frames)])).to(DEV)


def traffic_bytes(frames, h, w, out_bytes=1):
    return frames.numel() + frames.shape[0] * h * w * out_bytes


def test_torch_formulations_compute_the_same_thing():
    weights = torch.tensor(WEIGHTS, device=DEV)
    for name, (src, (h, w)) in WORKLOADS.items():
        frames = workload(src, 2)
        hip = ops.ingest_frames(frames, h, w).to(torch.int32)
        for fname, fn in FORMULATIONS.items():
            close = ((fn(frames, h, w, weights).to(torch.int32) - hip).abs() <= 1).float().mean().item()
            print(f"{name}: '{fname}' within 1 gray level of the HIP output on {100 * close:.3f} % of the pixels")
            assert close >= 0.99, (name, fname, close)


def test_hip_ingest_beats_torch_on_gpu_for_sixteen_frames():
    weights = torch.tensor(WEIGHTS, device=DEV)
    failed = []
    for name, (src, (h, w)) in WORKLOADS.items():
        frames = workload(src)
        hip = time_ms(lambda: ops.ingest_frames(frames, h, w))
        refs = {k: time_ms(lambda: fn(frames, h, w, weights)) for k, fn in FORMULATIONS.items()}
        best = min(refs, key=refs.get)
        print(f"{name}: 16 frames HIP {hip:.4f} ms ({traffic_bytes(frames, h, w) / hip / 1e6:.0f} GB/s of source + destination); "
              + "torch-on-GPU " + ", ".join(f"{k} {v:.3f} ms" for k, v in refs.items())
              + f"; yardstick: {best} ({refs[best] / hip:.1f}x)")
        if not hip < refs[best]:
            failed.append(name)
    assert not failed, failed
