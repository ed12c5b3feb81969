"""K28 rate on the GPU: mi_tracks_build and mi_tracks_triangulate for a batch of windows.

    python tools/tracks_bench.py [--windows 256] [--frames 8] [--keypoints 512] [--landmarks 400] [--span 2] [--slots 512] [--iters 10]
                                 [--embed]

The windows are synth_track_window's: a planted scene, 10 % wrong matches, lists padded with garbage.  --embed times the same
matches once more inside the largest node layout (16 frames x 1024 keypoints: 128 KiB of labels in LDS, one workgroup per CU)
-- what the LDS budget of the largest shape costs a window that does not need it.  Prints one JSON line: median milliseconds
per entry, windows per second and the mean counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_common import time_ms                                                         # noqa: E402
from onnx_image_processing_amd import ops                                              # noqa: E402
from onnx_image_processing_amd.synth import rgbd_camera, synth_track_window            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--landmarks", type=int, default=400)
    ap.add_argument("--span", type=int, default=2)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--embed", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    s = [synth_track_window(700 + i, a.frames, a.keypoints, a.landmarks, pair_span=a.span) for i in range(min(8, a.windows))]
    kp, pf, ij, mv, r, t = (torch.from_numpy(np.ascontiguousarray(np.stack([s[i % len(s)][j] for i in range(a.windows)]))).to(dev)
                            for j in (0, 2, 3, 4, 5, 6))
    t_build = time_ms(lambda: ops.tracks_build(kp, pf, ij, mv, None, 2, a.slots), a.iters)
    out = ops.tracks_build(kp, pf, ij, mv, None, 2, a.slots)
    cam = rgbd_camera()
    focal = float((cam[0, 0] + cam[1, 1]) / 2)
    obs = ops.normalise_keypoints(out[2], torch.from_numpy(np.linalg.inv(cam)).float().to(dev))
    args = (r, t, obs, out[1], 2, (3.0 / focal) ** 2, float(np.cos(np.radians(1.0))))
    t_tri = time_ms(lambda: ops.tracks_triangulate(*args), a.iters)
    ok = ops.tracks_triangulate(*args)[1]
    res = dict(windows=a.windows, frames=a.frames, keypoints=a.keypoints, pairs=int(pf.shape[1]), matches=int(mv.shape[2]), slots=a.slots,
               build_ms=round(t_build, 4), triangulate_ms=round(t_tri, 4), windows_per_s=round(a.windows / t_build * 1e3),
               counts=[round(v, 1) for v in out[5].float().mean(0).tolist()], triangulated=round(float(ok.float().sum(1).mean()), 1))
    if a.embed:
        big = torch.zeros((a.windows, 16, 1024, 2), device=dev)
        big[:, :a.frames, :a.keypoints] = kp
        t_big = time_ms(lambda: ops.tracks_build(big, pf, ij, mv, None, 2, a.slots), a.iters)
        same = all(torch.equal(x, y) for x, y in zip(ops.tracks_build(big, pf, ij, mv, None, 2, a.slots)[3:], out[3:]) if x.shape == y.shape)
        res.update(embedded_build_ms=round(t_big, 4), embedded_same_tracks=bool(same))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
