#!/usr/bin/env python3
"""Generate tests/golden/depth_frontend.npz by RUNNING THE REFERENCE depth modules on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_depth.py

Inputs are stored by seed and size (onnx_image_processing_amd/synth.py: synth_depth_frame; `millimetres` = 1: the frame
as rounded millimetre counts), outputs verbatim.  Per case <name>: <name>__seed, <name>__hw, <name>__hole_share,
<name>__millimetres, <name>__camera (scale, cx, cy, fx, fy of the depth camera); points cases: <name>__points and
<name>__normals (H, W, 3); alignment cases: <name>__rgb (cx, cy, fx, fy), <name>__rotation (3, 3), <name>__translation
(3,), <name>__aligned (H, W).  The alignment cases run with torch.set_num_threads(1): the reference's index_put_ with
duplicate indices gives different results with more threads.  The colour camera's field of view is wider than the depth
camera's, so that no source lands in column `width` / row `height`, where the reference raises IndexError; a case on
which the reference raises stops the generator.  Recorded: torch version and thread counts."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
# the reference's depth modules import each other by bare module name
sys.path.insert(0, "/root/reference/pytorch_model/depth")

import torch  # noqa: E402

from depth2pointcloud_with_normal import DepthToPointCloudWithNormal  # noqa: E402
from depth2pointcloud import DepthToPointCloud  # noqa: E402
from depth_align import DepthAlignment  # noqa: E402

sys.path.insert(1, ROOT)
from onnx_image_processing_amd.synth import synth_depth_frame  # noqa: E402

OUT = os.path.join(HERE, "depth_frontend.npz")


def frame(seed, h, w, hole_share, millimetres):
    d = synth_depth_frame(seed, h, w, hole_share=hole_share)
    if millimetres:
        d = np.round(d.astype(np.float64) * 1000.0).astype(np.float32)
    return d


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    a = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    b = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    c = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (c @ b @ a).astype(np.float32)


# name -> (seed, h, w, hole_share, millimetres, (scale, cx, cy, fx, fy))
POINTS = {
    "pn_metres": (21, 60, 80, 0.0, 0, (1.0, 40.7, 28.6, 65.5, 64.25)),
    "pn_metres_holes": (22, 48, 64, 0.1, 0, (1.0, 30.2, 25.1, 52.0, 53.5)),
    "pn_counts": (23, 40, 56, 0.0, 1, (0.001, 29.3, 18.4, 46.0, 45.25)),
    "pn_counts_holes_odd": (24, 37, 53, 0.1, 1, (0.001, 25.5, 19.25, 43.5, 44.0)),
}
# the depth camera of every alignment case, and colour cameras with a wider field of view
ALIGN_HW = (90, 120)
DEPTH_CAM = (1.0, 60.3, 44.2, 98.25, 98.0)
COUNTS_CAM = (0.001, 60.3, 44.2, 98.25, 98.0)
RGB = (59.1, 45.3, 88.5, 88.875)
SMALL_ROT = rotation(0.004, -0.006, 0.003)
# name -> (seed, hole_share, millimetres, depth camera, rgb, rotation, translation)
ALIGN = {
    "al_identity": (31, 0.0, 0, DEPTH_CAM, RGB, np.eye(3, dtype=np.float32), np.zeros(3, np.float32)),
    "al_rotation_baseline": (32, 0.0, 0, DEPTH_CAM, RGB, SMALL_ROT, np.float32([0.025, 0.0, 0.0])),
    "al_rotation_baseline_holes": (33, 0.1, 0, DEPTH_CAM, RGB, SMALL_ROT, np.float32([0.025, 0.0, 0.0])),
    "al_sideways_counts": (34, 0.0, 1, COUNTS_CAM, RGB, np.eye(3, dtype=np.float32), np.float32([-0.04, 0.0, 0.0])),
}


def main():
    threads = torch.get_num_threads()
    store = {"meta__torch_version": np.array(torch.__version__), "meta__threads": np.int64(threads)}
    for name, (seed, h, w, holes, mm, cam) in POINTS.items():
        scale, cx, cy, fx, fy = cam
        d = torch.from_numpy(frame(seed, h, w, holes, mm)).reshape(h, w, 1)
        pts, nrm = DepthToPointCloudWithNormal(scale, w, h, cx, cy, fx, fy)(d)
        assert torch.equal(pts, DepthToPointCloud(scale, w, h, cx, cy, fx, fy)(d))
        store.update({f"{name}__seed": np.int64(seed), f"{name}__hw": np.array([h, w], np.int64),
                      f"{name}__hole_share": np.float64(holes), f"{name}__millimetres": np.int64(mm),
                      f"{name}__camera": np.array(cam, np.float64), f"{name}__points": pts.numpy(),
                      f"{name}__normals": nrm.numpy()})
        print(f"{name:28s} {h}x{w} scale {scale:g} holes {holes:g}")
    torch.set_num_threads(1)
    h, w = ALIGN_HW
    for name, (seed, holes, mm, cam, rgb, rot, tr) in ALIGN.items():
        scale, cx, cy, fx, fy = cam
        d = torch.from_numpy(frame(seed, h, w, holes, mm)).reshape(h, w, 1)
        model = DepthAlignment(scale, w, h, cx, cy, fx, fy, *rgb, torch.from_numpy(rot), torch.from_numpy(tr))
        aligned = model(d.clone())                    # an IndexError of the reference ends the run here: no case is skipped
        store.update({f"{name}__seed": np.int64(seed), f"{name}__hw": np.array([h, w], np.int64),
                      f"{name}__hole_share": np.float64(holes), f"{name}__millimetres": np.int64(mm),
                      f"{name}__camera": np.array(cam, np.float64), f"{name}__rgb": np.array(rgb, np.float64),
                      f"{name}__rotation": rot, f"{name}__translation": tr,
                      f"{name}__aligned": aligned.reshape(h, w).numpy()})
        print(f"{name:28s} {h}x{w} filled {float((aligned != 0).float().mean()):.3f}")
    store["meta__align_threads"] = np.int64(torch.get_num_threads())
    store["meta__points_cases"] = np.array(list(POINTS))
    store["meta__align_cases"] = np.array(list(ALIGN))
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
