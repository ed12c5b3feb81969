"""K20 rate: the sizing pass of `ops.tsdf_surface` (classification of every voxel and cell of a 256^3 volume fused from 4 frames
of 640 x 480, one 8-byte read per voxel: 134 MB) beats a torch-on-GPU formulation of the same vertex-existence count written
here from stock ops: the seven shifted sign-change masks over observed pairs, summed.  A separate test shows, in float64, that
the formulation counts what the oracle states.  No ratio is fixed.  The full extraction (vertices, normals, triangles) and the
points-only form are timed and printed beside it.
Measured on an MI355X (8.9 % of the volume observed, 142,609 vertices, 281,910 triangles): sizing pass 0.230 ms (584 GB/s
against the 134 MB, 7.7x the 0.03 ms floor derived from K19's 4.3 TB/s) against 0.789 ms, 3.4x; full extraction 0.473 ms;
points only 0.377 ms."""
import numpy as np
import torch

import surface_oracle as SO
import tsdf_oracle as TO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU_PERF
HEIGHT, WIDTH, FRAMES, SIDE = 480, 640, 4, 256
BIG = ((SIDE, SIDE, SIDE), (-2.0, -2.6, 0.4), 0.015625, 0.0625)           # tests/test_gpu_tsdf_perf.py's volume
BYTES_PER_VOXEL = 8                                                       # the volume is read once
FLOOR_MS = 0.03                                                           # 134 MB at K19's measured 4.3 TB/s


def torch_vertex_count(volume, min_weight=1.0, dtype=torch.float32):
    """the number of vertices of one volume (NZ, NY, NX, 2) from stock torch ops -> a 0-dim int64 tensor"""
    tsdf, weight = volume[..., 0].to(dtype), volume[..., 1].to(dtype)
    obs = weight >= min_weight
    ins = obs & ~(tsdf > 0)
    nz, ny, nx = obs.shape
    total = torch.zeros((), dtype=torch.int64, device=volume.device)
    for e in range(1, 8):
        dx, dy, dz = e & 1, (e >> 1) & 1, (e >> 2) & 1
        p = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        q = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        total = total + (obs[p] & obs[q] & (ins[p] ^ ins[q])).sum()
    return total


def test_torch_formulation_counts_the_same_thing():
    """In float64 the stock formulation counts the float64 oracle's vertices, for both thresholds: an accurate statement of what
    the kernel is timed against."""
    for spec in (TO.ROOM, TO.ODD):
        vol = TO.fused_room(37, 53, spec)
        dev = torch.from_numpy(np.stack(vol, axis=-1)).to(DEV)
        for mw in (1.0, 2.0):
            want = SO.extract(vol, TO.grid_of(spec)[1], min_weight=mw, normals=False)["counts"][0]
            assert int(torch_vertex_count(dev, mw, torch.float64)) == want and want > 1000
            assert int(ops.tsdf_surface_counts(dev.float()[None], mw)[0, 0]) == want


def test_hip_sizing_pass_beats_torch_on_gpu_for_256_cubed():
    rooms = [synth_depth_room(800 + i, HEIGHT, WIDTH) for i in range(FRAMES - 1)]
    depth = torch.from_numpy(np.stack([rooms[0][0]] + [x[1] for x in rooms])).to(DEV)
    r = torch.from_numpy(np.stack([np.eye(3)] + [x[2] for x in rooms]).astype(np.float32)).to(DEV)
    t = torch.from_numpy(np.stack([np.zeros(3)] + [x[3] for x in rooms]).astype(np.float32)).to(DEV)
    dims, origin, vs, trunc = BIG
    m = TsdfVolume(torch.from_numpy(rgbd_camera(HEIGHT, WIDTH)), dims, vs, origin, truncation=trunc, size=(HEIGHT, WIDTH)).to(DEV)
    m.reset()
    m.integrate(depth[None], r[None], t[None])
    counts = ops.tsdf_surface_counts(m.volume)
    nv, nt = counts[0].tolist()
    assert int(torch_vertex_count(m.volume[0])) == nv and nv > 100000 and nt > 100000
    observed = float((m.volume[..., 1] > 0).float().mean())

    sizing = time_ms(lambda: ops.tsdf_surface_counts(m.volume))
    ref = time_ms(lambda: torch_vertex_count(m.volume[0]), iters=5, warmup=2)
    full = time_ms(lambda: m.extract_surface(nv, nt))
    points = time_ms(lambda: m.extract_points(nv))
    vertex, normal, tris, c = m.extract_surface(nv, nt)
    assert torch.equal(c, counts) and int(tris.min()) >= 0 and int(tris.max()) < nv and bool((vertex[..., 3] == 1).all())
    mbytes = SIDE ** 3 * BYTES_PER_VOXEL / 1e6
    print(f"{SIDE}^3 fused from {FRAMES} frames of {HEIGHT} x {WIDTH} ({observed:.3f} observed): {nv} vertices, {nt} triangles, "
          f"{float((normal[..., 3] != 0).float().mean()):.3f} with normals; sizing pass {sizing:.3f} ms ({mbytes / sizing:.0f} GB/s of "
          f"{mbytes:.0f} MB, {sizing / FLOOR_MS:.1f}x the {FLOOR_MS} ms floor derived from 4.3 TB/s); torch-on-GPU count {ref:.3f} ms "
          f"({ref / sizing:.1f}x); full extraction {full:.3f} ms ({mbytes / full:.0f} GB/s); points only {points:.3f} ms "
          f"({mbytes / points:.0f} GB/s)")
    assert sizing < ref
