"""K19 rate: `ops.tsdf_integrate` of 4 frames of 640 x 480 into a 256^3 volume (one pass over the volume, 16 bytes per voxel
per call: 268 MB) beats a torch-on-GPU formulation of the same update written here from stock ops: the voxel centres, the
projection, a `gather` of the depth and `where`, frame after frame.  A separate test shows, in float64, that the formulation
computes what the oracle states.  No ratio is fixed.
Measured on an MI355X: integrate 0.141 ms (1909 GB/s against the 268 MB) against 4.627 ms, 33x; one frame per call 0.063 ms
(4255 GB/s); raycast at 480 x 640 0.170 ms, 1.81 G rays/s with 98 % of the rays hitting; forward (raycast, surfel maps, 15
linearisations, compose, integrate) 0.709 ms, 1411 frames/s."""
import numpy as np
import torch

import tsdf_oracle as TO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU_PERF
HEIGHT, WIDTH, FRAMES, SIDE = 480, 640, 4, 256
BIG = ((SIDE, SIDE, SIDE), (-2.0, -2.6, 0.4), 0.015625, 0.0625)           # 4 m of room in 1.5625 cm voxels
BYTES_PER_VOXEL = 16                                                      # 8 read, 8 written, per call


def torch_integrate(volume, depth, r, t, cam, origin, voxel_size, truncation, max_weight, min_depth, max_depth, dtype=torch.float32):
    """the update of `ops.tsdf_integrate` for one volume (NZ, NY, NX, 2) and float depth (F, H, W) from stock torch ops, in
    `dtype` -> (tsdf, weight)"""
    nz, ny, nx = volume.shape[:3]
    f, h, w = depth.shape
    fx, fy, cx, cy = cam
    dev = volume.device
    tsdf, weight = volume[..., 0].to(dtype), volume[..., 1].to(dtype)
    px_, py_, pz_ = ((torch.arange(n, device=dev, dtype=dtype) + 0.5) * voxel_size + o for n, o in zip((nx, ny, nz), origin))
    p = (px_[None, None, :], py_[None, :, None], pz_[:, None, None])
    one = torch.ones((), dtype=dtype, device=dev)
    for i in range(f):
        R, T = r[i].to(dtype), t[i].to(dtype)
        q = [((R[j, 0] * p[0] + R[j, 1] * p[1]) + R[j, 2] * p[2]) + T[j] for j in range(3)]
        px = torch.floor(fx * (q[0] / q[2]) + cx + 0.5)
        py = torch.floor(fy * (q[1] / q[2]) + cy + 0.5)
        keep = (q[2] > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).nan_to_num(0).long()
        d = torch.gather(depth[i].reshape(-1).to(dtype), 0, idx.reshape(-1)).reshape(idx.shape)
        sdf = d - q[2]
        keep &= torch.isfinite(d) & (d >= min_depth) & (d <= max_depth) & (sdf >= -truncation)
        fv = torch.minimum(one, sdf / truncation)
        tsdf = torch.where(keep, (tsdf * weight + fv) / (weight + 1), tsdf)
        weight = torch.where(keep, torch.clamp(weight + 1, max=max_weight), weight)
    return tsdf, weight


def test_torch_formulation_computes_the_same_thing():
    """In float64 the stock formulation is the float64 oracle's update (the same operations; 1e-12 covers torch's own order of
    the three-term sums), with its weights on every voxel: an accurate statement of what the kernel is timed against."""
    h, w = 48, 64
    dims, grid = TO.grid_of(TO.ROOM)
    depth, R, t = TO.views(h, w)
    cam = TO.camera(h, w)[0]
    ref = TO.integrate(TO.reset(dims), depth, R, t, cam, grid, max_weight=3.0)
    vol = ops.tsdf_reset(torch.empty((1, dims[2], dims[1], dims[0], 2), dtype=torch.float32, device=DEV))[0]
    got = torch_integrate(vol, torch.from_numpy(depth).to(DEV), torch.from_numpy(R.astype(np.float32)).to(DEV),
                          torch.from_numpy(t.astype(np.float32)).to(DEV), cam, [float(o) for o in grid[0]], grid[1], grid[2], 3.0,
                          float(np.float32(TO.MIN_DEPTH)), float(np.float32(TO.MAX_DEPTH)), torch.float64)
    assert np.array_equal(got[1].cpu().numpy(), ref[1]) and ref[1].max() == 3 and (ref[1] > 0).mean() > 0.1
    assert np.abs(got[0].cpu().numpy() - ref[0]).max() <= 1e-12


def test_hip_integrate_beats_torch_on_gpu_for_4_frames_into_256_cubed():
    rooms = [synth_depth_room(800 + i, HEIGHT, WIDTH) for i in range(FRAMES - 1)]
    depth = torch.from_numpy(np.stack([rooms[0][0]] + [x[1] for x in rooms])).to(DEV)
    r = torch.from_numpy(np.stack([np.eye(3)] + [x[2] for x in rooms]).astype(np.float32)).to(DEV)
    t = torch.from_numpy(np.stack([np.zeros(3)] + [x[3] for x in rooms]).astype(np.float32)).to(DEV)
    K = rgbd_camera(HEIGHT, WIDTH)
    dims, origin, vs, trunc = BIG
    m = TsdfVolume(torch.from_numpy(K), dims, vs, origin, truncation=trunc, size=(HEIGHT, WIDTH)).to(DEV)
    cam = m.camera

    def hip_all():
        ops.tsdf_integrate(m.volume, depth[None], r[None], t[None], cam, origin, vs, trunc, 64.0)

    def hip_one():
        ops.tsdf_integrate(m.volume, depth[None, :1], r[None, :1], t[None, :1], cam, origin, vs, trunc, 64.0)

    state = m.volume[0].clone()
    hip = time_ms(hip_all)
    one = time_ms(hip_one)
    ref = time_ms(lambda: torch_integrate(state, depth, r, t, cam, origin, vs, trunc, 64.0, 0.1, 10.0), iters=5, warmup=2)
    m.reset()
    hip_all()
    assert float((m.volume[..., 1] > 0).float().mean()) > 0.02                      # the frames do land in the volume
    ray = time_ms(lambda: m.raycast(r[:1], t[:1]))
    hits = float((m.raycast(r[:1], t[:1])[0][..., 3] != 0).float().mean())
    live = torch.from_numpy(synth_depth_room(900, HEIGHT, WIDTH)[1])[None].to(DEV)
    whole = time_ms(lambda: m(live, r[:1], t[:1]))
    assert bool(m.track(live, r[:1], t[:1])[5].all()) and hits > 0.5
    mbytes = SIDE ** 3 * BYTES_PER_VOXEL / 1e6
    print(f"{FRAMES} frames of {HEIGHT} x {WIDTH} into {SIDE}^3: HIP integrate {hip:.3f} ms ({mbytes / hip:.0f} GB/s of {mbytes:.0f} MB per "
          f"call); one frame per call {one:.3f} ms ({mbytes / one:.0f} GB/s); torch-on-GPU formulation {ref:.3f} ms ({ref / hip:.1f}x); "
          f"raycast {HEIGHT} x {WIDTH} {ray:.3f} ms ({HEIGHT * WIDTH / ray / 1e3:.1f} M rays/s, {hits:.2f} of the rays hit); forward "
          f"(raycast, surfel maps, 15 linearisations, compose, integrate) {whole:.3f} ms ({1e3 / whole:.0f} frames/s)")
    assert hip < ref
