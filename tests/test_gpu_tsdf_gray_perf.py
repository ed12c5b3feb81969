"""K22 rate: `ops.tsdf_integrate_gray` of 4 frames of 640 x 480 (depth and gray) into a 256^3 volume and its intensity volume --
the workload of tests/test_gpu_tsdf_perf.py with gray frames rendered by photo_oracle.render -- beats a torch-on-GPU
formulation of the same joint update written here from stock ops.  A separate test shows, in float64, that the formulation
computes what the oracle states.  The only assertion on time is that the HIP call beats it; no ratio is fixed.  Printed beside
it: `ops.tsdf_integrate` on the same frames in the same run, the GB/s against 16 bytes per voxel (K19's traffic, what a voxel
outside every truncation band costs) and against 32 (both records read and written), the sampler at 480 x 640, and
DirectTsdfVolume.forward against TsdfVolume.forward.
Measured on an MI355X (1.4 % of the voxels inside a truncation band): integrate_gray 0.158 ms (1703 GB/s against 16 bytes per
voxel, 3406 against 32) beside tsdf_integrate's 0.140 ms on the same frames (1.12x); one frame per call 0.069 ms; the torch
formulation 6.048 ms (38x); the sampler at 480 x 640 0.020 ms beside the raycast's 0.166 ms; DirectTsdfVolume.forward 1.288 ms
(777 frames/s) against TsdfVolume.forward's 0.725 ms.  The same kernel with the intensity record loaded for every voxel
(DESIGN.md, K22): 0.158 ms against 0.155 for the 4 frames, 0.098 against 0.065 for one."""
import numpy as np
import torch

import photo_oracle as PO
import tsdf_gray_oracle as GO
import tsdf_oracle as TO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DirectTsdfVolume, TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU_PERF
HEIGHT, WIDTH, FRAMES, SIDE = 480, 640, 4, 256
BIG = ((SIDE, SIDE, SIDE), (-2.0, -2.6, 0.4), 0.015625, 0.0625)           # 4 m of room in 1.5625 cm voxels


def torch_integrate_gray(volume, intensity, depth, gray, r, t, cam, origin, voxel_size, truncation, max_weight, min_depth, max_depth,
                         dtype=torch.float32):
    """the update of `ops.tsdf_integrate_gray` for one volume and one intensity volume (NZ, NY, NX, 2) and float frames (F, H, W)
    from stock torch ops, in `dtype` -> (tsdf, weight, gray, gweight)"""
    nz, ny, nx = volume.shape[:3]
    f, h, w = depth.shape
    fx, fy, cx, cy = cam
    dev = volume.device
    tsdf, weight = volume[..., 0].to(dtype), volume[..., 1].to(dtype)
    gry, gwt = intensity[..., 0].to(dtype), intensity[..., 1].to(dtype)
    px_, py_, pz_ = ((torch.arange(n, device=dev, dtype=dtype) + 0.5) * voxel_size + o for n, o in zip((nx, ny, nz), origin))
    p = (px_[None, None, :], py_[None, :, None], pz_[:, None, None])
    one = torch.ones((), dtype=dtype, device=dev)
    for i in range(f):
        R, T = r[i].to(dtype), t[i].to(dtype)
        q = [((R[j, 0] * p[0] + R[j, 1] * p[1]) + R[j, 2] * p[2]) + T[j] for j in range(3)]
        px = torch.floor(fx * (q[0] / q[2]) + cx + 0.5)
        py = torch.floor(fy * (q[1] / q[2]) + cy + 0.5)
        keep = (q[2] > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).nan_to_num(0).long().reshape(-1)
        d = torch.gather(depth[i].reshape(-1).to(dtype), 0, idx).reshape(keep.shape)
        g = torch.gather(gray[i].reshape(-1).to(dtype), 0, idx).reshape(keep.shape)
        sdf = d - q[2]
        keep &= torch.isfinite(d) & (d >= min_depth) & (d <= max_depth) & (sdf >= -truncation)
        gkeep = keep & (sdf <= truncation) & torch.isfinite(g)
        fv = torch.minimum(one, sdf / truncation)
        tsdf = torch.where(keep, (tsdf * weight + fv) / (weight + 1), tsdf)
        weight = torch.where(keep, torch.clamp(weight + 1, max=max_weight), weight)
        gry = torch.where(gkeep, (gry * gwt + g) / (gwt + 1), gry)
        gwt = torch.where(gkeep, torch.clamp(gwt + 1, max=max_weight), gwt)
    return tsdf, weight, gry, gwt


def test_torch_formulation_computes_the_same_thing():
    """In float64 the stock formulation is the float64 oracle's joint update (the same operations; 1e-12 relative covers torch's
    own order of the three-term sums), with its weights on every voxel: an accurate statement of what the kernel is timed
    against."""
    h, w = 48, 64
    dims, grid = TO.grid_of(TO.ROOM)
    depth, R, t = TO.views(h, w)
    gray = GO.views_gray(h, w)
    cam = TO.camera(h, w)[0]
    ref = GO.integrate(TO.reset(dims), GO.reset(dims), depth, gray, R, t, cam, grid, max_weight=3.0)
    shape = (1, dims[2], dims[1], dims[0], 2)
    vol = ops.tsdf_reset(torch.empty(shape, dtype=torch.float32, device=DEV))[0]
    ivol = ops.tsdf_gray_reset(torch.empty(shape, dtype=torch.float32, device=DEV))[0]
    got = torch_integrate_gray(vol, ivol, torch.from_numpy(depth).to(DEV), torch.from_numpy(gray).to(DEV),
                               torch.from_numpy(R.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.float32)).to(DEV), cam,
                               [float(o) for o in grid[0]], grid[1], grid[2], 3.0, float(np.float32(TO.MIN_DEPTH)),
                               float(np.float32(TO.MAX_DEPTH)), torch.float64)
    got = [x.cpu().numpy() for x in got]
    assert np.array_equal(got[1], ref[0][1]) and np.array_equal(got[3], ref[1][1]) and ref[1][1].max() == 3 and (ref[1][1] > 0).mean() > 0.02
    assert np.abs(got[0] - ref[0][0]).max() <= 1e-12 and np.abs(got[2] - ref[1][0]).max() <= 1e-12 * 255


def test_hip_integrate_gray_beats_torch_on_gpu_for_4_frames_into_256_cubed():
    rooms = [synth_depth_room(800 + i, HEIGHT, WIDTH) for i in range(FRAMES - 1)]
    shades = [PO.render(*x) for x in rooms]
    depth = torch.from_numpy(np.stack([rooms[0][0]] + [x[1] for x in rooms])).to(DEV)
    gray = torch.from_numpy(np.stack([shades[0][0]] + [x[1] for x in shades])).to(DEV)
    r = torch.from_numpy(np.stack([np.eye(3)] + [x[2] for x in rooms]).astype(np.float32)).to(DEV)
    t = torch.from_numpy(np.stack([np.zeros(3)] + [x[3] for x in rooms]).astype(np.float32)).to(DEV)
    K = torch.from_numpy(rgbd_camera(HEIGHT, WIDTH))
    dims, origin, vs, trunc = BIG
    m = DirectTsdfVolume(K, dims, vs, origin, truncation=trunc, size=(HEIGHT, WIDTH)).to(DEV)
    k19 = TsdfVolume(K, dims, vs, origin, truncation=trunc, size=(HEIGHT, WIDTH)).to(DEV)
    cam = m.camera

    def hip_all():
        ops.tsdf_integrate_gray(m.volume, m.intensity, depth[None], gray[None], r[None], t[None], cam, origin, vs, trunc, 64.0)

    def hip_one():
        ops.tsdf_integrate_gray(m.volume, m.intensity, depth[None, :1], gray[None, :1], r[None, :1], t[None, :1], cam, origin, vs, trunc,
                                64.0)

    def k19_all():
        ops.tsdf_integrate(k19.volume, depth[None], r[None], t[None], cam, origin, vs, trunc, 64.0)

    state = (m.volume[0].clone(), m.intensity[0].clone())
    hip, plain, one = time_ms(hip_all), time_ms(k19_all), time_ms(hip_one)
    ref = time_ms(lambda: torch_integrate_gray(*state, depth, gray, r, t, cam, origin, vs, trunc, 64.0, 0.1, 10.0), iters=5, warmup=2)
    m.reset()
    k19.reset()
    hip_all()
    k19_all()
    assert torch.equal(m.volume.view(torch.uint8), k19.volume.view(torch.uint8))        # the same frames, K19's bits
    band = float((m.intensity[..., 1] > 0).float().mean())
    assert band > 0.01 and float((m.volume[..., 1] > 0).float().mean()) > band          # the frames do land; the band is a part of it
    vertex = k19.raycast(r[:1], t[:1])[0]
    sample = time_ms(lambda: ops.tsdf_sample_gray(m.intensity, vertex, origin, vs, r[:1], t[:1]))
    ray = time_ms(lambda: k19.raycast(r[:1], t[:1]))
    inten = ops.tsdf_sample_gray(m.intensity, vertex, origin, vs, r[:1], t[:1])
    hits = float((vertex[..., 3] != 0).float().mean())
    assert hits > 0.5 and torch.equal(inten[..., 3] != 0, vertex[..., 3] != 0)           # every hit has an intensity
    live = synth_depth_room(900, HEIGHT, WIDTH)
    live_d, live_g = torch.from_numpy(live[1])[None].to(DEV), torch.from_numpy(PO.render(*live)[1])[None].to(DEV)
    # the prediction is the truth of frame 1, not of the live frame: both trackers have a motion to find
    whole = time_ms(lambda: m(live_d, live_g, r[:1], t[:1]))
    parent = time_ms(lambda: k19(live_d, r[:1], t[:1]))
    assert bool(m.track(live_d, live_g, r[:1], t[:1])[7].all())
    mb16, mb32 = SIDE ** 3 * 16 / 1e6, SIDE ** 3 * 32 / 1e6
    print(f"{FRAMES} frames of {HEIGHT} x {WIDTH} into {SIDE}^3: HIP integrate_gray {hip:.3f} ms ({mb16 / hip:.0f} GB/s against 16 bytes "
          f"per voxel, {mb32 / hip:.0f} against 32; {band:.3f} of the voxels hold a gray value); ops.tsdf_integrate on the same "
          f"frames {plain:.3f} ms ({hip / plain:.2f}x); one frame per call {one:.3f} ms; torch-on-GPU formulation {ref:.3f} ms "
          f"({ref / hip:.1f}x); sampler at {HEIGHT} x {WIDTH} {sample:.3f} ms ({HEIGHT * WIDTH / sample / 1e3:.1f} M points/s, {hits:.2f} "
          f"of them hits) beside the raycast's {ray:.3f} ms; DirectTsdfVolume.forward {whole:.3f} ms ({1e3 / whole:.0f} frames/s) "
          f"against TsdfVolume.forward {parent:.3f} ms")
    assert hip < ref
