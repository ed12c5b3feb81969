"""K21 rate: ONE stride-1 photometric linearisation of 16 pairs of 480 x 640 maps (`ops.photo_linearise`: the bilinear gather,
gates and the 29-way reduction in two launches) beats a torch-on-GPU formulation of the same linearisation written here from
stock ops: projection, five `gather`s, masks, `einsum`.  A separate test shows, in float64, that the formulation computes what
`photo_linearise` computes.  No ratio is fixed.  The bytes-per-iteration figure is DESIGN.md's: 112 bytes per source pixel at
stride 1 (two 16-byte records streamed, five gathered), 551 MB for this workload; a joint iteration moves 176 bytes per
source pixel against K18's 64.
Measured on an MI355X: the stride-1 photometric linearisation 0.136 ms (8.5 us per pair-iteration, 4050 GB/s against the
551 MB the lanes request -- above what HBM delivers: neighbouring source pixels share footprint records, which come from
cache) against 3.302 ms, 24x; the default joint refinement (15 joint linearisations from identity) 2.308 ms, 6.9 k pairs/s,
beside `ops.icp_refine` on the same maps in the same process 1.006 ms: 2.29x, for a derived 176 B / 64 B = 2.75x; the module
with all four maps 2.464 ms, 6.5 k pairs/s, beside DenseRgbdRefiner 1.108 ms; the kernel has the float64 formulation's counts
and is within 1.5e-7 (A), 1.7e-6 (b) and 2.7e-6 (sum r^2) of its sums."""
import numpy as np
import torch

import icp_oracle as IO
import photo_oracle as PO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DenseRgbdRefiner, DirectRgbdRefiner
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU_PERF
HEIGHT, WIDTH, PAIRS = 480, 640, 16
ANGLE = float(np.deg2rad(IO.ANGLE_DEG))
SUMS_A_TOL, SUMS_B_TOL, SUMS_RR_TOL, COUNT_ALLOWANCE = 6.94e-6, 4.28e-5, 6.53e-5, 0       # tests/test_gpu_direct_rgbd.py, SUMS_TOL
BYTES_PER_SOURCE_PIXEL, JOINT_BYTES, ICP_BYTES = 112, 176, 64


def workload(pairs, h, w, distinct=4):
    """textured sphere rooms: depth and gray frames (pairs, h, w) of both views on the GPU (`distinct` rooms, repeated), their
    maps, the camera and a start pose per pair: the truth moved by IO.perturbed"""
    s = [synth_depth_room(700 + i, h, w) for i in range(min(distinct, pairs))]
    gray = [PO.render(*x) for x in s]
    pick = [i % len(s) for i in range(pairs)]
    d1, d2 = (torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in (0, 1))
    g1, g2 = (torch.from_numpy(np.stack([gray[i][j] for i in pick])).to(DEV) for j in (0, 1))
    K = rgbd_camera(h, w)
    k_inv = torch.from_numpy(IO.k_inv32(K)).to(DEV)
    start = [IO.perturbed(s[i][2], s[i][3]) for i in pick]
    wl = dict(d1=d1, d2=d2, g1=g1, g2=g2, K=K, cam=tuple(float(np.float32(c)) for c in IO.camera_of(K)),
              r=torch.from_numpy(np.stack([p[0] for p in start]).astype(np.float32)).to(DEV),
              t=torch.from_numpy(np.stack([p[1] for p in start]).astype(np.float32)).to(DEV))
    wl["m1"] = (*ops.surfel_maps(d1, k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP), ops.intensity_maps(g1))
    wl["m2"] = (*ops.surfel_maps(d2, k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP), ops.intensity_maps(g2))
    return wl


def torch_photo_linearise(v1, g1, v2, g2, r, t, cam, dist, thr, dtype=torch.float32):
    """the 29 sums (B, 29) of one stride-1 photometric linearisation from stock torch ops, in `dtype`"""
    B, h, w = v1.shape[:3]
    fx, fy, cx, cy = cam
    p, i1 = v1[..., :3].reshape(B, -1, 3).to(dtype), g1[..., 0].reshape(B, -1).to(dtype)
    ok1 = (v1[..., 3].reshape(B, -1) != 0) & (g1[..., 3].reshape(B, -1) != 0)
    rec2, ver2 = g2.reshape(B, -1, 4).to(dtype), v2.reshape(B, -1, 4).to(dtype)
    q = torch.einsum("bij,bnj->bni", r.to(dtype), p) + t.to(dtype)[:, None]
    u, v = fx * (q[..., 0] / q[..., 2]) + cx, fy * (q[..., 1] / q[..., 2]) + cy
    x0, y0, px, py = torch.floor(u), torch.floor(v), torch.floor(u + 0.5), torch.floor(v + 0.5)
    a, b = u - x0, v - y0
    inside = (q[..., 2] > 0) & (x0 >= 0) & (x0 <= w - 2) & (y0 >= 0) & (y0 <= h - 2)
    i00 = (y0.clamp(0, h - 2) * w + x0.clamp(0, w - 2)).nan_to_num(0).long()
    inn = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).nan_to_num(0).long()

    def take(src, idx):
        return torch.gather(src, 1, idx[..., None].expand(-1, -1, 4))
    c00, c01, c10, c11, n2 = take(rec2, i00), take(rec2, i00 + 1), take(rec2, i00 + w), take(rec2, i00 + w + 1), take(ver2, inn)
    top, bot = c00 + a[..., None] * (c01 - c00), c10 + a[..., None] * (c11 - c10)
    mix = top + b[..., None] * (bot - top)
    res = mix[..., 0] - i1
    keep = (ok1 & inside & (c00[..., 3] != 0) & (c01[..., 3] != 0) & (c10[..., 3] != 0) & (c11[..., 3] != 0) & (n2[..., 3] != 0)
            & ((q[..., 2] - n2[..., 2]).abs() <= dist) & (res.abs() <= thr))
    k0, k1 = (fx * mix[..., 1]) / q[..., 2], (fy * mix[..., 2]) / q[..., 2]
    k = torch.stack([k0, k1, -((k0 * q[..., 0] + k1 * q[..., 1]) / q[..., 2])], dim=-1)
    zero = torch.zeros((), dtype=dtype, device=q.device)
    res = torch.where(keep, res, zero)
    J = torch.where(keep[..., None], torch.cat([torch.cross(q, k, dim=-1), k], dim=-1), zero)
    A = torch.einsum("bni,bnj->bij", J, J)
    iu = torch.triu_indices(6, 6, device=q.device)
    return torch.cat([A[:, iu[0], iu[1]], torch.einsum("bni,bn->bi", J, res), (res * res).sum(1, keepdim=True),
                      keep.sum(1, keepdim=True).to(dtype)], dim=1)


def test_torch_formulation_computes_the_same_thing():
    """Run in float64 on the kernels' own maps the stock formulation is an accurate statement of the operation; the kernel
    agrees with it as the GPU suite asks of the kernel against the oracle: equal counts and the sums within that suite's
    tolerances, on that suite's (120, 160) textured rooms at the perturbed truth."""
    h, w = 120, 160
    s = [synth_depth_room(seed, h, w) for seed in (0, 1, 2)]
    gray = [PO.render(*x) for x in s]
    K = rgbd_camera(h, w)
    k_inv = torch.from_numpy(IO.k_inv32(K)).to(DEV)
    v1 = ops.surfel_maps(torch.from_numpy(np.stack([x[0] for x in s])).to(DEV), k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)[0]
    v2 = ops.surfel_maps(torch.from_numpy(np.stack([x[1] for x in s])).to(DEV), k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)[0]
    g1 = ops.intensity_maps(torch.from_numpy(np.stack([x[0] for x in gray])).to(DEV))
    g2 = ops.intensity_maps(torch.from_numpy(np.stack([x[1] for x in gray])).to(DEV))
    start = [IO.perturbed(x[2], x[3]) for x in s]
    r = torch.from_numpy(np.stack([p[0] for p in start]).astype(np.float32)).to(DEV)
    t = torch.from_numpy(np.stack([p[1] for p in start]).astype(np.float32)).to(DEV)
    cam = tuple(float(np.float32(c)) for c in IO.camera_of(K))
    got = ops.photo_linearise(v1, g1, v2, g2, r, t, cam, 1, IO.DIST, PO.INTENSITY_THRESHOLD).cpu().numpy()
    ref = torch_photo_linearise(v1, g1, v2, g2, r, t, cam, float(np.float32(IO.DIST)), PO.INTENSITY_THRESHOLD, torch.float64).cpu().numpy()
    for b in range(3):
        dev = IO.sums_deviation(got[b], ref[b])
        print(f"kernel against the float64 formulation, pair {b}: count {int(ref[b][28])}, A {dev[0]:.2e} b {dev[1]:.2e} r^2 {dev[2]:.2e} "
              f"count {dev[3]}")
        assert ref[b][28] > 0.8 * h * w
        assert dev[3] <= COUNT_ALLOWANCE and dev[0] <= SUMS_A_TOL and dev[1] <= SUMS_B_TOL and dev[2] <= SUMS_RR_TOL


def test_hip_photo_linearise_beats_torch_on_gpu_for_16_pairs():
    wl = workload(PAIRS, HEIGHT, WIDTH)
    m1, m2 = wl["m1"], wl["m2"]
    args = (m1[0], m1[2], m2[0], m2[2], wl["r"], wl["t"], wl["cam"])
    hip = time_ms(lambda: ops.photo_linearise(*args, 1, IO.DIST, PO.INTENSITY_THRESHOLD))
    ref = time_ms(lambda: torch_photo_linearise(*args, IO.DIST, PO.INTENSITY_THRESHOLD))
    eye, zero = torch.eye(3, device=DEV).repeat(PAIRS, 1, 1), torch.zeros(PAIRS, 3, device=DEV)
    icp = time_ms(lambda: ops.icp_refine(m1[:2], m2[:2], eye, zero, wl["cam"], IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR))
    joint_args = (m1, m2, eye, zero, wl["cam"], IO.SCHEDULE, IO.DIST, ANGLE, PO.PHOTO_WEIGHT, PO.INTENSITY_THRESHOLD, IO.MIN_CORR)
    joint = time_ms(lambda: ops.rgbd_refine(*joint_args))
    K = torch.from_numpy(wl["K"])
    direct, dense = DirectRgbdRefiner(K).to(DEV), DenseRgbdRefiner(K).to(DEV)
    whole = time_ms(lambda: direct(wl["d1"], wl["g1"], wl["d2"], wl["g2"]))
    whole_icp = time_ms(lambda: dense(wl["d1"], wl["d2"]))
    assert bool(ops.rgbd_refine(*joint_args)[8].all())
    mbytes = PAIRS * HEIGHT * WIDTH * BYTES_PER_SOURCE_PIXEL / 1e6
    print(f"{PAIRS} pairs of {HEIGHT} x {WIDTH}: HIP stride-1 photometric linearisation {hip:.3f} ms ({hip / PAIRS * 1e3:.1f} us per "
          f"pair-iteration, {mbytes / hip:.0f} GB/s of {mbytes:.0f} MB); torch-on-GPU formulation {ref:.3f} ms ({ref / hip:.1f}x); default "
          f"joint refine (15 joint linearisations) {joint:.3f} ms ({PAIRS / joint * 1e3:.0f} pairs/s) beside icp_refine on the same maps "
          f"{icp:.3f} ms: {joint / icp:.2f}x for {JOINT_BYTES} B / {ICP_BYTES} B = {JOINT_BYTES / ICP_BYTES:.2f}x derived; module with all four "
          f"maps {whole:.3f} ms ({PAIRS / whole * 1e3:.0f} pairs/s) beside DenseRgbdRefiner {whole_icp:.3f} ms")
    assert hip < ref
