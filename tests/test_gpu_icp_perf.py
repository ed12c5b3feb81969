"""K18 rate: ONE stride-1 linearisation of 16 pairs of 480 x 640 surfel maps (`ops.icp_linearise`: gather, gates and the
29-way reduction in two launches) beats a torch-on-GPU formulation of the same linearisation written here from stock ops:
projection, `gather`, masks, `einsum`.  A separate test shows, in float64, that the formulation computes what
`icp_linearise` computes.  No ratio is fixed.  The bytes-per-iteration figure is DESIGN.md's: 64 bytes per source pixel at
stride 1 (two 16-byte records streamed, two gathered), 315 MB for this workload.
Measured on an MI355X: the stride-1 linearisation 0.110 ms (6.9 us per pair-iteration, 2854 GB/s against the 315 MB)
against 2.772 ms, 25x; the default refinement (15 linearisations from identity) 1.006 ms, 15.9 k pairs/s; the module with both
surfel maps 1.118 ms, 14.3 k pairs/s; the kernel has the float64 formulation's counts and is within 2.8e-8 (A), 4.9e-6 (b) and
6.9e-6 (sum r^2) of its sums."""
import numpy as np
import torch

import icp_oracle as IO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DenseRgbdRefiner
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU_PERF
HEIGHT, WIDTH, PAIRS = 480, 640, 16
ANGLE = float(np.deg2rad(IO.ANGLE_DEG))
SUMS_A_TOL, SUMS_B_TOL, SUMS_RR_TOL, COUNT_ALLOWANCE = 4.08e-6, 1.90e-3, 1.53e-4, 0      # tests/test_gpu_icp.py
BYTES_PER_SOURCE_PIXEL = 64


def workload(pairs, h, w, distinct=4):
    """depth frames (pairs, h, w) of both views on the GPU (`distinct` rooms, repeated), their maps, the camera and a start
    pose per pair: the truth moved by IO.perturbed"""
    s = [synth_depth_room(700 + i, h, w) for i in range(min(distinct, pairs))]
    pick = [i % len(s) for i in range(pairs)]
    d1, d2 = (torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in (0, 1))
    K = rgbd_camera(h, w)
    k_inv = torch.from_numpy(IO.k_inv32(K)).to(DEV)
    start = [IO.perturbed(s[i][2], s[i][3]) for i in pick]
    wl = dict(d1=d1, d2=d2, K=K, cam=tuple(float(np.float32(c)) for c in IO.camera_of(K)),
              r=torch.from_numpy(np.stack([p[0] for p in start]).astype(np.float32)).to(DEV),
              t=torch.from_numpy(np.stack([p[1] for p in start]).astype(np.float32)).to(DEV))
    wl["m1"] = ops.surfel_maps(d1, k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)
    wl["m2"] = ops.surfel_maps(d2, k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)
    return wl


def torch_linearise(m1, m2, r, t, cam, dist, angle, dtype=torch.float32):
    """the 29 sums (B, 29) of one stride-1 linearisation from stock torch ops, in `dtype`"""
    B, h, w = m1[0].shape[:3]
    fx, fy, cx, cy = cam
    v1, n1 = m1[0][..., :3].reshape(B, -1, 3).to(dtype), m1[1][..., :3].reshape(B, -1, 3).to(dtype)
    v2, n2 = m2[0][..., :3].reshape(B, -1, 3).to(dtype), m2[1][..., :3].reshape(B, -1, 3).to(dtype)
    ok1, ok2 = m1[1][..., 3].reshape(B, -1) != 0, m2[1][..., 3].reshape(B, -1) != 0
    R, T = r.to(dtype), t.to(dtype)
    q = torch.einsum("bij,bnj->bni", R, v1) + T[:, None]
    rn = torch.einsum("bij,bnj->bni", R, n1)
    px = torch.floor(fx * (q[..., 0] / q[..., 2]) + cx + 0.5)
    py = torch.floor(fy * (q[..., 1] / q[..., 2]) + cy + 0.5)
    inside = (q[..., 2] > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).nan_to_num(0).long()
    idx3 = idx[..., None].expand(-1, -1, 3)
    p2, g2 = torch.gather(v2, 1, idx3), torch.gather(n2, 1, idx3)
    e = q - p2
    cos_thr = float(np.cos(np.float64(np.float32(angle))))
    keep = ok1 & inside & torch.gather(ok2, 1, idx) & ((e * e).sum(-1) <= dist * dist) & ((rn * g2).sum(-1) >= cos_thr)
    res = torch.where(keep, (g2 * e).sum(-1), torch.zeros((), dtype=dtype, device=q.device))
    J = torch.where(keep[..., None], torch.cat([torch.cross(q, g2, dim=-1), g2], dim=-1), torch.zeros((), dtype=dtype, device=q.device))
    A = torch.einsum("bni,bnj->bij", J, J)
    iu = torch.triu_indices(6, 6, device=q.device)
    return torch.cat([A[:, iu[0], iu[1]], torch.einsum("bni,bn->bi", J, res), (res * res).sum(1, keepdim=True),
                      keep.sum(1, keepdim=True).to(dtype)], dim=1)


def test_torch_formulation_computes_the_same_thing():
    """Run in float64 on the kernels' own maps the stock formulation is an accurate statement of the operation; the kernel
    agrees with it as the GPU suite asks of the kernel against the oracle: equal counts and the sums within that suite's
    tolerances, on that suite's (120, 160) rooms at the perturbed truth."""
    h, w = 120, 160
    s = [synth_depth_room(seed, h, w) for seed in (0, 1, 2)]
    K = rgbd_camera(h, w)
    k_inv = torch.from_numpy(IO.k_inv32(K)).to(DEV)
    m1 = ops.surfel_maps(torch.from_numpy(np.stack([x[0] for x in s])).to(DEV), k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)
    m2 = ops.surfel_maps(torch.from_numpy(np.stack([x[1] for x in s])).to(DEV), k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)
    start = [IO.perturbed(x[2], x[3]) for x in s]
    r = torch.from_numpy(np.stack([p[0] for p in start]).astype(np.float32)).to(DEV)
    t = torch.from_numpy(np.stack([p[1] for p in start]).astype(np.float32)).to(DEV)
    cam = tuple(float(np.float32(c)) for c in IO.camera_of(K))
    got = ops.icp_linearise(m1, m2, r, t, cam, 1, IO.DIST, ANGLE).cpu().numpy()
    ref = torch_linearise(m1, m2, r, t, cam, IO.DIST, ANGLE, torch.float64).cpu().numpy()
    for b in range(3):
        dev = IO.sums_deviation(got[b], ref[b])
        print(f"kernel against the float64 formulation, pair {b}: count {int(ref[b][28])}, A {dev[0]:.2e} b {dev[1]:.2e} r^2 {dev[2]:.2e} "
              f"count {dev[3]}")
        assert ref[b][28] > 0.8 * h * w
        assert dev[3] <= COUNT_ALLOWANCE and dev[0] <= SUMS_A_TOL and dev[1] <= SUMS_B_TOL and dev[2] <= SUMS_RR_TOL


def test_hip_linearise_beats_torch_on_gpu_for_16_pairs():
    wl = workload(PAIRS, HEIGHT, WIDTH)
    args = (wl["m1"], wl["m2"], wl["r"], wl["t"], wl["cam"])
    hip = time_ms(lambda: ops.icp_linearise(*args, 1, IO.DIST, ANGLE))
    ref = time_ms(lambda: torch_linearise(*args, IO.DIST, ANGLE))
    eye, zero = torch.eye(3, device=DEV).repeat(PAIRS, 1, 1), torch.zeros(PAIRS, 3, device=DEV)
    refine = time_ms(lambda: ops.icp_refine(wl["m1"], wl["m2"], eye, zero, wl["cam"], IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR))
    module = DenseRgbdRefiner(torch.from_numpy(wl["K"])).to(DEV)
    whole = time_ms(lambda: module(wl["d1"], wl["d2"]))
    ok = ops.icp_refine(wl["m1"], wl["m2"], eye, zero, wl["cam"], IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)[6]
    assert bool(ok.all())
    mbytes = PAIRS * HEIGHT * WIDTH * BYTES_PER_SOURCE_PIXEL / 1e6
    print(f"{PAIRS} pairs of {HEIGHT} x {WIDTH}: HIP stride-1 linearisation {hip:.3f} ms ({hip / PAIRS * 1e3:.1f} us per pair-iteration, "
          f"{mbytes / hip:.0f} GB/s of {mbytes:.0f} MB); torch-on-GPU formulation {ref:.3f} ms ({ref / hip:.1f}x); default refine "
          f"(15 linearisations) {refine:.3f} ms ({PAIRS / refine * 1e3:.0f} pairs/s); module with both surfel maps {whole:.3f} ms "
          f"({PAIRS / whole * 1e3:.0f} pairs/s)")
    assert hip < ref
