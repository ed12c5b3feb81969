"""K23 rate: normalise + pnp_ransac (128 hypotheses, 3 refinement rounds) on 256 pairs x 512 rows in two calls beat a
torch-on-GPU formulation that does LESS: it is handed the kernel's own poses rt_h, projects every row under every pose in
one batch of stock ops, forms the MSAC cost and takes the argmin -- no sampling, no P3P solve, no refinement, no inlier
mask.  A separate test shows that its cost is mi_pnp_hypotheses'.  mi_rigid_ransac (K17) on the same shape is timed for
comparison.  Measured on an MI355X: see DESIGN.md, "K23"."""
import numpy as np
import torch

import pnp_oracle as QO
import rigid_oracle as RO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import rgbd_camera, synth_rgbd_pair

pytestmark = GPU_PERF
HEIGHT, WIDTH = 240, 320
K = rgbd_camera(HEIGHT, WIDTH)
THR = QO.THR_PX / float((K[0, 0] + K[1, 1]) / 2)
PAIRS, N_ROWS, HYP = 256, 512, 128
COST_RTOL = 4.3e-3                       # tests/test_gpu_pnp.py, its tightest case


def workload(pairs=PAIRS, n=N_ROWS, hyp=HYP, seed=17, distinct=8):
    """keypoints of frame 2 (pairs, n, 2), the lifted points of frame 1 (pairs, n, 3) and, for the K17 comparison, of frame 2
    (`distinct` scenes at 240 x 320, 25 % outliers, 0.5 px, repeated)"""
    k_inv = torch.from_numpy(np.linalg.inv(K)).float().to(DEV)
    s = [synth_rgbd_pair(500 + i, n, 0.25, 0.5, 0.0, HEIGHT, WIDTH) for i in range(min(distinct, pairs))]
    pick = [i % len(s) for i in range(pairs)]
    k1, k2, d1, d2 = (torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in range(4))
    x1, v1 = ops.lift_keypoints(k1, d1, k_inv, 1.0, RO.MIN_DEPTH, RO.MAX_DEPTH)
    x2, v2 = ops.lift_keypoints(k2, d2, k_inv, 1.0, RO.MIN_DEPTH, RO.MAX_DEPTH)
    assert bool(v1.all()) and bool(v2.all())
    return dict(k2=k2, k_inv=k_inv, x1=x1, x2=x2, seed=seed, hyp=hyp)


def torch_score(rt_h, x, u, thr):
    """(cost (B, H), best (B,)) of the poses rt_h (B, H, 12) on the rows x (B, N, 3), u (B, N, 2), from stock torch ops"""
    r, t = rt_h[..., :9].reshape(*rt_h.shape[:2], 3, 3), rt_h[..., 9:]
    y = torch.einsum("bhij,bnj->bhni", r, x) + t[:, :, None]
    d = y[..., :2] / y[..., 2:] - u[:, None]
    d2 = (d * d).sum(-1)
    d2 = torch.where((y[..., 2] > 0) & torch.isfinite(d2), d2, torch.full_like(d2, float("inf")))
    cost = torch.clamp(d2, max=thr * thr).sum(-1)
    return cost, torch.argmin(cost, dim=1)


def hip_pose(w, rounds=3):
    u = ops.normalise_keypoints(w["k2"], w["k_inv"])
    return ops.pnp_ransac(w["x1"], u, None, w["hyp"], THR, rounds, w["seed"])


def test_torch_formulation_computes_the_same_cost():
    """the yardstick's cost of the kernel's own poses is the kernel's cost (float32 both, another summation order), and
    its argmin the kernel's selection wherever the two smallest costs are further apart than that tolerance"""
    w = workload(3, 97, 64, distinct=3)
    u = ops.normalise_keypoints(w["k2"], w["k_inv"])
    rt_h, cost, _ = ops.pnp_hypotheses(w["x1"], u, None, 64, THR, w["seed"])
    best_h = ops.pnp_ransac(w["x1"], u, None, 64, THR, 0, w["seed"])[3]
    tcost, tbest = torch_score(rt_h, w["x1"], u, THR)
    fin = torch.isfinite(cost)
    rel = ((cost - tcost).abs() / cost)[fin]
    print(f"accepted {fin.float().mean():.3f}; cost relative deviation max {rel.max():.2e}")
    assert fin.float().mean() >= 0.9 and rel.max() <= COST_RTOL
    two = torch.where(fin, cost, torch.full_like(cost, float("inf"))).sort(dim=1).values[:, :2]
    clear = two[:, 1] > two[:, 0] * (1 + COST_RTOL)
    tb = torch.where(fin, tcost, torch.full_like(tcost, float("inf"))).argmin(dim=1)
    assert torch.equal(tb[clear], best_h.long()[clear])


def test_hip_absolute_pose_beats_torch_on_gpu_for_256_pairs():
    w = workload()
    u = ops.normalise_keypoints(w["k2"], w["k_inv"])
    rt_h = ops.pnp_hypotheses(w["x1"], u, None, HYP, THR, w["seed"])[0]
    hip = time_ms(lambda: hip_pose(w))
    hip_hyp = time_ms(lambda: ops.pnp_hypotheses(w["x1"], u, None, HYP, THR, w["seed"]))
    rigid = time_ms(lambda: ops.rigid_ransac(w["x1"], w["x2"], None, HYP, RO.THR, 3, w["seed"]))
    ref = time_ms(lambda: torch_score(rt_h, w["x1"], u, THR))
    print(f"{PAIRS} pairs x {N_ROWS} rows x {HYP} hypotheses: HIP normalise + pnp_ransac (3 rounds) {hip:.3f} ms "
          f"({PAIRS / hip * 1e3:.0f} pairs/s), hypotheses alone {hip_hyp:.3f} ms; torch-on-GPU projection + cost + argmin of given "
          f"poses {ref:.3f} ms ({ref / hip:.1f}x); mi_rigid_ransac on the same shape {rigid:.3f} ms")
    assert hip < ref
