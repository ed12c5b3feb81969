"""K24 rate: normalise + homography_ransac (128 hypotheses, 3 refinement rounds) + homography_pose on 256 pairs x 512 rows
beat a torch-on-GPU formulation that does LESS: it is handed the kernel's own homographies h_h, transfers every row under
every one of them, both ways, in one batch of stock ops, forms the MSAC cost and takes the argmin -- no sampling, no
4-point solve, no refinement, no inlier mask, no decomposition.  A separate test shows that its cost is
mi_homography_hypotheses'.  mi_essential_ransac (K15) and mi_rigid_ransac (K17) on the same shape are timed for
comparison.  Measured on an MI355X: see DESIGN.md, "K24"."""
import numpy as np
import torch

from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_planar_two_view, two_view_camera

pytestmark = GPU_PERF
K = two_view_camera()
THR = 3.0 / 500.0
PAIRS, N_ROWS, HYP = 256, 512, 128
COST_RTOL = 4.4e-3                       # tests/test_gpu_homography.py


def workload(pairs=PAIRS, n=N_ROWS, hyp=HYP, seed=17, distinct=8):
    """keypoints of both frames (pairs, n, 2): `distinct` planar scenes, 25 % outliers, 0.5 px, repeated"""
    k_inv = torch.from_numpy(np.linalg.inv(K)).float().to(DEV)
    s = [synth_planar_two_view(500 + i, n, 0.25, 0.5) for i in range(min(distinct, pairs))]
    pick = [i % len(s) for i in range(pairs)]
    k1, k2 = (torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in range(2))
    return dict(k1=k1, k2=k2, k_inv=k_inv, seed=seed, hyp=hyp)


def torch_score(h_h, p1, p2, thr):
    """(cost (B, H), best (B,)) of the homographies h_h (B, H, 3, 3) on the rows p1, p2 (B, N, 2), from stock torch ops"""
    g_h = torch.linalg.inv(h_h)                                             # |det H| G: a positive multiple of the model's G
    one = torch.ones_like(p1[..., :1])
    x1, x2 = torch.cat([p1, one], -1), torch.cat([p2, one], -1)
    a = torch.einsum("bhij,bnj->bhni", h_h, x1)
    b = torch.einsum("bhij,bnj->bhni", g_h, x2)
    da = a[..., :2] / a[..., 2:] - p2[:, None]
    db = b[..., :2] / b[..., 2:] - p1[:, None]
    d2 = (da * da).sum(-1) + (db * db).sum(-1)
    d2 = torch.where((a[..., 2] > 0) & (b[..., 2] > 0) & torch.isfinite(d2), d2, torch.full_like(d2, float("inf")))
    cost = torch.clamp(d2, max=thr * thr).sum(-1)
    return cost, torch.argmin(cost, dim=1)


def hip_pose(w, rounds=3):
    p1, p2 = ops.normalise_keypoints(w["k1"], w["k_inv"]), ops.normalise_keypoints(w["k2"], w["k_inv"])
    h, inlier, _, _, _ = ops.homography_ransac(p1, p2, None, w["hyp"], THR, rounds, w["seed"])
    return ops.homography_pose(h, p1, p2, inlier)


def test_torch_formulation_computes_the_same_cost():
    """the yardstick's cost of the kernel's own homographies is the kernel's cost (float32 both, another summation order
    and another inverse), and its argmin the kernel's selection wherever the two smallest costs are further apart than
    that tolerance"""
    w = workload(3, 97, 64, distinct=3)
    p1, p2 = ops.normalise_keypoints(w["k1"], w["k_inv"]), ops.normalise_keypoints(w["k2"], w["k_inv"])
    h_h, cost, _ = ops.homography_hypotheses(p1, p2, None, 64, THR, w["seed"])
    best_h = ops.homography_ransac(p1, p2, None, 64, THR, 0, w["seed"])[2]
    fin = torch.isfinite(cost)
    safe = torch.where(fin[..., None, None], h_h, torch.eye(3, device=DEV).expand_as(h_h))     # refused: zero matrices
    tcost, _ = torch_score(safe, p1, p2, THR)
    rel = ((cost - tcost).abs() / cost)[fin]
    print(f"accepted {fin.float().mean():.3f}; cost relative deviation max {rel.max():.2e}")
    assert fin.float().mean() >= 0.3 and rel.max() <= COST_RTOL              # 0.75^4 = 32 % of the samples are all-inlier
    two = torch.where(fin, cost, torch.full_like(cost, float("inf"))).sort(dim=1).values[:, :2]
    clear = two[:, 1] > two[:, 0] * (1 + COST_RTOL)
    tb = torch.where(fin, tcost, torch.full_like(tcost, float("inf"))).argmin(dim=1)
    assert torch.equal(tb[clear], best_h.long()[clear])


def test_hip_planar_pose_beats_torch_on_gpu_for_256_pairs():
    w = workload()
    p1, p2 = ops.normalise_keypoints(w["k1"], w["k_inv"]), ops.normalise_keypoints(w["k2"], w["k_inv"])
    h_h, cost, _ = ops.homography_hypotheses(p1, p2, None, HYP, THR, w["seed"])
    safe = torch.where(torch.isfinite(cost)[..., None, None], h_h, torch.eye(3, device=DEV).expand_as(h_h)).contiguous()
    one = torch.ones_like(p1[..., :1])
    x1, x2 = torch.cat([p1, one], -1), torch.cat([p2, one], -1)              # the same rows as 3-D points for K17
    hip = time_ms(lambda: hip_pose(w))
    hip_hyp = time_ms(lambda: ops.homography_hypotheses(p1, p2, None, HYP, THR, w["seed"]))
    ess = time_ms(lambda: ops.essential_ransac(p1, p2, None, HYP, 1.0 / 500.0, 3, w["seed"]))
    rigid = time_ms(lambda: ops.rigid_ransac(x1, x2, None, HYP, 0.05, 3, w["seed"]))
    ref = time_ms(lambda: torch_score(safe, p1, p2, THR))
    print(f"{PAIRS} pairs x {N_ROWS} rows x {HYP} hypotheses: HIP normalise + homography_ransac (3 rounds) + homography_pose "
          f"{hip:.3f} ms ({PAIRS / hip * 1e3:.0f} pairs/s), hypotheses alone {hip_hyp:.3f} ms; torch-on-GPU transfer error + "
          f"cost + argmin of given homographies {ref:.3f} ms ({ref / hip:.1f}x); mi_essential_ransac on the same shape "
          f"{ess:.3f} ms, mi_rigid_ransac {rigid:.3f} ms")
    assert hip < ref
