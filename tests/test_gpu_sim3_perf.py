"""K30 rate: sim3_ransac (128 hypotheses, 3 refinement rounds, reprojection metric) on 256 pairs x 512 rows beats a
torch-on-GPU formulation of the hypothesis stage alone, written here from stock ops: batched gather of the samples, Kabsch by
a batched 3x3 torch.linalg.svd with Umeyama's scale, a batched symmetric reprojection error with the MSAC cost, argmin.  The
yardstick does LESS than the timed HIP call (no refinement, no inlier mask, no degeneracy or range test).  A separate test
shows that it computes the same thing as mi_sim3_hypotheses.  The measured times are in README.md and DESIGN.md."""
import numpy as np
import torch

import rigid_oracle as RO
import sim3_oracle as SO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_sim3_maps

pytestmark = GPU_PERF
THR = SO.THR_REPROJ
PAIRS, N_ROWS, HYP = 256, 512, 128
COST_RTOL = 1.5e-4                       # tests/test_gpu_sim3.py


def workload(pairs=PAIRS, n=N_ROWS, hyp=HYP, seed=17, distinct=8):
    """camera-frame points of both maps (pairs, n, 3) on the GPU (`distinct` scenes, repeated) and the sample indices the
    header's sampler draws, (pairs, hyp, 3)"""
    s = [synth_sim3_maps(500 + i, n, 0.25, 0.003, 2.5) for i in range(min(distinct, pairs))]
    pick = [i % len(s) for i in range(pairs)]
    x1, x2 = (torch.from_numpy(np.stack([s[i][j] for i in pick])).to(DEV) for j in range(2))
    return dict(x1=x1, x2=x2, seed=seed, hyp=hyp, idx=torch.from_numpy(RO.sample_ranks_batch(seed, pairs, hyp, n)).to(DEV))


def torch_hypotheses(x1, x2, idx, thr):
    """(s (B, H), R (B, H, 3, 3), t (B, H, 3), cost (B, H), count (B, H), best (B,)) from stock torch ops"""
    B, H = idx.shape[:2]
    flat = idx.reshape(B, H * 3)[..., None].expand(-1, -1, 3)
    a = torch.gather(x1, 1, flat).reshape(B, H, 3, 3)
    b = torch.gather(x2, 1, flat).reshape(B, H, 3, 3)
    ca, cb = a.mean(dim=2, keepdim=True), b.mean(dim=2, keepdim=True)
    da, db = a - ca, b - cb
    u, _, vt = torch.linalg.svd(da.transpose(-1, -2) @ db)                     # sum a b^T
    v = vt.transpose(-1, -2)
    fix = torch.ones_like(u[..., 0])
    fix[..., 2] = torch.linalg.det(v @ u.transpose(-1, -2))
    r = (v * fix[..., None, :]) @ u.transpose(-1, -2)
    s = (db * (da @ r.transpose(-1, -2))).sum((-1, -2)) / (da * da).sum((-1, -2))
    t = cb[:, :, 0] - s[..., None] * torch.einsum("bhij,bhj->bhi", r, ca[:, :, 0])
    y = s[..., None, None] * torch.einsum("bhij,bnj->bhni", r, x1) + t[:, :, None]
    w = torch.einsum("bhji,bhnj->bhni", r, x2[:, None] - t[:, :, None]) / s[..., None, None]
    p1, p2 = (x1[..., :2] / x1[..., 2:])[:, None], (x2[..., :2] / x2[..., 2:])[:, None]
    d2 = ((y[..., :2] / y[..., 2:] - p2) ** 2).sum(-1) + ((w[..., :2] / w[..., 2:] - p1) ** 2).sum(-1)
    front = (y[..., 2] > 0) & (w[..., 2] > 0) & (x1[..., 2] > 0)[:, None] & (x2[..., 2] > 0)[:, None]
    d2 = torch.where(front, d2, torch.full_like(d2, float("inf")))
    cost = torch.clamp(d2, max=thr * thr).sum(-1)
    count = (d2 <= thr * thr).sum(-1)
    return s, r, t, cost, count, torch.argmin(cost, dim=1)


def test_torch_formulation_computes_the_same_thing():
    """Kabsch by SVD with Umeyama's scale and Horn's quaternion with it are two closed forms of one least-squares similarity.
    Run in float64 the stock formulation is an accurate statement of the operation, and the kernel agrees with it as the GPU
    suite's parity test asks of the kernel against the oracle: the same inlier count to within 1 on >= 90 % of the hypotheses
    the kernel accepts (the formulation has no degeneracy test), the cost within that suite's COST_RTOL where the counts are
    equal, and the kernel's selected hypothesis costs the float64 minimum to that tolerance."""
    w = workload(3, 97, 64, distinct=3)
    _, cost, count = ops.sim3_hypotheses(w["x1"], w["x2"], None, 64, THR, ops.SIM3_REPROJ, w["seed"])
    _, _, _, dcost, dcount, _ = torch_hypotheses(w["x1"].double(), w["x2"].double(), w["idx"], THR)
    fin = torch.isfinite(cost)
    dk = (count.long() - dcount).abs()
    same = (dk == 0) & fin
    rel = ((cost.double() - dcost).abs() / dcost)[same]
    print(f"kernel against the float64 formulation: accepted {fin.float().mean():.3f}, equal counts {same.float().mean():.3f}, "
          f"|dcount| <= 1 {(dk <= 1)[fin].float().mean():.3f}; cost relative deviation on equal counts: max {rel.max():.2e}")
    assert fin.float().mean() >= 0.9 and (dk <= 1)[fin].float().mean() >= 0.90
    assert rel.max() <= COST_RTOL
    best = torch.argmin(cost, dim=1)
    least = torch.where(fin, dcost, torch.full_like(dcost, float("inf"))).min(dim=1).values
    chosen = dcost.gather(1, best[:, None])[:, 0]
    print(f"float64 cost of the kernel's selection over the float64 minimum - 1: {((chosen - least) / least).tolist()}")
    assert (chosen <= least * (1 + COST_RTOL)).all()


def test_hip_sim3_beats_torch_on_gpu_for_256_pairs():
    w = workload()
    hip = time_ms(lambda: ops.sim3_ransac(w["x1"], w["x2"], None, HYP, THR, ops.SIM3_REPROJ, 3, w["seed"]))
    hip_hyp = time_ms(lambda: ops.sim3_hypotheses(w["x1"], w["x2"], None, HYP, THR, ops.SIM3_REPROJ, w["seed"]))
    hip_point = time_ms(lambda: ops.sim3_ransac(w["x1"], w["x2"], None, HYP, 0.1, ops.SIM3_POINT, 3, w["seed"]))
    rigid = time_ms(lambda: ops.rigid_ransac(w["x1"], w["x2"], None, HYP, 0.1, 3, w["seed"]))
    ref = time_ms(lambda: torch_hypotheses(w["x1"], w["x2"], w["idx"], THR))
    print(f"{PAIRS} pairs x {N_ROWS} rows x {HYP} hypotheses: HIP sim3_ransac (reprojection, 3 rounds) {hip:.3f} ms ({PAIRS / hip * 1e3:.0f} "
          f"pairs/s), hypotheses alone {hip_hyp:.3f} ms, point metric {hip_point:.3f} ms, rigid_ransac on the same rows {rigid:.3f} ms; "
          f"torch-on-GPU hypotheses + argmin {ref:.3f} ms ({ref / hip:.1f}x)")
    assert hip < ref
