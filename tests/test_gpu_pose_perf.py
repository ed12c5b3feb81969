"""K15 rate: essential_ransac (256 hypotheses, 3 refinement rounds) + recover_pose on 256 pairs x 512 correspondences in
two calls beats a torch-on-GPU formulation of the hypothesis stage alone, written here from stock ops: batched gather of the
samples, Hartley normalisation, torch.linalg.eigh on A^T A, denormalisation, the (s, s, 0) projection by torch.linalg.svd, a
batched Sampson evaluation with the MSAC cost, argmin.  The yardstick does LESS than the timed HIP calls (no refinement, no
pose recovery).  A separate test shows that it computes the same thing as mi_essential_hypotheses."""
import numpy as np
import torch

import pose_oracle as PO
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_two_view, two_view_camera

pytestmark = GPU_PERF
K = two_view_camera()
THR = 1.0 / 500.0
PAIRS, N_CORR, HYP = 256, 512, 256


def workload(pairs=PAIRS, n=N_CORR, hyp=HYP, seed=17, distinct=16):
    """normalised points (pairs, n, 2) of both views on the GPU (`distinct` scenes, repeated) and the sample indices the
    header's sampler draws, (pairs, hyp, 8)"""
    k_inv = torch.from_numpy(np.linalg.inv(K)).float().to(DEV)
    s = [synth_two_view(500 + i, n, 0.25, 0.5) for i in range(min(distinct, pairs))]
    k1 = np.stack([s[i % len(s)][0] for i in range(pairs)])
    k2 = np.stack([s[i % len(s)][1] for i in range(pairs)])
    p1 = ops.normalise_keypoints(torch.from_numpy(k1).to(DEV), k_inv)
    p2 = ops.normalise_keypoints(torch.from_numpy(k2).to(DEV), k_inv)
    idx = torch.from_numpy(PO.sample_ranks_batch(seed, pairs, hyp, n)).to(DEV)
    return dict(p1=p1, p2=p2, idx=idx, seed=seed, hyp=hyp)


def torch_hypotheses(p1, p2, idx, thr):
    """(e_h (B, H, 3, 3), cost (B, H), count (B, H), best (B,)) from stock torch ops"""
    B, H = idx.shape[:2]
    flat = idx.reshape(B, H * 8)
    s1 = torch.gather(p1, 1, flat[..., None].expand(-1, -1, 2)).reshape(B, H, 8, 2)
    s2 = torch.gather(p2, 1, flat[..., None].expand(-1, -1, 2)).reshape(B, H, 8, 2)

    def hartley(s):
        c = s.mean(dim=2, keepdim=True)
        d = ((s - c) ** 2).sum(-1).mean(-1)
        sc = (2.0 ** 0.5) / torch.sqrt(d)
        return c[:, :, 0], sc, (s - c) * sc[..., None, None]
    c1, sc1, a1 = hartley(s1)
    c2, sc2, a2 = hartley(s2)
    x1, y1, x2, y2 = a1[..., 0], a1[..., 1], a2[..., 0], a2[..., 1]
    A = torch.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, torch.ones_like(x1)], dim=-1)
    _, vec = torch.linalg.eigh(A.transpose(-1, -2) @ A)
    eh = vec[..., 0].reshape(B, H, 3, 3)

    def tmat(c, sc):
        t = torch.zeros(B, H, 3, 3, device=c.device, dtype=c.dtype)
        t[..., 0, 0] = sc
        t[..., 1, 1] = sc
        t[..., 0, 2] = -sc * c[..., 0]
        t[..., 1, 2] = -sc * c[..., 1]
        t[..., 2, 2] = 1.0
        return t
    e = tmat(c2, sc2).transpose(-1, -2) @ eh @ tmat(c1, sc1)
    u, sv, vt = torch.linalg.svd(e)
    m = (sv[..., 0] + sv[..., 1]) / 2
    e = (u * torch.stack([m, m, torch.zeros_like(m)], dim=-1)[..., None, :]) @ vt
    ones = torch.ones_like(p1[..., :1])
    X1, X2 = torch.cat([p1, ones], -1), torch.cat([p2, ones], -1)              # (B, n, 3)
    ex = torch.einsum("bhij,bnj->bhni", e, X1)
    etx = torch.einsum("bhji,bnj->bhni", e, X2)
    r = (ex * X2[:, None]).sum(-1)
    den = ex[..., 0] ** 2 + ex[..., 1] ** 2 + etx[..., 0] ** 2 + etx[..., 1] ** 2
    d2 = r * r / den
    cost = torch.clamp(d2, max=thr * thr).sum(-1)
    count = (d2 <= thr * thr).sum(-1)
    return e, cost, count, torch.argmin(cost, dim=1)


def hip_pose(w, rounds=3):
    e, inl, _, _ = ops.essential_ransac(w["p1"], w["p2"], None, w["hyp"], THR, rounds, w["seed"])
    return ops.recover_pose(e, w["p1"], w["p2"], inl)


def test_torch_formulation_computes_the_same_thing():
    """The stock formulation takes the null vector from eigh of A^T A where the kernel eliminates the 8x9 system: the same
    vector.  Run in float64 it is an accurate statement of the operation, and the kernel agrees with it as the GPU suite's
    parity test asks of the kernel against the oracle: the same inlier count to within 1 on >= 90 % of the hypotheses, the
    cost within that suite's COST_RTOL = 1.2e-3 where the counts are equal, and the kernel's selected hypothesis costs the
    float64 minimum to that tolerance.  The float32 run that is timed squares the condition number of a minimal sample in
    A^T A, so single hypotheses of it can be percent off; it meets the same count cap against its own float64 run, and the
    median of its cost deviation stays inside the tolerance."""
    w = workload(3, 97, 64, distinct=3)
    e_h, cost, count = ops.essential_hypotheses(w["p1"], w["p2"], None, 64, THR, w["seed"])
    _, dcost, dcount, dbest = torch_hypotheses(w["p1"].double(), w["p2"].double(), w["idx"], THR)
    _, tcost, tcount, _ = torch_hypotheses(w["p1"], w["p2"], w["idx"], THR)
    dk = (count.long() - dcount).abs()
    same = dk == 0
    rel = ((cost.double() - dcost).abs() / dcost)[same]
    print(f"kernel against the float64 formulation: equal counts {same.float().mean():.3f}, |dcount| <= 1 {(dk <= 1).float().mean():.3f}; "
          f"cost relative deviation on equal counts: max {rel.max():.2e}")
    assert (dk <= 1).float().mean() >= 0.90
    assert rel.max() <= 1.2e-3
    best = torch.argmin(cost, dim=1)
    chosen, least = dcost.gather(1, best[:, None])[:, 0], dcost.gather(1, dbest[:, None])[:, 0]
    print(f"float64 cost of the kernel's selection over the float64 minimum - 1: {((chosen - least) / least).tolist()}")
    assert (chosen <= least * (1 + 1.2e-3)).all()
    tk = (tcount - dcount).abs()
    trel = ((tcost.double() - dcost).abs() / dcost)[tk == 0]
    print(f"float32 formulation against its float64 run: |dcount| <= 1 {(tk <= 1).float().mean():.3f}; cost relative deviation "
          f"median {trel.median():.2e} max {trel.max():.2e}")
    assert (tk <= 1).float().mean() >= 0.90 and trel.median() <= 1.2e-3


def test_hip_pose_beats_torch_on_gpu_for_256_pairs():
    w = workload()
    hip = time_ms(lambda: hip_pose(w))
    hip_hyp = time_ms(lambda: ops.essential_hypotheses(w["p1"], w["p2"], None, HYP, THR, w["seed"]))
    ref = time_ms(lambda: torch_hypotheses(w["p1"], w["p2"], w["idx"], THR))
    print(f"{PAIRS} pairs x {N_CORR} correspondences x {HYP} hypotheses: HIP ransac (3 rounds) + recover_pose {hip:.3f} ms "
          f"({PAIRS / hip * 1e3:.0f} pairs/s), hypotheses alone {hip_hyp:.3f} ms; torch-on-GPU hypotheses + argmin {ref:.3f} ms "
          f"({ref / hip:.1f}x)")
    assert hip < ref
