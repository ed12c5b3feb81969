"""K30 similarity alignment on the GPU against tests/sim3_oracle.py (the fp64 numpy restatement of
include/mi355x_match_sim3.h).

`apply` is compared bit for bit with the numpy restatement of the header's float64 arithmetic, the rotation bit for bit with
mi_rigid_hypotheses, and the power-of-two invariance is exact.  Everything else is fp32 kernels against an fp64 oracle, which
cannot agree bit for bit; each bound below is a deviation from the float64 oracle measured on the CPU on the very scenes these
tests use -- the larger of the SAME oracle run in float32 and of the kernels' arithmetic compiled for the host
(tests/native/sim3_host.cpp) -- times 2.  The scenes are synth_sim3_maps at scale 2.5, so translations are in map-2 units
with points up to 25 units from the camera; thresholds 0.1 (point) and 0.004 (reprojection).
  - per-hypothesis parity (25 % outliers, ray noise 0.003, (n, H) = (64, 200), (97, 200), (65, 65), 9 pairs, both metrics):
    every hypothesis accepted (cap: >= 90 %); the float32 oracle and the native lane had the float64 count to within 1 on
    100 % of them (cap: >= 90 %); over ALL accepted hypotheses the model deviated by at most 4.05e-4 deg / 2.82e-7 relative
    in s / 9.33e-5 in t (float32 oracle) and 7.57e-4 deg / 4.04e-7 / 1.19e-4 (native) -> HYP_ROT_DEG = 1.6e-3, HYP_S_REL =
    8.1e-7, HYP_T = 2.4e-4; on equal counts the MSAC cost by 7.41e-5 relative (float32 oracle, point metric; native 5.53e-5)
    -> COST_RTOL = 1.5e-4;
  - refit on the planted inliers (n = 64 / 97, ray noise 0 / 0.003, 12 pairs): float32 oracle 7.28e-6 deg, 2.08e-7, 6.90e-6;
    native 1.52e-5 deg, 3.46e-7, 1.08e-5 -> REFIT_ROT_DEG = 3.1e-5, REFIT_S_REL = 7.0e-7, REFIT_T = 2.2e-5; at n = 2048 (ray noise
    0.003, 3 pairs): float32 oracle 7.37e-6 deg, 2.01e-7, 1.75e-5; native 6.85e-6 deg, 6.06e-7, 1.94e-5 -> REFIT_2048 = 1.5e-5
    deg, 1.22e-6, 3.9e-5;
  - refined output (test_selection_is_exact's scenes, 3 rounds, both metrics): the float32 oracle is within 8.46e-6 deg,
    2.29e-7 and 6.22e-6 of the float64 run with equal inlier masks and equal best_h; a refined model is a refit of an inlier
    set, and the native refit deviates by more than that, so the refit's bounds hold here too;
  - a minimal solve (n = 3, H = 1): the bounds of tests/test_sim3_host.py, 6.9e-4 deg, 6.9e-7 and 1.9e-4 (192 samples).
  - rmse against the float64 evaluation of the same model over the same rows (test_selection_is_exact's scenes, 0 and 3
    rounds): float32 oracle 4.32e-7 (point) and 7.59e-9 (reprojection), the native program's strided sums 2.77e-7 and 1.99e-9
    -> RMSE_ABS = 8.7e-7 and 1.6e-8; the rmse of a minimal solve's own three rows (n = 3, H = 1), a fit residual and not an
    evaluation error: float32 oracle 1.42e-6 and 8.42e-8, native 2.70e-6 and 1.92e-7 -> SOLVE_RMSE = 5.4e-6 and 3.9e-7.
  - rows within 1e-3 relative of the threshold are left out of the mask comparisons; cap: at most 2 such rows per pair (the
    oracle: 0 on every pair of these scenes).
Reprojection against point metric (97 rows, 40 % outliers, ray noise 0.01, 128 hypotheses, 3 rounds, 5 scenes): the float64
and float32 oracles keep 45, 57, 53, 31, 39 of 58 planted inliers under the reprojection metric and 12, 19, 19, 12, 14 under
the point metric at the matched threshold (0.004 x the 15-unit median depth), none false, with equal masks and best_h;
|s / 2.5 - 1| = 5.04e-3, 1.39e-3, 3.31e-3, 2.42e-3, 2.71e-3 in both -> S_RECOVERY = 1.01e-2.  The result is also held to the
float64 oracle's per scene at the refit's bounds (on these scenes: float32 oracle 4.07e-6 deg / 8.69e-8 / 3.05e-6, the native
refit of the final inlier sets 1.07e-5 deg / 1.34e-7 / 6.58e-6).  Every scene has 25 to 35 all-inlier samples among its 128
(the test re-checks one exists).
Two windows sharing a frame (sim3_oracle.shared_frame_windows, 20 shared landmarks; tests/test_sim3_host.py runs the same
chain on tests/tracks_oracle.py).  Deviation from the planted (3, I, 0) and, after `apply`, of the shared frame's pose from
window B's, float64 / float32 oracle: reprojection metric 2.15e-5 in s, 3.47e-4 deg, 1.07e-4 in t, moved frame 3.47e-4 deg and
1.07e-4 in its centre -> E2E[REPROJ] = 4.3e-5, 7.0e-4 deg, 2.2e-4; point metric at 6e-3: 6.75e-5, 9.49e-4 deg, 5.33e-4 ->
E2E[POINT] = 1.4e-4, 1.9e-3 deg, 1.07e-3.  19 of the 20 shared landmarks lie within 6e-3 after `apply` under EITHER metric
(cap: >= 19; the twentieth is 1.2e-2 off along its ray, which the reprojection metric cannot see); inlier counts 20 and 19.
The model is also held to the float64 oracle's on the kernels' own pairs at the refit's bounds (float32 oracle 1.06e-6 deg /
1.26e-7 / 2.88e-6, native refit 1.44e-6 deg / 1.27e-7 / 2.95e-6).
align_trajectory (two random walks of 200 centres, the second with 150 valid): against the float64 refit the float32 oracle
deviates by 3.44e-5 deg / 2.34e-7 / 2.27e-5, the native refit by 1.36e-5 deg / 2.57e-7 / 8.57e-6 -> TRAJ = 6.9e-5 deg, 5.2e-7,
4.6e-5; the float64 refit is within 6.1e-7 deg and 4.9e-9 of the planted similarity -> 7.0e-5 deg and 5.3e-7 against the
planted; the float32 torch rmse of the float32 / native model is 1.32e-6 / 1.29e-6 (trajectory 0) and 1.22e-5 / 5.05e-6
(trajectory 1) from the float64 one -> TRAJ_RMSE = 2.7e-6, 2.5e-5."""
import functools

import numpy as np
import pytest
import torch

import pose_oracle as PO
import rigid_oracle as RO
import sim3_oracle as SO
from gpu_common import DEV, GPU, bits, gpu, same_bits, twice
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import LandmarkTracks, SimilarityEstimator
from onnx_image_processing_amd.synth import two_view_camera

pytestmark = GPU
SCALE = 2.5
THR = {SO.POINT: 0.1, SO.REPROJ: SO.THR_REPROJ}
METRICS = [SO.POINT, SO.REPROJ]
HYP_ROT_DEG, HYP_S_REL, HYP_T, COST_RTOL = 1.6e-3, 8.1e-7, 2.4e-4, 1.5e-4
REFIT_ROT_DEG, REFIT_S_REL, REFIT_T = 3.1e-5, 7.0e-7, 2.2e-5
REFIT_2048 = (1.5e-5, 1.22e-6, 3.9e-5)
SOLVE_ROT_DEG, SOLVE_S_REL, SOLVE_T = 6.9e-4, 6.9e-7, 1.9e-4
RMSE_ABS = {SO.POINT: 8.7e-7, SO.REPROJ: 1.6e-8}
SOLVE_RMSE = {SO.POINT: 5.4e-6, SO.REPROJ: 3.9e-7}
S_RECOVERY = 1.01e-2
BAND_CAP = 2                             # rows per pair within 1e-3 relative of the threshold, left out of a mask comparison
E2E = {SO.REPROJ: (4.3e-5, 7.0e-4, 2.2e-4), SO.POINT: (1.4e-4, 1.9e-3, 1.07e-3)}       # s relative, degrees, position
E2E_WITHIN = 19
TRAJ_ROT_DEG, TRAJ_S_REL, TRAJ_T, TRAJ_PLANTED_ROT_DEG, TRAJ_PLANTED_S_REL = 6.9e-5, 5.2e-7, 4.6e-5, 7.0e-5, 5.3e-7
TRAJ_RMSE = (2.7e-6, 2.5e-5)


@functools.lru_cache(maxsize=None)
def maps(seeds, n, outliers, ray_noise, scale=SCALE):
    out = SO.maps(seeds, n, outliers, ray_noise, scale)
    for a in (out[0], out[1], out[5]):
        a.setflags(write=False)
    return out


def model_error(s, R, t, ref):
    """(rotation deg, relative scale, translation) of a GPU model against the oracle's (s, R, t)"""
    return (PO.rotation_angle_deg(np.asarray(R, np.float64).reshape(3, 3), ref[1]), SO.scale_error(s, ref[0]),
            float(np.linalg.norm(np.asarray(t, np.float64) - ref[2])))


# ---- hypotheses ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,H", [(64, 200), (97, 200), (65, 65)])
def test_hypotheses_match_the_oracle_per_hypothesis(n, H, metric):
    seed = 7
    x1, x2, _, _, _, _ = maps((100, 101, 102), n, 0.25, 0.003)
    srt_h, cost, count = (x.cpu().numpy() for x in ops.sim3_hypotheses(*gpu(x1, x2), None, H, THR[metric], metric, seed))
    for b in range(3):
        osrt, oc, ok_, _ = SO.hypotheses(x1[b], x2[b], None, H, THR[metric], metric, seed, b)
        assert np.array_equal(np.isinf(cost[b]), np.isinf(oc))                 # equal refusals
        assert not srt_h[b][np.isinf(cost[b])].any() and not count[b][np.isinf(cost[b])].any()
        fin = np.isfinite(oc)
        dk = np.abs(count[b].astype(np.int64) - ok_)
        same = (dk == 0) & fin
        rel = np.abs(cost[b][same].astype(np.float64) - oc[same]) / oc[same]
        err = np.array([model_error(srt_h[b, h, 12], srt_h[b, h, :9], srt_h[b, h, 9:12], (osrt[h, 12], osrt[h, :9].reshape(3, 3), osrt[h, 9:12]))
                        for h in np.flatnonzero(fin)])
        print(f"metric {metric} n={n} H={H} pair {b}: accepted {fin.mean():.3f}, equal counts {np.mean(dk == 0):.3f}, |dcount| <= 1 "
              f"{np.mean(dk <= 1):.3f}; cost rel dev on equal counts max {rel.max():.2e}; rotation {err[:, 0].max():.2e} deg, scale "
              f"{err[:, 1].max():.2e}, translation {err[:, 2].max():.2e}")
        assert fin.mean() >= 0.90 and np.mean(dk <= 1) >= 0.90
        assert rel.max() <= COST_RTOL
        assert err[:, 0].max() <= HYP_ROT_DEG and err[:, 1].max() <= HYP_S_REL and err[:, 2].max() <= HYP_T


@pytest.mark.parametrize("n,H", [(3, 1), (64, 200), (97, 65), (2048, 64)])
def test_rotation_is_the_rigid_solvers_bit_for_bit(n, H):
    """the R of srt_h equals mi_rigid_hypotheses' R wherever both accept: the same rows, the same seed, the same solve"""
    x1, x2, _, _, _, _ = maps((100, 101, 102, 103, 104)[:2 if n == 2048 else 5], n, 0.25, 0.003)
    valid = np.ones(x1.shape[:2], bool)
    if n > 3:
        valid[1, ::5] = False
    g1, g2, gv = gpu(x1, x2, valid)
    rt_h, rcost, _ = ops.rigid_hypotheses(g1, g2, gv, H, 0.1, 13)
    both = torch.isfinite(rcost)
    for metric in METRICS:
        srt_h, cost, _ = ops.sim3_hypotheses(g1, g2, gv, H, THR[metric], metric, 13)
        assert torch.equal(torch.isfinite(cost), both)                       # scale 2.5: the range test refuses nothing here
        assert both.float().mean() >= (0.9 if n > 3 else 0.5)              # n = 3: five samples in all
        assert torch.equal(bits(srt_h[..., :9][both]), bits(rt_h[..., :9][both]))
        # the whole estimator at this shape: the selection is the hypotheses' first minimum, the mask is counted
        s, r, t, inlier, best_h, cnt, rmse, ok = ops.sim3_ransac(g1, g2, gv, H, THR[metric], metric, 3, 13)
        assert np.array_equal(best_h.cpu().numpy(), np.argmin(cost.cpu().numpy(), axis=1)) and torch.equal(cnt.long(), inlier.sum(1))
        assert not (inlier & ~gv).any() and torch.equal(ok, cnt >= 3)


@pytest.mark.parametrize("k", [-3, 1, 4])
def test_power_of_two_invariance_is_exact(k):
    """pts2 and the point threshold times 2^k: R, inlier and best_h bit-identical, s and t exactly 2^k times the originals"""
    n, H, f = 97, 65, np.float32(2.0 ** k)
    x1, x2, _, _, _, _ = maps((100, 101, 102), n, 0.25, 0.003)
    valid = np.ones((3, n), bool)
    valid[2, 3::7] = False
    g1, g2, gv = gpu(x1, x2, valid)
    g2k = gpu(x2 * f)
    for rounds in (0, 3):
        a = ops.sim3_ransac(g1, g2, gv, H, THR[SO.POINT], SO.POINT, rounds, 5)
        b = ops.sim3_ransac(g1, g2k, gv, H, float(np.float32(THR[SO.POINT]) * f), SO.POINT, rounds, 5)
        assert a[7].all() and torch.equal(a[7], b[7])
        assert torch.equal(bits(a[1]), bits(b[1])) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
        assert torch.equal(bits(a[0] * float(f)), bits(b[0])) and torch.equal(bits(a[2] * float(f)), bits(b[2]))
        assert torch.equal(bits(a[6] * float(f)), bits(b[6]))                # the rmse is in frame 2's units
    ha = ops.sim3_hypotheses(g1, g2, gv, H, THR[SO.POINT], SO.POINT, 5)
    hb = ops.sim3_hypotheses(g1, g2k, gv, H, float(np.float32(THR[SO.POINT]) * f), SO.POINT, 5)
    assert torch.equal(bits(ha[0][..., :9]), bits(hb[0][..., :9])) and torch.equal(bits(ha[0][..., 9:] * float(f)), bits(hb[0][..., 9:]))
    assert torch.equal(ha[2], hb[2]) and torch.equal(bits(ha[1] * float(f) * float(f)), bits(hb[1]))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,H", [(64, 1), (97, 64), (64, 200)])
def test_selection_is_exact(n, H, metric):
    thr = THR[metric]
    x1, x2, _, _, _, _ = maps((100, 101, 102), n, 0.25, 0.003)
    valid = np.ones((3, n), bool)
    valid[2, 3::7] = False
    g1, g2, v = gpu(x1, x2, valid)
    srt_h, cost, count = ops.sim3_hypotheses(g1, g2, v, H, thr, metric, 9)
    s, r, t, inlier, best_h, cnt, rmse, ok = ops.sim3_ransac(g1, g2, v, H, thr, metric, 0, 9)
    cost_np = cost.cpu().numpy()
    q1, q2 = x1.astype(np.float64), x2.astype(np.float64)
    for b in range(3):
        bh = int(np.argmin(cost_np[b]))                                        # numpy: the first minimum
        assert int(best_h[b]) == bh
        if not bool(ok[b]):                                                    # H = 1: the only sample may explain < 3 rows
            assert int(count[b, bh]) < 3 and int(cnt[b]) == 0 and not inlier[b].any() and float(s[b]) == 1.0
            continue
        assert torch.equal(bits(r[b].reshape(9)), bits(srt_h[b, bh, :9])) and torch.equal(bits(t[b]), bits(srt_h[b, bh, 9:12]))
        assert torch.equal(bits(s[b:b + 1]), bits(srt_h[b, bh, 12:13]))
        assert int(cnt[b]) == int(count[b, bh]) == int(inlier[b].sum())
        got = inlier[b].cpu().numpy()
        assert not (got & ~valid[b]).any()
        d2 = SO.dist2(float(s[b]), r[b].cpu().numpy().astype(np.float64), t[b].cpu().numpy().astype(np.float64), q1[b], q2[b], metric)
        clear = np.abs(d2 / thr ** 2 - 1) > 1e-3                               # not within rounding of the threshold
        assert (~clear & valid[b]).sum() <= BAND_CAP
        assert np.array_equal(got[clear], ((d2 <= thr ** 2) & valid[b])[clear])
        assert abs(float(rmse[b]) - np.sqrt(d2[got].mean())) <= RMSE_ABS[metric]
    # refinement never raises the float64 cost; more rounds keep that
    for rounds in (3, 8):
        s3, r3, t3, inl3, bh3, cnt3, rmse3, ok3 = ops.sim3_ransac(g1, g2, v, H, thr, metric, rounds, 9)
        assert torch.equal(bh3, best_h)
        for b in range(3):
            if not bool(ok[b]):
                continue
            a, bb = q1[b][valid[b]], q2[b][valid[b]]
            c0 = SO.step_cost(float(s[b]), r[b].cpu().numpy().astype(np.float64), t[b].cpu().numpy().astype(np.float64), a, bb, thr, metric)
            c3 = SO.step_cost(float(s3[b]), r3[b].cpu().numpy().astype(np.float64), t3[b].cpu().numpy().astype(np.float64), a, bb, thr, metric)
            assert bool(ok3[b]) and c3 <= c0 * (1 + COST_RTOL)
        if rounds != 3:
            continue
        # the refined model and mask are the oracle's (float64, the header's step cost)
        for b in range(3):
            so, Ro, to, mo, bho, cno, rmo, oko = SO.ransac(x1[b], x2[b], valid[b], H, thr, metric, 3, 9, b)
            assert bool(ok3[b]) == oko
            if not oko:
                continue
            rot, ds, dt = model_error(float(s3[b]), r3[b].cpu().numpy(), t3[b].cpu().numpy(), (so, Ro, to))
            print(f"refined metric {metric} n={n} H={H} pair {b}: rotation {rot:.2e} deg, scale {ds:.2e}, translation {dt:.2e} against the "
                  f"oracle; count {int(cnt3[b])} / {cno}")
            assert int(bh3[b]) == bho and rot <= REFIT_ROT_DEG and ds <= REFIT_S_REL and dt <= REFIT_T
            d2 = SO.dist2(so, Ro, to, q1[b], q2[b], metric)
            clear = np.abs(d2 / thr ** 2 - 1) > 1e-3
            assert (~clear & valid[b]).sum() <= BAND_CAP
            assert np.array_equal(inl3[b].cpu().numpy()[clear], mo[clear])
            got3 = inl3[b].cpu().numpy()
            d3 = SO.dist2(float(s3[b]), r3[b].cpu().numpy().astype(np.float64), t3[b].cpu().numpy().astype(np.float64), q1[b], q2[b], metric)
            assert abs(float(rmse3[b]) - np.sqrt(d3[got3].mean())) <= RMSE_ABS[metric]


# ---- refit ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,noise", [(64, 0.0), (64, 0.003), (97, 0.0), (97, 0.003), (2048, 0.003)])
def test_refit_matches_the_oracle(n, noise):
    x1, x2, s, R, t, inl = maps((100, 101, 102), n, 0.25, noise)
    inl = inl.copy()
    inl[1, :] &= np.arange(n) % 3 != 0                                         # a middle pair with a different mask
    g1, g2 = gpu(x1, x2)
    sg, r, tg, ok = ops.sim3_refit(g1, g2, gpu(inl))
    assert ok.all()
    # the refit's sums are K17's in K17's order: the same rotation, bit for bit
    assert torch.equal(bits(r), bits(ops.rigid_refit(g1, g2, gpu(inl))[0]))
    for b in range(3):
        ref = SO.refit(x1[b], x2[b], inl[b])
        rot, ds, dt = model_error(float(sg[b]), r[b].cpu().numpy(), tg[b].cpu().numpy(), ref)
        print(f"refit n={n} noise={noise} pair {b}: rotation {rot:.2e} deg, scale {ds:.2e}, translation {dt:.2e}")
        bound = REFIT_2048 if n == 2048 else (REFIT_ROT_DEG, REFIT_S_REL, REFIT_T)
        assert rot <= bound[0] and ds <= bound[1] and dt <= bound[2]
    # 2 rows; collinear rows (in frame 1 only: pair 1; in both: pair 2)
    few = np.zeros((3, n), bool)
    few[0, np.flatnonzero(inl[0])[:2]] = True
    few[1:, :8] = True
    line = torch.from_numpy((np.outer(np.arange(8.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]).astype(np.float32)).to(DEV)
    y1, y2 = g1.clone(), g2.clone()
    y1[1, :8] = line
    y1[2, :8] = line
    y2[2, :8] = SCALE * line + 0.25
    sg, r, tg, ok = ops.sim3_refit(y1, y2, gpu(few))
    assert not ok.any() and torch.equal(r, torch.eye(3, device=DEV).expand(3, 3, 3)) and not tg.any() and (sg == 1).all()


# ---- the two metrics -------------------------------------------------------------------------------------------------------------

def test_reprojection_metric_keeps_the_inliers_that_ray_noise_takes_from_the_point_metric():
    n, H, seeds = 97, 128, (300, 301, 302, 303, 304)
    x1, x2, s, R, t, inl = maps(seeds, n, 0.4, 0.01)
    for b in range(5):                                                         # every scene has an all-inlier sample
        assert any(inl[b][RO.sample_ranks(11, b, h, n)].all() for h in range(H)), seeds[b]
    g1, g2 = gpu(x1, x2)
    rp = SimilarityEstimator("reprojection", 2.0, focal=500.0, num_hypotheses=H, refine_rounds=3, seed=11).to(DEV)
    pt = SimilarityEstimator("point", SO.THR_REPROJ * 6.0 * SCALE, num_hypotheses=H, refine_rounds=3, seed=11).to(DEV)
    a, p = rp(g1, g2), pt(g1, g2)
    for b in range(5):
        ia, ip = a[3][b].cpu().numpy(), p[3][b].cpu().numpy()
        print(f"seed {seeds[b]}: planted {inl[b].sum()}; reprojection keeps {(ia & inl[b]).sum()} (false {(ia & ~inl[b]).sum()}), s error "
              f"{float(a[0][b]) / SCALE - 1:.2e}, rmse {float(a[5][b]):.3f} px; point keeps {(ip & inl[b]).sum()} (false "
              f"{(ip & ~inl[b]).sum()}), s error {float(p[0][b]) / SCALE - 1:.2e}")
        assert bool(a[6][b]) and (ia & inl[b]).sum() > (ip & inl[b]).sum()
        assert int(a[4][b]) == ia.sum() and (ia & inl[b]).sum() >= 30
        assert SO.scale_error(float(a[0][b]), SCALE) <= S_RECOVERY
        so, Ro, to, mo, _, cno, _, oko = SO.ransac(x1[b], x2[b], None, H, SO.THR_REPROJ, SO.REPROJ, 3, 11, b)
        rot, ds, dt = model_error(float(a[0][b]), a[1][b].cpu().numpy(), a[2][b].cpu().numpy(), (so, Ro, to))
        print(f"    against the oracle: rotation {rot:.2e} deg, scale {ds:.2e}, translation {dt:.2e}; count {ia.sum()} / {cno}")
        d2 = SO.dist2(so, Ro, to, x1[b].astype(np.float64), x2[b].astype(np.float64), SO.REPROJ)
        clear = np.abs(d2 / SO.THR_REPROJ ** 2 - 1) > 1e-3
        assert oko and (~clear).sum() <= BAND_CAP and np.array_equal(ia[clear], mo[clear])
        assert rot <= REFIT_ROT_DEG and ds <= REFIT_S_REL and dt <= REFIT_T
        assert 0 < float(a[5][b]) <= 2.0                                       # pixels: below the threshold


# ---- apply -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames,landmarks", [(4, 97), (0, 300), (16, 0), (1, 2048)])
def test_apply_is_the_float64_formula_rounded_once(frames, landmarks):
    rng = np.random.default_rng(frames + landmarks)
    B = 3
    s = rng.uniform(0.3, 4.0, B).astype(np.float32)
    R = np.stack([SO.rodrigues(rng.normal(size=3) * 0.5) for _ in range(B)]).astype(np.float32)
    t = rng.normal(size=(B, 3)).astype(np.float32) * 3
    Rk = np.stack([[SO.rodrigues(rng.normal(size=3) * 0.5) for _ in range(frames)] for _ in range(B)]).astype(np.float32).reshape(B, frames, 3, 3)
    tk = rng.normal(size=(B, frames, 3)).astype(np.float32) * 2
    X = (rng.normal(size=(B, landmarks, 3)) * 4 + [0, 0, 8]).astype(np.float32)
    m = SimilarityEstimator().to(DEV)

    def run():
        out = m.apply(*gpu(s, R, t), gpu(Rk) if frames else None, gpu(tk) if frames else None, gpu(X) if landmarks else None)
        return tuple(None if o is None else o.cpu().numpy() for o in out)
    ro, to, xo = twice("sim3_apply", run)
    assert (ro is None) == (frames == 0) and (xo is None) == (landmarks == 0)
    for b in range(B):
        wr, wt, wx = SO.apply(s[b], R[b], t[b], Rk[b] if frames else None, tk[b] if frames else None, X[b] if landmarks else None)
        if frames:
            assert np.array_equal(bits(ro[b]), bits(wr)) and np.array_equal(bits(to[b]), bits(wt))
        if landmarks:
            assert np.array_equal(bits(xo[b]), bits(wx))
    if frames and landmarks:                                                   # R_k' X' + t_k' = s (R_k X + t_k), to float32 rounding
        lhs = np.einsum("bfij,bnj->bfni", ro.astype(np.float64), xo.astype(np.float64)) + to[:, :, None].astype(np.float64)
        rhs = s[:, None, None, None] * (np.einsum("bfij,bnj->bfni", Rk.astype(np.float64), X.astype(np.float64)) + tk[:, :, None].astype(np.float64))
        # the stored R_k', t_k', X' are each within half an ulp: values up to ~100 (s 4 x |X| 25), 3 products of them
        assert np.abs(lhs - rhs).max() <= 4 * 100 * 6e-8 * 4
    single = m.apply(*(x[0] for x in gpu(s, R, t)), gpu(Rk)[0] if frames else None, gpu(tk)[0] if frames else None, gpu(X)[0] if landmarks else None)
    assert all((a is None and c is None) or np.array_equal(bits(a.cpu().numpy()), bits(c[0])) for a, c in zip(single, (ro, to, xo)))


# ---- the whole path --------------------------------------------------------------------------------------------------------------

def test_two_windows_sharing_a_frame_are_aligned_end_to_end():
    """sim3_oracle.shared_frame_windows: frames 0..3 and 3..5 of one noise-free scene, tracked and triangulated as two windows
    with the true poses, the second in a map of its own (scale 3, rotated, shifted).  landmark_pairs on the shared frame's
    keypoints -> forward -> apply: window A's pose of the shared frame and its landmarks land on window B's.  Both points of a
    pair lie on ONE ray of the shared keyframe, so the reprojection metric cannot see how far along it they are apart; both
    metrics have to place the shared frame and leave the shared landmarks within 6e-3 of each other, all but the one whose two
    triangulations differ.  Bounds and caps: module docstring."""
    K = two_view_camera()
    A, B = SO.shared_frame_windows()
    (kpA, pfA, ijA, mvA, RA, tA), (kpB, pfB, ijB, mvB, RB, tB) = A, B
    tracks = LandmarkTracks(torch.from_numpy(K), max_landmarks=64).to(DEV)
    oa, ob = tracks(*gpu(*A)), tracks(*gpu(*B))
    pointsA, okA, kp_trackA = oa[0], oa[3], oa[5]
    pointsB, okB, kp_trackB = ob[0], ob[3], ob[5]
    k = kpA.shape[1]
    ij = torch.arange(k, device=DEV, dtype=torch.int32)[:, None].expand(k, 2).contiguous()       # the shared frame against itself
    p1, p2, valid = SimilarityEstimator.landmark_pairs(ij, torch.ones(k, dtype=torch.bool, device=DEV), kp_trackA, 3, pointsA, okA,
                                                       gpu(RA), gpu(tA), kp_trackB, 0, pointsB, okB, gpu(RB), gpu(tB))
    shared = int(valid.sum())
    assert shared == 20
    q1, q2, vn = p1.cpu().numpy(), p2.cpu().numpy(), valid.cpu().numpy()
    centre = lambda Rx, tx: -(np.asarray(Rx, np.float64).T @ np.asarray(tx, np.float64))
    la, lb = kp_trackA[3].long().clamp(min=0), kp_trackB[0].long().clamp(min=0)
    for est in (SimilarityEstimator("reprojection", 2.0, focal=500.0, num_hypotheses=128, refine_rounds=3, seed=3).to(DEV),
                SimilarityEstimator("point", SO.E2E_TOL, num_hypotheses=128, refine_rounds=3, seed=3).to(DEV)):
        s_tol, rot_tol, pos_tol = E2E[est.metric_id]
        s, R, t, inlier, count, rmse, ok = est(p1, p2, valid)
        # the kernels' own pairs through the float64 oracle: the same selection, mask and, to the refit's bounds, model
        so, Ro, to, mo, bho, cno, _, oko = SO.ransac(q1, q2, vn, 128, est.kernel_threshold, est.metric_id, 3, 3, 0)
        rot, ds, dt = model_error(float(s), R.cpu().numpy(), t.cpu().numpy(), (so, Ro, to))
        d2 = SO.dist2(so, Ro, to, q1.astype(np.float64), q2.astype(np.float64), est.metric_id)
        clear = np.abs(d2 / est.kernel_threshold ** 2 - 1) > 1e-3
        assert bool(ok) and oko and int(count) == cno and (~clear & vn).sum() <= BAND_CAP
        assert np.array_equal(inlier.cpu().numpy()[clear], mo[clear])
        assert rot <= REFIT_ROT_DEG and ds <= REFIT_S_REL and dt <= REFIT_T
        # the points are in the shared frame's CAMERA frame on both sides: the similarity between them is (sigma, I, 0)
        r_id = PO.rotation_angle_deg(R.cpu().numpy(), np.eye(3))
        print(f"{est.metric}: shared landmarks {shared}, inliers {int(count)}, s error {SO.scale_error(float(s), SO.E2E_SIGMA):.2e}, rotation "
              f"{r_id:.2e} deg, |t| {float(t.norm()):.2e}, rmse {float(rmse):.2e}; against the oracle {rot:.2e} deg, {ds:.2e}, {dt:.2e}")
        assert SO.scale_error(float(s), SO.E2E_SIGMA) <= s_tol and r_id <= rot_tol and float(t.norm()) <= pos_tol
        # camera frame A3 -> map B: compose with the shared frame's poses, then move the whole of window A
        s_ab, R_ab, t_ab = SO.compose_to_map(float(s), R.cpu().numpy(), t.cpu().numpy(), RA[3], tA[3], RB[0], tB[0])
        Rm, tm, Xm = est.apply(s, gpu(R_ab.astype(np.float32)), gpu(t_ab.astype(np.float32)), gpu(RA), gpu(tA), pointsA)
        rot = PO.rotation_angle_deg(Rm[3].cpu().numpy(), RB[0])
        dc = float(np.linalg.norm(centre(Rm[3].cpu().numpy(), tm[3].cpu().numpy()) - centre(RB[0], tB[0])))
        dist = (Xm[la] - pointsB[lb]).norm(dim=1)
        within = int((dist[valid] <= SO.E2E_TOL).sum())
        print(f"    moved window: shared frame rotation {rot:.2e} deg, centre {dc:.2e}; shared landmarks within {SO.E2E_TOL}: {within} of "
              f"{shared}, its inliers' max {float(dist[inlier].max()):.2e}")
        assert rot <= rot_tol and dc <= pos_tol and within >= E2E_WITHIN


def test_align_trajectory_recovers_a_planted_similarity():
    rng = np.random.default_rng(4)
    B, n = 2, 200
    steps = rng.normal(size=(B, n, 3)) * [0.3, 0.05, 0.3]
    est_c = np.cumsum(steps, axis=1).astype(np.float32)
    s0 = np.array([0.37, 12.0])
    R0 = np.stack([SO.rodrigues([0.2, 1.1, -0.3]), SO.rodrigues([-2.0, 0.4, 0.9])])
    t0 = np.array([[3.0, -1.0, 7.0], [-40.0, 15.0, 2.0]])
    ref_c = (s0[:, None, None] * np.einsum("bij,bnj->bni", R0, est_c.astype(np.float64)) + t0[:, None]).astype(np.float32)
    valid = np.ones((B, n), bool)
    valid[1, 150:] = False
    held = ref_c.copy()
    held[1, 150:] = 1e6                                                        # rows that are not valid do not count
    m = SimilarityEstimator("point", 0.1).to(DEV)
    s, R, t, rmse = m.align_trajectory(*gpu(est_c, held, valid))
    for b in range(B):
        v = valid[b]
        ref = SO.refit(est_c[b], ref_c[b], v)
        rot, ds, dt = model_error(float(s[b]), R[b].cpu().numpy(), t[b].cpu().numpy(), ref)
        want = np.sqrt((np.linalg.norm(ref[0] * (est_c[b][v].astype(np.float64) @ ref[1].T) + ref[2] - ref_c[b][v], axis=1) ** 2).mean())
        print(f"trajectory {b}: against the oracle rotation {rot:.2e} deg, scale {ds:.2e}, translation {dt:.2e}; against the planted "
              f"s {SO.scale_error(float(s[b]), s0[b]):.2e}, rotation {PO.rotation_angle_deg(R[b].cpu().numpy(), R0[b]):.2e} deg; rmse "
              f"{float(rmse[b]):.2e} (float64 {want:.2e})")
        assert rot <= TRAJ_ROT_DEG and ds <= TRAJ_S_REL and dt <= TRAJ_T
        assert SO.scale_error(float(s[b]), s0[b]) <= TRAJ_PLANTED_S_REL and PO.rotation_angle_deg(R[b].cpu().numpy(), R0[b]) <= TRAJ_PLANTED_ROT_DEG
        assert abs(float(rmse[b]) - want) <= TRAJ_RMSE[b]
    single = m.align_trajectory(*(x[0] for x in gpu(est_c, held, valid)))
    assert all(torch.equal(bits(x.reshape(-1)), bits(y[0].reshape(-1))) for x, y in zip(single, (s, R, t, rmse)))


def test_degenerate_pairs_and_small_shapes():
    """n = 3 with H = 1: the only sample; n = 4 with 2 valid rows and with none; all-collinear points; a scale out of range"""
    x1, x2, _, _, _, _ = maps((20, 21, 22), 3, 0.0, 0.0)
    g1, g2 = gpu(x1, x2)
    for metric in METRICS:
        srt_h, cost, count = ops.sim3_hypotheses(g1, g2, None, 1, THR[metric], metric, 0)
        assert srt_h.shape == (3, 1, 13) and (count == 3).all() and torch.isfinite(cost).all()
        s, r, t, inlier, best_h, cnt, rmse, ok = ops.sim3_ransac(g1, g2, None, 1, THR[metric], metric, 3, 0)
        assert ok.all() and inlier.all() and cnt.tolist() == [3, 3, 3] and best_h.tolist() == [0, 0, 0]
        for b in range(3):                                                     # the oracle's solve of the same three rows
            rot, ds, dt = model_error(float(s[b]), r[b].cpu().numpy(), t[b].cpu().numpy(), SO.solve_minimal(x1[b], x2[b]))
            assert rot <= SOLVE_ROT_DEG and ds <= SOLVE_S_REL and dt <= SOLVE_T
            assert float(rmse[b]) <= SOLVE_RMSE[metric]                       # the float32 residual of an exact fit
    x1, x2, _, _, _, _ = maps((23, 24, 25), 4, 0.0, 0.0)
    valid = np.ones((3, 4), bool)
    valid[1, 2:] = False
    valid[2] = False
    g1, g2, vv = gpu(x1, x2, valid)
    eye = torch.eye(3, device=DEV)
    for metric in METRICS:
        srt_h, cost, count = ops.sim3_hypotheses(g1, g2, vv, 64, THR[metric], metric, 3)
        assert torch.isinf(cost[1:]).all() and (cost[1:] > 0).all() and not count[1:].any() and not srt_h[1:].any()
        s, r, t, inlier, best_h, cnt, rmse, ok = ops.sim3_ransac(g1, g2, vv, 64, THR[metric], metric, 3, 3)
        assert ok.tolist() == [True, False, False] and int(cnt[0]) == 4
        assert torch.equal(r[1:], eye.expand(2, 3, 3)) and not t[1:].any() and not inlier[1:].any() and (s[1:] == 1).all()
        assert cnt[1:].tolist() == [0, 0] and best_h[1:].tolist() == [0, 0] and not rmse[1:].any()
    s2, r2, t2, ok2 = ops.sim3_refit(g1, g2, vv)
    assert ok2.tolist() == [True, False, False] and torch.equal(r2[1:], eye.expand(2, 3, 3)) and not t2[1:].any() and (s2[1:] == 1).all()
    # all-collinear points: every sample is degenerate.  A scale of 2.5e-4 or 2.5e4: every sample is refused by the range.
    line = torch.from_numpy((np.outer(np.arange(16.0), [0.1, 0.2, 0.05]) + [0.3, -0.2, 4.0]).astype(np.float32)).to(DEV)[None]
    x1, x2, _, _, _, _ = maps((26,), 16, 0.0, 0.0)
    g1, g2 = gpu(x1, x2)
    for a, b in ((line, SCALE * line + 0.1), (g1, g2 * 1e-4), (g1 * 1e-4, g2)):
        for metric in METRICS:
            srt_h, cost, count = ops.sim3_hypotheses(a, b, None, 64, THR[metric], metric, 1)
            assert torch.isinf(cost).all() and not count.any() and not srt_h.any()
            s, r, t, inlier, _, cnt, rmse, ok = ops.sim3_ransac(a, b, None, 64, THR[metric], metric, 3, 1)
            assert not bool(ok[0]) and torch.equal(r[0], eye) and not t.any() and not inlier.any() and int(cnt[0]) == 0 and float(s[0]) == 1.0
        assert not bool(ops.sim3_refit(a, b, torch.ones(1, 16, dtype=torch.bool, device=DEV))[3][0])


# ---- the contract ----------------------------------------------------------------------------------------------------------------

def _raw_sim3(x1, x2, v, H, metric, rounds, seed, fill):
    """sim3_hypotheses, sim3_ransac, sim3_refit and sim3_apply through the C ABI into outputs and a workspace that were filled
    with `fill` bytes first"""
    b, n = x1.shape[:2]
    thr = THR[metric]

    def dirty(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(fill)
        return t
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    srt_h, cost, count = dirty((b, H, 13), f32), dirty((b, H), f32), dirty((b, H), i32)
    N.call("mi_sim3_hypotheses", x1.data_ptr(), x2.data_ptr(), v.data_ptr(), b, n, H, thr, metric, seed, srt_h.data_ptr(), cost.data_ptr(),
           count.data_ptr(), N.stream_ptr())
    wbytes = int(N.load_sim3().mi_sim3_ransac_workspace_bytes(b, n, H))
    ws = dirty((wbytes,), u8)
    s, r, t, inl = dirty((b,), f32), dirty((b, 3, 3), f32), dirty((b, 3), f32), dirty((b, n), u8)
    bh, cnt, rmse, ok = dirty((b,), i32), dirty((b,), i32), dirty((b,), f32), dirty((b,), u8)
    N.call("mi_sim3_ransac", x1.data_ptr(), x2.data_ptr(), v.data_ptr(), b, n, H, thr, metric, rounds, seed, s.data_ptr(), r.data_ptr(),
           t.data_ptr(), inl.data_ptr(), bh.data_ptr(), cnt.data_ptr(), rmse.data_ptr(), ok.data_ptr(), ws.data_ptr(), wbytes, N.stream_ptr())
    s2, r2, t2, ok2 = dirty((b,), f32), dirty((b, 3, 3), f32), dirty((b, 3), f32), dirty((b,), u8)
    N.call("mi_sim3_refit", x1.data_ptr(), x2.data_ptr(), inl.data_ptr(), b, n, s2.data_ptr(), r2.data_ptr(), t2.data_ptr(), ok2.data_ptr(),
           N.stream_ptr())
    ro, to, xo = dirty((b, 1, 3, 3), f32), dirty((b, 1, 3), f32), dirty((b, n, 3), f32)
    xin = torch.where(v.bool()[..., None], x1, torch.zeros_like(x1))         # invalid rows may hold anything: not moved here
    N.call("mi_sim3_apply", s.data_ptr(), r.data_ptr(), t.data_ptr(), b, 1, n, r2.data_ptr(), t2.data_ptr(), xin.data_ptr(), ro.data_ptr(),
           to.data_ptr(), xo.data_ptr(), N.stream_ptr())
    return [srt_h, cost, count, s, r, t, inl, bh, cnt, rmse, ok, s2, r2, t2, ok2, ro, to, xo]


@pytest.mark.parametrize("metric", METRICS)
def test_outputs_are_fully_written_reproducible_and_blind_to_invalid_rows(metric):
    n, H = 97, 200
    x1, x2, _, _, _, _ = maps((100, 101, 102, 103, 104), n, 0.25, 0.003)
    valid = np.ones((5, n), np.uint8)
    valid[0, 5::9] = 0
    valid[1, :7] = 0
    valid[4, 2:] = 0                                                          # two rows: ok = 0
    g1, g2, v = gpu(x1, x2, valid)

    def run(a1, a2, fill):
        return tuple(o.cpu().numpy() for o in _raw_sim3(a1, a2, v, H, metric, 3, 21, fill))
    a = twice("sim3 entries", lambda: run(g1, g2, 0xFF))                     # 0xFF bytes: NaN floats, -1 integers
    b = run(g1, g2, 0x00)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))      # every output byte written
    assert not any(np.isnan(a[i]).any() for i in (0, 3, 4, 5, 9, 11, 12, 13, 15, 16, 17))
    assert set(np.unique(a[6]).tolist()) <= {0, 1} and not (a[6].astype(bool) & ~valid.astype(bool)).any()
    assert a[10].tolist() == [1, 1, 1, 1, 0] and a[14].tolist() == [1, 1, 1, 1, 0]
    assert a[3][4] == 1 and np.array_equal(a[4][4], np.eye(3)) and not a[5][4].any() and not a[6][4].any() and a[8][4] == 0 and a[9][4] == 0
    assert np.isinf(a[1][4]).all() and not a[0][4].any() and not a[2][4].any()
    # invalid rows may hold anything: NaN and 1e30 in the points
    y1, y2 = g1.clone(), g2.clone()
    y1[~v.bool()] = float("nan")
    y2[~v.bool()] = 1e30
    c = run(y1, y2, 0xFF)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, c))
    # the entries without a sampler do not depend on the batch position; the sampled ones give a pair alone what they give it
    # as item 0 of a batch
    perm = [2, 0, 1, 4, 3]
    inl = torch.from_numpy(a[6])[perm].contiguous().to(DEV)
    s_p, r_p, t_p, ok_p = ops.sim3_refit(g1[perm].contiguous(), g2[perm].contiguous(), inl)
    assert np.array_equal(bits(s_p.cpu().numpy()), bits(a[11][perm])) and np.array_equal(bits(r_p.cpu().numpy()), bits(a[12][perm]))
    assert np.array_equal(bits(t_p.cpu().numpy()), bits(a[13][perm])) and np.array_equal(ok_p.cpu().numpy(), a[14][perm].astype(bool))
    alone = _raw_sim3(g1[:1].contiguous(), g2[:1].contiguous(), v[:1].contiguous(), H, metric, 3, 21, 0xFF)
    assert all(np.array_equal(bits(x.cpu().numpy()), bits(y[:1])) for x, y in zip(alone, a))


def test_the_module_replays_from_one_graph():
    n, H = 64, 64
    sets = [[gpu(x) for x in maps(s, n, 0.25, 0.003)[:2]] for s in ((100, 101, 102), (103, 104, 105), (106, 107, 108))]
    m = SimilarityEstimator("reprojection", 2.0, focal=500.0, num_hypotheses=H, seed=4).to(DEV)
    mp = SimilarityEstimator("point", 0.1, num_hypotheses=H, seed=4).to(DEV)

    def run(x1, x2):
        a, p = m(x1, x2), mp(x1, x2)
        return tuple(a) + tuple(p) + tuple(m.apply(a[0], a[1], a[2], a[1][:, None].contiguous(), a[2][:, None].contiguous(), x1)) + \
            tuple(mp.align_trajectory(x1, x2, p[3]))
    eager = [[x.clone() for x in run(*s)] for s in sets]
    static = [x.clone() for x in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(*static)
    for i in (1, 2, 0):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[i]), i
