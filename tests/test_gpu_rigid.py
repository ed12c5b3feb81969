"""K17 metric RGB-D pose on the GPU against tests/rigid_oracle.py (the fp64 numpy restatement of include/mi355x_match.h).

The lift is compared bit for bit with a numpy restatement of the header's float32 arithmetic.  Everything after it is
fp32 kernels against an fp64 oracle, which cannot agree bit for bit, so every tolerance below is the deviation of the SAME
oracle run in float32 from its float64 run (measured on the CPU on the very scenes these tests use, lifted by the header's
float32 arithmetic), times the margin K15 uses for a different operation order (4 for values, 2 for angles):
  - per-hypothesis parity (0.5 px, depth noise 0.001 z^2, (n, H) = (64, 200), (97, 200), (65, 65), 9 pairs): the float32
    oracle had the float64 oracle's inlier count to within 1 on 100 % of the hypotheses (cap to hold here: >= 90 %); on
    hypotheses of equal count its MSAC cost deviated by at most 9.72e-6 relative -> COST_RTOL = 3.9e-5 (the kernels'
    arithmetic run on the CPU: 2.75e-5);
  - refit on the planted inliers (n = 64 / 97, with and without noise, 12 pairs): rotation 7.99e-6 deg, translation
    2.35e-6 m -> REFIT_ROT_DEG = 1.6e-5, REFIT_T_M = 9.4e-6 (the kernels' arithmetic on the CPU: 1.01e-5 deg, 2.33e-6 m);
  - ground truth (noise-free, 25 % / 40 % outliers, n = 33 / 64 / 96, H = 64, 18 scenes): the float64 oracle is within
    2.85e-6 deg and 2.19e-7 m of the truth (float32 pixels and depths), the float32 oracle within 7.39e-5 deg and 5.43e-6 m
    of the float64 oracle; both marked every planted inlier and no other row -> GT_ROT_DEG = 2.85e-6 + 2 * 7.39e-5 =
    1.5e-4, GT_T_M = 2.19e-7 + 4 * 5.43e-6 = 2.2e-5.
  - refined output (test_selection_is_exact's scenes, 3 rounds, the oracle with the header's float64 step cost): the
    float32 run is within 8.78e-6 deg and 1.23e-6 m of the float64 run, with equal inlier masks -> REFINED_ROT_DEG =
    1.8e-5, REFINED_T_M = 4.9e-6;
  - a minimal solve (n = 3, H = 1): the bounds of tests/test_rigid_host.py, 6.2e-4 deg and 1.6e-4 m (192 minimal samples).
Every seed of the ground-truth cases has an all-inlier sample under the sampler (9 to 33 of 64; the test re-checks it): 0
seeds dropped."""
import functools

import numpy as np
import pytest
import torch

import pose_oracle as PO
import rigid_oracle as RO
from gpu_common import DEV, GPU, bits, k_inv, same_bits
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import RelativePoseEstimator, RgbdPoseEstimator
from onnx_image_processing_amd.synth import rgbd_camera

pytestmark = GPU
K = rgbd_camera()
THR = RO.THR
COST_RTOL, REFIT_ROT_DEG, REFIT_T_M, GT_ROT_DEG, GT_T_M = 3.9e-5, 1.6e-5, 9.4e-6, 1.5e-4, 2.2e-5
REFINED_ROT_DEG, REFINED_T_M, SOLVE_ROT_DEG, SOLVE_T_M = 1.8e-5, 4.9e-6, 6.2e-4, 1.6e-4
GT_SEED = 11
GT_SCENES = (200, 201, 202)


@functools.lru_cache(maxsize=None)
def scenes(seeds, n, outliers, noise_px, depth_noise):
    return RO.scenes(seeds, n, outliers, noise_px, depth_noise)


def lifted(k1, k2, d1, d2):
    """the kernels' own lifted points and joint validity, on the GPU and as numpy arrays"""
    x1, v1 = ops.lift_keypoints(torch.from_numpy(k1).to(DEV), torch.from_numpy(d1).to(DEV), k_inv(K), 1.0, RO.MIN_DEPTH, RO.MAX_DEPTH)
    x2, v2 = ops.lift_keypoints(torch.from_numpy(k2).to(DEV), torch.from_numpy(d2).to(DEV), k_inv(K), 1.0, RO.MIN_DEPTH, RO.MAX_DEPTH, v1)
    return x1, x2, v2, x1.cpu().numpy(), x2.cpu().numpy(), v2.cpu().numpy()


# ---- lift ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(37, 53), (480, 640)])
@pytest.mark.parametrize("u16", [False, True])
def test_lift_is_the_headers_arithmetic_bit_for_bit(h, w, u16):
    rng = np.random.default_rng(h + u16)
    B, n = 2, 70
    kcam = np.array([[0.8 * w, 0.0, w / 2.0 - 0.3], [0.0, 0.9 * w, h / 2.0 + 0.2], [0.0, 0.0, 1.0]])
    ki = np.linalg.inv(kcam).astype(np.float32)
    kp = np.stack([rng.uniform(-2, h + 2, (B, n)), rng.uniform(-2, w + 2, (B, n))], axis=-1).astype(np.float32)
    kp[:, :12, 0] = h / 2.0                                                 # the edge cases sit on a row inside the frame
    kp[0, :4, 1] = [-0.5, -0.6, w - 0.5, w - 0.51]                          # -> px = 0, -1 (out), w (out), w - 1
    kp[1, :4, 0] = [-0.5, -0.6, h - 0.5, h - 0.51]
    kp[1, :4, 1] = w / 2.0
    kp[0, 4] = [np.nan, 3.0]
    kp[0, 5] = [3.0, np.inf]
    kp[0, 6] = [-np.inf, 3.0]
    kp[0, 7:12, 1] = np.arange(7, 12)                                       # pixels (h / 2, 7 .. 11): special depths
    scale = 0.001 if u16 else 1.0
    row = int(np.floor(h / 2.0 + 0.5))                                      # py of the keypoints at y = h / 2
    if u16:
        depth = rng.integers(50, 12000, (B, h, w)).astype(np.uint16)        # 0.05 m .. 12 m: below min, above max
        depth[0, row, 7:11] = [0, 99, 100, 10001]
    else:
        depth = rng.uniform(0.05, 12.0, (B, h, w)).astype(np.float32)
        depth[0, row, 7:12] = [0.0, np.nan, np.inf, 0.0999, 10.001]
    vin = np.ones((B, n), bool)
    vin[:, 20:24] = False                                                   # valid_in cleared
    for use_vin in (False, True):
        pts, ok = ops.lift_keypoints(torch.from_numpy(kp).to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(ki).to(DEV),
                                     scale, 0.1, 10.0, torch.from_numpy(vin).to(DEV) if use_vin else None)
        for b in range(B):
            ref, rok = RO.lift_f32(kp[b], depth[b], ki, scale, 0.1, 10.0, vin[b] if use_vin else None)
            assert np.array_equal(ok[b].cpu().numpy(), rok)
            assert np.array_equal(bits(pts[b].cpu().numpy()), bits(ref))
            assert not pts[b].cpu().numpy()[~rok].any()
        okn = ok.cpu().numpy()
        assert okn.any() and (~okn).any()
        assert not okn[0, 1] and not okn[0, 2] and not okn[0, 4:7].any() and not okn[1, 1] and not okn[1, 2]
        if use_vin:
            assert not okn[:, 20:24].any()
    # the ray's bits are mi_normalise_keypoints': with depth 1 and z_scale 1 the point is (xn * 1, yn * 1, 1)
    ones = torch.ones((B, h, w), device=DEV)
    inside = np.stack([rng.uniform(0, h - 1, (B, n)), rng.uniform(0, w - 1, (B, n))], axis=-1).astype(np.float32)
    pts, ok = ops.lift_keypoints(torch.from_numpy(inside).to(DEV), ones, torch.from_numpy(ki).to(DEV), 1.0, 0.1, 10.0)
    rays = ops.normalise_keypoints(torch.from_numpy(inside).to(DEV), torch.from_numpy(ki).to(DEV))
    assert ok.all() and torch.equal(bits(pts[..., :2]), bits(rays)) and (pts[..., 2] == 1).all()


# ---- hypotheses ----------------------------------------------------------------------------------------------------------------

def test_sampler_all_inlier_hypotheses_explain_every_planted_inlier():
    """noise-free scenes: a hypothesis whose 3 sampled ranks (the oracle's restatement of the header's sampler) are all
    planted inliers is the true motion, so its count reaches the number of planted inliers -- which it can only do if the
    kernel drew those very rows.  Pair 1 has invalid rows (ranks are over the VALID rows)."""
    n, H, seed = 64, 200, 5
    k1, k2, d1, d2, _, _, inl = scenes((10, 11, 12), n, 0.25, 0.0, 0.0)
    x1, x2, v, _, _, vn = lifted(k1, k2, d1, d2)
    valid = vn.copy()
    valid[1, ::5] = False
    _, _, count = ops.rigid_hypotheses(x1, x2, torch.from_numpy(valid).to(DEV), H, THR, seed)
    count = count.cpu().numpy()
    checked = 0
    for b in range(3):
        vidx = np.flatnonzero(valid[b])
        planted = int((inl[b] & valid[b]).sum())
        for h in range(H):
            rows = vidx[RO.sample_ranks(seed, b, h, len(vidx))]
            if inl[b][rows].all():
                checked += 1
                assert count[b, h] >= planted, (b, h, count[b, h], planted)
    assert checked >= 20, checked


@pytest.mark.parametrize("n,H", [(64, 200), (97, 200), (65, 65)])
def test_hypotheses_match_the_oracle_per_hypothesis(n, H):
    seed = 7
    k1, k2, d1, d2, _, _, _ = scenes((100, 101, 102), n, 0.25, 0.5, 0.001)
    x1, x2, v, q1, q2, vn = lifted(k1, k2, d1, d2)
    rt_h, cost, count = (x.cpu().numpy() for x in ops.rigid_hypotheses(x1, x2, v, H, THR, seed))
    for b in range(3):
        ort, oc, ok_, _ = RO.hypotheses(q1[b], q2[b], vn[b], H, THR, seed, b)
        assert np.array_equal(np.isinf(cost[b]), np.isinf(oc))
        dk = np.abs(count[b].astype(np.int64) - ok_)
        same = (dk == 0) & np.isfinite(oc) & np.isfinite(cost[b])
        rel = np.abs(cost[b][same].astype(np.float64) - oc[same]) / oc[same]
        print(f"n={n} H={H} pair {b}: equal counts {np.mean(dk == 0):.3f}, |dcount| <= 1 {np.mean(dk <= 1):.3f}; "
              f"cost rel dev on equal counts max {rel.max():.2e} median {np.median(rel):.2e}; inf {np.isinf(cost[b]).sum()}")
        assert np.mean(dk <= 1) >= 0.90
        assert rel.max() <= COST_RTOL


@pytest.mark.parametrize("n,H", [(64, 1), (97, 64), (64, 200)])
def test_selection_is_exact(n, H):
    k1, k2, d1, d2, _, _, _ = scenes((100, 101, 102), n, 0.25, 0.5, 0.001)
    x1, x2, v, q1, q2, vn = lifted(k1, k2, d1, d2)
    valid = vn.copy()
    valid[2, 3::7] = False
    v = torch.from_numpy(valid).to(DEV)
    rt_h, cost, count = ops.rigid_hypotheses(x1, x2, v, H, THR, 9)
    r, t, inlier, best_h, cnt, rmse, ok = ops.rigid_ransac(x1, x2, v, H, THR, 0, 9)
    cost_np = cost.cpu().numpy()
    for b in range(3):
        bh = int(np.argmin(cost_np[b]))                                        # numpy: the first minimum
        assert int(best_h[b]) == bh
        if not bool(ok[b]):                                                    # H = 1: the only sample may explain < 3 rows
            assert int(count[b, bh]) < 3 and int(cnt[b]) == 0 and not inlier[b].any()
            continue
        assert torch.equal(bits(r[b].reshape(9)), bits(rt_h[b, bh, :9])) and torch.equal(bits(t[b]), bits(rt_h[b, bh, 9:]))
        assert int(cnt[b]) == int(count[b, bh]) == int(inlier[b].sum())
        assert not (inlier[b].cpu().numpy() & ~valid[b]).any()
        R64, t64 = r[b].cpu().numpy().astype(np.float64), t[b].cpu().numpy().astype(np.float64)
        d2 = RO.dist2(R64, t64, q1[b].astype(np.float64), q2[b].astype(np.float64))
        clear = np.abs(d2 / THR ** 2 - 1) > 1e-3                               # not within rounding of the threshold
        assert np.array_equal(inlier[b].cpu().numpy()[clear], ((d2 <= THR ** 2) & valid[b])[clear])
        got = inlier[b].cpu().numpy()
        # float32 residuals of points up to 9.5 m from the camera: each component of u is off by at most 4 roundings of
        # 9.5 m (2.3e-6 m), |u| by 4e-6 m; the float32 sum and root add 1e-5 relative (observed on an MI355X on noise-free
        # scenes, where the RMSE is all evaluation error: 4.5e-7 to 1.36e-6 m)
        assert abs(float(rmse[b]) - np.sqrt(d2[got].mean())) <= 4e-6 + 1e-5 * np.sqrt(d2[got].mean())
    # refinement never makes the cost worse
    r3, t3, inl3, bh3, cnt3, rmse3, ok3 = ops.rigid_ransac(x1, x2, v, H, THR, 3, 9)
    assert torch.equal(bh3, best_h)
    for b in range(3):
        if not bool(ok[b]):
            continue
        a, bb = q1[b][valid[b]].astype(np.float64), q2[b][valid[b]].astype(np.float64)
        c0 = RO.score(r[b].cpu().numpy().astype(np.float64), t[b].cpu().numpy().astype(np.float64), a, bb, THR)[0]
        c3 = RO.score(r3[b].cpu().numpy().astype(np.float64), t3[b].cpu().numpy().astype(np.float64), a, bb, THR)[0]
        assert bool(ok3[b]) and c3 <= c0 * (1 + COST_RTOL)
    # the refined motion and mask are the oracle's (float64, the header's step cost)
    for b in range(3):
        Ro, to, mo, bho, cno, rmo, oko = RO.ransac(q1[b], q2[b], valid[b], H, THR, 3, 9, b, cost64=True)
        assert bool(ok3[b]) == oko
        if not oko:
            continue
        rot, dt = PO.rotation_angle_deg(r3[b].cpu().numpy(), Ro), RO.translation_error(t3[b].cpu().numpy(), to)
        print(f"refined n={n} H={H} pair {b}: rotation {rot:.2e} deg, translation {dt:.2e} m against the oracle; count {int(cnt3[b])} / {cno}")
        assert int(bh3[b]) == bho and rot <= REFINED_ROT_DEG and dt <= REFINED_T_M
        d2 = RO.dist2(Ro, to, q1[b].astype(np.float64), q2[b].astype(np.float64))
        clear = np.abs(d2 / THR ** 2 - 1) > 1e-3
        assert np.array_equal(inl3[b].cpu().numpy()[clear], mo[clear])


# ---- refit ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,noise", [(64, (0.0, 0.0)), (64, (0.5, 0.001)), (97, (0.0, 0.0)), (97, (0.5, 0.001))])
def test_refit_matches_the_oracle(n, noise):
    k1, k2, d1, d2, _, _, inl = scenes((100, 101, 102), n, 0.25, *noise)
    inl = inl.copy()
    inl[1, :] &= np.arange(n) % 3 != 0                                         # a middle pair with a different mask
    x1, x2, v, q1, q2, vn = lifted(k1, k2, d1, d2)
    mask = inl & vn
    r, t, ok = ops.rigid_refit(x1, x2, torch.from_numpy(mask).to(DEV))
    assert ok.all()
    for b in range(3):
        Rr, tr, _ = RO.refit(q1[b], q2[b], mask[b])
        rot, dt = PO.rotation_angle_deg(r[b].cpu().numpy(), Rr), RO.translation_error(t[b].cpu().numpy(), tr)
        print(f"refit n={n} noise={noise} pair {b}: rotation {rot:.2e} deg, translation {dt:.2e} m")
        assert rot <= REFIT_ROT_DEG and dt <= REFIT_T_M
    # 2 rows; collinear rows (in frame 1 only: pair 1; in both: pair 2)
    few = np.zeros((3, n), bool)
    few[0, [int(np.flatnonzero(mask[0])[0]), int(np.flatnonzero(mask[0])[1])]] = True
    few[1:, :8] = True
    line = torch.from_numpy((np.outer(np.arange(8.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]).astype(np.float32)).to(DEV)
    y1, y2 = x1.clone(), x2.clone()
    y1[1, :8] = line
    y1[2, :8] = line
    y2[2, :8] = line + 0.25
    r, t, ok = ops.rigid_refit(y1, y2, torch.from_numpy(few).to(DEV))
    assert not ok.any() and torch.equal(r, torch.eye(3, device=DEV).expand(3, 3, 3)) and not t.any()


# ---- the whole path --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 64, 96])
@pytest.mark.parametrize("outliers", [0.25, 0.40])
def test_ground_truth_pose_from_depth_frames(n, outliers):
    H = 64
    k1, k2, d1, d2, R, t, inl = scenes(GT_SCENES, n, outliers, 0.0, 0.0)
    for b in range(3):                                                         # every seed has an all-inlier sample
        assert any(inl[b][RO.sample_ranks(GT_SEED, b, h, n)].all() for h in range(H)), GT_SCENES[b]
    m = RgbdPoseEstimator(torch.from_numpy(K), num_hypotheses=H, distance_threshold=THR, refine_rounds=3, seed=GT_SEED).to(DEV)
    tk1, tk2 = torch.from_numpy(k1).to(DEV), torch.from_numpy(k2).to(DEV)
    Rg, tg, mask, rmse, ok = m(tk1, tk2, torch.from_numpy(d1).to(DEV), torch.from_numpy(d2).to(DEV).unsqueeze(1))
    rel = RelativePoseEstimator(torch.from_numpy(K), num_hypotheses=1024, seed=GT_SEED).to(DEV)
    _, t_unit, _, _, ok_rel = rel(tk1, tk2)
    for b in range(3):
        got = mask[b].cpu().numpy()
        rot, dt = PO.rotation_angle_deg(Rg[b].cpu().numpy(), R[b]), RO.translation_error(tg[b].cpu().numpy(), t[b])
        print(f"n={n} outliers={outliers} seed {GT_SCENES[b]}: recall {(got & inl[b]).sum()}/{inl[b].sum()}, false {(got & ~inl[b]).sum()}, "
              f"rotation {rot:.2e} deg, |t - t_true| {dt:.2e} m, rmse {float(rmse[b]):.2e} m")
        assert bool(ok[b]) and (got & inl[b]).sum() == inl[b].sum()
        assert rot <= GT_ROT_DEG and dt <= GT_T_M
        assert abs(float(torch.linalg.det(Rg[b].double().cpu())) - 1) < 1e-5
        # the convention of RelativePoseEstimator: the same direction of motion (the inverse motion would be near 180 deg)
        assert bool(ok_rel[b]) and PO.direction_angle_deg(tg[b].cpu().numpy(), t_unit[b].cpu().numpy()) < 90.0
    # unbatched input gives unbatched output with the same bits for pair 0
    single = m(tk1[0], tk2[0], torch.from_numpy(d1[0]).to(DEV), torch.from_numpy(d2[0]).to(DEV))
    assert single[0].shape == (3, 3) and single[2].shape == (n,) and single[4].dim() == 0
    assert all(torch.equal(x, y[0]) for x, y in zip(single, (Rg, tg, mask, rmse, ok)))
    # uint16 millimetres: the same scene through depth_scale = 0.001.  Rounding to 1 mm moves a point by at most 0.5 mm
    # along its ray; over points spread by more than 1 m that is at most 5e-4 rad = 0.03 deg of rotation, and 0.5 mm plus that
    # rotation at the centroid's 6 m = 3.5 mm of translation (worst case; a least-squares fit over >= 20 points is far inside)
    m16 = RgbdPoseEstimator(torch.from_numpy(K), depth_scale=0.001, num_hypotheses=H, distance_threshold=THR, seed=GT_SEED).to(DEV)
    mm1, mm2 = (torch.from_numpy(np.round(d * 1000.0).astype(np.uint16)).to(DEV) for d in (d1, d2))
    R16, t16, mask16, _, ok16 = m16(tk1, tk2, mm1, mm2)
    for b in range(3):
        print(f"    millimetre depth, seed {GT_SCENES[b]}: rotation {PO.rotation_angle_deg(R16[b].cpu().numpy(), R[b]):.2e} deg, "
              f"|t - t_true| {RO.translation_error(t16[b].cpu().numpy(), t[b]):.2e} m")
        assert bool(ok16[b]) and (mask16[b].cpu().numpy() & inl[b]).sum() == inl[b].sum()
        assert PO.rotation_angle_deg(R16[b].cpu().numpy(), R[b]) < 0.03 and RO.translation_error(t16[b].cpu().numpy(), t[b]) < 3.5e-3


def test_degenerate_pairs_and_small_shapes():
    """n = 3 with H = 1: the only sample; n = 4 with 2 valid rows and with none; all-collinear points"""
    k1, k2, d1, d2, R, t, _ = scenes((20, 21, 22), 3, 0.0, 0.0, 0.0)
    x1, x2, v, q1, q2, vn = lifted(k1, k2, d1, d2)
    assert vn.all()
    rt_h, cost, count = ops.rigid_hypotheses(x1, x2, None, 1, THR, 0)
    assert rt_h.shape == (3, 1, 12) and (count == 3).all() and torch.isfinite(cost).all()
    r, tt, inlier, best_h, cnt, rmse, ok = ops.rigid_ransac(x1, x2, None, 1, THR, 3, 0)
    assert ok.all() and inlier.all() and cnt.tolist() == [3, 3, 3] and best_h.tolist() == [0, 0, 0]
    for b in range(3):                                                         # the oracle's solve of the same three rows
        Ro, to = RO.solve_minimal(q1[b], q2[b])
        assert PO.rotation_angle_deg(r[b].cpu().numpy(), Ro) <= SOLVE_ROT_DEG and RO.translation_error(tt[b].cpu().numpy(), to) <= SOLVE_T_M
        assert float(rmse[b]) <= 4e-6                                          # the float32 evaluation floor (test_selection_is_exact)
    k1, k2, d1, d2, _, _, _ = scenes((23, 24, 25), 4, 0.0, 0.0, 0.0)
    x1, x2, v, _, _, vn = lifted(k1, k2, d1, d2)
    valid = vn.copy()
    valid[1, 2:] = False
    valid[2] = False
    vv = torch.from_numpy(valid).to(DEV)
    rt_h, cost, count = ops.rigid_hypotheses(x1, x2, vv, 64, THR, 3)
    assert torch.isinf(cost[1:]).all() and (cost[1:] > 0).all() and not count[1:].any() and not rt_h[1:].any()
    r, tt, inlier, best_h, cnt, rmse, ok = ops.rigid_ransac(x1, x2, vv, 64, THR, 3, 3)
    assert ok.tolist() == [True, False, False] and int(cnt[0]) == 4
    assert torch.equal(r[1:], torch.eye(3, device=DEV).expand(2, 3, 3)) and not tt[1:].any() and not inlier[1:].any()
    assert cnt[1:].tolist() == [0, 0] and best_h[1:].tolist() == [0, 0] and not rmse[1:].any()
    r2, t2, ok2 = ops.rigid_refit(x1, x2, vv)
    assert ok2.tolist() == [True, False, False] and torch.equal(r2[1:], torch.eye(3, device=DEV).expand(2, 3, 3)) and not t2[1:].any()
    # all-collinear points: every sample is degenerate
    line = torch.from_numpy((np.outer(np.arange(16.0), [0.1, 0.2, 0.05]) + [0.3, -0.2, 4.0]).astype(np.float32)).to(DEV)[None]
    rt_h, cost, count = ops.rigid_hypotheses(line, line + 0.1, None, 64, THR, 1)
    assert torch.isinf(cost).all() and not count.any() and not rt_h.any()
    r, tt, inlier, _, cnt, rmse, ok = ops.rigid_ransac(line, line + 0.1, None, 64, THR, 3, 1)
    assert not bool(ok[0]) and torch.equal(r[0], torch.eye(3, device=DEV)) and not tt.any() and not inlier.any() and int(cnt[0]) == 0


# ---- the contract ----------------------------------------------------------------------------------------------------------------

def _raw_calls(kp1, kp2, dep1, dep2, vin, H, rounds, seed, fill):
    """both lifts, rigid_hypotheses, rigid_ransac and rigid_refit through the C ABI into outputs and a workspace that were
    filled with `fill` bytes first"""
    b, n = kp1.shape[:2]
    h, w = dep1.shape[1:]

    def dirty(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(fill)
        return t
    ki = k_inv(K)
    x1, v1, x2, v2 = dirty((b, n, 3), torch.float32), dirty((b, n), torch.uint8), dirty((b, n, 3), torch.float32), dirty((b, n), torch.uint8)
    N.call("mi_lift_keypoints", kp1.data_ptr(), dep1.data_ptr(), 0, b, n, h, w, ki.data_ptr(), 1.0, 0.1, 10.0, vin.data_ptr(),
           x1.data_ptr(), v1.data_ptr(), N.stream_ptr())
    N.call("mi_lift_keypoints", kp2.data_ptr(), dep2.data_ptr(), 0, b, n, h, w, ki.data_ptr(), 1.0, 0.1, 10.0, v1.data_ptr(),
           x2.data_ptr(), v2.data_ptr(), N.stream_ptr())
    return [x1, v1, x2, v2] + _raw_rigid(x1, x2, v2, H, rounds, seed, fill)


def _raw_rigid(x1, x2, v, H, rounds, seed, fill):
    b, n = x1.shape[:2]

    def dirty(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(fill)
        return t
    rt_h, cost, count = dirty((b, H, 12), torch.float32), dirty((b, H), torch.float32), dirty((b, H), torch.int32)
    N.call("mi_rigid_hypotheses", x1.data_ptr(), x2.data_ptr(), v.data_ptr(), b, n, H, THR, seed, rt_h.data_ptr(), cost.data_ptr(),
           count.data_ptr(), N.stream_ptr())
    wbytes = int(N.load().mi_rigid_ransac_workspace_bytes(b, n, H))
    ws = dirty((wbytes,), torch.uint8)
    r, t, inl = dirty((b, 3, 3), torch.float32), dirty((b, 3), torch.float32), dirty((b, n), torch.uint8)
    bh, cnt, rmse, ok = dirty((b,), torch.int32), dirty((b,), torch.int32), dirty((b,), torch.float32), dirty((b,), torch.uint8)
    N.call("mi_rigid_ransac", x1.data_ptr(), x2.data_ptr(), v.data_ptr(), b, n, H, THR, rounds, seed, r.data_ptr(), t.data_ptr(),
           inl.data_ptr(), bh.data_ptr(), cnt.data_ptr(), rmse.data_ptr(), ok.data_ptr(), ws.data_ptr(), wbytes, N.stream_ptr())
    r2, t2, ok2 = dirty((b, 3, 3), torch.float32), dirty((b, 3), torch.float32), dirty((b,), torch.uint8)
    N.call("mi_rigid_refit", x1.data_ptr(), x2.data_ptr(), inl.data_ptr(), b, n, r2.data_ptr(), t2.data_ptr(), ok2.data_ptr(),
           N.stream_ptr())
    return [rt_h, cost, count, r, t, inl, bh, cnt, rmse, ok, r2, t2, ok2]


def test_outputs_are_fully_written_reproducible_and_blind_to_invalid_rows():
    n, H = 97, 200
    k1, k2, d1, d2, _, _, _ = scenes((100, 101, 102), n, 0.25, 0.5, 0.001)
    vin = np.ones((3, n), np.uint8)
    vin[0, 5::9] = 0
    vin[1, :7] = 0
    args = [torch.from_numpy(x).to(DEV) for x in (k1, k2, d1, d2, vin)]
    a = _raw_calls(*args, H, 3, 21, 0xFF)                                       # 0xFF bytes: NaN floats, -1 integers
    b = _raw_calls(*args, H, 3, 21, 0x00)
    assert same_bits(a, b)                                                    # every output byte written; two runs agree
    assert not any(torch.isnan(x).any() for x in (a[0], a[2], a[4], a[5], a[7], a[8], a[12], a[14], a[15]))
    v = a[3]
    assert set(torch.unique(v).tolist()) <= {0, 1} and set(torch.unique(a[9]).tolist()) <= {0, 1}
    assert not (v.bool() & ~args[4].bool()).any() and not (a[9].bool() & ~v.bool()).any()      # inlier <= valid <= valid_in
    assert a[13].bool().all() and a[16].bool().all()
    # invalid rows may hold anything: NaN and 1e30 in the points, NaN in the keypoints
    x1, x2 = a[0].clone(), a[2].clone()
    x1[~v.bool()] = float("nan")
    x2[~v.bool()] = 1e30
    assert same_bits(a[4:], _raw_rigid(x1, x2, v, H, 3, 21, 0xFF))
    kk1 = args[0].clone()
    kk1[~args[4].bool()] = float("nan")
    assert same_bits(a, _raw_calls(kk1, *args[1:], H, 3, 21, 0xFF))
    # the entries without a sampler do not depend on the batch position
    perm = [2, 0, 1]
    r_p, t_p, ok_p = ops.rigid_refit(a[0][perm].contiguous(), a[2][perm].contiguous(), a[9][perm].contiguous())
    assert torch.equal(bits(r_p), bits(a[14][perm])) and torch.equal(bits(t_p), bits(a[15][perm])) and torch.equal(ok_p, a[16][perm].bool())
    p_p, v_p = ops.lift_keypoints(args[0][perm].contiguous(), args[2][perm].contiguous(), k_inv(K), 1.0, 0.1, 10.0, args[4][perm].contiguous())
    assert torch.equal(bits(p_p), bits(a[0][perm])) and torch.equal(v_p, a[1][perm].bool())


def test_lift_ransac_and_the_module_replay_from_one_graph():
    n, H = 64, 64
    sets = [scenes(s, n, 0.25, 0.5, 0.001)[:4] for s in ((100, 101, 102), (103, 104, 105), (106, 107, 108))]
    sets = [[torch.from_numpy(x).to(DEV) for x in s] for s in sets]
    m = RgbdPoseEstimator(torch.from_numpy(K), num_hypotheses=H, seed=4).to(DEV)
    ki = k_inv(K)

    def run(k1, k2, d1, d2):
        x1, v1 = ops.lift_keypoints(k1, d1, ki, 1.0, 0.1, 10.0)
        x2, v2 = ops.lift_keypoints(k2, d2, ki, 1.0, 0.1, 10.0, v1)
        return (x1, x2, v2) + tuple(ops.rigid_ransac(x1, x2, v2, H, THR, 3, 4)) + tuple(m(k1, k2, d1, d2))
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
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, eager[i])), i
