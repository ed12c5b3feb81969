"""K23 absolute pose on the GPU against tests/pnp_oracle.py (the float64 numpy oracle of include/mi355x_match.h, whose P3P
solver is Grunert's quartic through numpy.roots, not the header's).

float32 kernels against a float64 oracle cannot agree bit for bit, and a P3P solve is ill-conditioned on a small share of
samples, so every tolerance below is the deviation of pnp_oracle's FLOAT32 RESTATEMENT of the kernels' arithmetic (whose
bits the host build of csrc/pnp_math.h returns, tests/test_pnp_host.py) from the float64 oracle, measured on the CPU on the
very scenes these tests use, times the project's margins (4 for values, 2 for angles):
  - per-hypothesis parity (0.5 px, 25 % outliers, 9 pairs each): the restatement had the oracle's inlier count to within 1
    on 99.78 % / 99.94 % / 100 % / 100 % of the hypotheses at (n, H) = (64, 200) / (97, 200) / (65, 65) / (4, 1) (to hold
    here: >= 90 %; one hypothesis of 4194 was refused by one side only); on those its MSAC cost deviated by at most
    1.08e-3 / 2.43e-3 / 3.06e-3 / 7.28e-3 relative (medians 2.2e-7 to 1.8e-5: the maxima are ill-conditioned samples)
    -> COST_RTOL = 4.3e-3 / 9.7e-3 / 1.2e-2 / 2.9e-2;
  - refit on the planted inliers from a start 2 deg and 6 cm off (n = 64 / 97 with and without 0.5 px, n = 4; 15 pairs):
    rotation 1.88e-5 deg, translation 2.03e-6 m, info 2.85e-7 of its largest element -> REFIT_ROT_DEG = 3.8e-5,
    REFIT_T_M = 8.1e-6, INFO_RTOL = 1.2e-6;
  - ground truth (noise-free, 25 % / 40 % outliers, n = 33 / 64 / 96 / 2048, H = 64, 24 scenes): the float64 oracle is
    within 3.29e-6 deg and 4.42e-7 m of the truth (float32 pixels and points), the restatement within 8.10e-6 deg and
    3.87e-7 m of the oracle; both marked every planted inlier and no other row -> GT_ROT_DEG = 3.29e-6 + 2 * 8.10e-6 =
    2.0e-5, GT_T_M = 4.42e-7 + 4 * 3.87e-7 = 2.0e-6;
  - a minimal solve (n = 4): the bounds of tests/test_pnp_host.py, 5.2e-2 deg and 1.7e-2 m (192 minimal samples).
Every seed of the ground-truth cases has an all-inlier sample under the sampler (4 to 24 of 64; the test re-checks it): 0
seeds dropped."""
import functools

import numpy as np
import pytest
import torch

import pnp_oracle as QO
import pose_oracle as PO
import rigid_oracle as RO
from gpu_common import DEV, GPU, bits, gpu, k_inv, same_bits
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import AbsolutePoseEstimator, RgbdPoseEstimator
from onnx_image_processing_amd.synth import rgbd_camera, synth_rgbd_pair

pytestmark = GPU
K = rgbd_camera()
FOCAL = 500.0
THR = QO.THR_PX / FOCAL
COST_RTOL = {(64, 200): 4.3e-3, (97, 200): 9.7e-3, (65, 65): 1.2e-2, (4, 1): 2.9e-2}
REFIT_ROT_DEG, REFIT_T_M, INFO_RTOL, GT_ROT_DEG, GT_T_M = 3.8e-5, 8.1e-6, 1.2e-6, 2.0e-5, 2.0e-6
SOLVE_ROT_DEG, SOLVE_T_M = 5.2e-2, 1.7e-2
GT_SEED = 11
GT_SCENES = (200, 201, 202)
D = np.float64


@functools.lru_cache(maxsize=None)
def scenes(seeds, n, outliers, noise_px):
    return QO.scenes(seeds, n, outliers, noise_px)


@functools.lru_cache(maxsize=None)
def raw_scenes(seeds, n, outliers, noise_px):
    """the same scenes as keypoints and depth frames: k1, k2 (B, n, 2), d1, d2 (B, 480, 640), lists of R and t, inlier masks"""
    s = [synth_rgbd_pair(seed, n, outliers, noise_px, 0.0) for seed in seeds]
    return tuple(np.stack([x[j] for x in s]) for j in range(4)) + ([x[4] for x in s], [x[5] for x in s], np.stack([x[6] for x in s]))


def perturbed(R, t):
    w = np.deg2rad(2.0) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    return (QO._exp(w) @ R).astype(np.float32), (t + [0.03, -0.02, 0.05]).astype(np.float32)


# ---- hypotheses -----------------------------------------------------------------------------------------------------------------

def test_normalised_points_are_the_oracles_bits():
    """what the tests feed the oracle is what mi_normalise_keypoints gives the kernels"""
    k1, k2, d1, d2, _, _, _ = raw_scenes((100, 101, 102), 97, 0.25, 0.5)
    got = ops.normalise_keypoints(gpu(k2), k_inv(K)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), QO.normalise_f32(k2, np.linalg.inv(K).astype(np.float32)).view(np.uint32))


def test_sampler_all_inlier_hypotheses_explain_every_planted_inlier():
    """noise-free scenes: a hypothesis whose 4 sampled ranks (the oracle's restatement of the header's sampler) are all
    planted inliers is the true pose, so its count reaches the number of planted inliers -- which it can only do if the
    kernel drew those very rows.  Pair 1 has invalid rows (ranks are over the VALID rows)."""
    n, H, seed = 64, 200, 5
    p3, p2, _, _, inl, thr = scenes((10, 11, 12), n, 0.25, 0.0)
    valid = np.ones((3, n), bool)
    valid[1, ::5] = False
    _, _, count = ops.pnp_hypotheses(*gpu(p3, p2, valid), H, thr, seed)
    count = count.cpu().numpy()
    checked = short = 0
    for b in range(3):
        vidx = np.flatnonzero(valid[b])
        planted = int((inl[b] & valid[b]).sum())
        for h in range(H):
            if inl[b][vidx[QO.sample_ranks(seed, b, h, len(vidx))]].all():
                checked += 1
                short += count[b, h] < planted
    print(f"{checked} all-inlier hypotheses, {short} of them short of the planted count")
    assert checked >= 60 and short == 0


@pytest.mark.parametrize("n,H", [(64, 200), (97, 200), (65, 65), (4, 1)])
def test_hypotheses_match_the_oracle_per_hypothesis(n, H):
    seed = 7
    p3, p2, _, _, _, thr = scenes(tuple(range(100, 109)), n, 0.25 if n > 4 else 0.0, 0.5)
    rt_h, cost, count = (x.cpu().numpy() for x in ops.pnp_hypotheses(*gpu(p3, p2), None, H, thr, seed))
    total = within = 0
    rels = []
    for b in range(9):
        _, oc, ok_, _ = QO.hypotheses(p3[b], p2[b], None, H, thr, seed, b)
        both = np.isfinite(cost[b]) & np.isfinite(oc)
        neither = np.isinf(cost[b]) & np.isinf(oc)
        near = both & (np.abs(count[b].astype(np.int64) - ok_) <= 1)
        assert not count[b][np.isinf(cost[b])].any() and not rt_h[b][np.isinf(cost[b])].any() and (cost[b] > 0).all()
        total += H
        within += int((near | neither).sum())
        rels.append(np.abs(cost[b][near].astype(D) - oc[near]) / oc[near])
    rels = np.concatenate(rels)
    print(f"n={n} H={H}: |dcount| <= 1 on {within / total:.4f} of {total} hypotheses; cost relative deviation on those: max "
          f"{rels.max():.3e} median {np.median(rels):.3e}; refused {np.isinf(cost).sum()}")
    assert within >= 0.90 * total
    assert rels.max() <= COST_RTOL[(n, H)]


@pytest.mark.parametrize("n,H", [(64, 1), (97, 64), (65, 65), (64, 200)])
def test_selection_is_exact_and_zero_rounds_return_the_hypothesis(n, H):
    p3, p2, _, _, _, thr = scenes((100, 101, 102), n, 0.25, 0.5)
    valid = np.ones((3, n), bool)
    valid[2, 3::7] = False
    x, u, v = gpu(p3, p2, valid)
    rt_h, cost, count = ops.pnp_hypotheses(x, u, v, H, thr, 9)
    r, t, inlier, best_h, cnt, rmse, info, ok = ops.pnp_ransac(x, u, v, H, thr, 0, 9)
    cost_np = cost.cpu().numpy()
    for b in range(3):
        bh = int(np.argmin(cost_np[b]))                                        # numpy: the first minimum
        assert int(best_h[b]) == bh
        if not bool(ok[b]):                                                    # H = 1: the only sample may explain < 4 rows
            assert int(count[b, bh]) < 4 and int(cnt[b]) == 0 and not inlier[b].any() and not info[b].any()
            continue
        assert torch.equal(bits(r[b].reshape(9)), bits(rt_h[b, bh, :9])) and torch.equal(bits(t[b]), bits(rt_h[b, bh, 9:]))
        assert int(cnt[b]) == int(count[b, bh]) == int(inlier[b].sum())
        assert not (inlier[b].cpu().numpy() & ~valid[b]).any()
        R64, t64 = r[b].cpu().numpy().astype(D), t[b].cpu().numpy().astype(D)
        d2 = QO.dist2(R64, t64, p3[b].astype(D), p2[b].astype(D))
        clear = np.abs(d2 / thr ** 2 - 1) > 1e-3                               # not within rounding of the threshold
        got = inlier[b].cpu().numpy()
        assert np.array_equal(got[clear], ((d2 <= thr ** 2) & valid[b])[clear])
        # float32 evaluation of x / z - u at |u| <= 0.7: a few roundings of 6e-8 per component, 1e-5 relative from the sum
        assert abs(float(rmse[b]) - np.sqrt(d2[got].mean())) <= 4e-7 + 1e-5 * np.sqrt(d2[got].mean())
        A = QO.linearise(R64, t64, p3[b][got], p2[b][got])[0]
        assert np.abs(info[b].cpu().numpy() - A).max() <= 1e-5 * np.abs(A).max() and torch.equal(info[b], info[b].T)
    # refinement never makes the cost worse, and the refined pose and mask are the oracle's given the kernel's selection
    r3, t3, inl3, bh3, cnt3, rmse3, info3, ok3 = ops.pnp_ransac(x, u, v, H, thr, 3, 9)
    assert torch.equal(bh3, best_h)
    for b in range(3):
        if not bool(ok[b]):
            continue
        a, bb = p3[b][valid[b]].astype(D), p2[b][valid[b]].astype(D)
        c0 = QO.score(r[b].cpu().numpy().astype(D), t[b].cpu().numpy().astype(D), a, bb, thr)[0]
        c3 = QO.score(r3[b].cpu().numpy().astype(D), t3[b].cpu().numpy().astype(D), a, bb, thr)[0]
        print(f"n={n} H={H} pair {b}: cost {c0:.4e} -> {c3:.4e} after 3 rounds, count {int(cnt[b])} -> {int(cnt3[b])}")
        # both costs are float64 here; the kernel compared float32 evaluations, each d^2 off by up to 2 d * 2e-7, which is
        # 4e-4 of d^2 at the 0.5 px (1e-3) level of these scenes
        assert bool(ok3[b]) and c3 <= c0 * (1 + 8e-4)


# ---- refit ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,noise", [(64, 0.0), (64, 0.5), (97, 0.0), (97, 0.5), (4, 0.0)])
def test_refit_matches_the_oracle(n, noise):
    p3, p2, Rs, ts, inl, thr = scenes((100, 101, 102), n, 0.25 if n > 4 else 0.0, noise)
    mask = inl.copy()
    if n > 4:
        mask[1, :] &= np.arange(n) % 3 != 0                                    # a middle pair with a different mask
    start = [perturbed(Rs[b], ts[b]) for b in range(3)]
    r0, t0 = np.stack([s[0] for s in start]), np.stack([s[1] for s in start])
    x, u, m, gr0, gt0 = gpu(p3, p2, mask, r0, t0)
    r, t, info, ok = ops.pnp_refit(x, u, m, gr0, gt0)
    assert ok.all()
    for b in range(3):
        Rr, tr, A, oko = QO.refit(p3[b], p2[b], mask[b], r0[b], t0[b])
        assert oko
        rot, dt = PO.rotation_angle_deg(r[b].cpu().numpy(), Rr), RO.translation_error(t[b].cpu().numpy(), tr)
        da = np.abs(info[b].cpu().numpy() - A).max() / np.abs(A).max()
        print(f"refit n={n} noise={noise} pair {b}: rotation {rot:.2e} deg, translation {dt:.2e} m, info {da:.2e}; "
              f"from the truth {PO.rotation_angle_deg(r[b].cpu().numpy(), Rs[b]):.2e} deg")
        assert rot <= REFIT_ROT_DEG and dt <= REFIT_T_M and da <= INFO_RTOL
        assert torch.equal(info[b], info[b].T) and abs(float(torch.linalg.det(r[b].double().cpu())) - 1) < 1e-5
    if n == 4:
        return
    # 3 rows; rows on one line through the camera centre's side (rank-deficient); rows behind the camera: refused, the start returned
    few = np.zeros((3, n), bool)
    few[0, np.flatnonzero(mask[0])[:3]] = True
    few[1:, :8] = True
    y = x.clone()
    y[1, :8] = torch.from_numpy((np.outer(np.ones(8), [0.3, -0.2, 4.0])).astype(np.float32)).to(DEV)   # one point eight times
    y[2, :8] = -x[2, :8]                                                       # behind the camera under the start
    r, t, info, ok = ops.pnp_refit(y, u, gpu(few), gr0, gt0)
    assert not ok.any() and torch.equal(bits(r), bits(gr0)) and torch.equal(bits(t), bits(gt0)) and not info.any()


# ---- the whole path --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 64, 96, 2048])
@pytest.mark.parametrize("outliers", [0.25, 0.40])
def test_ground_truth_pose(n, outliers):
    H = 64
    p3, p2, R, t, inl, thr = scenes(GT_SCENES, n, outliers, 0.0)
    k1, k2, d1, _, _, _, _ = raw_scenes(GT_SCENES, n, outliers, 0.0)
    for b in range(3):                                                         # every seed has an all-inlier sample
        assert QO.has_all_inlier_sample(GT_SEED, b, H, np.ones(n, bool), inl[b]), GT_SCENES[b]
    m = AbsolutePoseEstimator(torch.from_numpy(K), num_hypotheses=H, ransac_threshold=QO.THR_PX, refine_rounds=3, seed=GT_SEED).to(DEV)
    x, kp2 = gpu(p3, k2)
    Rg, tg, mask, rmse_px, info, ok = m(x, kp2)
    for b in range(3):
        got = mask[b].cpu().numpy()
        rot, dt = PO.rotation_angle_deg(Rg[b].cpu().numpy(), R[b]), RO.translation_error(tg[b].cpu().numpy(), t[b])
        print(f"n={n} outliers={outliers} seed {GT_SCENES[b]}: recall {(got & inl[b]).sum()}/{inl[b].sum()}, false {(got & ~inl[b]).sum()}, "
              f"rotation {rot:.2e} deg, |t - t_true| {dt:.2e} m, rmse {float(rmse_px[b]):.2e} px")
        assert bool(ok[b]) and np.array_equal(got, inl[b])
        assert rot <= GT_ROT_DEG and dt <= GT_T_M
        assert abs(float(torch.linalg.det(Rg[b].double().cpu())) - 1) < 1e-5 and float(rmse_px[b]) < 0.01
        assert np.linalg.eigvalsh(info[b].cpu().numpy().astype(D)).min() > 0
    # unbatched input gives unbatched output with the same bits for pair 0
    single = m(x[0], kp2[0])
    assert single[0].shape == (3, 3) and single[2].shape == (n,) and single[4].shape == (6, 6) and single[5].dim() == 0
    assert all(torch.equal(a, bb[0]) for a, bb in zip(single, (Rg, tg, mask, rmse_px, info, ok)))
    # forward_rgbd is the lift through the module's own K_inv (torch's float32 inverse, which may differ from the scenes'
    # by a rounding), then forward
    tk1, td1 = gpu(k1, d1)
    x1, v1 = ops.lift_keypoints(tk1, td1, m.K_inv, 1.0, 0.1, 10.0)
    assert bool(v1.all())
    assert all(torch.equal(bits(a), bits(bb)) for a, bb in zip(m.forward_rgbd(tk1, kp2, td1), m(x1, kp2)))


def test_depth_holes_in_the_second_frame():
    """frame 2 has depth at 2 of the matched keypoints only: RgbdPoseEstimator has nothing to work with, the 3-D to 2-D
    solve returns the true motion in the depth's units"""
    n, H = 64, 64
    k1, k2, d1, d2, R, t, inl = raw_scenes(GT_SCENES, n, 0.25, 0.0)
    holes = np.zeros_like(d2)
    for b in range(3):
        q = np.floor(k2[b][np.flatnonzero(inl[b])[:2]] + np.float32(0.5)).astype(int)
        holes[b, q[:, 0], q[:, 1]] = d2[b, q[:, 0], q[:, 1]]
    Kt = torch.from_numpy(K)
    tk1, tk2, td1, th2 = gpu(k1, k2, d1, holes)
    ok17 = RgbdPoseEstimator(Kt, num_hypotheses=H, seed=GT_SEED).to(DEV)(tk1, tk2, td1, th2)[4]
    assert not ok17.any()
    m = AbsolutePoseEstimator(Kt, num_hypotheses=H, seed=GT_SEED).to(DEV)
    Rg, tg, mask, rmse_px, info, ok = m.forward_rgbd(tk1, tk2, td1.unsqueeze(1))
    for b in range(3):
        rot, dt = PO.rotation_angle_deg(Rg[b].cpu().numpy(), R[b]), RO.translation_error(tg[b].cpu().numpy(), t[b])
        print(f"depth holes, seed {GT_SCENES[b]}: rotation {rot:.2e} deg, |t - t_true| {dt:.2e} m (|t| = {np.linalg.norm(t[b]):.2f} m)")
        assert bool(ok[b]) and np.array_equal(mask[b].cpu().numpy(), inl[b]) and rot <= GT_ROT_DEG and dt <= GT_T_M
    # millimetre counts: the translation comes out in depth * depth_scale.  Rounding to 1 mm moves a point by at most 0.5 mm
    # along its ray; over points spread by more than 1 m that is at most 5e-4 rad = 0.03 deg, and 3.5 mm at the centroid's 6 m
    mm = torch.from_numpy(np.round(d1 * 1000.0).astype(np.uint16)).to(DEV)
    R16, t16, mask16, _, _, ok16 = m.forward_rgbd(tk1, tk2, mm, depth_scale=0.001)
    for b in range(3):
        assert bool(ok16[b]) and (mask16[b].cpu().numpy() & inl[b]).sum() == inl[b].sum()
        assert PO.rotation_angle_deg(R16[b].cpu().numpy(), R[b]) < 0.03 and RO.translation_error(t16[b].cpu().numpy(), t[b]) < 3.5e-3


def _failed(r, t, inlier, best_h, cnt, rmse, info, ok, b):
    return (not bool(ok[b]) and torch.equal(r[b], torch.eye(3, device=DEV)) and not t[b].any() and not inlier[b].any()
            and int(cnt[b]) == 0 and float(rmse[b]) == 0.0 and not info[b].any())


@pytest.mark.parametrize("batch", [1, 3])
def test_degenerate_pairs_and_small_shapes(batch):
    seeds = (20, 21, 22)[:batch]
    for n in (1, 3):                                                           # fewer than 4 rows
        p3, p2, _, _, _, thr = scenes(seeds, n, 0.0, 0.0)
        x, u = gpu(p3, p2)
        rt_h, cost, count = ops.pnp_hypotheses(x, u, None, 65, thr, 0)
        assert torch.isinf(cost).all() and (cost > 0).all() and not count.any() and not rt_h.any()
        out = ops.pnp_ransac(x, u, None, 65, thr, 3, 0)
        assert all(_failed(*out, b) for b in range(batch)) and not out[3].any()
        r, t, info, ok = ops.pnp_refit(x, u, gpu(np.ones((batch, n), bool)), *gpu(np.stack([np.eye(3, dtype=np.float32)] * batch),
                                                                                      np.zeros((batch, 3), np.float32)))
        assert not ok.any() and torch.equal(r, torch.eye(3, device=DEV).expand(batch, 3, 3)) and not t.any() and not info.any()
    # n = 4: every sample is the four rows in some order
    p3, p2, R, t, _, thr = scenes(seeds, 4, 0.0, 0.0)
    x, u = gpu(p3, p2)
    out = ops.pnp_ransac(x, u, None, 64, thr, 3, 0)
    for b in range(batch):
        rot, dt = PO.rotation_angle_deg(out[0][b].cpu().numpy(), R[b]), RO.translation_error(out[1][b].cpu().numpy(), t[b])
        print(f"n=4 pair {b}: rotation {rot:.2e} deg, translation {dt:.2e} m, rmse {float(out[5][b]) * FOCAL:.2e} px")
        assert bool(out[7][b]) and out[2][b].all() and int(out[4][b]) == 4 and rot <= SOLVE_ROT_DEG and dt <= SOLVE_T_M
    # n = 64 with 3 valid rows, and with none
    p3, p2, R, t, inl, thr = scenes(seeds, 64, 0.25, 0.0)
    x, u = gpu(p3, p2)
    for keep in (3, 0):
        valid = np.zeros((batch, 64), bool)
        valid[:, :keep] = True
        rt_h, cost, count = ops.pnp_hypotheses(x, u, gpu(valid), 64, thr, 3)
        assert torch.isinf(cost).all() and not count.any() and not rt_h.any()
        out = ops.pnp_ransac(x, u, gpu(valid), 64, thr, 3, 3)
        assert all(_failed(*out, b) for b in range(batch))
    # all model points on one line: every sample is degenerate
    line = np.stack([(np.outer(np.arange(16.0), [0.1, 0.2, 0.05]) + [0.3, -0.2, 4.0]).astype(np.float32)] * batch)
    lu = (line[..., :2] / line[..., 2:]).astype(np.float32)
    rt_h, cost, count = ops.pnp_hypotheses(*gpu(line, lu), None, 64, thr, 1)
    assert torch.isinf(cost).all() and not count.any() and not rt_h.any()
    assert all(_failed(*ops.pnp_ransac(*gpu(line, lu), None, 64, thr, 3, 1), b) for b in range(batch))
    # every point BEHIND the camera that sees these pixels (the mirrored scene: X' = -X - 2 R^T t has R X' + t = -(R X + t)).
    # A P3P solution needs three positive depths and the score puts z <= 0 beyond the threshold, so the planted pose is out
    # of reach.  With 4 rows nothing else explains all four (the float64 and the float32 oracle agree: ok = 0 for these
    # seeds); with 64 rows a chance pose may explain 4 or 5 (the oracles find such), every one of them in FRONT of it.
    def mirror(pts):
        return np.stack([(-pts[b].astype(D) - 2.0 * (R[b].T @ t[b])).astype(np.float32) for b in range(batch)])
    p4, u4, R, t, _, _ = scenes(seeds, 4, 0.0, 0.0)
    assert all(_failed(*ops.pnp_ransac(*gpu(mirror(p4), u4), None, 64, thr, 3, 3), b) for b in range(batch))
    p3, p2, R, t, inl, thr = scenes(seeds, 64, 0.25, 0.0)
    xm = gpu(mirror(p3))
    out = ops.pnp_ransac(xm, u, None, 64, thr, 3, 3)
    for b in range(batch):
        got = out[2][b].cpu().numpy()
        z = (mirror(p3)[b].astype(D) @ out[0][b].cpu().numpy().astype(D).T + out[1][b].cpu().numpy().astype(D))[:, 2]
        print(f"mirrored scene, pair {b}: ok {bool(out[7][b])}, {int(out[4][b])} inliers of {int(inl[b].sum())} planted")
        assert (z[got] > 0).all() and int(out[4][b]) == got.sum() < inl[b].sum() // 2
    true_rt = gpu(np.stack([np.concatenate([R[b].ravel(), t[b]]).astype(np.float32) for b in range(batch)]))
    r, tt, info, ok = ops.pnp_refit(xm, u, gpu(inl[:batch]), true_rt[:, :9].reshape(batch, 3, 3).contiguous(), true_rt[:, 9:].contiguous())
    assert not ok.any() and not info.any()


# ---- the contract ----------------------------------------------------------------------------------------------------------------

def _raw_pnp(x, u, v, H, rounds, seed, fill, thr):
    """pnp_hypotheses, pnp_ransac and pnp_refit through the C ABI into outputs and a workspace filled with `fill` bytes first"""
    b, n = x.shape[:2]

    def dirty(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(fill)
        return t
    rt_h, cost, count = dirty((b, H, 12), torch.float32), dirty((b, H), torch.float32), dirty((b, H), torch.int32)
    N.call("mi_pnp_hypotheses", x.data_ptr(), u.data_ptr(), v.data_ptr(), b, n, H, thr, seed, rt_h.data_ptr(), cost.data_ptr(),
           count.data_ptr(), N.stream_ptr())
    wbytes = int(N.load().mi_pnp_ransac_workspace_bytes(b, n, H))
    ws = dirty((wbytes,), torch.uint8)
    r, t, inl = dirty((b, 3, 3), torch.float32), dirty((b, 3), torch.float32), dirty((b, n), torch.uint8)
    bh, cnt, rmse, ok = dirty((b,), torch.int32), dirty((b,), torch.int32), dirty((b,), torch.float32), dirty((b,), torch.uint8)
    info = dirty((b, 6, 6), torch.float32)
    N.call("mi_pnp_ransac", x.data_ptr(), u.data_ptr(), v.data_ptr(), b, n, H, thr, rounds, seed, r.data_ptr(), t.data_ptr(),
           inl.data_ptr(), bh.data_ptr(), cnt.data_ptr(), rmse.data_ptr(), info.data_ptr(), ok.data_ptr(), ws.data_ptr(), wbytes,
           N.stream_ptr())
    r2, t2, ok2, info2 = dirty((b, 3, 3), torch.float32), dirty((b, 3), torch.float32), dirty((b,), torch.uint8), dirty((b, 6, 6), torch.float32)
    N.call("mi_pnp_refit", x.data_ptr(), u.data_ptr(), inl.data_ptr(), r.data_ptr(), t.data_ptr(), b, n, r2.data_ptr(), t2.data_ptr(),
           info2.data_ptr(), ok2.data_ptr(), N.stream_ptr())
    return [rt_h, cost, count, r, t, inl, bh, cnt, rmse, info, ok, r2, t2, info2, ok2]


def test_outputs_are_fully_written_reproducible_and_blind_to_invalid_rows():
    n, H = 97, 200
    p3, p2, _, _, _, thr = scenes((100, 101, 102), n, 0.25, 0.5)
    vin = np.ones((3, n), np.uint8)
    vin[0, 5::9] = 0
    vin[1, :7] = 0
    x, u, v = gpu(p3, p2, vin)
    a = _raw_pnp(x, u, v, H, 3, 21, 0xFF, thr)                                  # 0xFF bytes: NaN floats, -1 integers
    b = _raw_pnp(x, u, v, H, 3, 21, 0x00, thr)
    assert same_bits(a, b)                                                    # every output byte written; two runs agree
    assert not any(torch.isnan(t).any() for t in (a[0], a[1], a[3], a[4], a[8], a[9], a[11], a[12], a[13]))
    assert set(torch.unique(a[5]).tolist()) <= {0, 1} and not (a[5].bool() & ~v.bool()).any()      # inlier <= valid
    assert a[10].bool().all() and a[14].bool().all()
    # invalid rows may hold anything: NaN in the points, 1e30 in the pixels
    y, w = x.clone(), u.clone()
    y[~v.bool()] = float("nan")
    w[~v.bool()] = 1e30
    assert same_bits(a, _raw_pnp(y, w, v, H, 3, 21, 0xFF, thr))
    # the entry without a sampler does not depend on the batch position
    perm = [2, 0, 1]
    r_p, t_p, info_p, ok_p = ops.pnp_refit(x[perm].contiguous(), u[perm].contiguous(), a[5][perm].contiguous(), a[3][perm].contiguous(),
                                           a[4][perm].contiguous())
    assert torch.equal(bits(r_p), bits(a[11][perm])) and torch.equal(bits(t_p), bits(a[12][perm]))
    assert torch.equal(bits(info_p), bits(a[13][perm])) and torch.equal(ok_p, a[14][perm].bool())


def test_normalise_ransac_and_the_module_replay_from_one_graph():
    n, H = 64, 64
    sets = []
    for s in ((100, 101, 102), (103, 104, 105), (106, 107, 108)):
        k1, k2, d1, _, _, _, _ = raw_scenes(s, n, 0.25, 0.5)
        sets.append(list(gpu(scenes(s, n, 0.25, 0.5)[0], k1, k2, d1)))
    m = AbsolutePoseEstimator(torch.from_numpy(K), num_hypotheses=H, seed=4).to(DEV)
    ki = k_inv(K)

    def run(x, k1, k2, d1):
        u = ops.normalise_keypoints(k2, ki)
        return (u,) + tuple(ops.pnp_ransac(x, u, None, H, THR, 3, 4)) + tuple(m(x, k2)) + tuple(m.forward_rgbd(k1, k2, d1))
    eager = [[t.clone() for t in run(*s)] for s in sets]
    static = [t.clone() for t in sets[0]]
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
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out, eager[i])), i
