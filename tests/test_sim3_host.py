"""K30 similarity alignment without a GPU: the host-side argument checks of the five entries (MI_E_* before any launch, in
the header's order of precedence), the Python module's constructor and its refusal of CPU tensors, the exports through the
`pytorch_model` alias, synth_sim3_maps, the numpy oracle's own sanity and degenerate cases, and the kernels' arithmetic
(csrc/sim3_math.h on csrc/rigid_math.h and csrc/pose_sampler.h) compiled for the host in tests/native/sim3_host.cpp, plain
and under the host's address and undefined-behaviour sanitizers.

Tolerances of the native program against the float64 oracle, measured on this file's own scenes (3 scenes x 64 minimal
samples of synth_sim3_maps(seed, 64, 0.25, 0.003, 2.5); the refit on the planted inliers of n = 64 / 97 with ray noise 0 and
0.003, 12 sets), the larger of the float32 oracle's and the native program's deviation, times 2:
  - minimal solve (192 samples): float32 oracle 3.44e-4 deg, 2.69e-7 relative in s, 9.33e-5 in t; native 1.90e-4 deg, 3.44e-7,
    5.23e-5 -> SOLVE_ROT_DEG = 6.9e-4, SOLVE_S_REL = 6.9e-7, SOLVE_T = 1.9e-4;
  - refit: float32 oracle 7.28e-6 deg, 2.08e-7, 6.90e-6; native 1.52e-5 deg, 3.46e-7, 1.08e-5 -> REFIT_ROT_DEG = 3.1e-5,
    REFIT_S_REL = 7.0e-7, REFIT_T = 2.2e-5.
t is in map-2 units at scale 2.5 (points up to 25 units from the camera)."""
import ctypes

import numpy as np
import pytest
import torch

import pose_oracle as PO
import rigid_oracle as RO
import sim3_oracle as SO
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import synth_sim3_maps

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
SCALE = 2.5
SOLVE_ROT_DEG, SOLVE_S_REL, SOLVE_T = 6.9e-4, 6.9e-7, 1.9e-4
REFIT_ROT_DEG, REFIT_S_REL, REFIT_T = 3.1e-5, 7.0e-7, 2.2e-5


@pytest.fixture(scope="module")
def lib():
    return N.load_sim3()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


p_keepalive = []


def test_the_section_has_a_header_and_a_library_of_its_own(lib):
    assert sorted(N.SIM3_SIGNATURES) == ["mi_sim3_apply", "mi_sim3_hypotheses", "mi_sim3_ransac", "mi_sim3_ransac_workspace_bytes",
                                         "mi_sim3_refit"]
    assert not set(N.SIM3_SIGNATURES) & set(N.SIGNATURES)
    assert N.SIM3_CONSTANTS["MI_SIM3_MAX_N"] == 2048 and N.SIM3_CONSTANTS["MI_SIM3_POINT"] == 0 and N.SIM3_CONSTANTS["MI_SIM3_REPROJ"] == 1
    assert N.SIM3_CONSTANTS["MI_SIM3_MIN_SCALE"] == 1e-3 and N.SIM3_CONSTANTS["MI_SIM3_MAX_SCALE"] == 1e3
    assert N.library_of("mi_sim3_refit") is lib and N.library_of("mi_rigid_refit") is N.load()
    assert not hasattr(N.load(), "mi_sim3_refit")                            # the product library exports its own header only
    assert lib.mi_sim3_ransac_workspace_bytes.restype is ctypes.c_size_t


def test_hypotheses_argument_checks(lib, p):
    f = lib.mi_sim3_hypotheses
    good = [p, p, p, 1, 8, 4, 0.05, 1, 0, p, p, p, None]
    for i in (0, 1, 9, 10, 11):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i
    a = list(good)
    a[2] = None                                                              # valid may be NULL; nothing else wrong -> a launch
    a[3] = 0                                                                 # ... so make the shape wrong: SHAPE, not NULL
    assert f(*a) == SHAPE
    for batch, n, h, thr, metric, want in ((0, 8, 4, 0.05, 0, SHAPE), (1, 0, 4, 0.05, 0, SHAPE), (1, -3, 4, 0.05, 1, SHAPE),
                                           (1, 8, 0, 0.05, 0, SHAPE), (1, 2049, 4, 0.05, 0, PARAM), (70000, 8, 4, 0.05, 0, PARAM),
                                           (1, 8, 65537, 0.05, 0, PARAM), (1, 8, 4, 0.0, 0, PARAM), (1, 8, 4, -1.0, 1, PARAM),
                                           (1, 8, 4, float("nan"), 0, PARAM), (1, 8, 4, float("inf"), 0, PARAM),
                                           (1, 8, 4, 0.05, 2, PARAM), (1, 8, 4, 0.05, -1, PARAM),
                                           (1, 8, 0, 0.05, 2, SHAPE), (0, 8, 4, 0.0, 2, SHAPE)):          # shape before parameters
        assert f(p, p, p, batch, n, h, thr, metric, 0, p, p, p, None) == want, (batch, n, h, thr, metric)
    assert f(None, p, p, 0, 8, 4, 0.05, 0, 0, p, p, p, None) == NULL         # NULL before shape


def test_refit_argument_checks(lib, p):
    f = lib.mi_sim3_refit
    for i in (0, 1, 2, 5, 6, 7, 8):
        a = [p, p, p, 1, 8, p, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    assert f(p, p, p, 1, 0, p, p, p, p, None) == SHAPE and f(p, p, p, 0, 8, p, p, p, p, None) == SHAPE
    assert f(p, p, p, 1, 4096, p, p, p, p, None) == PARAM and f(p, p, p, 65536, 8, p, p, p, p, None) == PARAM
    assert f(p, p, p, 0, 4096, p, p, p, p, None) == SHAPE and f(p, p, None, 0, 8, p, p, p, p, None) == NULL


def test_ransac_argument_checks(lib, p):
    f, wb = lib.mi_sim3_ransac, lib.mi_sim3_ransac_workspace_bytes
    need = wb(3, 97, 200)
    assert need >= 3 * 200 * (13 + 1 + 1) * 4 and need % 16 == 0
    assert wb(3, 0, 200) == 0 and wb(3, 97, 0) == 0 and wb(3, 3000, 200) == 0 and wb(0, 97, 200) == 0
    assert wb(3, 97, 65537) == 0 and wb(65536, 97, 200) == 0 and wb(3, 2048, 128) > 0
    good = [p, p, p, 3, 97, 200, 0.05, 1, 3, 0, p, p, p, p, p, p, p, p, p, need, None]
    for i in (0, 1, 10, 11, 12, 13, 14, 15, 16, 17, 18):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=3, n=97, h=200, thr=0.05, metric=1, rounds=3, ws=p, wbytes=need)
        a.update(kw)
        return f(p, p, p, a["batch"], a["n"], a["h"], a["thr"], a["metric"], a["rounds"], 0, p, p, p, p, p, p, p, p, a["ws"], a["wbytes"],
                 None)
    assert call(n=0) == SHAPE and call(h=0) == SHAPE and call(batch=0) == SHAPE
    assert call(thr=0.0) == PARAM and call(thr=-0.5) == PARAM and call(thr=float("inf")) == PARAM
    assert call(metric=2) == PARAM and call(metric=-1) == PARAM
    assert call(rounds=-1) == PARAM and call(rounds=9) == PARAM and call(n=2049) == PARAM and call(h=65537) == PARAM
    assert call(wbytes=need - 1) == CAPACITY                                # workspace too small
    assert call(ws=p + 4) == ALIGN                                          # misaligned workspace
    # precedence: shape, parameters, alignment, capacity
    assert call(n=0, metric=2, ws=p + 4, wbytes=0) == SHAPE and call(metric=2, ws=p + 4, wbytes=0) == PARAM
    assert call(rounds=9, ws=p + 4, wbytes=0) == PARAM and call(ws=p + 4, wbytes=0) == ALIGN


def test_apply_argument_checks(lib, p):
    f = lib.mi_sim3_apply
    good = [p, p, p, 2, 4, 16, p, p, p, p, p, p, None]
    for i in (0, 1, 2, 6, 7, 8, 9, 10, 11):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i
    # a side that is absent may be NULL, and then nothing of the call is wrong up to the launch: checked by the shape refusals
    assert f(p, p, p, 0, 0, 16, None, None, p, None, None, p, None) == SHAPE
    assert f(p, p, p, 0, 4, 0, p, p, None, p, p, None, None) == SHAPE
    assert f(p, p, p, 2, 0, 0, None, None, None, None, None, None, None) == SHAPE
    assert f(p, p, p, 2, -1, 16, None, None, p, None, None, p, None) == SHAPE and f(p, p, p, 2, 4, -1, p, p, None, p, p, None, None) == SHAPE
    assert f(p, p, p, 65536, 4, 16, p, p, p, p, p, p, None) == PARAM
    assert f(p, p, p, 2, 1 << 24, 1, p, p, p, p, p, p, None) == PARAM
    assert f(p, p, p, 0, 1 << 24, 1, p, p, p, p, p, p, None) == SHAPE       # shape before parameters


def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import SimilarityEstimator
    m = SimilarityEstimator()
    assert (m.metric, m.threshold, m.focal, m.num_hypotheses, m.refine_rounds, m.seed) == ("reprojection", 0.004, None, 128, 3, 0)
    m = SimilarityEstimator("reprojection", 2.0, focal=500.0)
    assert m.kernel_threshold == 0.004 and m.metric_id == ops.SIM3_REPROJ
    mp = SimilarityEstimator("point", 0.05)
    assert mp.kernel_threshold == 0.05 and mp.metric_id == ops.SIM3_POINT
    for kw in (dict(metric="pixel"), dict(metric="point"), dict(metric="point", threshold=0.05, focal=500.0), dict(threshold=0.0),
               dict(threshold=float("inf")), dict(focal=0.0), dict(focal=float("nan")), dict(num_hypotheses=0), dict(refine_rounds=-1),
               dict(refine_rounds=9)):
        with pytest.raises(ValueError):
            SimilarityEstimator(**kw)
    z = torch.zeros(1, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(z[0], z[0], torch.ones(16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"\(B, N, 3\) or \(N, 3\)"):
        m(torch.zeros(2, 16, 2), torch.zeros(2, 16, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.align_trajectory(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.apply(torch.ones(1), torch.eye(3)[None], torch.zeros(1, 3), None, None, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sim3_hypotheses(z, z, None, 8, 0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sim3_refit(z, z, torch.ones(1, 16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sim3_ransac(z, z, None, 8, 0.05)
    with pytest.raises(RuntimeError, match="supported: 1 .. 2048"):
        ops.sim3_ransac(torch.zeros(1, 3000, 3), torch.zeros(1, 3000, 3), None, 8, 0.05)
    with pytest.raises(RuntimeError, match=r"must both be \(B, N, 3\)"):
        ops.sim3_hypotheses(torch.zeros(1, 16, 2), torch.zeros(1, 16, 2), None, 8, 0.05)
    with pytest.raises(RuntimeError, match="metric must be"):
        ops.sim3_hypotheses(z, z, None, 8, 0.05, metric=2)
    with pytest.raises(RuntimeError, match="needs frame poses or points"):
        ops.sim3_apply(torch.ones(1), torch.eye(3)[None], torch.zeros(1, 3), None, None, None)
    # the torch-only helpers run anywhere
    s, R, t = torch.tensor([2.0]), torch.from_numpy(SO.rodrigues(np.array([0.1, -0.2, 0.3]))).float()[None], torch.tensor([[0.5, -1.0, 2.0]])
    si, Ri, ti = SimilarityEstimator.inverse(s, R, t)
    x = torch.tensor([[[0.3, -0.7, 4.0]]])
    y = s[:, None, None] * (x @ R.transpose(1, 2)) + t[:, None]
    assert torch.allclose(si[:, None, None] * (y @ Ri.transpose(1, 2)) + ti[:, None], x, atol=1e-6)
    Rp, tp = SimilarityEstimator.as_pose(s, R, t)
    yp = x @ Rp.transpose(1, 2) + tp[:, None]
    assert torch.allclose(yp[..., :2] / yp[..., 2:], y[..., :2] / y[..., 2:], atol=1e-6)     # the same projection


def test_landmark_pairs_gathers_camera_frame_points():
    """plain torch: runs on the CPU.  Two windows of 2 frames; keypoint i of keyframe 1 belongs to slot (i + 1) % 5 when i < 5."""
    from onnx_image_processing_amd.pytorch_model.geometry import SimilarityEstimator
    rng = np.random.default_rng(0)
    K_, L = 6, 5
    kp_track1 = torch.full((1, 2, K_), -1, dtype=torch.int32)
    kp_track1[0, 1, :5] = (torch.arange(5) + 1) % 5
    kp_track2 = torch.full((1, 2, K_), -1, dtype=torch.int32)
    kp_track2[0, 0, :5] = torch.arange(5)
    kp_track2[0, 0, 5] = -2                                                   # a conflicting component
    pts1, pts2 = torch.from_numpy(rng.normal(size=(1, L, 3))).float(), torch.from_numpy(rng.normal(size=(1, L, 3))).float()
    ok1, ok2 = torch.ones(1, L, dtype=torch.bool), torch.ones(1, L, dtype=torch.bool)
    ok2[0, 3] = False
    R1 = torch.from_numpy(np.stack([SO.rodrigues(rng.normal(size=3) * 0.2) for _ in range(2)])).float()[None]
    R2 = torch.from_numpy(np.stack([SO.rodrigues(rng.normal(size=3) * 0.2) for _ in range(2)])).float()[None]
    t1, t2 = torch.from_numpy(rng.normal(size=(1, 2, 3))).float(), torch.from_numpy(rng.normal(size=(1, 2, 3))).float()
    ij = torch.tensor([[[0, 0], [1, 1], [2, 3], [5, 2], [3, 5], [-1, 0], [4, 6], [4, 4]]], dtype=torch.int32)
    mv = torch.tensor([[True, True, True, True, True, True, True, False]])
    a, b, v = SimilarityEstimator.landmark_pairs(ij, mv, kp_track1, 1, pts1, ok1, R1, t1, kp_track2, torch.tensor([0]), pts2, ok2, R2, t2)
    assert v.tolist() == [[True, True, False, False, False, False, False, False]]  # slot 3 not ok; kp 5 no slot; -2; -1; 6 out of range
    assert torch.allclose(a[0, 0], R1[0, 1] @ pts1[0, 1] + t1[0, 1], atol=1e-6) and torch.allclose(b[0, 1], R2[0, 0] @ pts2[0, 1] + t2[0, 0], atol=1e-6)
    assert not a[0, 2:].any() and not b[0, 2:].any()
    u = SimilarityEstimator.landmark_pairs(ij[0], mv[0], kp_track1[0], 1, pts1[0], ok1[0], R1[0], t1[0], kp_track2[0], 0, pts2[0], ok2[0],
                                           R2[0], t2[0])
    assert all(torch.equal(x, y[0]) for x, y in zip(u, (a, b, v)))


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    import pytorch_model
    from pytorch_model.geometry import SimilarityEstimator
    assert SimilarityEstimator is real.SimilarityEstimator and "SimilarityEstimator" in real.__all__
    from pytorch_model.geometry.similarity import SimilarityEstimator as again
    assert again is SimilarityEstimator and "SimilarityEstimator" in pytorch_model.__doc__


def test_synth_sim3_maps_is_deterministic_and_consistent():
    a, b = synth_sim3_maps(3, 64, 0.25, 0.01, SCALE), synth_sim3_maps(3, 64, 0.25, 0.01, SCALE)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    x1, x2, s, R, t, inl = synth_sim3_maps(3, 64, 0.25, 0.0, SCALE)
    assert x1.shape == (64, 3) and x1.dtype == np.float32 and x2.dtype == np.float32 and inl.sum() == 48 and inl.dtype == bool
    assert s == SCALE and abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 0.4 * SCALE) < 1e-12
    res = np.linalg.norm(s * (x1 @ R.T) + t - x2, axis=1)
    assert res[inl].max() < 1e-5 and (res[~inl] > 0.1).all()                  # float32 coordinates up to 25 units
    assert (x1[:, 2] >= 3 - 1e-6).all() and (x2[:, 2] > 0).all()
    assert not np.array_equal(x1, synth_sim3_maps(4, 64, 0.25, 0.0, SCALE)[0])
    # the noise is along the rays: the projection of a point into its own camera does not move
    n1, n2 = synth_sim3_maps(3, 64, 0.25, 0.02, SCALE)[:2]
    assert np.abs(n1[:, :2] / n1[:, 2:] - x1[:, :2] / x1[:, 2:]).max() < 1e-6 and np.abs(n2[:, :2] / n2[:, 2:] - x2[:, :2] / x2[:, 2:]).max() < 1e-6
    assert 0.01 < np.std(n1[:, 2] / x1[:, 2] - 1) < 0.03
    for bad in (dict(n=0), dict(outliers=1.5), dict(ray_noise=-1.0), dict(scale=0.0)):
        with pytest.raises(ValueError):
            synth_sim3_maps(**{**dict(seed=0, n=8, outliers=0.0, ray_noise=0.0, scale=1.0), **bad})


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("scale", [0.4, 2.5])
def test_oracle_is_exact_on_noise_free_scenes(seed, scale):
    """a minimal solve on three planted inliers, the refit on all of them and the whole RANSAC under both metrics return the
    true similarity, in float64 and in float32; the score of the true similarity marks exactly the planted inliers"""
    x1, x2, s, R, t, inl = synth_sim3_maps(seed, 64, 0.4, 0.0, scale)
    for metric, thr in ((SO.POINT, SO.THR_POINT * scale), (SO.REPROJ, SO.THR_REPROJ)):
        cost, count, d2 = SO.score(s, R, t, x1.astype(np.float64), x2.astype(np.float64), thr, metric)
        assert count == inl.sum() and d2[inl].max() < 1e-10
    sel = np.flatnonzero(inl)[:3]
    sm, Rm, tm = SO.solve_minimal(x1[sel], x2[sel])
    assert PO.rotation_angle_deg(Rm, R) < 1e-3 and SO.scale_error(sm, s) < 1e-5 and np.linalg.norm(tm - t) < 1e-4 * scale
    for dtype, rot_tol, rel_tol in ((np.float64, 1e-5, 1e-6), (np.float32, 1e-3, 1e-4)):
        sr, Rr, tr, ok = SO.refit(x1, x2, inl, dtype)
        assert ok and PO.rotation_angle_deg(Rr, R) < rot_tol and SO.scale_error(sr, s) < rel_tol and np.linalg.norm(tr - t) < rel_tol * scale
        for metric, thr in ((SO.POINT, SO.THR_POINT * scale), (SO.REPROJ, SO.THR_REPROJ)):
            sn, Rn, tn, mask, best_h, cnt, rmse, ok = SO.ransac(x1, x2, None, 64, thr, metric, 3, 11, 0, dtype)
            assert ok and np.array_equal(mask, inl) and cnt == inl.sum() and rmse < 1e-4 * scale
            assert PO.rotation_angle_deg(Rn, R) < rot_tol and SO.scale_error(sn, s) < rel_tol and np.linalg.norm(tn - t) < rel_tol * scale
            assert abs(np.linalg.det(Rn.astype(np.float64)) - 1) < 1e-5


def test_oracle_degenerate_cases():
    x1, x2, s, R, t, _ = synth_sim3_maps(7, 16, 0.0, 0.0, SCALE)
    valid = np.zeros(16, bool)
    valid[:2] = True                                                          # n < 3
    for metric in (SO.POINT, SO.REPROJ):
        srt_h, cost, count, _ = SO.hypotheses(x1, x2, valid, 4, 0.05, metric, 0)
        assert np.isinf(cost).all() and not count.any() and not srt_h.any()
        assert SO.ransac(x1, x2, valid, 4, 0.05, metric, 3, 0)[7] is False
    sr, Rr, tr, ok = SO.refit(x1, x2, valid)
    assert ok is False and sr == 1 and np.array_equal(Rr, np.eye(3)) and not tr.any()
    line = np.outer(np.arange(3.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]      # collinear
    assert SO.solve_minimal(line, x2[:3]) is None and SO.solve_minimal(x1[:3], line) is None
    assert SO.solve_minimal(x1[[0, 0, 1]], x2[[0, 0, 1]]) is None           # a repeated point
    line8 = np.outer(np.arange(8.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]
    assert SO.refit(line8, SCALE * (line8 @ R.T) + t, np.ones(8, bool))[3] is False
    # the scale's range: inside at 1e-3 * 1.01 and 1e3 * 0.99, refused beyond it, in the minimal solve and in the refit
    for k, accepted in ((1.01e-3, True), (0.99e-3, False), (0.99e3, True), (1.01e3, False)):
        y2 = k * (x1.astype(np.float64) @ R.T) + t
        m = SO.solve_minimal(x1[:3].astype(np.float64), y2[:3])
        assert (m is not None) == accepted and (not accepted or SO.scale_error(m[0], k) < 1e-9)
        assert SO.refit(x1.astype(np.float64), y2, np.ones(16, bool))[3] == accepted
    # points behind either camera are never inliers of the reprojection metric
    y1, y2 = x1.astype(np.float64).copy(), x2.astype(np.float64).copy()
    y1[0, 2] = -y1[0, 2]
    y2[1] = -y2[1]
    d2 = SO.dist2(s, R, t, y1, y2, SO.REPROJ)
    assert np.isinf(d2[:2]).all() and np.isfinite(d2[2:]).all()
    cost, count, _ = SO.score(s, R, t, y1, y2, 0.004, SO.REPROJ)
    assert count == 14 and abs(cost - 2 * 0.004 ** 2) < 1e-9
    # apply: the identity R_k' X' + t_k' = s (R_k X + t_k)
    rng = np.random.default_rng(1)
    Rk = np.stack([SO.rodrigues(rng.normal(size=3) * 0.3) for _ in range(4)]).astype(np.float32)
    tk = rng.normal(size=(4, 3)).astype(np.float32)
    ro, to, xo = SO.apply(s, R, t, Rk, tk, x1)
    assert ro.dtype == np.float32 and xo.shape == x1.shape
    lhs = np.einsum("fij,nj->fni", ro.astype(np.float64), xo.astype(np.float64)) + to[:, None].astype(np.float64)
    rhs = s * (np.einsum("fij,nj->fni", Rk.astype(np.float64), x1.astype(np.float64)) + tk[:, None].astype(np.float64))
    assert np.abs(lhs - rhs).max() < 2e-5                                     # float32 roundings of values up to 30
    assert SO.apply(s, R, t, None, None, x1)[:2] == (None, None) and SO.apply(s, R, t, Rk, tk)[2] is None


def test_shared_frame_scene_leaves_the_oracle_inside_the_gpu_tests_bounds():
    """the end-to-end chain of tests/test_gpu_sim3.py on the oracles (tracks_oracle, landmark_pairs on the CPU, sim3_oracle in
    float64 and float32): 20 shared landmarks, the planted (3, I, 0) and the shared frame's pose within that test's bounds, 19
    landmarks within 6e-3 after `apply` under either metric, no row within 1e-3 of a threshold"""
    import test_gpu_sim3 as G
    from onnx_image_processing_amd.pytorch_model.geometry import SimilarityEstimator
    from onnx_image_processing_amd.synth import two_view_camera
    K = two_view_camera()
    A, B = SO.shared_frame_windows()
    pA, okA, ktA = SO.oracle_tracks(A, K)
    pB, okB, ktB = SO.oracle_tracks(B, K)
    k = A[0].shape[1]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    ij = torch.arange(k, dtype=torch.int32)[:, None].expand(k, 2).contiguous()
    p1, p2, valid = (x.numpy() for x in SimilarityEstimator.landmark_pairs(
        ij, torch.ones(k, dtype=torch.bool), T(ktA), 3, T(pA), T(okA), T(A[4]), T(A[5]), T(ktB), 0, T(pB), T(okB), T(B[4]), T(B[5])))
    assert valid.sum() == 20
    la, lb = np.maximum(ktA[3], 0), np.maximum(ktB[0], 0)
    centre = lambda Rx, tx: -(np.asarray(Rx, np.float64).T @ np.asarray(tx, np.float64))
    for metric, thr, want_count in ((SO.REPROJ, 2.0 / 500.0, 20), (SO.POINT, SO.E2E_TOL, 19)):
        s_tol, rot_tol, pos_tol = G.E2E[metric]
        for dtype in (np.float64, np.float32):
            s, R, t, inl, _, cnt, _, ok = SO.ransac(p1, p2, valid, 128, thr, metric, 3, 3, 0, dtype)
            assert ok and cnt == want_count
            d2 = SO.dist2(s, R, t, p1.astype(dtype), p2.astype(dtype), metric)
            assert not ((np.abs(d2 / thr ** 2 - 1) <= 1e-3) & valid).any()
            # half the GPU test's bounds: they are twice what is measured here
            assert SO.scale_error(s, SO.E2E_SIGMA) <= s_tol / 2 * 1.01 and np.linalg.norm(t) <= pos_tol / 2 * 1.01
            assert PO.rotation_angle_deg(np.asarray(R, np.float64), np.eye(3)) <= rot_tol / 2 * 1.01
            ro, to, xo = SO.apply(*SO.compose_to_map(s, R, t, A[4][3], A[5][3], B[4][0], B[5][0]), A[4], A[5], pA)
            assert PO.rotation_angle_deg(ro[3], B[4][0]) <= rot_tol / 2 * 1.01
            assert np.linalg.norm(centre(ro[3], to[3]) - centre(B[4][0], B[5][0])) <= pos_tol / 2 * 1.01
            dist = np.linalg.norm(xo[la].astype(np.float64) - pB[lb], axis=1)
            assert (dist[valid] <= SO.E2E_TOL).sum() == G.E2E_WITHIN


# tests/native/sim3_host.cpp: the kernels' own sampler, Horn solver, scale and scores, compiled for the host
sim3_host = host_program("sim3_host.cpp", hip=True)


@pytest.fixture(scope="module")
def sim3_host_san(tmp_path_factory):
    """the same program under the host's address and undefined-behaviour sanitizers (a stand-alone program)"""
    return build_host(tmp_path_factory.mktemp("sim3_host_san"), "sim3_host.cpp", hip=True, extra=SANITIZE)


def _rows(a, b):
    return "\n".join(" ".join("%.9g" % x for x in row) for row in np.concatenate([a, b], axis=1))


def _model(f):
    m = np.array(f, np.float64)
    return m[12], m[:9].reshape(3, 3), m[9:12]


def _minimal_samples():
    samples, meta = [], []
    for b, seed in enumerate((100, 101, 102)):
        x1, x2 = synth_sim3_maps(seed, 64, 0.25, 0.003, SCALE)[:2]
        for h in range(64):
            r = RO.sample_ranks(7, b, h, 64)
            samples.append(_rows(x1[r], x2[r]))
            meta.append((x1[r], x2[r]))
    line = (np.outer(np.arange(3.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]).astype(np.float32)
    tail = [(line, meta[0][1]), (meta[0][0], line), (meta[0][0][[0, 0, 1]], meta[0][1][[0, 0, 1]]),     # collinear x 2, repeated
            (meta[0][0], (meta[0][1] * np.float32(1e-4))), (meta[0][0] * np.float32(1e-4), meta[0][1])]  # s about 2.5e-4, 2.5e4
    return samples + [_rows(a, b) for a, b in tail], meta, len(tail)


def test_native_minimal_solver_matches_the_oracle(sim3_host):
    """s3_solve_minimal on the host: on 3 scenes x 64 samples its (s, R, t) is the float64 oracle's within the measured
    tolerance (module docstring) and its R is rg_solve_minimal's bit for bit; collinear and repeated-point samples and scales
    outside the range are refused with zeros"""
    samples, meta, n_tail = _minimal_samples()
    out = run_host(sim3_host, "solve", "\n".join(samples))
    assert len(out) == len(samples)
    for f in out[-n_tail:]:
        assert f[0] == "0" and not any(float(x) for x in f[1:14])
    assert all(f[14] == "1" for f in out)                                   # the shared rotation
    rot, sc, tr = [], [], []
    for (a, b), f in zip(meta, out):
        ref = SO.solve_minimal(a, b)
        assert (f[0] == "1") == (ref is not None)
        if ref is None:
            continue
        s, R, t = _model(f[1:14])
        assert abs(np.linalg.det(R) - 1) < 1e-5
        rot.append(PO.rotation_angle_deg(R, ref[1]))
        sc.append(SO.scale_error(s, ref[0]))
        tr.append(float(np.linalg.norm(t - ref[2])))
    print(f"native minimal solver, {len(rot)} samples: rotation max {max(rot):.3e} deg, scale max {max(sc):.3e}, translation max {max(tr):.3e}")
    assert len(rot) >= 180 and max(rot) <= SOLVE_ROT_DEG and max(sc) <= SOLVE_S_REL and max(tr) <= SOLVE_T


def test_native_fit_matches_the_oracle_and_refuses_degenerate_sets(sim3_host):
    rot, sc, tr = [], [], []
    for n in (64, 97):
        for noise in (0.0, 0.003):
            for seed in (100, 101, 102):
                x1, x2, s, R, t, inl = synth_sim3_maps(seed, n, 0.25, noise, SCALE)
                if seed == 101:
                    inl = inl & (np.arange(n) % 3 != 0)
                out = run_host(sim3_host, "fit", f"{inl.sum()}\n" + _rows(x1[inl], x2[inl]))
                ref = SO.refit(x1, x2, inl)
                assert out[0][0] == "1" and ref[3]
                gs, gR, gt = _model(out[0][1:14])
                rot.append(PO.rotation_angle_deg(gR, ref[1]))
                sc.append(SO.scale_error(gs, ref[0]))
                tr.append(float(np.linalg.norm(gt - ref[2])))
                if noise == 0.0:
                    assert PO.rotation_angle_deg(gR, R) < 1e-3 and SO.scale_error(gs, s) < 1e-5 and np.linalg.norm(gt - t) < 1e-3
    print(f"native refit, {len(rot)} sets: rotation max {max(rot):.3e} deg, scale max {max(sc):.3e}, translation max {max(tr):.3e}")
    assert max(rot) <= REFIT_ROT_DEG and max(sc) <= REFIT_S_REL and max(tr) <= REFIT_T
    x1, x2, s, R, t, inl = synth_sim3_maps(100, 64, 0.0, 0.0, SCALE)
    line = (np.outer(np.arange(8.0), [1.0, 2.0, 0.5]) + [0.3, -0.2, 4.0]).astype(np.float32)
    text = "\n".join(["8", _rows(line, (SCALE * (line @ R.T) + t).astype(np.float32)), "2", _rows(x1[:2], x2[:2]),
                      "64", _rows(x1, x2 * np.float32(1e-4)), "64", _rows(x1 * np.float32(1e-4), x2)])
    out = run_host(sim3_host, "fit", text)
    assert len(out) == 4 and all(f[0] == "0" and not any(float(x) for x in f[1:]) for f in out)


@pytest.mark.parametrize("metric", [SO.POINT, SO.REPROJ])
def test_native_hypothesis_lane_matches_the_oracle(sim3_host, metric):
    """the hypothesis kernel's lane on the host (sample, solve, serial score): equal refusals, the oracle's count within 1 on
    >= 90 % of the hypotheses, the cost on equal counts within the GPU suite's COST_RTOL (tests/test_gpu_sim3.py)"""
    thr = {SO.POINT: 0.1, SO.REPROJ: SO.THR_REPROJ}[metric]
    x1, x2 = synth_sim3_maps(101, 97, 0.25, 0.003, SCALE)[:2]
    x1, x2 = x1.copy(), x2.copy()
    x2[5] = -x2[5]                                                            # behind camera 2
    out = run_host(sim3_host, ["hyp", str(metric), "%.9g" % thr, "7", "1", "200"], "97\n" + _rows(x1, x2))
    srt, cost, count, _ = SO.hypotheses(x1, x2, None, 200, thr, metric, 7, 1)
    got_cost, got_count = np.array([float(f[1]) for f in out]), np.array([int(f[2]) for f in out])
    assert np.array_equal(np.isinf(got_cost), np.isinf(cost)) and np.isfinite(cost).mean() >= 0.9
    dk = np.abs(got_count - count)
    same = (dk == 0) & np.isfinite(cost)
    rel = np.abs(got_cost[same] - cost[same]) / cost[same]
    print(f"native lane, metric {metric}: |dcount| <= 1 {np.mean(dk <= 1):.3f}, cost rel dev on equal counts max {rel.max():.2e}")
    assert np.mean(dk <= 1) >= 0.9 and rel.max() <= 1.5e-4


@pytest.mark.parametrize("metric", [SO.POINT, SO.REPROJ])
def test_native_rmse_is_the_float64_evaluation_within_the_gpu_tests_bound(sim3_host, metric):
    """the selection kernel's count and rmse on the host (strided partial sums) under the float32 oracle's refined model: the
    count is the oracle's, the rmse the float64 evaluation of the same model over the same rows within half of
    tests/test_gpu_sim3.py's RMSE_ABS, which is twice the largest deviation measured"""
    import test_gpu_sim3 as G
    thr = G.THR[metric]
    for seed, b in ((100, 0), (101, 1), (102, 2)):
        x1, x2 = synth_sim3_maps(seed, 97, 0.25, 0.003, SCALE)[:2]
        s, R, t, inl, _, cnt, _, ok = SO.ransac(x1, x2, None, 64, thr, metric, 3, 9, b, np.float32)
        assert ok
        out = run_host(sim3_host, ["rmse", str(metric), "%.9g" % thr], " ".join("%.9g" % v for v in SO.pack(s, R, t)) + "\n97\n" + _rows(x1, x2))
        d2 = SO.dist2(float(s), R.astype(np.float64), t.astype(np.float64), x1.astype(np.float64), x2.astype(np.float64), metric)
        assert int(out[0][0]) == cnt and abs(float(out[0][1]) - np.sqrt(d2[inl].mean())) <= G.RMSE_ABS[metric] / 2 * 1.01


def test_native_program_is_clean_under_the_host_sanitizers(sim3_host, sim3_host_san):
    """every mode once more under -fsanitize=address,undefined: the same output, no report (run_host checks stderr)"""
    samples, _, _ = _minimal_samples()
    x1, x2 = synth_sim3_maps(100, 65, 0.25, 0.003, SCALE)[:2]
    sets = "\n".join(["65", _rows(x1, x2), "2", _rows(x1[:2], x2[:2]), "0"])
    for args, text in (("solve", "\n".join(samples[:40] + samples[-5:])), ("fit", sets),
                       (["hyp", "1", "0.004", "3", "2", "65"], "65\n" + _rows(x1, x2)), (["hyp", "0", "0.1", "3", "0", "4"], "2\n" + _rows(x1[:2], x2[:2])),
                       (["rmse", "1", "0.004"], "1 0 0 0 1 0 0 0 1 0 0 0 2.5\n65\n" + _rows(x1, x2)),
                       (["rmse", "0", "0.1"], "1 0 0 0 1 0 0 0 1 0 0 0 1\n0")):
        assert run_host(sim3_host_san, args, text) == run_host(sim3_host, args, text)
