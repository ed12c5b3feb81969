"""K25 windowed bundle adjustment without a GPU: the host-side argument checks of the four entries (MI_E_* before any
launch), the workspace size, the Python module's constructor and its refusal of CPU tensors, the exports through the
`pytorch_model` alias, the numpy oracle's own sanity (gradients against finite differences, the Schur step against the
dense normal equations, convergence below the cost of the planted truth), the kernels' arithmetic (csrc/ba_math.h)
compiled for the host in tests/native/ba_host.cpp -- once more under the host sanitizers --, the condition every parity
window of tests/test_gpu_ba.py must meet (the oracle has converged) and the MEASUREMENTS behind every tolerance of that file,
asserted against its constants so that neither can drift from the other."""
import ctypes

import numpy as np
import pytest
import torch

import ba_oracle as BO
import test_gpu_ba as G
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import rgbd_camera, synth_ba_window

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
K = rgbd_camera()
F32, F64 = np.float32, np.float64
MARGIN = 4.0


@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


p_keepalive = []
NAN, INF = float("nan"), float("inf")


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_cost_argument_checks(lib, p):
    f = lib.mi_ba_cost
    for i in (0, 1, 2, 3, 4, 9, 10, 11):
        a = [p, p, p, p, p, 3, 6, 48, 0.004, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    for batch, fr, lm, hub, want in ((0, 6, 48, 0.0, SHAPE), (3, 1, 48, 0.0, SHAPE), (3, 6, 0, 0.0, SHAPE), (3, -2, 48, 0.0, SHAPE),
                                     (65536, 6, 48, 0.0, PARAM), (3, 17, 48, 0.0, PARAM), (3, 6, 2049, 0.0, PARAM),
                                     (3, 6, 48, -0.001, PARAM), (3, 6, 48, NAN, PARAM), (3, 6, 48, INF, PARAM)):
        assert f(p, p, p, p, p, batch, fr, lm, hub, p, p, p, None) == want, (batch, fr, lm, hub)


def test_workspace_size(lib):
    wb = lib.mi_ba_workspace_bytes
    assert wb(3, 6, 48) == 3 * 13 * 48 * 4 and wb(3, 6, 65) == 3 * 13 * 68 * 4 and wb(1, 2, 1) == 13 * 4 * 4
    assert wb(3, 6, 48) % 16 == 0 and wb(3, 16, 2048) % 16 == 0 and wb(65535, 16, 2048) == 65535 * 13 * 2048 * 4
    assert wb(0, 6, 48) == 0 and wb(3, 1, 48) == 0 and wb(3, 17, 48) == 0 and wb(3, 6, 0) == 0 and wb(3, 6, 2049) == 0
    assert wb(65536, 6, 48) == 0
    assert wb(3, 6, 48) == wb(3, 16, 48)                                   # the frames do not enter; batch and landmarks do


def test_linearise_argument_checks(lib, p):
    f, need = lib.mi_ba_linearise, lib.mi_ba_workspace_bytes(3, 6, 48)
    for i in (0, 1, 2, 3, 4, 10, 11, 12, 13):
        a = [p, p, p, p, p, 3, 6, 48, 2, 0.004, p, p, p, p, need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, fr=6, lm=48, nf=2, hub=0.004, ws=p, wbytes=need):
        return f(p, p, p, p, p, batch, fr, lm, nf, hub, p, p, p, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(fr=1) == SHAPE and call(lm=0) == SHAPE
    assert call(batch=65536) == PARAM and call(fr=17) == PARAM and call(lm=2049) == PARAM
    assert call(nf=0) == PARAM and call(nf=7) == PARAM and call(nf=-2) == PARAM
    assert call(hub=-1.0) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(nf=0, wbytes=0) == PARAM                                    # parameters are judged before the workspace


def test_refine_argument_checks(lib, p):
    f, need = lib.mi_ba_refine, lib.mi_ba_workspace_bytes(3, 6, 48)
    for i in (0, 1, 2, 3, 4, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20):
        a = [p, p, p, p, p, 3, 6, 48, 2, 10, 0.004, p, p, p, p, p, p, p, p, p, p, need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, fr=6, lm=48, nf=2, it=10, hub=0.004, ws=p, wbytes=need):
        return f(p, p, p, p, p, batch, fr, lm, nf, it, hub, p, p, p, p, p, p, p, p, p, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(fr=1) == SHAPE and call(fr=0) == SHAPE and call(lm=0) == SHAPE and call(lm=-1) == SHAPE
    assert call(batch=65536) == PARAM and call(fr=17) == PARAM and call(lm=2049) == PARAM
    assert call(nf=0) == PARAM and call(nf=-1) == PARAM and call(nf=7) == PARAM
    assert call(it=0) == PARAM and call(it=33) == PARAM and call(it=-1) == PARAM
    assert call(hub=-1e-9) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM and call(hub=-INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(wbytes=0) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(it=0, wbytes=0) == PARAM and call(lm=0, it=0) == SHAPE      # shape, then parameters, then the workspace
    assert lib.mi_abi_version() == 3


def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import BundleAdjuster
    assert (ops.BA_MAX_FRAMES, ops.BA_MAX_LANDMARKS, ops.BA_MAX_ITERATIONS) == (16, 2048, 32)
    Kt = torch.from_numpy(K)
    m = BundleAdjuster(Kt)
    assert (m.iterations, m.huber_px, m.num_fixed, m.outlier_rounds, m.outlier_px, m.focal) == (10, 2.0, 1, 1, 3.0, 500.0)
    assert torch.allclose(m.K_inv @ m.K, torch.eye(3), atol=1e-6) and m.K.dtype == torch.float32
    for kw in (dict(iterations=0), dict(iterations=33), dict(huber_px=-1.0), dict(huber_px=float("nan")), dict(num_fixed=0),
               dict(num_fixed=17), dict(outlier_rounds=-1), dict(outlier_px=0.0)):
        with pytest.raises(ValueError):
            BundleAdjuster(Kt, **kw)
    with pytest.raises(ValueError, match="3x3"):
        BundleAdjuster(torch.eye(4))
    r, t, x, kp, v = torch.eye(3).repeat(2, 4, 1, 1), torch.zeros(2, 4, 3), torch.ones(2, 9, 3), torch.zeros(2, 4, 9, 2), torch.ones(2, 4, 9, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(r, t, x, kp, v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(r[0], t[0], x[0], kp[0], v[0])
    with pytest.raises(RuntimeError, match=r"\(B, F, L, 2\) or \(F, L, 2\)"):
        m(r, t, x, torch.zeros(2, 4, 9, 3), v)
    for call in (lambda: ops.ba_cost(r, t, x, kp, v), lambda: ops.ba_linearise(r, t, x, kp, v), lambda: ops.ba_refine(r, t, x, kp, v)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match=r"poses must be \(B, F, 3, 3\)"):
        ops.ba_refine(r[0], t, x, kp, v)
    with pytest.raises(RuntimeError, match="expected t"):
        ops.ba_refine(r, t, x, kp[:, :3], v)
    with pytest.raises(RuntimeError, match="supported: 2 .. 16 and 1 .. 2048"):
        ops.ba_cost(torch.eye(3).repeat(1, 17, 1, 1), torch.zeros(1, 17, 3), x[:1], torch.zeros(1, 17, 9, 2), torch.ones(1, 17, 9))
    with pytest.raises(RuntimeError, match="huber"):
        ops.ba_cost(r, t, x, kp, v, -1.0)


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import BundleAdjuster
    assert BundleAdjuster is real.BundleAdjuster and "BundleAdjuster" in real.__all__
    from pytorch_model.geometry.bundle_adjustment import BundleAdjuster as again
    assert again is BundleAdjuster


# ---- the generator and the oracle -------------------------------------------------------------------------------------------------
def _window(seed, F, L, nf, vis=1.0, out=0.0, **kw):
    R0, t0, X0, kp, v, R, t, X, o = synth_ba_window(seed, F, L, vis, 0.5, out, num_fixed=nf, **kw)
    return dict(R0=R0, t0=t0, X0=X0, obs=BO.normalise(kp, K), vis=v, R=R, t=t, X=X, outlier=o, kp=kp)


def test_generator_contract():
    w = _window(3, 6, 48, 2, 0.7, 0.05)
    assert w["R0"].dtype == F32 and w["kp"].dtype == F32 and w["kp"].shape == (6, 48, 2) and w["vis"].dtype == bool
    assert np.array_equal(w["R0"][:2], w["R"][:2].astype(F32)) and np.array_equal(w["t0"][:2], w["t"][:2].astype(F32))      # the gauge is true
    assert not np.array_equal(w["R0"][2:], w["R"][2:].astype(F32)) and np.abs(w["X0"] - w["X"]).max() > 0.01
    assert 0.5 < w["vis"].mean() < 0.85 and not (w["outlier"] & ~w["vis"]).any() and w["outlier"].sum() == round(0.05 * w["vis"].sum())
    xc = np.einsum("fij,lj->fli", w["R"], w["X"]) + w["t"][:, None]
    px = np.stack([500.0 * xc[..., 1] / xc[..., 2] + 240.0, 500.0 * xc[..., 0] / xc[..., 2] + 320.0], -1)
    inl = w["vis"] & ~w["outlier"]
    assert np.abs(w["kp"] - px)[inl].max() < 3.0 and np.abs(w["kp"] - px)[w["outlier"]].max() > 20.0
    again = synth_ba_window(3, 6, 48, 0.7, 0.5, 0.05, num_fixed=2)
    assert all(np.array_equal(a, b) for a, b in zip(again[:5], (w["R0"], w["t0"], w["X0"], w["kp"], w["vis"])))
    with pytest.raises(ValueError):
        synth_ba_window(3, 6, 48, num_fixed=7)


def test_oracle_gradients_match_finite_differences():
    """d cost = 2 g . d(omega, tau) and 2 h . dX, also under the Huber term (d rho = 2 w r . dr)"""
    for hub in (0.0, 0.002):
        w = _window(11, 4, 20, 1, 0.8, 0.1)
        R, t, X = w["R0"].astype(F64), w["t0"].astype(F64), w["X0"].astype(F64)
        lin = BO.linearise(R, t, X, w["obs"], w["vis"], 1, hub)
        c = lambda Ra, ta, Xa: BO.cost(Ra, ta, Xa, w["obs"], w["vis"], hub)[1]
        eps = 1e-6
        for f in (1, 3):
            for k in range(6):
                d = np.zeros(6)
                d[k] = eps
                Rp, tp, Rm, tm = R.copy(), t.copy(), R.copy(), t.copy()
                Rp[f], tp[f] = BO.exp_so3(d[:3]) @ R[f], BO.exp_so3(d[:3]) @ t[f] + d[3:]
                Rm[f], tm[f] = BO.exp_so3(-d[:3]) @ R[f], BO.exp_so3(-d[:3]) @ t[f] - d[3:]
                fd = (c(Rp, tp, X) - c(Rm, tm, X)) / (2 * eps)
                assert abs(fd - 2 * lin["g"][f][k]) <= 1e-6 * max(1.0, abs(fd)), (hub, f, k, fd, 2 * lin["g"][f][k])
        for l in (0, 7, 19):
            for k in range(3):
                Xp, Xm = X.copy(), X.copy()
                Xp[l, k] += eps
                Xm[l, k] -= eps
                fd = (c(R, t, Xp) - c(R, t, Xm)) / (2 * eps)
                want = 2 * lin["h"][l][k] if lin["active"][l] else 0.0
                assert abs(fd - want) <= 1e-6 * max(1.0, abs(fd)), (hub, l, k, fd, want)


def test_oracle_schur_step_is_the_dense_normal_equations_step():
    for F, L, nf, vis, lam in ((3, 20, 1, 1.0, 1e-4), (5, 30, 2, 0.7, 1e-2), (4, 16, 1, 0.6, 1.0)):
        w = _window(5, F, L, nf, vis)
        R, t, X = w["R0"].astype(F64), w["t0"].astype(F64), w["X0"].astype(F64)
        lin = BO.linearise(R, t, X, w["obs"], w["vis"], nf, 0.0, lam)
        assert not lin["frozen"].any()
        ok, _, _, _, dp, dX = BO.step(lin, R, t, X, nf)
        act = np.flatnonzero(lin["active"])
        n, A = 6 * (F - nf), len(act)
        H, rhs = np.zeros((n + 3 * A, n + 3 * A)), np.zeros(n + 3 * A)
        for f in range(nf, F):
            p0 = 6 * (f - nf)
            H[p0:p0 + 6, p0:p0 + 6] = lin["U"][f]
            rhs[p0:p0 + 6] = lin["g"][f]
            for a, l in enumerate(act):
                H[p0:p0 + 6, n + 3 * a:n + 3 * a + 3] = lin["W"][f][l]
                H[n + 3 * a:n + 3 * a + 3, p0:p0 + 6] = lin["W"][f][l].T
        for a, l in enumerate(act):
            H[n + 3 * a:n + 3 * a + 3, n + 3 * a:n + 3 * a + 3] = lin["V"][l]
            rhs[n + 3 * a:n + 3 * a + 3] = lin["h"][l]
        H = H + lam * np.diag(np.diag(H))
        full = np.linalg.solve(H, -rhs)
        assert ok and np.abs(full[:n] - dp).max() <= 1e-9 * max(1.0, np.abs(dp).max())
        assert np.abs(full[n:].reshape(A, 3) - dX[act]).max() <= 1e-9 * max(1.0, np.abs(dX).max())
        assert not dX[~lin["active"]].any()


def test_oracle_converges_below_the_truth_and_towards_it():
    """num_fixed = 2 (the scale is pinned): the final cost is below the cost at the planted truth, and the pose and point
    errors shrink; num_fixed = 1: the cost only (the scale is free, so the state matches the truth up to a similarity).
    The points start 0.2 m off per axis: at 0.5 px of noise and these baselines the optimum itself is 0.08 to 0.22 m (rms)
    from the truth, so the generator's default start of 0.05 m has nothing to shrink."""
    for seed, F, L, vis in ((1, 6, 48, 0.7), (2, 8, 130, 1.0), (3, 3, 65, 1.0)):
        w = _window(seed, F, L, 2, vis, point_noise=0.2)
        res = BO.refine(w["R0"], w["t0"], w["X0"], w["obs"], w["vis"], 2, 10, 0.0)
        truth = BO.cost(w["R"].astype(F32), w["t"].astype(F32), w["X"], w["obs"], w["vis"], 0.0)[1]
        assert res["ok"] and res["cost"] < truth < res["cost0"]
        act = BO.active(w["vis"])
        rot0 = max(BO.rotation_angle_deg(w["R0"][f], w["R"][f]) for f in range(F))
        rot1 = max(BO.rotation_angle_deg(res["R"][f], w["R"][f]) for f in range(F))
        assert rot1 < rot0 and np.abs(res["t"] - w["t"]).max() < np.abs(w["t0"] - w["t"]).max()
        assert np.sqrt(((res["X"] - w["X"])[act] ** 2).mean()) < np.sqrt(((w["X0"] - w["X"])[act] ** 2).mean())
        assert res["costs"][4] <= 1.01 * res["cost"]                       # within 1 % of the final cost after 4 iterations
    for seed, F, L in ((1, 2, 12), (2, 16, 64)):
        w = _window(seed, F, L, 1)
        res = BO.refine(w["R0"], w["t0"], w["X0"], w["obs"], w["vis"], 1, 10, 0.0)
        truth = BO.cost(w["R"].astype(F32), w["t"].astype(F32), w["X"], w["obs"], w["vis"], 0.0)[1]
        assert res["ok"] and res["cost"] < truth < res["cost0"]


def test_oracle_refusals_and_inactive_landmarks():
    w = _window(4, 3, 20, 1)
    X = w["X0"].copy()
    X[5] = (0.0, 0.0, -3.0)
    res = BO.refine(w["R0"], w["t0"], X, w["obs"], w["vis"], 1, 5, 0.0)
    assert not res["ok"] and np.isinf(res["cost0"]) and np.array_equal(res["X"], X) and not res["point_ok"].any()
    v = np.zeros_like(w["vis"])
    v[1] = True
    res = BO.refine(w["R0"], w["t0"], w["X0"], w["obs"], v, 1, 5, 0.0)
    assert not res["ok"] and res["cost0"] == 0.0 and res["cost"] == 0.0
    v = w["vis"].copy()
    v[1:, 5] = False                                       # landmark 5, behind the cameras, is seen once: it takes no part
    res = BO.refine(w["R0"], w["t0"], X, w["obs"], v, 1, 5, 0.0)
    assert res["ok"] and not res["point_ok"][5] and np.array_equal(res["X"][5], X[5]) and res["cost"] < res["cost0"]


def test_module_scheme_on_the_oracle_clears_exactly_the_planted_outliers():
    """BundleAdjuster's two passes restated on the CPU for the windows of tests/test_gpu_ba.py's end-to-end test: what that
    test asserts of the GPU (no planted outlier kept, no inlier lost, final cost below the truth's) holds for the oracle"""
    w = G.windows("8x130")
    for i in range(3):
        first = BO.refine(w["R0"][i], w["t0"][i], w["X0"][i], w["obs"][i], w["vis"][i], 1, G.ITERATIONS, 2.0 / G.FOCAL)
        e2, _, _ = BO.cost(first["R"], first["t"], first["X"], w["obs"][i], w["vis"][i], 0.0)
        vis2 = w["vis"][i] & ~(e2 > (3.0 / G.FOCAL) ** 2)
        assert np.array_equal(vis2, w["vis"][i] & ~w["outlier"][i])
        margin = np.abs(np.sqrt(e2[w["vis"][i]]) * G.FOCAL - 3.0).min()
        assert margin > 0.05, margin                       # no observation sits at the gate, where float32 could decide otherwise
        second = BO.refine(first["R"], first["t"], first["X"], w["obs"][i], vis2, 1, G.ITERATIONS, 0.0)
        truth = BO.cost(w["R"][i].astype(F32), w["t"][i].astype(F32), w["X"][i], w["obs"][i], vis2, 0.0)[1]
        assert second["ok"] and second["cost"] < truth


# ---- the kernels' arithmetic on the host ---------------------------------------------------------------------------------------
# tests/native/ba_host.cpp: the kernels' own lines, 3x3 inverse and LDL^T, compiled for the host
ba_host = host_program("ba_host.cpp", hip=True)


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _fmt(row, spec="%.9g"):
    return " ".join(spec % x for x in row)


def _lines_input():
    """frame 2 of a window with outliers (so that both branches of the Huber term are taken), one point behind the camera and
    one exactly in its plane"""
    w = _window(9, 4, 64, 1, 1.0, 0.3)
    X = w["X0"].copy()
    X[3] = (0.3, -0.2, -4.0)
    rt = np.concatenate([w["R0"][2].ravel(), w["t0"][2]])
    X[4] = w["R0"][2].T.astype(F64) @ (np.array([0.5, 0.5, 0.0]) - w["t0"][2])          # z within rounding of 0
    return w, X.astype(F32), rt.astype(F32), w["obs"][2]


def _lines_text(hub, rt, X, uv):
    return "%.9g\n%s\n" % (hub, _fmt(rt)) + "\n".join(_fmt(np.concatenate([x, o])) for x, o in zip(X, uv))


def test_native_lines_return_the_restatements_bits(ba_host):
    w, X, rt, uv = _lines_input()
    for hub in (0.0, F32(0.02)):
        out = np.array([[float(v) for v in ln] for ln in run_host(ba_host, "lines", _lines_text(hub, rt, X, uv))], F64)
        ln = BO.frame_lines(rt[:9].reshape(3, 3), rt[9:], X, uv, hub, F32)
        assert not ln["ok"][3] and ln["ok"].sum() >= 62 and np.array_equal(out[:, 0] != 0, ln["ok"])
        want = np.concatenate([ln["ju"], ln["jv"], ln["xu"], ln["xv"], ln["ru"][:, None], ln["rv"][:, None], ln["e2"][:, None],
                               ln["w"][:, None], ln["rho"][:, None], ln["rho"][:, None], ln["e2"][:, None]], axis=1)
        assert np.array_equal(_bits(out[:, 1:]), _bits(want))
        if hub > 0:
            assert (ln["w"][ln["ok"]] < 1).sum() >= 10 and (ln["w"][ln["ok"]] == 1).sum() >= 10      # both branches
        # ... and the float64 oracle is what they approximate
        l64 = BO.frame_lines(rt[:9].reshape(3, 3), rt[9:], X, uv, hub, F64)
        k = ln["ok"] & l64["ok"]
        assert np.abs(ln["ju"][k] - l64["ju"][k]).max() < 1e-5 and np.abs(ln["xv"][k] - l64["xv"][k]).max() < 1e-5


def _inv3_input():
    w = _window(9, 4, 64, 1)
    rows = []
    for lam in (0.0, 1e-4, 10.0):
        lin = BO.linearise(w["R0"], w["t0"], w["X0"], w["obs"], w["vis"], 1, 0.0, 0.0, F32)
        V = lin["V"]
        rows += [(lam, V[l, 0, 0], V[l, 0, 1], V[l, 0, 2], V[l, 1, 1], V[l, 1, 2], V[l, 2, 2]) for l in range(64)]
    rows += [(0.0, 0, 0, 0, 0, 0, 0), (0.0, 1, 0, 0, 1, 0, 0), (0.0, 1, 1, 1, 1, 1, 1), (1e-4, 4, 2, 0, 1, 0, 3), (0.0, 1, 0, 0, 1, 0, 1e-7),
             (0.0, NAN, 0, 0, 1, 0, 1), (0.0, -1, 0, 0, -1, 0, -1), (0.0, 1e30, 0, 0, 1e30, 0, 1e30)]
    return np.array(rows, F32)


def test_native_inverse_returns_the_restatements_bits(ba_host):
    rows = _inv3_input()
    out = np.array([[float(v) for v in ln] for ln in run_host(ba_host, "inv3", "\n".join(_fmt(r) for r in rows))], F64)
    ok = np.zeros(len(rows), bool)
    vi = np.zeros((len(rows), 6), F32)
    for lam in np.unique(rows[:, 0]):
        k = rows[:, 0] == lam
        vi[k], ok[k] = BO.inv3(rows[k, 1:], lam, F32)
    assert np.array_equal(out[:, 0] != 0, ok) and np.array_equal(_bits(out[:, 1:]), _bits(vi))
    assert ok[:192].all() and ok[-8:].tolist() == [False, False, False, True, False, False, False, False]
    m = rows[5, 1:].astype(F64)
    full = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
    got = np.array([[vi[5, 0], vi[5, 1], vi[5, 2]], [vi[5, 1], vi[5, 3], vi[5, 4]], [vi[5, 2], vi[5, 4], vi[5, 5]]], F64)
    assert np.abs(got @ full - np.eye(3)).max() < 1e-3


def _ldlt_input():
    rng = np.random.default_rng(7)
    systems = []
    for n in (0, 1, 6, 42, 90):
        a = rng.standard_normal((n, n + 3))
        systems.append((a @ a.T, rng.standard_normal(n)))
    w = _window(2, 6, 48, 1, 0.7)
    lin = BO.linearise(w["R0"], w["t0"], w["X0"], w["obs"], w["vis"], 1, 0.0, 1e-4)
    systems.append((lin["S"], lin["b"]))
    sing = systems[2][0].copy()
    sing[3] = sing[2]
    sing[:, 3] = sing[:, 2]
    systems.append((sing, systems[2][1]))                                   # rank-deficient: refused
    systems.append((-systems[2][0], systems[2][1]))                         # negative definite: refused
    return systems


def _ldlt_text(systems):
    return "\n".join("%d\n%s\n%s" % (len(b), _fmt(S[np.triu_indices(len(b))], "%.17g"), _fmt(b, "%.17g")) for S, b in systems)


def test_native_ldlt_returns_the_restatements_bits(ba_host):
    systems = _ldlt_input()
    out = run_host(ba_host, "ldlt", _ldlt_text(systems))
    assert len(out) == len(systems)
    for (S, b), ln in zip(systems, out):
        x, ok = BO.ldlt_solve(S, b)
        assert bool(int(ln[0])) == ok
        got = np.array([float(v) for v in ln[1:]], F64)
        assert np.array_equal(got.view(np.uint64), (x if ok else np.zeros(len(b))).view(np.uint64))
        if ok and len(b):
            assert np.abs(S @ x + b).max() <= 1e-9 * max(1.0, np.abs(b).max()) * np.linalg.cond(S)
    assert [bool(int(ln[0])) for ln in out] == [True] * 6 + [False, False]


def test_native_harness_under_the_host_sanitizers(tmp_path):
    """the same stand-alone program built with the host's address and undefined-behaviour sanitizers, run once over every mode"""
    exe = build_host(tmp_path, "ba_host.cpp", hip=True, extra=SANITIZE)
    w, X, rt, uv = _lines_input()
    assert len(run_host(exe, "lines", _lines_text(F32(0.02), rt, X, uv))) == 64
    assert len(run_host(exe, "inv3", "\n".join(_fmt(r) for r in _inv3_input()))) == 200
    assert len(run_host(exe, "ldlt", _ldlt_text(_ldlt_input()))) == 8


# ---- the condition on the parity windows, and the measurements behind the GPU tolerances ---------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_the_oracle_has_converged_on_every_parity_window(name):
    a, b = G.oracle_refine(name), G.oracle_refine(name, 2 * G.ITERATIONS)
    for i in range(3):
        rel, dx = abs(a[i]["cost"] - b[i]["cost"]) / b[i]["cost"], np.abs(a[i]["X64"] - b[i]["X64"]).max()
        print(f"{name}[{i}] cost after {G.ITERATIONS} vs {2 * G.ITERATIONS} iterations: {rel:.2e} relative, points {dx:.2e} m")
        assert a[i]["ok"] and rel <= 1e-6 and dx <= 1e-4


@pytest.fixture(scope="module")
def measured():
    """the largest deviation of the float32 restatement from the float64 oracle, per quantity, over every parity window"""
    m = dict(e2=0.0, cost=0.0, lin=0.0, rot=0.0, t=0.0, x=0.0, rcost=0.0)
    for name in G.NAMES:
        w = G.windows(name)
        F = w["R0"].shape[1]
        r64, r32 = G.oracle_refine(name), G.oracle_refine(name, G.ITERATIONS, True)
        for i in range(3):
            a = (w["R0"][i], w["t0"][i], w["X0"][i], w["obs"][i], w["vis"][i])
            e64, c64, _ = BO.cost(*a, w["huber"])
            e32, c32, _ = BO.cost(*a, w["huber"], F32)
            m["e2"] = max(m["e2"], (np.abs(e32 - e64) / np.maximum(e64, G.E2_FLOOR)).max())
            m["cost"] = max(m["cost"], abs(c32 - c64) / c64)
            if w["nf"] < F:
                l64, l32 = BO.linearise(*a, w["nf"], w["huber"]), BO.linearise(*a, w["nf"], w["huber"], 0.0, F32)
                scale = np.abs(np.diag(l64["S"])).max()
                m["lin"] = max(m["lin"], np.abs(l32["S"] - l64["S"]).max() / scale, np.abs(l32["b"] - l64["b"]).max() / scale)
            rot, dt, dx, dc = G.refine_deviation(w, i, r32[i], r64[i])
            m["rot"], m["t"], m["x"], m["rcost"] = max(m["rot"], rot), max(m["t"], dt), max(m["x"], dx), max(m["rcost"], dc)
    print("float32 restatement vs float64 oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    return m


def test_gpu_tolerances_are_four_times_their_measurements(measured):
    m = measured
    for const, value in ((G.E2_RTOL, m["e2"]), (G.COST_RTOL, m["cost"]), (G.LIN_TOL, m["lin"]), (G.REFINE_ROT_DEG, m["rot"]),
                         (G.REFINE_T_M, m["t"]), (G.REFINE_X_M, m["x"]), (G.REFINE_COST_RTOL, m["rcost"])):
        assert value > 0 and MARGIN * value <= const <= 16 * MARGIN * value, (const, value)
