"""K27 pose-graph optimisation without a GPU: the numpy oracle's own sanity (the analytic lines against central differences up
to 150 degrees, e = (w, tau) for a measurement perturbed by (w, tau), the PCG form against the dense solve on every refine
scene), the kernels' arithmetic (csrc/pgo_math.h) compiled for the host in tests/native/pgo_host.cpp -- by hipcc, as plain
C++, and once more under the host sanitizers -- against the float64 oracle, the host-side argument checks of the four entries
(MI_E_* before any launch), the Python module's constructor, its refusal of CPU tensors and the alias import, the generator's
contract, and the MEASUREMENTS behind every tolerance of tests/test_gpu_pgo.py, asserted against its constants so that
neither can drift from the other."""
import ctypes

import numpy as np
import pytest
import torch

import pgo_oracle as PO
import test_gpu_pgo as G
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import synth_pose_graph

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
MARGIN = 4.0
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return N.load()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _random_edge(rng, angle):
    """poses of two nodes and a measurement whose residual is (angle * axis, tau) exactly"""
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    Ri, Rj = PO.exp_so3(rng.standard_normal(3)), PO.exp_so3(rng.standard_normal(3))
    ti, tj, tau = rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3)
    Rp = Rj @ Ri.T
    Ew = PO.exp_so3(angle * ax)
    return Ri, ti, Rj, tj, Ew.T @ Rp, Ew.T @ (tj - Rp @ ti - tau), np.concatenate([angle * ax, tau])


def _residual(Ri, ti, Rj, tj, Rz, tz):
    return PO.residual(Ri[None], ti[None], Rj[None], tj[None], Rz[None], tz[None])


def test_oracle_residual_is_the_perturbation_of_the_measurement():
    rng = np.random.default_rng(3)
    for angle in np.radians([0.0, 1e-6, 0.3, 5.0, 60.0, 120.0, 150.0, 160.0, 179.0]):
        Ri, ti, Rj, tj, Rz, tz, want = _random_edge(rng, angle)
        e = _residual(Ri, ti, Rj, tj, Rz, tz)[0][0]
        assert np.abs(e - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (angle, e, want)


def test_oracle_lines_match_central_differences():
    """h = 1e-6: truncation about h^2, round-off about 1e-16 / h = 1e-10; the bound is 1e-7 of max |J|"""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    for angle in np.radians([0.0, 0.5, 10.0, 14.0, 15.0, 45.0, 90.0, 120.0, 140.0, 150.0]):
        Ri, ti, Rj, tj, Rz, tz, _ = _random_edge(rng, angle)
        e, Rp, u = _residual(Ri, ti, Rj, tj, Rz, tz)
        Ji, Jj = PO.lines(e, Rp, u)
        for side, J in ((0, Ji[0]), (1, Jj[0])):
            for k in range(6):
                d = np.zeros(6)
                d[k] = h

                def moved(s):
                    Ex = PO.exp_so3(s * d[:3])
                    if side == 0:
                        return _residual(Ex @ Ri, Ex @ ti + s * d[3:], Rj, tj, Rz, tz)[0][0]
                    return _residual(Ri, ti, Ex @ Rj, Ex @ tj + s * d[3:], Rz, tz)[0][0]
                fd = (moved(1.0) - moved(-1.0)) / (2 * h)
                worst = max(worst, np.abs(fd - J[:, k]).max() / np.abs(J).max())
    print(f"analytic lines vs central differences: {worst:.2e} of max |J|")
    assert worst <= 1e-7


def test_oracle_gradient_is_the_derivative_of_the_cost_under_huber():
    w = G.graphs("7x12")
    a = (w["R0"][0].astype(F64), w["t0"][0].astype(F64), *G.one(w, 0))
    lin = PO.linearise(*a, w["fixed"][0], 3.0)
    h = 1e-6
    for n in (1, 4):
        for k in range(6):
            d = np.zeros((7, 6))
            d[n, k] = h
            cp = PO.cost(*PO.update(a[0], a[1], d), *a[2:], 3.0)[1]
            cm = PO.cost(*PO.update(a[0], a[1], -d), *a[2:], 3.0)[1]
            fd = (cp - cm) / (2 * h)
            assert abs(fd - 2 * lin["g"][n, k]) <= 1e-6 * max(1.0, abs(fd)), (n, k, fd, 2 * lin["g"][n, k])


@pytest.mark.parametrize("name", G.REFINE_NAMES)
def test_the_pcg_form_reaches_the_dense_forms_cost_on_every_refine_scene(name):
    for i, (a, b) in enumerate(zip(G.oracle_refine(name), G.oracle_refine(name, False, True))):
        rel = abs(a["cost"] - b["cost"]) / b["cost"]
        print(f"{name}[{i}] form (a) {a['cost']:.4f}, form (b) {b['cost']:.4f}: {rel:.2e}")
        assert a["ok"] and b["ok"] and a["cost"] < a["cost0"] and rel <= 0.01


def test_oracle_refusals():
    w = G.graphs("7x12")
    a = (w["R0"][0], w["t0"][0], *G.one(w, 0))
    none = PO.refine(*a[:6], np.zeros(12, bool), w["fixed"][0], 3, 8)
    assert not none["ok"] and none["cost0"] == 0.0 and np.array_equal(none["R"], a[0])
    for fixed in (np.zeros(7, bool), np.ones(7, bool)):
        res = PO.refine(*a, fixed, 3, 8)
        assert not res["ok"] and np.isinf(res["cost0"]) and np.isinf(res["cost"]) and not res["chi2"].any()


def test_generator_contract():
    g = synth_pose_graph(5, 64, 4, 0.01, 0.02, false_loops=2)
    R0, t0, ei, zr, zt, info, fixed, protected, R, t, false_edge = g
    assert R0.dtype == F32 and ei.dtype == np.int32 and ei.shape == (69, 2) and info.shape == (69, 6, 6) and zr.dtype == F32
    assert fixed.tolist() == [True] + [False] * 63 and protected.sum() == 63 and false_edge.sum() == 2 and not (protected & false_edge).any()
    assert [tuple(e) for e in ei[63:67]] == [(0, 32), (8, 40), (16, 48), (24, 56)]
    assert np.array_equal(R0[0], R[0].astype(F32)) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.allclose(np.diag(info[0]), [1e4] * 3 + [2500.0] * 3) and not (info[0] - np.diag(np.diag(info[0]))).any()
    ones = np.ones(69, bool)
    chi2 = PO.cost(R, t, ei, zr, zt, info, ones)[0]
    assert chi2[:67].mean() < 12 and chi2[:67].max() < 40 and chi2[67:].min() > 1e3          # 6 degrees of freedom; the false loops are gross
    assert PO.cost(R0, t0, ei[:63], zr[:63], zt[:63], info[:63], ones[:63])[1] < 1e-3          # the start is the chained odometry
    drift = np.abs(t0 - t).max()
    assert 0.02 < drift < 2.0
    again = synth_pose_graph(5, 64, 4, 0.01, 0.02, false_loops=2)
    assert all(np.array_equal(x, y) for x, y in zip(g, again))
    with pytest.raises(ValueError):
        synth_pose_graph(1, 1, 0, 0.01, 0.02)
    with pytest.raises(ValueError):
        synth_pose_graph(1, 6, 4, 0.01, 0.02)


# ---- the kernels' arithmetic on the host --------------------------------------------------------------------------------------------
pgo_host = host_program("pgo_host.cpp", hip=True)
pgo_plain = host_program("pgo_host.cpp", hip=False)
EDGE_FIELDS = (("e", 6), ("chi2", 1), ("w", 1), ("rho", 1), ("Ji", 36), ("Jj", 36), ("Hii", 36), ("Hjj", 36), ("Hij", 36), ("gi", 6), ("gj", 6))


def _fmt(row, spec="%.9g"):
    return " ".join(spec % x for x in row)


def _edge_rows():
    """every active edge of four scenes at their starts, residual rotations from a few to 159 degrees"""
    rows = []
    for name in ("7x12", "hub", "parallel", "large-angle"):
        w = G.graphs(name)
        for b in range(3):
            for e, (i, j) in enumerate(w["ei"][b]):
                rows.append(np.concatenate([w["R0"][b, i].ravel(), w["t0"][b, i], w["R0"][b, j].ravel(), w["t0"][b, j], w["zr"][b, e].ravel(),
                                            w["zt"][b, e], w["info"][b, e].ravel()]))
    return np.array(rows, F32)


def _edge_text(rows, huber):
    return "%.9g\n" % huber + "\n".join(_fmt(r) for r in rows)


def _edge_oracle(rows, huber, dtype=F64):
    r = rows.astype(dtype)
    Ri, ti, Rj, tj, Rz, tz, O = (r[:, 0:9].reshape(-1, 3, 3), r[:, 9:12], r[:, 12:21].reshape(-1, 3, 3), r[:, 21:24],
                                 r[:, 24:33].reshape(-1, 3, 3), r[:, 33:36], PO.omega(r[:, 36:].reshape(-1, 6, 6)))
    e, Rp, u = PO.residual(Ri, ti, Rj, tj, Rz, tz)
    chi2 = np.einsum("ea,eab,eb->e", e, O, e)
    w, rho = PO._rho(chi2, huber)
    Ji, Jj = PO.lines(e, Rp, u)
    oe = np.einsum("eab,eb->ea", O, e)
    T = lambda J: np.swapaxes(J, 1, 2)
    wz = w[:, None, None]
    return dict(e=e, chi2=chi2, w=w, rho=rho, Ji=Ji, Jj=Jj, Hii=wz * (T(Ji) @ O @ Ji), Hjj=wz * (T(Jj) @ O @ Jj), Hij=wz * (T(Ji) @ O @ Jj),
                gi=w[:, None] * np.einsum("eba,eb->ea", Ji, oe), gj=w[:, None] * np.einsum("eba,eb->ea", Jj, oe))


def _split(out):
    res, at = {}, 0
    for k, n in EDGE_FIELDS:
        res[k] = out[:, at:at + n]
        at += n
    assert at == out.shape[1]
    return res


def test_native_edge_arithmetic_matches_the_float64_oracle(pgo_host, pgo_plain):
    """bounds: 4 x what the oracle's own float32 run deviates from its float64 run on the same rows, per quantity, relative to
    the quantity's largest magnitude in the row (printed); the plain C++ build returns the hipcc build's bits"""
    rows = _edge_rows()
    for huber in (0.0, 15.0):                              # the starts are 0.05 rad and 0.1 m off: chi runs from 5 to 300
        text = _edge_text(rows, huber)
        raw = run_host(pgo_host, "edge", text)
        assert raw == run_host(pgo_plain, "edge", text)
        got = _split(np.array([[float(v) for v in ln] for ln in raw], F64))
        want, single = _edge_oracle(rows, huber), _edge_oracle(rows, huber, F32)
        assert len(raw) == len(rows) and np.degrees(np.linalg.norm(want["e"][:, :3], axis=1)).max() > 150
        if huber > 0:
            assert (want["w"] < 1).sum() >= 10 and (want["w"] == 1).sum() >= 10                    # both branches
        for k, n in EDGE_FIELDS:
            ref = want[k].reshape(len(rows), -1)
            scale = np.abs(ref).max(1, keepdims=True)
            bound = MARGIN * (np.abs(single[k].reshape(len(rows), -1).astype(F64) - ref) / scale).max()
            dev = (np.abs(got[k] - ref) / scale).max()
            print(f"huber {huber} {k}: native {dev:.2e}, 4 x float32 oracle {bound:.2e}")
            assert dev <= bound, (k, dev, bound)
        assert np.array_equal(got["Hii"].reshape(-1, 6, 6), got["Hii"].reshape(-1, 6, 6).transpose(0, 2, 1))


def _precond_rows():
    lin = PO.linearise(*(G.graphs("hub")[k][0] for k in ("R0", "t0", "ei", "zr", "zt", "info", "valid", "fixed")), 3.0)
    rng = np.random.default_rng(5)
    rows = [np.concatenate([[lam], lin["diag"][n].ravel(), rng.standard_normal(6)]) for lam in (0.0, 1e-4, 10.0) for n in (1, 5, 40, 79)]
    sing = lin["diag"][5].copy()
    sing[3] = sing[2]
    sing[:, 3] = sing[:, 2]
    rows += [np.concatenate([[0.0], m.ravel(), np.ones(6)]) for m in (sing, -lin["diag"][5], np.zeros((6, 6)), np.eye(6))]
    return np.array(rows, F32)


def test_native_preconditioner_solve_matches_the_float64_oracle(pgo_host):
    rows = _precond_rows()
    out = np.array([[float(v) for v in ln] for ln in run_host(pgo_host, "precond", "\n".join(_fmt(r) for r in rows))], F64)
    assert out[:, 0].tolist() == [1.0] * 12 + [0.0, 0.0, 0.0, 1.0]
    for row, got in zip(rows, out):
        D, r = row[1:37].reshape(6, 6).astype(F64), row[37:].astype(F64)
        z = PO.block_solve(D, row[0], r)
        assert (z is not None) == bool(got[0])
        if z is None:
            assert not got[1:].any()
            continue
        z32 = PO.block_solve(D, row[0], r, F32)
        bound = MARGIN * np.abs(z32 - z).max() / np.abs(z).max()
        dev = np.abs(got[1:] - z).max() / np.abs(z).max()
        M = D + F64(F32(row[0])) * np.diag(np.diag(D))
        assert dev <= max(bound, 1e-6) and np.abs(M @ z - r).max() <= 1e-9 * np.abs(r).max() * np.linalg.cond(M)


def test_native_harness_under_the_host_sanitizers(tmp_path):
    """the same stand-alone program built with the host's address and undefined-behaviour sanitizers, run once over every mode"""
    exe = build_host(tmp_path, "pgo_host.cpp", hip=True, extra=SANITIZE)
    rows = _edge_rows()
    assert len(run_host(exe, "edge", _edge_text(rows, 3.0))) == len(rows)
    assert len(run_host(exe, "precond", "\n".join(_fmt(r) for r in _precond_rows()))) == 16


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    wb = lib.mi_pgo_workspace_bytes
    assert wb(1, 2, 1) > 0 and wb(3, 64, 70) == 3 * wb(1, 64, 70) and wb(1, 64, 70) % 16 == 0 and wb(65535, 1024, 4096) == 65535 * wb(1, 1024, 4096)
    assert wb(1, 1024, 4096) >= 4096 * 120 * 4 + 1024 * 24 * 8
    assert wb(0, 64, 70) == 0 and wb(3, 1, 70) == 0 and wb(3, 64, 0) == 0 and wb(3, 1025, 70) == 0 and wb(3, 64, 4097) == 0 and wb(65536, 64, 70) == 0
    assert wb(1, 64, 70) < wb(1, 65, 70) and wb(1, 64, 70) < wb(1, 64, 71)


def test_cost_argument_checks(lib, p):
    f = lib.mi_pgo_cost
    for i in (0, 1, 2, 3, 4, 5, 6, 11, 12, 13):
        a = [p, p, p, p, p, p, p, 3, 64, 70, 3.0, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    for batch, n, e, hub, want in ((0, 64, 70, 0.0, SHAPE), (3, 1, 70, 0.0, SHAPE), (3, 64, 0, 0.0, SHAPE), (3, -2, 70, 0.0, SHAPE),
                                   (65536, 64, 70, 0.0, PARAM), (3, 1025, 70, 0.0, PARAM), (3, 64, 4097, 0.0, PARAM),
                                   (3, 64, 70, -0.001, PARAM), (3, 64, 70, NAN, PARAM), (3, 64, 70, INF, PARAM), (3, 0, 4097, NAN, SHAPE)):
        assert f(p, p, p, p, p, p, p, batch, n, e, hub, p, p, p, None) == want, (batch, n, e, hub)


def test_linearise_argument_checks(lib, p):
    f, need = lib.mi_pgo_linearise, lib.mi_pgo_workspace_bytes(3, 64, 70)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16):
        a = [p, p, p, p, p, p, p, p, 3, 64, 70, 3.0, p, p, p, p, p, need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, n=64, e=70, hub=3.0, ws=p, wbytes=need):
        return f(p, p, p, p, p, p, p, p, batch, n, e, hub, p, p, p, p, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(n=1) == SHAPE and call(e=0) == SHAPE
    assert call(batch=65536) == PARAM and call(n=1025) == PARAM and call(e=4097) == PARAM
    assert call(hub=-1.0) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(hub=-1.0, wbytes=0) == PARAM                                # parameters are judged before the workspace


def test_refine_argument_checks(lib, p):
    f, need = lib.mi_pgo_refine, lib.mi_pgo_workspace_bytes(3, 64, 70)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 14, 15, 16, 17, 18, 19, 20, 21, 22):
        a = [p, p, p, p, p, p, p, p, 3, 64, 70, 10, 64, 3.0, p, p, p, p, p, p, p, p, p, need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, n=64, e=70, it=10, trips=64, hub=3.0, ws=p, wbytes=need):
        return f(p, p, p, p, p, p, p, p, batch, n, e, it, trips, hub, p, p, p, p, p, p, p, p, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(n=1) == SHAPE and call(n=0) == SHAPE and call(e=0) == SHAPE and call(e=-1) == SHAPE
    assert call(batch=65536) == PARAM and call(n=1025) == PARAM and call(e=4097) == PARAM
    assert call(it=0) == PARAM and call(it=33) == PARAM and call(it=-1) == PARAM
    assert call(trips=0) == PARAM and call(trips=257) == PARAM and call(trips=-1) == PARAM
    assert call(hub=-1e-9) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM and call(hub=-INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(wbytes=0) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(it=0, wbytes=0) == PARAM and call(e=0, it=0) == SHAPE       # shape, then parameters, then the workspace
    assert N.load().mi_abi_version() == 3


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import PoseGraphOptimizer
    assert (ops.PGO_MAX_NODES, ops.PGO_MAX_EDGES, ops.PGO_MAX_ITERATIONS, ops.PGO_MAX_PCG) == (1024, 4096, 32, 256)
    m = PoseGraphOptimizer()
    assert (m.iterations, m.pcg_iterations, m.huber, m.outlier_rounds, m.outlier_chi2) == (10, 64, 3.0, 1, 16.81)
    for kw in (dict(iterations=0), dict(iterations=33), dict(pcg_iterations=0), dict(pcg_iterations=257), dict(huber=-1.0),
               dict(huber=float("nan")), dict(outlier_rounds=-1), dict(outlier_chi2=0.0)):
        with pytest.raises(ValueError):
            PoseGraphOptimizer(**kw)
    w = G.graphs("7x12")
    a = [torch.from_numpy(w[k].copy()) for k in ("R0", "t0", "ei", "zr", "zt", "info", "fixed")]
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*(x[0] for x in a))
    with pytest.raises(RuntimeError, match=r"\(B, E, 2\) or \(E, 2\)"):
        m(a[0], a[1], a[2][..., :1], *a[3:])
    with pytest.raises(RuntimeError, match="edge_valid and protected"):
        m(*a, torch.ones(3, 5, dtype=torch.bool))
    valid = torch.ones(3, 12, dtype=torch.bool)
    for call in (lambda: ops.pgo_cost(*a[:6]), lambda: ops.pgo_linearise(*a), lambda: ops.pgo_refine(*a, valid)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match=r"poses must be \(B, N, 3, 3\)"):
        ops.pgo_refine(a[0][0], *a[1:])
    with pytest.raises(RuntimeError, match="expected t"):
        ops.pgo_refine(a[0], a[1], a[2], a[3][:, :5], *a[4:])
    with pytest.raises(RuntimeError, match="fixed must be"):
        ops.pgo_refine(*a[:6], a[6][:, :3])
    with pytest.raises(RuntimeError, match="supported: 2 .. 1024 and 1 .. 4096"):
        ops.pgo_cost(a[0][:, :1], a[1][:, :1], *a[2:6])
    with pytest.raises(RuntimeError, match="huber"):
        ops.pgo_cost(*a[:6], None, -1.0)
    with pytest.raises(RuntimeError, match="pcg_iterations"):
        ops.pgo_refine(*a, valid, 10, 257)


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import PoseGraphOptimizer
    assert PoseGraphOptimizer is real.PoseGraphOptimizer and "PoseGraphOptimizer" in real.__all__
    from pytorch_model.geometry.pose_graph import PoseGraphOptimizer as again
    assert again is PoseGraphOptimizer


# ---- the measurements behind the GPU tolerances ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    """the largest deviation of the oracle's float32 run from its float64 run, per quantity, over every scene"""
    m = dict(chi2=0.0, cost=0.0, lin=0.0, rot=0.0, t=0.0, rcost=0.0)
    for name in G.NAMES:
        w = G.graphs(name)
        for i in range(3):
            a = (w["R0"][i], w["t0"][i], *G.one(w, i))
            c64, k64, _ = PO.cost(*a, w["huber"])
            c32, k32, _ = PO.cost(*a, w["huber"], F32)
            m["chi2"] = max(m["chi2"], (np.abs(c32 - c64) / np.maximum(c64, G.CHI2_FLOOR)).max())
            m["cost"] = max(m["cost"], abs(k32 - k64) / k64)
            l64, l32 = PO.linearise(*a, w["fixed"][i], w["huber"]), PO.linearise(*a, w["fixed"][i], w["huber"], F32)
            m["lin"] = max(m["lin"], max(np.abs(l32[k] - l64[k]).max() for k in ("diag", "off", "g")) / np.abs(l64["diag"]).max())
    for name in G.REFINE_NAMES:
        for r32, r64 in zip(G.oracle_refine(name, True), G.oracle_refine(name)):
            rot, dt, dc = G.refine_deviation(r32, r64)
            m["rot"], m["t"], m["rcost"] = max(m["rot"], rot), max(m["t"], dt), max(m["rcost"], dc)
    g = G.clean_ring()
    res = PO.refine(g["R0"], g["t0"], g["ei"], g["zr"], g["zt"], g["info"], g["valid"], g["fixed"], G.CLEAN_ITERATIONS, G.CLEAN_TRIPS, 0.0, F32)
    m["clean_rot"], m["clean_t"] = G.recovery_error(res["R"], res["t"], g)
    print("float32 oracle vs float64 oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    return m


def test_gpu_tolerances_are_four_times_their_measurements(measured):
    m = measured
    for const, value in ((G.CHI2_RTOL, m["chi2"]), (G.COST_RTOL, m["cost"]), (G.LIN_TOL, m["lin"]), (G.REFINE_ROT_DEG, m["rot"]),
                         (G.REFINE_T_M, m["t"]), (G.REFINE_COST_RTOL, m["rcost"]), (G.RECOVER_ROT_DEG, m["clean_rot"]),
                         (G.RECOVER_T_M, m["clean_t"])):
        assert value > 0 and MARGIN * value <= const <= 16 * MARGIN * value, (const, value)
