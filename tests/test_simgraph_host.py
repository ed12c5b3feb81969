"""K31 Sim(3) pose-graph optimisation without a GPU: the numpy oracle's own sanity (e = (w, tau, sigma) for a measurement
perturbed by (w, tau, sigma) up to 179 degrees and scales 0.2 .. 5, the analytic 7x7 lines against central differences on
both sides at scales != 1, the gradient under Huber against the cost's derivative, the PCG form against the dense solve on
every refine scene, agreement with tests/pgo_oracle.py on a scale-consistent graph at scale 1), the kernels' arithmetic
(csrc/simgraph_math.h) compiled for the host in tests/native/simgraph_host.cpp -- by hipcc, as plain C++, and once more under
the host sanitizers -- against the float64 oracle, the host-side argument checks of the five entries (MI_E_* before any
launch), the section's place in the binding, the Python module's constructor and its refusal of CPU tensors, the generator's
contract, and the MEASUREMENTS behind every tolerance of tests/test_gpu_simgraph.py, asserted against its constants so that
neither can drift from the other."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import pgo_oracle as PO
import simgraph_oracle as SO
import test_gpu_pgo as G6
import test_gpu_simgraph as G
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.build import SIMGRAPH_LIB
from onnx_image_processing_amd.synth import synth_pose_graph, synth_sim3_graph

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
MARGIN = 4.0
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return N.load_simgraph()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _random_edge(rng, angle, sigma):
    """states of two nodes (scales 0.2 .. 5) and a measurement whose residual is (angle * axis, tau, sigma) exactly"""
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    Ri, Rj = SO.exp_so3(rng.standard_normal(3)), SO.exp_so3(rng.standard_normal(3))
    ti, tj, tau = rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3)
    si, sj = np.exp(rng.uniform(np.log(0.2), np.log(5.0), 2))
    sp, Rp = sj / si, Rj @ Ri.T
    Ew, k = SO.exp_so3(angle * ax), np.exp(-sigma)
    z = (k * sp, Ew.T @ Rp, k * (Ew.T @ (tj - sp * (Rp @ ti) - tau)))
    return (si, Ri, ti), (sj, Rj, tj), z, np.concatenate([angle * ax, tau, [sigma]])


def _residual(ni, nj, z):
    a = lambda v: np.asarray(v, F64)[None]
    return SO.residual(a(ni[0]), a(ni[1]), a(ni[2]), a(nj[0]), a(nj[1]), a(nj[2]), a(z[0]), a(z[1]), a(z[2]))


def test_oracle_residual_is_the_perturbation_of_the_measurement():
    rng = np.random.default_rng(3)
    for angle in np.radians([0.0, 1e-6, 0.3, 5.0, 60.0, 120.0, 150.0, 160.0, 179.0]):
        for sigma in np.log([0.2, 0.9, 1.0, 5.0]):
            ni, nj, z, want = _random_edge(rng, angle, sigma)
            e = _residual(ni, nj, z)[0][0]
            assert np.abs(e - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (angle, sigma, e, want)


def _moved(node, d, sgn):
    s, R, t = SO.update(np.array([node[0]]), node[1][None], node[2][None], sgn * d[None])
    return s[0], R[0], t[0]


def test_oracle_lines_match_central_differences():
    """h = 1e-6: truncation about h^2, round-off about 1e-16 / h = 1e-10; the bound is 1e-7 of max |J|.  Both sides, all 7
    coordinates, node scales 0.2 .. 5, residual scales 0.5 and 2"""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    for angle in np.radians([0.0, 0.5, 10.0, 14.0, 15.0, 45.0, 90.0, 120.0, 140.0, 150.0]):
        for sigma in np.log([0.5, 2.0]):
            ni, nj, z, _ = _random_edge(rng, angle, sigma)
            assert abs(ni[0] - 1) > 1e-3 and abs(nj[0] - 1) > 1e-3
            e, Rp, u, sp = _residual(ni, nj, z)
            Ji, Jj = SO.lines(e, Rp, u, sp)
            for side, J in ((0, Ji[0]), (1, Jj[0])):
                for k in range(7):
                    d = np.zeros(7)
                    d[k] = h
                    if side == 0:
                        fd = (_residual(_moved(ni, d, 1.0), nj, z)[0][0] - _residual(_moved(ni, d, -1.0), nj, z)[0][0]) / (2 * h)
                    else:
                        fd = (_residual(ni, _moved(nj, d, 1.0), z)[0][0] - _residual(ni, _moved(nj, d, -1.0), z)[0][0]) / (2 * h)
                    worst = max(worst, np.abs(fd - J[:, k]).max() / np.abs(J).max())
    print(f"analytic lines vs central differences: {worst:.2e} of max |J|")
    assert worst <= 1e-7


def test_oracle_gradient_is_the_derivative_of_the_cost_under_huber():
    w = G.graphs("scale")
    a = (*(x.astype(F64) for x in G.start(w, 0)), *G.one(w, 0))
    huber = 15.0                                           # the start is 0.05 rad, 0.1 m and 0.05 off: chi runs from 11 to 115
    lin = SO.linearise(*a, w["fixed"][0], huber)
    assert (lin["chi2"] > huber ** 2).sum() >= 3 and (lin["chi2"] < huber ** 2).sum() >= 3            # both branches of the Huber term
    h = 1e-6
    for n in (1, 4):
        for k in range(7):
            d = np.zeros((12, 7))
            d[n, k] = h
            cp = SO.cost(*SO.update(*a[:3], d), *a[3:], huber)[1]
            cm = SO.cost(*SO.update(*a[:3], -d), *a[3:], huber)[1]
            fd = (cp - cm) / (2 * h)
            assert abs(fd - 2 * lin["g"][n, k]) <= 1e-6 * max(1.0, abs(fd)), (n, k, fd, 2 * lin["g"][n, k])


@pytest.mark.parametrize("name", G.REFINE_NAMES)
def test_the_pcg_form_reaches_the_dense_forms_cost_on_every_refine_scene(name):
    for i, (a, b) in enumerate(zip(G.oracle_refine(name), G.oracle_refine(name, False, True))):
        rel = abs(a["cost"] - b["cost"]) / b["cost"]
        print(f"{name}[{i}] form (a) {a['cost']:.4f}, form (b) {b['cost']:.4f}: {rel:.2e}")
        assert a["ok"] and b["ok"] and a["cost"] < a["cost0"] and rel <= 0.01


def test_at_scale_one_the_oracle_agrees_with_the_pose_graph_oracle():
    """every scale 1 and every measured scale 1.  On a noisy graph the 6x6 corners of the system, its gradient and its cost are
    K27's (the same arithmetic with factors of 1: 1e-12).  On a noise-free graph -- consistent in scale and in pose, so the truth
    is the optimum of both problems -- the two refinements end at the same poses, and the scales stay at 1 (1e-8: both runs
    have converged to float64 round-off of the truth; a wrong line would leave 1e-2)."""
    R0, t0, ei, zr, zt, info6, fixed = synth_pose_graph(3, 16, 2, 0.01, 0.02)[:7]
    E = len(ei)
    ones, info7 = np.ones(E, bool), np.zeros((E, 7, 7), F32)
    info7[:, :6, :6] = info6
    info7[:, 6, 6] = 1e4
    for huber in (0.0, 1.0):
        lin6 = PO.linearise(R0, t0, ei, zr, zt, info6, ones, fixed, huber)
        lin7 = SO.linearise(np.ones(16), R0, t0, ei, np.ones(E), zr, zt, info7, ones, fixed, huber)
        scale = np.abs(lin6["diag"]).max()
        assert np.abs(lin7["diag"][:, :6, :6] - lin6["diag"]).max() <= 1e-12 * scale and np.abs(lin7["off"][:, :6, :6] - lin6["off"]).max() <= 1e-12 * scale
        assert np.abs(lin7["g"][:, :6] - lin6["g"]).max() <= 1e-12 * scale and abs(lin7["cost"] - lin6["cost"]) <= 1e-12 * lin6["cost"]
        assert (lin7["chi2"] > 1).any() or huber == 0
    g = G6.clean_ring()
    E = len(g["ei"])
    info7 = np.tile(np.eye(7, dtype=F32), (E, 1, 1))
    six = PO.refine(g["R0"], g["t0"], g["ei"], g["zr"], g["zt"], g["info"], g["valid"], g["fixed"], 12, 64, 0.0, dense=True)
    seven = SO.refine(np.ones(32, F32), g["R0"], g["t0"], g["ei"], np.ones(E, F32), g["zr"], g["zt"], info7, g["valid"], g["fixed"], 12, 64, 0.0,
                      dense=True)
    rot = max(PO.rotation_angle_deg(a, b) for a, b in zip(seven["R64"], six["R64"]))
    dt, ds = np.abs(seven["t64"] - six["t64"]).max(), np.abs(seven["s64"] - 1).max()
    print(f"7-DoF at scale 1 vs 6-DoF on the noise-free ring: rot {rot:.2e} deg, t {dt:.2e} m, scales off 1 by {ds:.2e}; "
          f"cost {seven['cost']:.3e} vs {six['cost']:.3e}")
    assert six["ok"] and seven["ok"] and rot <= 1e-6 and dt <= 1e-8 and ds <= 1e-8


def test_oracle_refusals():
    w = G.graphs("7x12")
    a = (*G.start(w, 0), *G.one(w, 0))
    none = SO.refine(*a[:8], np.zeros(12, bool), w["fixed"][0], 3, 8)
    assert not none["ok"] and none["cost0"] == 0.0 and np.array_equal(none["R"], a[1])
    for fixed in (np.zeros(7, bool), np.ones(7, bool)):
        res = SO.refine(*a, fixed, 3, 8)
        assert not res["ok"] and np.isinf(res["cost0"]) and np.isinf(res["cost"]) and not res["chi2"].any()
    for bad in (0.0, -1.0, NAN):
        s = a[0].copy()
        s[3] = bad
        res = SO.refine(s, *a[1:], w["fixed"][0], 3, 8)
        assert not res["ok"] and np.isinf(res["cost0"]) and np.array_equal(res["s"], s, equal_nan=True)


def test_generator_contract():
    g = synth_sim3_graph(5, 64, 4, 0.01, 0.02, 0.01, 0.004, false_loops=2)
    s0, R0, t0, ei, zs, zr, zt, info, fixed, protected, s, R, t, false_edge = g
    assert s0.dtype == F32 and R0.dtype == F32 and ei.dtype == np.int32 and ei.shape == (69, 2) and info.shape == (69, 7, 7) and zs.dtype == F32
    assert fixed.tolist() == [True] + [False] * 63 and protected.sum() == 63 and false_edge.sum() == 2 and not (protected & false_edge).any()
    assert [tuple(e) for e in ei[63:67]] == [(0, 32), (8, 40), (16, 48), (24, 56)]
    assert np.array_equal(ei, synth_pose_graph(5, 64, 4, 0.01, 0.02, false_loops=2)[2]) and np.array_equal(R, synth_pose_graph(5, 64, 4, 0.0, 0.0)[8])
    assert (s == 1).all() and (zs[:63] == 1).all() and (zs[63:67] != 1).all() and np.abs(np.log(zs[63:67])).max() < 0.05
    assert np.allclose(np.diag(info[0]), [1e4] * 3 + [2500.0] * 3 + [1e4]) and not (info[0] - np.diag(np.diag(info[0]))).any()
    assert np.allclose(s0, np.exp(0.004 * np.arange(64)), rtol=1e-6) and np.array_equal(R0[0], R[0].astype(F32))
    ones = np.ones(69, bool)
    chi2 = SO.cost(s, R, t, ei, zs, zr, zt, info, ones)[0]
    assert chi2[:67].mean() < 14 and chi2[:67].max() < 45 and chi2[67:].min() > 1e3          # 7 degrees of freedom; the false loops are gross
    # the start is the chained odometry with the drift: each odometry edge is off by the drift in the scale and by
    # (exp(drift) - 1) t_z, 0.004 x 0.15 m, in the translation, and by nothing else
    c0 = SO.cost(s0, R0, t0, ei[:63], zs[:63], zr[:63], zt[:63], info[:63], ones[:63])[0]
    assert np.allclose(c0, (0.004 / 0.01) ** 2, rtol=0.05)
    before = np.linalg.norm(SO.camera_centres(s0, R0, t0) - SO.camera_centres(s, R, t), axis=1).max()
    assert 0.02 < before < 2.0
    again = synth_sim3_graph(5, 64, 4, 0.01, 0.02, 0.01, 0.004, false_loops=2)
    assert all(np.array_equal(x, y) for x, y in zip(g, again))
    flat = synth_sim3_graph(5, 64, 4, 0.01, 0.02, 0.01, 0.0)
    assert (flat[0] == 1).all() and SO.cost(*flat[:8], np.ones(67, bool))[0][:63].max() < 1e-3          # no drift: the chained odometry
    with pytest.raises(ValueError):
        synth_sim3_graph(1, 1, 0, 0.01, 0.02, 0.01, 0.0)
    with pytest.raises(ValueError):
        synth_sim3_graph(1, 8, 1, 0.01, 0.02, -1.0, 0.0)


# ---- the kernels' arithmetic on the host --------------------------------------------------------------------------------------------
simgraph_host = host_program("simgraph_host.cpp", hip=True)
simgraph_plain = host_program("simgraph_host.cpp", hip=False)
EDGE_FIELDS = (("e", 7), ("chi2", 1), ("w", 1), ("rho", 1), ("Ji", 49), ("Jj", 49), ("Hii", 49), ("Hjj", 49), ("Hij", 49), ("gi", 7), ("gj", 7))


def _fmt(row, spec="%.9g"):
    return " ".join(spec % x for x in row)


def _edge_rows():
    """every active edge of five scenes at their starts: residual rotations from a few degrees to far from small, scales from
    0.2 to 5"""
    rows = []
    for name in ("7x12", "hub", "parallel", "large-angle", "scale"):
        w = G.graphs(name)
        for b in range(3):
            for e, (i, j) in enumerate(w["ei"][b]):
                rows.append(np.concatenate([[w["s0"][b, i]], w["R0"][b, i].ravel(), w["t0"][b, i], [w["s0"][b, j]], w["R0"][b, j].ravel(), w["t0"][b, j],
                                            [w["zs"][b, e]], w["zr"][b, e].ravel(), w["zt"][b, e], w["info"][b, e].ravel()]))
    return np.array(rows, F32)


def _edge_text(rows, huber):
    return "%.9g\n" % huber + "\n".join(_fmt(r) for r in rows)


def _edge_oracle(rows, huber, dtype=F64):
    r = rows.astype(dtype)
    si, Ri, ti, sj, Rj, tj, zs, Rz, tz = (r[:, 0], r[:, 1:10].reshape(-1, 3, 3), r[:, 10:13], r[:, 13], r[:, 14:23].reshape(-1, 3, 3), r[:, 23:26],
                                          r[:, 26], r[:, 27:36].reshape(-1, 3, 3), r[:, 36:39])
    O = SO.omega(r[:, 39:].reshape(-1, 7, 7))
    e, Rp, u, sp = SO.residual(si, Ri, ti, sj, Rj, tj, zs, Rz, tz)
    chi2 = np.einsum("ea,eab,eb->e", e, O, e)
    w, rho = SO._rho(chi2, huber)
    Ji, Jj = SO.lines(e, Rp, u, sp)
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


def test_native_edge_arithmetic_matches_the_float64_oracle(simgraph_host, simgraph_plain):
    """bounds: 4 x what the oracle's own float32 run deviates from its float64 run on the same rows, per quantity, relative to
    the quantity's largest magnitude in the row (printed); the plain C++ build returns the hipcc build's bits"""
    rows = _edge_rows()
    for huber in (0.0, 15.0):
        text = _edge_text(rows, huber)
        raw = run_host(simgraph_host, "edge", text)
        assert raw == run_host(simgraph_plain, "edge", text)
        got = _split(np.array([[float(v) for v in ln] for ln in raw], F64))
        want, single = _edge_oracle(rows, huber), _edge_oracle(rows, huber, F32)
        assert len(raw) == len(rows) and np.degrees(np.linalg.norm(want["e"][:, :3], axis=1)).max() > 150 and np.abs(want["e"][:, 6]).max() > 0.5
        if huber > 0:
            assert (want["w"] < 1).sum() >= 10 and (want["w"] == 1).sum() >= 10                    # both branches
        for k, n in EDGE_FIELDS:
            ref = want[k].reshape(len(rows), -1)
            scale = np.abs(ref).max(1, keepdims=True)
            bound = MARGIN * (np.abs(single[k].reshape(len(rows), -1).astype(F64) - ref) / scale).max()
            dev = (np.abs(got[k] - ref) / scale).max()
            print(f"huber {huber} {k}: native {dev:.2e}, 4 x float32 oracle {bound:.2e}")
            assert dev <= bound, (k, dev, bound)
        assert np.array_equal(got["Hii"].reshape(-1, 7, 7), got["Hii"].reshape(-1, 7, 7).transpose(0, 2, 1))
        assert np.array_equal(got["Hjj"].reshape(-1, 7, 7), got["Hjj"].reshape(-1, 7, 7).transpose(0, 2, 1))


def _precond_rows():
    w = G.graphs("hub")
    lin = SO.linearise(*G.start(w, 0), *G.one(w, 0), w["fixed"][0], 3.0)
    rng = np.random.default_rng(5)
    rows = [np.concatenate([[lam], lin["diag"][n].ravel(), rng.standard_normal(7)]) for lam in (0.0, 1e-4, 10.0) for n in (1, 5, 40, 79)]
    sing = lin["diag"][5].copy()
    sing[3] = sing[2]
    sing[:, 3] = sing[:, 2]
    rows += [np.concatenate([[0.0], m.ravel(), np.ones(7)]) for m in (sing, -lin["diag"][5], np.zeros((7, 7)), np.eye(7))]
    return np.array(rows, F32)


def test_native_preconditioner_solve_matches_the_float64_oracle(simgraph_host):
    rows = _precond_rows()
    out = np.array([[float(v) for v in ln] for ln in run_host(simgraph_host, "precond", "\n".join(_fmt(r) for r in rows))], F64)
    assert out[:, 0].tolist() == [1.0] * 12 + [0.0, 0.0, 0.0, 1.0]
    for row, got in zip(rows, out):
        D, r = row[1:50].reshape(7, 7).astype(F64), row[50:].astype(F64)
        z = SO.block_solve(D, row[0], r)
        assert (z is not None) == bool(got[0])
        if z is None:
            assert not got[1:].any()
            continue
        z32 = SO.block_solve(D, row[0], r, F32)
        bound = MARGIN * np.abs(z32 - z).max() / np.abs(z).max()
        dev = np.abs(got[1:] - z).max() / np.abs(z).max()
        M = D + F64(F32(row[0])) * np.diag(np.diag(D))
        assert dev <= max(bound, 1e-6) and np.abs(M @ z - r).max() <= 1e-9 * np.abs(r).max() * np.linalg.cond(M)


def _update_rows():
    rng = np.random.default_rng(9)
    rows = []
    for angle in (0.0, 1e-9, 1e-3, 0.5, 3.0):
        for sigma in (0.0, -1.5, 0.01, 1.2):
            ax = rng.standard_normal(3)
            ax /= np.linalg.norm(ax)
            rows.append(np.concatenate([SO.exp_so3(rng.standard_normal(3)).ravel(), rng.standard_normal(3), [np.exp(rng.uniform(-1.6, 1.6))],
                                        angle * ax, rng.standard_normal(3), [sigma]]))
    return np.array(rows)


def test_native_update_and_correction_match_the_oracle(simgraph_host, simgraph_plain):
    """the update is float64 on both sides (libm's sin, cos, exp against numpy's: 1e-14 relative, a few ulps of each); the
    correction is float64 in a stated order rounded once: the same bits"""
    rows = _update_rows()
    text = "\n".join(_fmt(r, "%.17g") for r in rows)
    out = np.array([[float(v) for v in ln] for ln in run_host(simgraph_host, "update", text)])
    assert len(out) == len(rows)
    for row, got in zip(rows, out):
        s, R, t = SO.update(row[12:13], row[:9].reshape(1, 3, 3), row[9:12][None], row[13:][None])
        want = np.concatenate([R.ravel(), t.ravel(), s])
        assert np.abs(got - want).max() <= 1e-14 * max(1.0, np.abs(want).max()), (row, got, want)
    w = G.graphs("scale")
    rng = np.random.default_rng(11)
    crow = []
    for b in range(3):
        for n in range(12):
            crow.append(np.concatenate([SO.exp_so3(rng.standard_normal(3)).ravel(), rng.standard_normal(3), [w["s0"][b, n]], w["R0"][b, n].ravel(),
                                        w["t0"][b, n], 20 * rng.uniform(-1, 1, 3)]))
    crow = np.array(crow, F32)
    ctext = "\n".join(_fmt(r) for r in crow)
    raw = run_host(simgraph_host, "correct", ctext)
    assert raw == run_host(simgraph_plain, "correct", ctext)
    got = np.array([[float(v) for v in ln] for ln in raw]).astype(F32)
    for row, g in zip(crow, got):
        r_o, t_o, x_o = SO.correct(row[:9].reshape(1, 3, 3), row[9:12][None], row[12:13], row[13:22].reshape(1, 3, 3), row[22:25][None],
                                   row[25:28][None], np.zeros(1, np.int32))
        want = np.concatenate([r_o.ravel(), t_o.ravel(), x_o.ravel()])
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (row, g, want)


def test_native_harness_under_the_host_sanitizers(tmp_path):
    """the same stand-alone program built with the host's address and undefined-behaviour sanitizers, run once over every mode"""
    exe = build_host(tmp_path, "simgraph_host.cpp", hip=True, extra=SANITIZE)
    rows = _edge_rows()
    assert len(run_host(exe, "edge", _edge_text(rows, 3.0))) == len(rows)
    assert len(run_host(exe, "precond", "\n".join(_fmt(r) for r in _precond_rows()))) == 16
    assert len(run_host(exe, "update", "\n".join(_fmt(r, "%.17g") for r in _update_rows()))) == 20
    assert len(run_host(exe, "correct", _fmt(np.arange(1, 29, dtype=F32)))) == 1


# ---- the section in the binding and the library ---------------------------------------------------------------------------------------
NAMES = ["mi_simgraph_correct", "mi_simgraph_cost", "mi_simgraph_linearise", "mi_simgraph_refine", "mi_simgraph_workspace_bytes"]


def test_the_section_has_a_header_and_a_library_of_its_own(lib):
    assert sorted(N.SIMGRAPH_SIGNATURES) == NAMES
    assert not set(NAMES) & set(N.SIGNATURES) and not set(NAMES) & set(N.SIM3_SIGNATURES) and not set(NAMES) & set(N.DEBUG_SIGNATURES)
    assert all(N.library_of(n) is lib for n in NAMES) and N.library_of("mi_pgo_refine") is N.load() and N.library_of("mi_sim3_apply") is N.load_sim3()
    assert N.SIMGRAPH_CONSTANTS == dict(MI_SIMGRAPH_MAX_NODES=1024, MI_SIMGRAPH_MAX_EDGES=4096, MI_SIMGRAPH_MAX_ITERATIONS=32,
                                        MI_SIMGRAPH_MAX_PCG=256, MI_SIMGRAPH_MAX_ROWS=16777216)
    assert N.RESTYPES["mi_simgraph_workspace_bytes"] is ctypes.c_size_t and N.RESTYPES["mi_simgraph_refine"] is ctypes.c_int
    r = subprocess.run(["nm", "-D", "--defined-only", SIMGRAPH_LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(ln.split()[-1] for ln in r.stdout.splitlines() if ln.split()[-1].startswith("mi_")) == NAMES
    assert [ln for ln in r.stdout.splitlines() if " T " in ln and not ln.split()[-1].startswith("mi_")] == []


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    wb = lib.mi_simgraph_workspace_bytes
    assert wb(1, 2, 1) > 0 and wb(3, 64, 70) == 3 * wb(1, 64, 70) and wb(1, 64, 70) % 16 == 0 and wb(65535, 1024, 4096) == 65535 * wb(1, 1024, 4096)
    assert wb(1, 1024, 4096) >= 4096 * 161 * 4 + 1024 * 26 * 8
    assert wb(0, 64, 70) == 0 and wb(3, 1, 70) == 0 and wb(3, 64, 0) == 0 and wb(3, 1025, 70) == 0 and wb(3, 64, 4097) == 0 and wb(65536, 64, 70) == 0
    assert wb(1, 64, 70) < wb(1, 65, 70) and wb(1, 64, 70) < wb(1, 64, 71)


def test_cost_argument_checks(lib, p):
    f = lib.mi_simgraph_cost
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15):
        a = [p, p, p, p, p, p, p, p, p, 3, 64, 70, 3.0, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    for batch, n, e, hub, want in ((0, 64, 70, 0.0, SHAPE), (3, 1, 70, 0.0, SHAPE), (3, 64, 0, 0.0, SHAPE), (3, -2, 70, 0.0, SHAPE),
                                   (65536, 64, 70, 0.0, PARAM), (3, 1025, 70, 0.0, PARAM), (3, 64, 4097, 0.0, PARAM),
                                   (3, 64, 70, -0.001, PARAM), (3, 64, 70, NAN, PARAM), (3, 64, 70, INF, PARAM), (3, 0, 4097, NAN, SHAPE)):
        assert f(p, p, p, p, p, p, p, p, p, batch, n, e, hub, p, p, p, None) == want, (batch, n, e, hub)


def test_linearise_argument_checks(lib, p):
    f, need = lib.mi_simgraph_linearise, lib.mi_simgraph_workspace_bytes(3, 64, 70)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 18):
        a = [p] * 10 + [3, 64, 70, 3.0, p, p, p, p, p, need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, n=64, e=70, hub=3.0, ws=p, wbytes=need):
        return f(*[p] * 10, batch, n, e, hub, p, p, p, p, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(n=1) == SHAPE and call(e=0) == SHAPE
    assert call(batch=65536) == PARAM and call(n=1025) == PARAM and call(e=4097) == PARAM
    assert call(hub=-1.0) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(hub=-1.0, wbytes=0) == PARAM                                # parameters are judged before the workspace


def test_refine_argument_checks(lib, p):
    f, need = lib.mi_simgraph_refine, lib.mi_simgraph_workspace_bytes(3, 64, 70)
    for i in list(range(10)) + list(range(16, 26)):
        a = [p] * 10 + [3, 64, 70, 10, 64, 3.0] + [p] * 10 + [need, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, n=64, e=70, it=10, trips=64, hub=3.0, ws=p, wbytes=need):
        return f(*[p] * 10, batch, n, e, it, trips, hub, *[p] * 9, ws, wbytes, None)
    assert call(batch=0) == SHAPE and call(n=1) == SHAPE and call(n=0) == SHAPE and call(e=0) == SHAPE and call(e=-1) == SHAPE
    assert call(batch=65536) == PARAM and call(n=1025) == PARAM and call(e=4097) == PARAM
    assert call(it=0) == PARAM and call(it=33) == PARAM and call(it=-1) == PARAM
    assert call(trips=0) == PARAM and call(trips=257) == PARAM and call(trips=-1) == PARAM
    assert call(hub=-1e-9) == PARAM and call(hub=NAN) == PARAM and call(hub=INF) == PARAM and call(hub=-INF) == PARAM
    assert call(wbytes=need - 1) == CAPACITY and call(wbytes=0) == CAPACITY and call(ws=p + 4) == ALIGN
    assert call(it=0, wbytes=0) == PARAM and call(e=0, it=0) == SHAPE       # shape, then parameters, then the workspace


def test_correct_argument_checks(lib, p):
    f = lib.mi_simgraph_correct
    for i in (0, 1, 2, 3, 4, 10, 11):                                       # the pose arrays are needed when there are nodes
        a = [p] * 7 + [3, 5, 9, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    for i in (5, 6, 12):                                                    # ... the landmark arrays when there are landmarks
        a = [p] * 7 + [3, 5, 9, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    assert f(*[p] * 7, 0, 5, 9, p, p, p, None) == SHAPE and f(*[p] * 7, 3, -1, 9, p, p, p, None) == SHAPE
    assert f(*[p] * 7, 3, 5, -1, p, p, p, None) == SHAPE and f(*[None] * 7, 3, 0, 0, None, None, None, None) == SHAPE
    assert f(*[p] * 7, 65536, 5, 9, p, p, p, None) == PARAM and f(*[p] * 7, 3, 16777216, 1, p, p, p, None) == PARAM
    assert f(*[p] * 7, 0, 16777216, 1, p, p, p, None) == SHAPE              # shape before parameters


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import SimilarityGraphOptimizer
    assert (ops.SIMGRAPH_MAX_NODES, ops.SIMGRAPH_MAX_EDGES, ops.SIMGRAPH_MAX_ITERATIONS, ops.SIMGRAPH_MAX_PCG) == (1024, 4096, 32, 256)
    m = SimilarityGraphOptimizer()
    assert (m.iterations, m.pcg_iterations, m.huber, m.outlier_rounds, m.outlier_chi2) == (10, 64, 3.0, 1, 18.48)
    for kw in (dict(iterations=0), dict(iterations=33), dict(pcg_iterations=0), dict(pcg_iterations=257), dict(huber=-1.0),
               dict(huber=float("nan")), dict(outlier_rounds=-1), dict(outlier_chi2=0.0)):
        with pytest.raises(ValueError):
            SimilarityGraphOptimizer(**kw)
    w = G.graphs("7x12")
    a = [torch.from_numpy(w[k].copy()) for k in ("s0", "R0", "t0", "ei", "zs", "zr", "zt", "info", "fixed")]
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*(x[0] for x in a))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(None, *a[1:])
    with pytest.raises(RuntimeError, match=r"\(B, E, 2\) or \(E, 2\)"):
        m(*a[:3], a[3][..., :1], *a[4:])
    with pytest.raises(RuntimeError, match="edge_valid and protected"):
        m(*a, torch.ones(3, 5, dtype=torch.bool))
    valid = torch.ones(3, 12, dtype=torch.bool)
    for call in (lambda: ops.simgraph_cost(*a[:8]), lambda: ops.simgraph_linearise(*a), lambda: ops.simgraph_refine(*a, valid),
                 lambda: ops.simgraph_correct(a[1], a[2], a[0], a[1], a[2], a[2], a[3][:, :7, 0])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match=r"rotations must be \(B, N, 3, 3\)"):
        ops.simgraph_refine(a[0], a[1][0], *a[2:])
    with pytest.raises(RuntimeError, match="expected s"):
        ops.simgraph_refine(*a[:4], a[4][:, :5], *a[5:])
    with pytest.raises(RuntimeError, match="expected s"):
        ops.simgraph_refine(a[0][:, :3], *a[1:])
    with pytest.raises(RuntimeError, match="fixed must be"):
        ops.simgraph_refine(*a[:8], a[8][:, :3])
    with pytest.raises(RuntimeError, match="supported: 2 .. 1024 and 1 .. 4096"):
        ops.simgraph_cost(a[0][:, :1], a[1][:, :1], a[2][:, :1], *a[3:8])
    with pytest.raises(RuntimeError, match="huber"):
        ops.simgraph_cost(*a[:8], None, -1.0)
    with pytest.raises(RuntimeError, match="pcg_iterations"):
        ops.simgraph_refine(*a, valid, 10, 257)
    with pytest.raises(RuntimeError, match="given together"):
        ops.simgraph_correct(a[1], a[2], None, a[1], a[2], None, None)
    with pytest.raises(RuntimeError, match="needs poses or points"):
        ops.simgraph_correct(None, None, None, None, None, None, None)
    # the helpers that are plain torch work anywhere
    zs, zr, zt = SimilarityGraphOptimizer.edges_from_state(a[1], a[2], a[3], a[0])
    i, j = w["ei"][1, 4]
    assert zs.dtype == torch.float32 and tuple(zs.shape) == (3, 12) and abs(float(zs[1, 4]) - w["s0"][1, j] / w["s0"][1, i]) < 1e-6
    want = w["t0"][1, j].astype(F64) - float(zs[1, 4]) * (zr[1, 4].double().numpy() @ w["t0"][1, i].astype(F64))
    assert np.abs(zt[1, 4].numpy() - want).max() < 1e-5
    i7 = SimilarityGraphOptimizer.information_from_pose(torch.ones(2, 5, 6, 6), torch.full((2, 5), 9.0))
    assert tuple(i7.shape) == (2, 5, 7, 7) and float(i7[1, 2, 6, 6]) == 9.0 and float(i7[..., 6, :6].abs().max()) == 0.0


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import SimilarityGraphOptimizer
    assert SimilarityGraphOptimizer is real.SimilarityGraphOptimizer and "SimilarityGraphOptimizer" in real.__all__
    from pytorch_model.geometry.similarity_graph import SimilarityGraphOptimizer as again
    assert again is SimilarityGraphOptimizer


# ---- the measurements behind the GPU tolerances ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    """the largest deviation of the oracle's float32 run from its float64 run, per quantity, over every scene"""
    m = dict(chi2=0.0, cost=0.0, lin=0.0, rot=0.0, t=0.0, s=0.0, centre=0.0, rcost=0.0)
    for name in G.NAMES:
        w = G.graphs(name)
        for i in range(3):
            a = (*G.start(w, i), *G.one(w, i))
            c64, k64, _ = SO.cost(*a, w["huber"])
            c32, k32, _ = SO.cost(*a, w["huber"], F32)
            m["chi2"] = max(m["chi2"], (np.abs(c32 - c64) / np.maximum(c64, G.CHI2_FLOOR)).max())
            m["cost"] = max(m["cost"], abs(k32 - k64) / k64)
            l64, l32 = SO.linearise(*a, w["fixed"][i], w["huber"]), SO.linearise(*a, w["fixed"][i], w["huber"], F32)
            m["lin"] = max(m["lin"], max(np.abs(l32[k] - l64[k]).max() for k in ("diag", "off", "g")) / np.abs(l64["diag"]).max())
    for name in G.REFINE_NAMES:
        for r32, r64 in zip(G.oracle_refine(name, True), G.oracle_refine(name)):
            rot, dt, ds, dc, dcost = G.refine_deviation(r32, r64)
            m["rot"], m["t"], m["s"], m["centre"], m["rcost"] = max(m["rot"], rot), max(m["t"], dt), max(m["s"], ds), max(m["centre"], dc), max(m["rcost"], dcost)
    g = G.clean_ring()
    res = SO.refine(g["s0"], g["R0"], g["t0"], g["ei"], g["zs"], g["zr"], g["zt"], g["info"], g["valid"], g["fixed"], G.CLEAN_ITERATIONS,
                    G.CLEAN_TRIPS, 0.0, F32)
    m["clean_rot"], m["clean_t"], m["clean_s"] = G.recovery_error(res["s"], res["R"], res["t"], g)
    print("float32 oracle vs float64 oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    return m


def test_gpu_tolerances_are_four_times_their_measurements(measured):
    m = measured
    for const, value in ((G.CHI2_RTOL, m["chi2"]), (G.COST_RTOL, m["cost"]), (G.LIN_TOL, m["lin"]), (G.REFINE_ROT_DEG, m["rot"]),
                         (G.REFINE_T_M, m["t"]), (G.REFINE_S_RTOL, m["s"]), (G.REFINE_CENTRE_M, m["centre"]), (G.REFINE_COST_RTOL, m["rcost"]),
                         (G.RECOVER_ROT_DEG, m["clean_rot"]), (G.RECOVER_T_M, m["clean_t"]), (G.RECOVER_S_RTOL, m["clean_s"])):
        assert value > 0 and MARGIN * value <= const <= 16 * MARGIN * value, (const, value)
