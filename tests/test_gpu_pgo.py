"""K27 pose-graph optimisation on the GPU against the float64 oracle (tests/pgo_oracle.py): mi_pgo_cost, mi_pgo_linearise and
mi_pgo_refine at the smallest shapes at which each mechanism can go wrong, and what the contract makes exact, bit for bit.

Tolerances.  Each constant below is at least 4 x the largest deviation of the oracle's float32 run from its float64 run over
every graph of SCENES (cost, linearise) and REFINE_SCENES (refine), rounded up to a round figure; tests/test_pgo_host.py
measures them on the CPU and asserts the relation (the 4 x is for the kernel's lanes-strided and cross-wave sums, which are
ordered differently from numpy's).  Measured (worst scene):
  chi2, relative to max(chi2, 1e-3) .................. 5.13e-6 (257x300)  -> CHI2_RTOL 2.5e-5
  cost, relative ..................................... 1.63e-7 (edgeless) -> COST_RTOL 1e-6
  diag, off and g, relative to max |diag| ............ 6.54e-7 (257x300)  -> LIN_TOL 3e-6
  refined rotations, degrees ......................... 1.14e-3 (65+4)     -> REFINE_ROT_DEG 5e-3
  refined translations, metres ....................... 9.67e-5 (65+4)     -> REFINE_T_M 4e-4
  refined cost, relative ............................. 2.22e-6 (257+8)    -> REFINE_COST_RTOL 1e-5
  noise-free ring, distance from the truth ........... 3.19e-6 deg, 1.30e-7 m (the float32 run's; the float64 run's:
                                                       1.99e-6 deg, 6.4e-8 m, the rounding of the float32 result)
                                                       -> RECOVER_ROT_DEG 2e-5, RECOVER_T_M 6e-7
The gauge is a fixed node, so refined poses are compared as they are.  The refine scenes are ones on which the stated
algorithm (form (a), fixed PCG trips) ends within 1 % of the dense solve's cost (form (b)); tests/test_pgo_host.py asserts it."""
import functools

import numpy as np
import pytest
import torch

import pgo_oracle as PO
from gpu_common import DEV, GPU, gpu, same_bits, twice
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import PoseGraphOptimizer
from onnx_image_processing_amd.synth import synth_pose_graph

pytestmark = GPU
F32, F64 = np.float32, np.float64

CHI2_RTOL, CHI2_FLOOR = 2.5e-5, 1e-3
COST_RTOL = 1e-6
LIN_TOL = 3e-6
REFINE_ROT_DEG, REFINE_T_M, REFINE_COST_RTOL = 5e-3, 4e-4, 1e-5
RECOVER_ROT_DEG, RECOVER_T_M = 2e-5, 6e-7
SIGMA = (0.01, 0.02)                    # rad, m: the measurement noise of every scene but the noise-free one


def chain(n):
    return [(k, k + 1) for k in range(n - 1)]


def chords(n, count):
    """`count` distinct chords (i, j), j - i >= 2, spread over the ring"""
    out = []
    for c in range(count):
        i = (c * 7) % (n - 2)
        j = i + 2 + (c * 5) % (n - 2 - i)
        out.append((i, j))
    return out


def make_graph(seed, n, pairs, start=(0.05, 0.1), fixed=(0,), sigma=SIGMA):
    """a graph over the pairs on synth_pose_graph's ring: measurements with noise in the residual's coordinates, the start the
    truth perturbed by N(0, start) (rad, m) except at the fixed nodes"""
    R, t = synth_pose_graph(seed, n, 0, 0.0, 0.0)[8:10]
    rng = np.random.default_rng(seed)
    E = len(pairs)
    zr, zt = np.zeros((E, 3, 3)), np.zeros((E, 3))
    for e, (i, j) in enumerate(pairs):
        Rp = R[j] @ R[i].T
        Ew = PO.exp_so3(sigma[0] * rng.standard_normal(3))
        zr[e], zt[e] = Ew.T @ Rp, Ew.T @ (t[j] - Rp @ t[i] - sigma[1] * rng.standard_normal(3))
    fx = np.zeros(n, bool)
    fx[list(fixed)] = True
    R0, t0 = R.copy(), t.copy()
    for k in np.flatnonzero(~fx):
        Ew = PO.exp_so3(start[0] * rng.standard_normal(3))
        R0[k], t0[k] = Ew @ R[k], Ew @ t[k] + start[1] * rng.standard_normal(3)
    info = np.tile(np.diag([1 / sigma[0] ** 2 if sigma[0] > 0 else 1.0] * 3 + [1 / sigma[1] ** 2 if sigma[1] > 0 else 1.0] * 3), (E, 1, 1))
    return dict(R0=R0.astype(F32), t0=t0.astype(F32), ei=np.array(pairs, np.int32).reshape(E, 2), zr=zr.astype(F32), zt=zt.astype(F32),
                info=info.astype(F32), valid=np.ones(E, bool), fixed=fx, R=R, t=t)


def _ragged(seed):
    """10 nodes, 14 edges, one of each kind of inactive edge at a place that depends on the seed"""
    g = make_graph(seed, 10, chain(10) + chords(10, 5))
    k = seed % 4
    g["ei"][k] = (-1, 3)
    g["ei"][k + 1] = (4, 4)
    g["ei"][k + 2] = (2, 10)
    g["info"][k + 3, 1, 4] = np.nan
    g["valid"][k + 4] = False
    g["zt"][13 - k, 2] = np.inf
    return g


# name -> (builder of one graph from a seed, Huber width, the three graphs' seeds)
SCENES = {
    "2x1": (lambda s: make_graph(s, 2, [(0, 1)]), 0.0, (1, 2, 3)),
    "3x3": (lambda s: make_graph(s, 3, [(0, 1), (1, 2), (0, 2)]), 0.0, (1, 2, 3)),
    "7x12": (lambda s: make_graph(s, 7, chain(7) + chords(7, 6)), 3.0, (1, 2, 3)),
    "64x70": (lambda s: make_graph(s, 64, chain(64) + chords(64, 7)), 3.0, (1, 2, 3)),
    "65x70": (lambda s: make_graph(s, 65, chain(65) + chords(65, 6)), 0.0, (1, 2, 3)),            # one node past a wave
    "257x300": (lambda s: make_graph(s, 257, chain(257) + chords(257, 44)), 3.0, (1, 2, 3)),       # more nodes than threads
    "hub": (lambda s: make_graph(s, 80, chain(80) + [(5, k) for k in range(8, 78)]), 3.0, (1, 2, 3)),     # a node of degree 72
    "parallel": (lambda s: make_graph(s, 4, chain(4) + [(1, 2), (2, 1)]), 0.0, (1, 2, 3)),         # three edges on one pair
    "ragged": (_ragged, 3.0, (1, 2, 3)),
    "edgeless": (lambda s: make_graph(s, 6, chain(5) + [(0, 2), (1, 4)]), 0.0, (1, 2, 3)),         # node 5 has no edge
    "one-free": (lambda s: make_graph(s, 6, chain(6) + [(0, 3), (1, 3), (3, 5)], fixed=(0, 1, 2, 4, 5)), 3.0, (1, 2, 3)),
    "large-angle": (lambda s: make_graph(s, 5, chain(5) + [(0, 2), (1, 4)], start=(0.7, 0.5)), 0.0, (1, 2, 3)),   # residual rotations far from small
}
NAMES = list(SCENES)
KEYS = ("R0", "t0", "ei", "zr", "zt", "info", "valid", "fixed")


@functools.lru_cache(maxsize=None)
def graphs(name):
    """the batch of a scene: dict of arrays stacked over its three graphs, and the Huber width"""
    build, huber, seeds = SCENES[name]
    parts = [build(s) for s in seeds]
    out = {k: np.stack([p[k] for p in parts]) for k in KEYS + ("R", "t")}
    out["huber"] = huber
    return out


def one(w, i):
    """graph i of a batch as the oracle's positional arguments after (R, t): (ei, zr, zt, info, valid)"""
    return w["ei"][i], w["zr"][i], w["zt"][i], w["info"][i], w["valid"][i]


def state(w):
    return gpu(*(w[k] for k in KEYS))


# name -> (nodes, loops, LM iterations, PCG trips, seeds): synth_pose_graph's noisy ring from the chained odometry
REFINE_SCENES = {"64+4": (64, 4, 8, 40, (1, 2, 3)), "65+4": (65, 4, 8, 40, (1, 2, 3)), "257+8": (257, 8, 8, 80, (1, 2))}
REFINE_NAMES = list(REFINE_SCENES)
REFINE_HUBER = 3.0


@functools.lru_cache(maxsize=None)
def rings(name):
    n, loops, _, _, seeds = REFINE_SCENES[name]
    parts = [synth_pose_graph(s, n, loops, *SIGMA) for s in seeds]
    out = {k: np.stack([p[i] for p in parts]) for i, k in enumerate(("R0", "t0", "ei", "zr", "zt", "info", "fixed", "protected", "R", "t"))}
    out["valid"] = np.ones(out["ei"].shape[:2], bool)
    out["huber"] = REFINE_HUBER
    return out


@functools.lru_cache(maxsize=None)
def oracle_refine(name, single=False, dense=False):
    w = rings(name)
    _, _, its, trips, seeds = REFINE_SCENES[name]
    return [PO.refine(w["R0"][i], w["t0"][i], *one(w, i), w["fixed"][i], its, trips, w["huber"], F32 if single else F64, dense)
            for i in range(len(seeds))]


def refine_deviation(res, ref):
    """(rotation deg, translation m, relative cost) between a result and the oracle's"""
    rot = max(PO.rotation_angle_deg(a, b) for a, b in zip(np.asarray(res["R"], F64), ref["R64"]))
    return rot, float(np.abs(np.asarray(res["t"], F64) - ref["t64"]).max()), abs(res["cost"] - ref["cost"]) / ref["cost"]


@functools.lru_cache(maxsize=None)
def clean_ring():
    """a noise-free ring of 32 nodes with 2 loops, started from perturbed poses: the truth is the optimum, cost 0"""
    pairs = [tuple(p) for p in synth_pose_graph(4, 32, 2, 0.0, 0.0)[2]]
    return make_graph(4, 32, pairs, start=(0.02, 0.05), sigma=(0.0, 0.0))          # (its information is the identity)


CLEAN_ITERATIONS, CLEAN_TRIPS = 10, 64


def recovery_error(R, t, g):
    return max(PO.rotation_angle_deg(a, b) for a, b in zip(np.asarray(R, F64), g["R"])), float(np.abs(np.asarray(t, F64) - g["t"]).max())


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cost_matches_the_oracle(name):
    w = graphs(name)
    r, t, ei, zr, zt, info, valid, fixed = state(w)
    chi2, cost, active = ops.pgo_cost(r, t, ei, zr, zt, info, valid, w["huber"])
    for i in range(3):
        chi2_o, c_o, act_o = PO.cost(w["R0"][i], w["t0"][i], *one(w, i), w["huber"])
        assert np.array_equal(active[i].cpu().numpy(), act_o)
        got = chi2[i].cpu().numpy()
        assert not got[~act_o].any()
        dev = np.abs(got - chi2_o) / np.maximum(chi2_o, CHI2_FLOOR)
        print(f"{name}[{i}] chi2 {dev.max():.3e} cost {abs(float(cost[i]) - c_o) / c_o:.3e}")
        assert dev.max() <= CHI2_RTOL and abs(float(cost[i]) - c_o) <= COST_RTOL * c_o
    if name == "ragged":
        assert [int(a.sum()) for a in active] == [8, 8, 8]


@pytest.mark.parametrize("name", NAMES)
def test_linearise_matches_the_oracle(name):
    w = graphs(name)
    r, t, ei, zr, zt, info, valid, fixed = state(w)
    diag, off, g, cost = ops.pgo_linearise(r, t, ei, zr, zt, info, fixed, valid, w["huber"])
    for i in range(3):
        lin = PO.linearise(w["R0"][i], w["t0"][i], *one(w, i), w["fixed"][i], w["huber"])
        dg, og, gg = (a[i].cpu().numpy().astype(F64) for a in (diag, off, g))
        scale = np.abs(lin["diag"]).max()
        dd, do, dgr = np.abs(dg - lin["diag"]).max() / scale, np.abs(og - lin["off"]).max() / scale, np.abs(gg - lin["g"]).max() / scale
        print(f"{name}[{i}] diag {dd:.3e} off {do:.3e} g {dgr:.3e}")
        assert max(dd, do, dgr) <= LIN_TOL
        assert np.array_equal(dg, dg.transpose(0, 2, 1))
        assert not dg[~lin["live"]].any() and not gg[~lin["live"]].any() and not og[~lin["act"]].any()
        touch = w["fixed"][i][np.clip(w["ei"][i], 0, len(dg) - 1)].any(1)
        assert not og[touch & lin["act"]].any()
        assert abs(float(cost[i]) - lin["cost"]) <= COST_RTOL * lin["cost"]


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_refine_matches_the_oracle(name):
    w = rings(name)
    _, _, its, trips, seeds = REFINE_SCENES[name]
    out = ops.pgo_refine(*gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"]), its, trips, w["huber"])
    ro, to, chi2, cost0, cost, accepted, info, ok = out
    assert ok.all() and (accepted >= 1).all() and (cost < cost0).all()
    refs = oracle_refine(name)
    for i in range(len(seeds)):
        res = dict(R=ro[i].cpu().numpy(), t=to[i].cpu().numpy(), cost=float(cost[i]))
        rot, dt, dc = refine_deviation(res, refs[i])
        print(f"{name}[{i}] rot {rot:.3e} deg t {dt:.3e} m cost {dc:.3e} ({float(cost0[i]):.1f} -> {float(cost[i]):.3f}, accepted {int(accepted[i])})")
        assert rot <= REFINE_ROT_DEG and dt <= REFINE_T_M and dc <= REFINE_COST_RTOL
        assert abs(float(cost0[i]) - refs[i]["cost0"]) <= COST_RTOL * refs[i]["cost0"]


# ---- exact by contract ------------------------------------------------------------------------------------------------------------
def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def test_the_same_call_twice_gives_the_same_bits():
    w = graphs("ragged")
    a = state(w)
    twice("pgo_cost", lambda: _np(ops.pgo_cost(*a[:7], w["huber"])))
    twice("pgo_linearise", lambda: _np(ops.pgo_linearise(*a[:6], a[7], a[6], w["huber"])))
    twice("pgo_refine", lambda: _np(ops.pgo_refine(*a[:6], a[7], a[6], 4, 16, w["huber"])))
    r = rings("65+4")
    b = gpu(r["R0"], r["t0"], r["ei"], r["zr"], r["zt"], r["info"], r["fixed"], r["valid"])
    twice("pgo_refine 65+4", lambda: _np(ops.pgo_refine(*b, 4, 20, REFINE_HUBER)))


def test_a_graph_alone_equals_the_graph_inside_a_batch():
    r = rings("65+4")
    b = gpu(r["R0"], r["t0"], r["ei"], r["zr"], r["zt"], r["info"], r["fixed"], r["valid"])
    pick = [0, 1, 2, 1, 0]                                  # graph 0 at positions 0 and last of a batch of 5
    five = tuple(a[pick].contiguous() for a in b)
    alone = tuple(a[:1].contiguous() for a in b)
    for call in (lambda a: ops.pgo_refine(*a, 4, 20, REFINE_HUBER), lambda a: ops.pgo_linearise(*a, REFINE_HUBER),
                 lambda a: ops.pgo_cost(*a[:6], a[7], REFINE_HUBER)):
        solo, batch = call(alone), call(five)
        assert same_bits(solo, [o[:1] for o in batch]) and same_bits(solo, [o[4:] for o in batch])


def _raw_refine(a, n, e, its, trips, huber, fill):
    """mi_pgo_refine on outputs and a workspace filled with the byte `fill`"""
    b = a[0].shape[0]
    def mk(shape, dt):
        return torch.full((int(np.prod(shape)) * dt.itemsize,), fill, dtype=torch.uint8, device=DEV).view(dt).reshape(shape)
    outs = [mk((b, n, 3, 3), torch.float32), mk((b, n, 3), torch.float32), mk((b, e), torch.float32), mk((b,), torch.float32),
            mk((b,), torch.float32), mk((b,), torch.int32), mk((b, n, 6, 6), torch.float32), mk((b,), torch.uint8)]
    wbytes = int(N.load().mi_pgo_workspace_bytes(b, n, e))
    work = torch.full(((wbytes + 15) // 16 * 16,), fill, dtype=torch.uint8, device=DEV)
    r, t, ei, zr, zt, info, fixed, valid = a
    N.call("mi_pgo_refine", r.data_ptr(), t.data_ptr(), ei.data_ptr(), zr.data_ptr(), zt.data_ptr(), info.data_ptr(),
           valid.view(torch.uint8).data_ptr(), fixed.view(torch.uint8).data_ptr(), b, n, e, its, trips, float(huber),
           *(o.data_ptr() for o in outs), work.data_ptr(), wbytes, N.stream_ptr())
    torch.cuda.synchronize()
    return outs


def test_poisoned_workspace_and_outputs_change_nothing():
    w = graphs("ragged")
    a = gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"])
    zero, ones, mid = (_raw_refine(a, 10, 14, 4, 16, w["huber"], f) for f in (0, 0xFF, 0x7F))
    assert same_bits(zero, ones) and same_bits(zero, mid)
    assert all(torch.isfinite(o.float()).all() for o in zero)


def test_refused_graphs_return_their_inputs():
    w = graphs("7x12")
    R0, t0, fixed, valid = w["R0"].copy(), w["t0"].copy(), np.stack([w["fixed"][0]] * 4), np.stack([w["valid"][0]] * 4)
    R0, t0 = np.stack([R0[0]] * 4), np.stack([t0[0]] * 4)
    valid[0] = False                                       # no active edge: cost 0
    fixed[1] = False                                       # no fixed node
    fixed[2] = True                                        # no free node
    R0[3, 4, 1, 1] = np.nan                                # the initial cost is not finite
    rep = lambda k: np.stack([w[k][0]] * 4)
    a = gpu(R0, t0, rep("ei"), rep("zr"), rep("zt"), rep("info"), fixed, valid)
    ro, to, chi2, cost0, cost, accepted, info, ok = ops.pgo_refine(*a, 5, 16, 3.0)
    assert not ok.any() and not accepted.any() and not chi2.any() and not info.any()
    assert same_bits((ro, to), a[:2])
    assert cost0.tolist() == [0.0, np.inf, np.inf, np.inf] and cost.tolist() == cost0.tolist()
    # ... and a refused graph does not disturb its neighbour in the batch
    valid[1:] = w["valid"][0]
    fixed[1:] = w["fixed"][0]
    R0[3] = w["R0"][0]
    a = gpu(R0, t0, rep("ei"), rep("zr"), rep("zt"), rep("info"), fixed, valid)
    out = ops.pgo_refine(*a, 5, 16, 3.0)
    assert out[7].tolist() == [False, True, True, True] and same_bits([o[1:2] for o in out], [o[3:4] for o in out])


def test_fixed_and_edgeless_nodes_return_their_inputs():
    for name, frozen in (("edgeless", [0, 5]), ("one-free", [0, 1, 2, 4, 5])):
        w = graphs(name)
        r, t, ei, zr, zt, info, valid, fixed = state(w)
        ro, to, chi2, cost0, cost, accepted, inf, ok = ops.pgo_refine(r, t, ei, zr, zt, info, fixed, valid, 6, 16, w["huber"])
        assert ok.all() and (cost < cost0).all()
        assert same_bits((ro[:, frozen], to[:, frozen]), (r[:, frozen], t[:, frozen]))
        moved = [k for k in range(6) if k not in frozen]
        assert not torch.equal(ro[:, moved], r[:, moved]) and not inf[:, frozen].any() and inf[:, moved].diagonal(dim1=2, dim2=3).min() > 0


@pytest.mark.parametrize("name", ["ragged", "65+4"])
def test_info_is_the_diagonal_of_a_separate_linearisation_at_the_result(name):
    w = graphs(name) if name in SCENES else rings(name)
    a = gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"])
    ro, to, chi2, cost0, cost, accepted, info, ok = ops.pgo_refine(*a, 6, 20, w["huber"])
    diag, _, _, c = ops.pgo_linearise(ro, to, *a[2:], w["huber"])
    assert ok.all() and same_bits((info, cost), (diag, c))
    chi2_sep, c_sep, _ = ops.pgo_cost(ro, to, *a[2:6], a[7], w["huber"])
    assert same_bits((chi2, cost), (chi2_sep, c_sep))


# ---- ground truth -----------------------------------------------------------------------------------------------------------------
def test_a_noise_free_ring_is_recovered():
    g = clean_ring()
    a = gpu(*(g[k][None] for k in ("R0", "t0", "ei", "zr", "zt", "info", "fixed", "valid")))
    ro, to, chi2, cost0, cost, accepted, info, ok = ops.pgo_refine(*a, CLEAN_ITERATIONS, CLEAN_TRIPS, 0.0)
    rot, dt = recovery_error(ro[0].cpu().numpy(), to[0].cpu().numpy(), g)
    rot0, dt0 = recovery_error(g["R0"], g["t0"], g)
    print(f"noise-free ring: {rot0:.3f} deg, {dt0:.3f} m -> {rot:.3e} deg, {dt:.3e} m; cost {float(cost0[0]):.3e} -> {float(cost[0]):.3e}")
    assert ok.all() and rot0 > 1.0 and dt0 > 0.05 and rot <= RECOVER_ROT_DEG and dt <= RECOVER_T_M


def test_a_noisy_ring_gets_cheaper_and_reports_the_chi2_of_its_result():
    w = rings("64+4")
    a = gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"])
    ro, to, chi2, cost0, cost, accepted, info, ok = ops.pgo_refine(*a, 8, 40, REFINE_HUBER)
    chi2_sep, _, active = ops.pgo_cost(ro, to, *a[2:6], a[7], 0.0)
    assert ok.all() and (cost < cost0).all() and active.all() and same_bits((chi2,), (chi2_sep,))
    before = np.array([np.abs(w["t0"][i] - w["t"][i]).max() for i in range(3)])
    after = np.array([np.abs(to[i].cpu().numpy() - w["t"][i]).max() for i in range(3)])
    print(f"64+4: drift at the worst node {before} m -> {after} m")
    assert (after < before).all()


def test_the_module_clears_a_false_loop_and_keeps_the_true_edges():
    n, loops = 64, 4
    g = synth_pose_graph(1, n, loops, *SIGMA, false_loops=1)
    R0, t0, ei, zr, zt, info, fixed, protected, R, t, false_edge = g
    a = gpu(R0, t0, ei, zr, zt, info, fixed)
    pgo = PoseGraphOptimizer(iterations=8, pcg_iterations=40)
    ro, to, valid_out, chi2, cost0, cost, inf, ok = pgo(*a, None, gpu(protected))
    assert bool(ok) and np.array_equal(valid_out.cpu().numpy(), ~false_edge) and float(cost) < float(cost0)
    # the run without the false edge, from the same start: two passes as well
    keep = ~false_edge
    b = gpu(R0, t0, ei[keep], zr[keep], zt[keep], info[keep], fixed)
    r2, t2, v2, _, _, cost2, _, ok2 = pgo(*b, None, gpu(protected[keep]))
    rot = max(PO.rotation_angle_deg(x, y) for x, y in zip(ro.cpu().numpy(), r2.cpu().numpy()))
    dt, dc = float((to - t2).abs().max()), abs(float(cost) - float(cost2)) / float(cost2)
    print(f"with the false loop cleared vs never there: rot {rot:.3e} deg t {dt:.3e} m cost {dc:.3e}")
    assert bool(ok2) and bool(v2.all()) and rot <= REFINE_ROT_DEG and dt <= REFINE_T_M and dc <= REFINE_COST_RTOL
    # batched input, a refused graph beside it, gives the same bits for the good one
    two = tuple(torch.stack([x, x]) for x in a)
    fx = two[6].clone()
    fx[1] = False
    out = pgo(*two[:6], fx, None, torch.stack([gpu(protected)] * 2))
    assert out[7].tolist() == [True, False] and same_bits([o[:1] for o in out], [o[None] for o in (ro, to, valid_out, chi2, cost0, cost, inf, ok)])
    assert same_bits((out[0][1], out[1][1]), (a[0], a[1])) and bool(out[2][1].all())


def test_one_graph_at_the_caps():
    n, e = ops.PGO_MAX_NODES, ops.PGO_MAX_EDGES
    g = make_graph(7, n, chain(n) + chords(n, e - (n - 1)), start=(0.01, 0.02))
    a = gpu(*(g[k][None] for k in ("R0", "t0", "ei", "zr", "zt", "info", "fixed", "valid")))
    ro, to, chi2, cost0, cost, accepted, info, ok = ops.pgo_refine(*a, 2, 8, 3.0)
    assert bool(ok.all()) and all(bool(torch.isfinite(o).all()) for o in (ro, to, chi2, cost0, cost, info))
    print(f"caps: cost {float(cost0):.1f} -> {float(cost):.1f}, accepted {int(accepted)}")
    assert float(cost) <= float(cost0)


def test_refine_captures_into_a_graph_and_replays_to_the_eager_bits():
    w = rings("64+4")
    a = gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"])
    eager = ops.pgo_refine(*a, 4, 20, REFINE_HUBER)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):        # one stream, one kernel node, no forked branch
            captured = ops.pgo_refine(*a, 4, 20, REFINE_HUBER)
    for o in captured:
        o.view(torch.uint8).fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, eager)
