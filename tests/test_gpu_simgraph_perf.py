"""K31 rate: mi_simgraph_linearise on 64 graphs x 128 nodes x 256 edges beats a torch-on-GPU formulation of the same undamped
linearisation (batched residuals, 7x7 lines and blocks from stock torch ops, index_add over the nodes); that the formulation
computes mi_simgraph_linearise's system is shown on a small ragged batch first and on the timed tensors themselves.
mi_pgo_linearise (K27, 6 degrees of freedom) is timed on the same shape beside it, one damped step (mi_simgraph_refine with
iterations = 1, 64 PCG trips) on the same batch and the whole mi_simgraph_refine (10 x 64) on 256 graphs x 256 nodes x 512
edges are timed and printed; only the comparison with the torch formulation is asserted.  Measured: see DESIGN.md, "K31"."""
import numpy as np
import torch

import test_gpu_pgo_perf as P6
import test_gpu_simgraph as G
from gpu_common import DEV, GPU, time_ms
from onnx_image_processing_amd import ops

pytestmark = GPU
GRAPHS, NODES, EDGES, TRIPS = 64, 128, 256, 64
FULL_GRAPHS, FULL_NODES, FULL_EDGES, FULL_ITERATIONS = 256, 256, 512, 10
HUBER = 3.0


def workload(graphs=GRAPHS, nodes=NODES, edges=EDGES, distinct=8):
    """`distinct` graphs (a chain and chords, scales 0.8 .. 1.25, the start 0.05 rad, 0.1 m and 0.05 in the log-scale off the
    truth), repeated: (s, R, t, edge_index, s_meas, R_meas, t_meas, information, fixed, edge_valid) on the GPU"""
    pairs = G.chain(nodes) + G.chords(nodes, edges - (nodes - 1))
    s = [G.make_graph(800 + i, nodes, pairs) for i in range(min(distinct, graphs))]
    pick = [i % len(s) for i in range(graphs)]
    return [torch.from_numpy(np.ascontiguousarray(np.stack([s[i][k] for i in pick]))).to(DEV) for k in G.CALL]


def torch_linearise(s, R, t, ei, zs, zr, zt, info, fixed, valid, huber):
    """(diag (B, N, 7, 7), off (B, E, 7, 7), g (B, N, 7), live (B, N)) from stock torch ops, float32.  Log without the branch
    towards pi: every residual rotation of these graphs is far below 154 degrees."""
    B, N = R.shape[:2]
    E = ei.shape[1]
    i, j = ei[..., 0].long(), ei[..., 1].long()
    act = valid & (i != j) & (i >= 0) & (i < N) & (j >= 0) & (j < N) & torch.isfinite(zr).all((2, 3)) & torch.isfinite(zt).all(2) \
        & torch.isfinite(info).all((2, 3)) & torch.isfinite(zs) & (zs > 0)
    i, j = torch.where(act, i, torch.zeros_like(i)), torch.where(act, j, torch.ones_like(j))
    zr, zt, info = (torch.where(act.view(B, E, *([1] * (a.dim() - 2))), a, torch.zeros_like(a)) for a in (zr, zt, info))
    zs = torch.where(act, zs, torch.ones_like(zs))
    bi = torch.arange(B, device=R.device)[:, None]
    si, Ri, ti, sj, Rj, tj = s[bi, i], R[bi, i], t[bi, i], s[bi, j], R[bi, j], t[bi, j]
    Rp = Rj @ Ri.transpose(-1, -2)
    Rd = Rp @ zr.transpose(-1, -2)
    sp = sj / si
    sd = sp / zs
    u = sd[..., None] * (Rd @ zt[..., None])[..., 0]
    td = tj - sp[..., None] * (Rp @ ti[..., None])[..., 0] - u
    v = 0.5 * torch.stack([Rd[..., 2, 1] - Rd[..., 1, 2], Rd[..., 0, 2] - Rd[..., 2, 0], Rd[..., 1, 0] - Rd[..., 0, 1]], -1)
    sn = v.norm(dim=-1)
    theta = torch.atan2(sn, 0.5 * (Rd.diagonal(dim1=-2, dim2=-1).sum(-1) - 1))
    phi = torch.where(sn < 1e-4, 1 + sn * sn / 6, theta / sn.clamp_min(1e-30))[..., None] * v
    th2 = (phi * phi).sum(-1)
    h = 0.5 * th2.sqrt()
    k = torch.where(th2 < 0.0625, 1 / 12 + th2 / 720 + th2 * th2 / 30240, (1 - h * torch.cos(h) / torch.sin(h).clamp_min(1e-30)) / th2.clamp_min(1e-30))
    eye = torch.eye(3, device=R.device)
    jl = eye - 0.5 * P6._hat(phi) + k[..., None, None] * (phi[..., :, None] * phi[..., None, :] - th2[..., None, None] * eye)
    Ji, Jj = torch.zeros(B, E, 7, 7, device=R.device), torch.zeros(B, E, 7, 7, device=R.device)
    Jj[..., :3, :3], Jj[..., 3:6, :3], Jj[..., 3:6, 3:6], Jj[..., 3:6, 6], Jj[..., 6, 6] = jl, -P6._hat(td), eye, td, 1.0
    Ji[..., :3, :3], Ji[..., 3:6, :3], Ji[..., 3:6, 3:6], Ji[..., 3:6, 6], Ji[..., 6, 6] = -(jl @ Rp), -(P6._hat(u) @ Rp), -sp[..., None, None] * Rp, u, -1.0
    O = info.triu() + info.triu(1).transpose(-1, -2)
    e = torch.cat([phi, td, torch.log(sd)[..., None]], -1)
    oe = (O @ e[..., None])[..., 0]
    chi = (e * oe).sum(-1).clamp_min(0).sqrt()
    w = torch.where((chi > huber) & (huber > 0), huber / chi.clamp_min(1e-30), torch.ones_like(chi)) * act
    wz = w[..., None, None]
    Hii, Hjj, Hij = wz * (Ji.transpose(-1, -2) @ O @ Ji), wz * (Jj.transpose(-1, -2) @ O @ Jj), wz * (Ji.transpose(-1, -2) @ O @ Jj)
    gi, gj = w[..., None] * (Ji.transpose(-1, -2) @ oe[..., None])[..., 0], w[..., None] * (Jj.transpose(-1, -2) @ oe[..., None])[..., 0]
    flat_i, flat_j = (bi * N + i).reshape(-1), (bi * N + j).reshape(-1)
    diag = torch.zeros(B * N, 49, device=R.device).index_add_(0, flat_i, Hii.reshape(-1, 49)).index_add_(0, flat_j, Hjj.reshape(-1, 49))
    g = torch.zeros(B * N, 7, device=R.device).index_add_(0, flat_i, gi.reshape(-1, 7)).index_add_(0, flat_j, gj.reshape(-1, 7))
    deg = torch.zeros(B * N, device=R.device).index_add_(0, flat_i, act.float().reshape(-1)).index_add_(0, flat_j, act.float().reshape(-1))
    live = (deg.view(B, N) > 0) & ~fixed
    diag = diag.view(B, N, 7, 7) * live[..., None, None]
    g = g.view(B, N, 7) * live[..., None]
    off = Hij * (~(fixed[bi, i] | fixed[bi, j]))[..., None, None]
    return diag, off, g, live


def system_deviation(a, huber):
    diag, off, g, _ = ops.simgraph_linearise(*a, huber)
    d_t, o_t, g_t, _ = torch_linearise(*a, huber)
    scale = diag.abs().amax((1, 2, 3))
    return tuple(float(((x - y).abs().flatten(1).amax(1) / scale).max()) for x, y in ((diag, d_t), (off, o_t), (g, g_t)))


def test_torch_formulation_computes_the_same_system():
    """the yardstick's diag, off and g are mi_simgraph_linearise's within the linearise tolerance of tests/test_gpu_simgraph.py
    (float32 both, another summation order) on a ragged batch: every kind of inactive edge, fixed nodes, Huber weights"""
    w = G.graphs("ragged")
    a = G.state(w)
    dd, do, dg = system_deviation(a, w["huber"])
    print(f"ragged: diag {dd:.2e}, off {do:.2e}, g {dg:.2e} of max |diag|")
    assert max(dd, do, dg) <= G.LIN_TOL


def test_one_step_on_64_graphs_is_timed_and_linearises_the_formulations_system():
    a = workload()
    a6 = P6.workload()
    hip = time_ms(lambda: ops.simgraph_refine(*a, 1, TRIPS, HUBER))
    lin = time_ms(lambda: ops.simgraph_linearise(*a, HUBER))
    lin6 = time_ms(lambda: ops.pgo_linearise(*a6, HUBER))
    cost = time_ms(lambda: ops.simgraph_cost(*a[:8], a[9], HUBER))
    ref = time_ms(lambda: torch_linearise(*a, HUBER))
    out = ops.simgraph_refine(*a, 1, TRIPS, HUBER)
    print(f"{GRAPHS} graphs x {NODES} nodes x {EDGES} edges: HIP mi_simgraph_refine, one step of {TRIPS} PCG trips, {hip:.3f} ms; "
          f"mi_simgraph_linearise {lin:.3f} ms ({lin / lin6:.2f}x mi_pgo_linearise's {lin6:.3f} ms); mi_simgraph_cost {cost:.3f} ms; "
          f"the torch-on-GPU linearisation alone {ref:.3f} ms ({ref / lin:.1f}x mi_simgraph_linearise); "
          f"cost {float(out[4].mean()):.0f} -> {float(out[5].mean()):.0f}")
    assert out[8].all() and (out[5] < out[4]).all()
    dd, do, dg = system_deviation(a, HUBER)                 # the two timed linearisations give the same system on the timed tensors
    print(f"on the timed tensors: diag {dd:.2e}, off {do:.2e}, g {dg:.2e} of max |diag|")
    assert max(dd, do, dg) <= G.LIN_TOL
    assert lin < ref


def test_the_full_refine_is_timed():
    a = workload(FULL_GRAPHS, FULL_NODES, FULL_EDGES)
    ms = time_ms(lambda: ops.simgraph_refine(*a, FULL_ITERATIONS, TRIPS, HUBER), iters=5, warmup=2)
    out = ops.simgraph_refine(*a, FULL_ITERATIONS, TRIPS, HUBER)
    print(f"{FULL_GRAPHS} graphs x {FULL_NODES} nodes x {FULL_EDGES} edges: mi_simgraph_refine, {FULL_ITERATIONS} x {TRIPS}, {ms:.3f} ms "
          f"({FULL_GRAPHS / ms * 1e3:.0f} graphs/s, {ms / FULL_ITERATIONS:.3f} ms per iteration); accepted steps "
          f"{out[6].float().mean():.1f}, cost {float(out[4].mean()):.0f} -> {float(out[5].mean()):.1f}")
    assert out[8].all() and (out[5] < out[4]).all()
