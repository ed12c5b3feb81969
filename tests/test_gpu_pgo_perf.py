"""K27 rate: mi_pgo_linearise on 64 graphs x 128 nodes x 256 edges beats a torch-on-GPU formulation of the same undamped
linearisation (batched residuals, lines and blocks from stock torch ops, index_add over the nodes); that the formulation
computes mi_pgo_linearise's system is shown on a small ragged batch and on the timed tensors themselves.  One damped step
(mi_pgo_refine with iterations = 1, 64 PCG trips) on the same batch and the whole mi_pgo_refine (10 x 64) on 256 graphs x 256
nodes x 512 edges are timed and printed; no earlier path exists to compare them with.  The comparison of the whole step with
a dense scatter + torch.linalg.cholesky + cholesky_solve formulation is not here: that formulation aborted inside torch's
batched Cholesky solve at (64, 768, 768) on the MI355X it was tried on ("K27").  Measured: see DESIGN.md, "K27"."""
import numpy as np
import torch

import test_gpu_pgo as G
from gpu_common import DEV, GPU, time_ms
from onnx_image_processing_amd import ops

pytestmark = GPU
GRAPHS, NODES, EDGES, TRIPS = 64, 128, 256, 64
FULL_GRAPHS, FULL_NODES, FULL_EDGES, FULL_ITERATIONS = 256, 256, 512, 10
HUBER = 3.0


def workload(graphs=GRAPHS, nodes=NODES, edges=EDGES, distinct=8):
    """`distinct` graphs (a chain and chords, the start 0.05 rad and 0.1 m off the truth), repeated:
    (R, t, edge_index, R_meas, t_meas, information, fixed, edge_valid) on the GPU"""
    pairs = G.chain(nodes) + G.chords(nodes, edges - (nodes - 1))
    s = [G.make_graph(800 + i, nodes, pairs) for i in range(min(distinct, graphs))]
    pick = [i % len(s) for i in range(graphs)]
    return [torch.from_numpy(np.ascontiguousarray(np.stack([s[i][k] for i in pick]))).to(DEV)
            for k in ("R0", "t0", "ei", "zr", "zt", "info", "fixed", "valid")]


def _hat(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack([torch.stack([z, -v[..., 2], v[..., 1]], -1), torch.stack([v[..., 2], z, -v[..., 0]], -1),
                        torch.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def torch_linearise(R, t, ei, zr, zt, info, fixed, valid, huber):
    """(diag (B, N, 6, 6), off (B, E, 6, 6), g (B, N, 6), live (B, N)) from stock torch ops, float32.  Log without the branch
    towards pi: every residual rotation of these graphs is far below 154 degrees."""
    B, N = R.shape[:2]
    E = ei.shape[1]
    i, j = ei[..., 0].long(), ei[..., 1].long()
    act = valid & (i != j) & (i >= 0) & (i < N) & (j >= 0) & (j < N) & torch.isfinite(zr).all((2, 3)) & torch.isfinite(zt).all(2) \
        & torch.isfinite(info).all((2, 3))
    i, j = torch.where(act, i, torch.zeros_like(i)), torch.where(act, j, torch.ones_like(j))
    zr, zt, info = (torch.where(act.view(B, E, *([1] * (a.dim() - 2))), a, torch.zeros_like(a)) for a in (zr, zt, info))
    bi = torch.arange(B, device=R.device)[:, None]
    Ri, ti, Rj, tj = R[bi, i], t[bi, i], R[bi, j], t[bi, j]
    Rp = Rj @ Ri.transpose(-1, -2)
    Rd = Rp @ zr.transpose(-1, -2)
    u = (Rd @ zt[..., None])[..., 0]
    td = tj - (Rp @ ti[..., None])[..., 0] - u
    v = 0.5 * torch.stack([Rd[..., 2, 1] - Rd[..., 1, 2], Rd[..., 0, 2] - Rd[..., 2, 0], Rd[..., 1, 0] - Rd[..., 0, 1]], -1)
    s = v.norm(dim=-1)
    theta = torch.atan2(s, 0.5 * (Rd.diagonal(dim1=-2, dim2=-1).sum(-1) - 1))
    phi = torch.where(s < 1e-4, 1 + s * s / 6, theta / s.clamp_min(1e-30))[..., None] * v
    th2 = (phi * phi).sum(-1)
    h = 0.5 * th2.sqrt()
    k = torch.where(th2 < 0.0625, 1 / 12 + th2 / 720 + th2 * th2 / 30240, (1 - h * torch.cos(h) / torch.sin(h).clamp_min(1e-30)) / th2.clamp_min(1e-30))
    eye = torch.eye(3, device=R.device)
    jl = eye - 0.5 * _hat(phi) + k[..., None, None] * (phi[..., :, None] * phi[..., None, :] - th2[..., None, None] * eye)
    Ji, Jj = torch.zeros(B, E, 6, 6, device=R.device), torch.zeros(B, E, 6, 6, device=R.device)
    Jj[..., :3, :3], Jj[..., 3:, :3], Jj[..., 3:, 3:] = jl, -_hat(td), eye
    Ji[..., :3, :3], Ji[..., 3:, :3], Ji[..., 3:, 3:] = -(jl @ Rp), -(_hat(u) @ Rp), -Rp
    O = info.triu() + info.triu(1).transpose(-1, -2)
    e = torch.cat([phi, td], -1)
    oe = (O @ e[..., None])[..., 0]
    chi = (e * oe).sum(-1).clamp_min(0).sqrt()
    w = torch.where((chi > huber) & (huber > 0), huber / chi.clamp_min(1e-30), torch.ones_like(chi)) * act
    wz = w[..., None, None]
    Hii, Hjj, Hij = wz * (Ji.transpose(-1, -2) @ O @ Ji), wz * (Jj.transpose(-1, -2) @ O @ Jj), wz * (Ji.transpose(-1, -2) @ O @ Jj)
    gi, gj = w[..., None] * (Ji.transpose(-1, -2) @ oe[..., None])[..., 0], w[..., None] * (Jj.transpose(-1, -2) @ oe[..., None])[..., 0]
    flat_i, flat_j = (bi * N + i).reshape(-1), (bi * N + j).reshape(-1)
    diag = torch.zeros(B * N, 36, device=R.device).index_add_(0, flat_i, Hii.reshape(-1, 36)).index_add_(0, flat_j, Hjj.reshape(-1, 36))
    g = torch.zeros(B * N, 6, device=R.device).index_add_(0, flat_i, gi.reshape(-1, 6)).index_add_(0, flat_j, gj.reshape(-1, 6))
    deg = torch.zeros(B * N, device=R.device).index_add_(0, flat_i, act.float().reshape(-1)).index_add_(0, flat_j, act.float().reshape(-1))
    live = (deg.view(B, N) > 0) & ~fixed
    diag = diag.view(B, N, 6, 6) * live[..., None, None]
    g = g.view(B, N, 6) * live[..., None]
    off = Hij * (~(fixed[bi, i] | fixed[bi, j]))[..., None, None]
    return diag, off, g, live


def system_deviation(a, huber):
    diag, off, g, _ = ops.pgo_linearise(*a, huber)
    d_t, o_t, g_t, _ = torch_linearise(*a, huber)
    scale = diag.abs().amax((1, 2, 3))
    return tuple(float(((x - y).abs().flatten(1).amax(1) / scale).max()) for x, y in ((diag, d_t), (off, o_t), (g, g_t)))


def test_torch_formulation_computes_the_same_system():
    """the yardstick's diag, off and g are mi_pgo_linearise's within the linearise tolerance of tests/test_gpu_pgo.py (float32
    both, another summation order) on a ragged batch: every kind of inactive edge, fixed nodes, Huber weights"""
    w = G.graphs("ragged")
    a = G.gpu(w["R0"], w["t0"], w["ei"], w["zr"], w["zt"], w["info"], w["fixed"], w["valid"])
    dd, do, dg = system_deviation(a, w["huber"])
    print(f"ragged: diag {dd:.2e}, off {do:.2e}, g {dg:.2e} of max |diag|")
    assert max(dd, do, dg) <= G.LIN_TOL


def test_one_step_on_64_graphs_is_timed_and_linearises_the_formulations_system():
    a = workload()
    hip = time_ms(lambda: ops.pgo_refine(*a, 1, TRIPS, HUBER))
    lin = time_ms(lambda: ops.pgo_linearise(*a, HUBER))
    cost = time_ms(lambda: ops.pgo_cost(*a[:6], a[7], HUBER))
    ref = time_ms(lambda: torch_linearise(*a, HUBER))
    out = ops.pgo_refine(*a, 1, TRIPS, HUBER)
    print(f"{GRAPHS} graphs x {NODES} nodes x {EDGES} edges: HIP mi_pgo_refine, one step of {TRIPS} PCG trips, {hip:.3f} ms; "
          f"mi_pgo_linearise {lin:.3f} ms; mi_pgo_cost {cost:.3f} ms; the torch-on-GPU linearisation alone {ref:.3f} ms "
          f"({ref / lin:.1f}x mi_pgo_linearise); cost {float(out[3].mean()):.0f} -> {float(out[4].mean()):.0f}")
    assert out[7].all() and (out[4] < out[3]).all()
    dd, do, dg = system_deviation(a, HUBER)                 # the two timed linearisations give the same system on the timed tensors
    print(f"on the timed tensors: diag {dd:.2e}, off {do:.2e}, g {dg:.2e} of max |diag|")
    assert max(dd, do, dg) <= G.LIN_TOL
    assert lin < ref


def test_the_full_refine_is_timed():
    a = workload(FULL_GRAPHS, FULL_NODES, FULL_EDGES)
    ms = time_ms(lambda: ops.pgo_refine(*a, FULL_ITERATIONS, TRIPS, HUBER), iters=5, warmup=2)
    out = ops.pgo_refine(*a, FULL_ITERATIONS, TRIPS, HUBER)
    print(f"{FULL_GRAPHS} graphs x {FULL_NODES} nodes x {FULL_EDGES} edges: mi_pgo_refine, {FULL_ITERATIONS} x {TRIPS}, {ms:.3f} ms "
          f"({FULL_GRAPHS / ms * 1e3:.0f} graphs/s, {ms / FULL_ITERATIONS:.3f} ms per iteration); accepted steps "
          f"{out[5].float().mean():.1f}, cost {float(out[3].mean()):.0f} -> {float(out[4].mean()):.1f}")
    assert out[7].all() and (out[4] < out[3]).all()
