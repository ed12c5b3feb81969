"""K25 rate: mi_ba_linearise on 256 windows x 8 frames x 512 landmarks -- the shape the geometry heads are quoted at -- beats a
torch-on-GPU formulation of the same undamped linearisation with its Schur complement (batched einsum, torch.linalg.inv of
the landmark blocks) followed by torch.linalg.solve of the reduced system, which the kernel does not even do in that entry.
That the formulation computes mi_ba_linearise's S and b is shown on a small ragged batch and on the timed tensors themselves.  The whole mi_ba_refine (10 iterations) on
the same batch is timed and printed.  Measured on an MI355X: see DESIGN.md, "K25"."""
import numpy as np
import torch

import test_gpu_ba as G
from gpu_common import DEV, GPU, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_ba_window

pytestmark = GPU
WINDOWS, FRAMES, LANDMARKS, ITERATIONS, NUM_FIXED = 256, 8, 512, 10, 1
HUBER = 2.0 / G.FOCAL


def workload(windows=WINDOWS, frames=FRAMES, landmarks=LANDMARKS, distinct=8):
    """`distinct` windows with 5 % outliers, repeated: (R, t, X, obs, vis) on the GPU"""
    s = [synth_ba_window(700 + i, frames, landmarks, 1.0, 0.5, 0.05, num_fixed=NUM_FIXED) for i in range(min(distinct, windows))]
    pick = [i % len(s) for i in range(windows)]
    R, t, X, kp, vis = (np.stack([s[i][j] for i in pick]) for j in range(5))
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (R, t, X, G.BO.normalise(kp, G.K), vis)]


def torch_linearise(R, t, X, obs, vis, nf, huber):
    """(S (B, n, n), b (B, n), dp (B, n)) for the free frames, n = 6 (F - nf), from stock torch ops, float32"""
    B, F, L = vis.shape
    act = vis.sum(1) >= 2
    m = (vis & act[:, None]).float()
    xc = torch.einsum("bfij,blj->bfli", R, X) + t[:, :, None]
    iz = 1.0 / xc[..., 2]
    xn, yn = xc[..., 0] * iz, xc[..., 1] * iz
    zero = torch.zeros_like(iz)
    Jp = torch.stack([torch.stack([-(xn * yn), 1 + xn * xn, -yn, iz, zero, -(xn * iz)], -1),
                      torch.stack([-(1 + yn * yn), xn * yn, xn, zero, iz, -(yn * iz)], -1)], -2)               # (B, F, L, 2, 6)
    A = torch.stack([torch.stack([iz, zero, -(xn * iz)], -1), torch.stack([zero, iz, -(yn * iz)], -1)], -2)      # (B, F, L, 2, 3)
    Jx = torch.einsum("bflij,bfjk->bflik", A, R)
    r = torch.stack([xn, yn], -1) - obs
    r = torch.where(vis[..., None], r, torch.zeros_like(r))                     # unseen entries may hold anything
    e = r.norm(dim=-1)
    w = torch.where((e > huber) & (huber > 0), huber / e.clamp_min(1e-30), torch.ones_like(e)) * m
    V = torch.einsum("bfl,bflki,bflkj->blij", w, Jx, Jx)
    h = torch.einsum("bfl,bflki,bflk->bli", w, Jx, r)
    Jp, Jx, w, r = Jp[:, nf:], Jx[:, nf:], w[:, nf:], r[:, nf:]
    U = torch.einsum("bfl,bflki,bflkj->bfij", w, Jp, Jp)
    g = torch.einsum("bfl,bflki,bflk->bfi", w, Jp, r)
    W = torch.einsum("bfl,bflki,bflkj->bflij", w, Jp, Jx)
    eye = torch.eye(3, device=R.device).expand(B, L, 3, 3)
    Vi = torch.linalg.inv(torch.where(act[..., None, None], V, eye)) * act[..., None, None].float()
    Y = torch.einsum("bflic,blcd->bflid", W, Vi)
    n = 6 * (F - nf)
    S = -torch.einsum("bflic,bgljc->bfigj", Y, W)                               # (B, F', 6, F', 6)
    idx = torch.arange(F - nf, device=R.device)
    S[:, idx, :, idx, :] = S[:, idx, :, idx, :] + U.permute(1, 0, 2, 3)         # the diagonal blocks
    S = S.reshape(B, n, n)
    b = (g - torch.einsum("bflic,blc->bfi", Y, h)).reshape(B, n)
    return S, b, torch.linalg.solve(S, -b)


def test_torch_formulation_computes_the_same_system():
    """the yardstick's S and b are mi_ba_linearise's within the linearise tolerance of tests/test_gpu_ba.py (float32 both,
    another summation order and another 3x3 inverse)"""
    R, t, X, obs, vis = workload(3, 6, 130, distinct=3)
    vis = vis.clone()
    vis[:, 2, ::5] = False
    vis[:, 1:, 7] = False                                                       # an inactive landmark
    s, b, _ = ops.ba_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER)
    S_t, b_t, dp = torch_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER)
    n0 = 6 * NUM_FIXED
    scale = s.diagonal(dim1=1, dim2=2).abs().amax(1)
    ds = ((s[:, n0:, n0:] - S_t).abs().amax((1, 2)) / scale).max()
    db = ((b[:, n0:] - b_t).abs().amax(1) / scale).max()
    print(f"S {float(ds):.2e}, b {float(db):.2e} of max |diag S|")
    assert ds <= G.LIN_TOL and db <= G.LIN_TOL and torch.isfinite(dp).all()


def test_hip_linearise_beats_torch_on_gpu_for_256_windows():
    R, t, X, obs, vis = workload()
    hip = time_ms(lambda: ops.ba_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER))
    ref = time_ms(lambda: torch_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER))
    cost = time_ms(lambda: ops.ba_cost(R, t, X, obs, vis, HUBER))
    refine = time_ms(lambda: ops.ba_refine(R, t, X, obs, vis, NUM_FIXED, ITERATIONS, HUBER))
    out = ops.ba_refine(R, t, X, obs, vis, NUM_FIXED, ITERATIONS, HUBER)
    print(f"{WINDOWS} windows x {FRAMES} frames x {LANDMARKS} landmarks: HIP mi_ba_linearise {hip:.3f} ms, torch-on-GPU einsum + "
          f"linalg linearisation, Schur complement and solve {ref:.3f} ms ({ref / hip:.1f}x); mi_ba_cost {cost:.3f} ms; mi_ba_refine, "
          f"{ITERATIONS} iterations, {refine:.3f} ms ({WINDOWS / refine * 1e3:.0f} windows/s, {refine / ITERATIONS:.3f} ms per iteration); "
          f"accepted steps {out[6].float().mean():.1f}, cost {float(out[4].mean() * G.FOCAL ** 2):.0f} -> {float(out[5].mean() * G.FOCAL ** 2):.0f} px^2")
    assert out[8].all() and (out[5] < out[4]).all()
    # the two timed calls compute the same system on the timed tensors
    s, b, _ = ops.ba_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER)
    S_t, b_t, _ = torch_linearise(R, t, X, obs, vis, NUM_FIXED, HUBER)
    n0 = 6 * NUM_FIXED
    scale = s.diagonal(dim1=1, dim2=2).abs().amax(1)
    ds = ((s[:, n0:, n0:] - S_t).abs().amax((1, 2)) / scale).max()
    db = ((b[:, n0:] - b_t).abs().amax(1) / scale).max()
    print(f"on the timed tensors: S {float(ds):.2e}, b {float(db):.2e} of max |diag S|")
    assert ds <= G.LIN_TOL and db <= G.LIN_TOL
    assert hip < ref
