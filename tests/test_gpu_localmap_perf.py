"""K29 rate: mi_localmap_match on 256 frames x 2048 landmarks x 1024 keypoints x 256 bits at a radius of 40 px beats a
torch-on-GPU formulation of the same outputs (a batched float64 projection, a (B, L, K) distance mask, Hamming distances by a
matrix product on the unpacked bits, a masked two-smallest by topk, scatter_reduce(amin) for the claims); that the formulation
computes mi_localmap_match's outputs is shown first, on a small ragged batch and on the timed tensors themselves.
mi_localmap_descriptors on 256 x 8 frames x 512 keypoints x 512 slots is timed and printed; no earlier path exists to compare it
with.  Measured: see DESIGN.md, "K29"."""
import functools

import numpy as np
import torch

import test_gpu_localmap as G
from gpu_common import GPU_PERF, gpu, time_ms
from onnx_image_processing_amd import ops

pytestmark = GPU_PERF
FRAMES, LANDMARKS, KEYPOINTS, NUM_BITS, RADIUS = 256, 2048, 1024, 256, 40.0
BIG = 0x7FFFFFFF


def small_batch():
    return G._ragged_batch()


@functools.lru_cache(maxsize=None)
def distinct_cases(distinct=4):
    return tuple(G.random_case(700 + i, LANDMARKS, KEYPOINTS, NUM_BITS, radius=RADIUS) for i in range(distinct))


def batch_tensors(cases, repeat=1):
    """(the nine arrays on the GPU, the seven scalars) of a batch made of `cases`, each `repeat` times in turn"""
    pick = [cases[i % len(cases)] for i in range(len(cases) * repeat)]
    arrays = []
    for k in G.ARRAYS:
        rows = "points" if k == "point_valid" else "kp"
        arrays.append(None if all(c[k] is None for c in pick) else
                      gpu(np.stack([np.ones(len(c[rows]), bool) if c[k] is None else c[k] for c in pick])))
    c = cases[0]
    return arrays, (c["height"], c["width"], c["min_depth"], c["max_depth"], c["radius"], c["max_distance"], c["ratio"])


def _unpack(bits):
    """(B, N, W) int32 -> (B, N, 32 W) float32 of 0 / 1"""
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[..., None] >> shifts) & 1).reshape(*bits.shape[:2], -1).float()


def torch_match(points, point_valid, rep_bits, r, t, cam, kp, kp_valid, kp_bits, height, width, min_depth, max_depth, radius, max_distance, ratio):
    """mi_localmap_match's seven outputs from stock torch ops; every float64 operation is a kernel of its own, so nothing is fused"""
    B, L, _ = points.shape
    K = kp.shape[1]
    A = 32 * rep_bits.shape[-1] + 1
    dev = points.device
    X, R, T, C = points.double(), r.double(), t.double(), cam.double()
    lo, hi, rad = (float(np.float32(v)) for v in (min_depth, max_depth, radius))
    q = [((R[:, i, 0:1] * X[..., 0] + R[:, i, 1:2] * X[..., 1]) + R[:, i, 2:3] * X[..., 2]) + T[:, i:i + 1] for i in range(3)]
    z = q[2]
    u, v = C[:, 0:1] * (q[0] / z) + C[:, 2:3], C[:, 1:2] * (q[1] / z) + C[:, 3:4]
    view = torch.isfinite(q[0]) & torch.isfinite(q[1]) & torch.isfinite(z) & (z >= lo) & (z <= hi) & (u >= 0) & (u <= width - 1) & (v >= 0) & (v <= height - 1)
    if point_valid is not None:
        view &= point_valid != 0
    du, dv = kp[:, None, :, 1].double() - u[:, :, None], kp[:, None, :, 0].double() - v[:, :, None]
    inside = (du * du + dv * dv <= rad * rad) & view[:, :, None]
    del du, dv
    if kp_valid is not None:
        inside &= (kp_valid != 0)[:, None, :]
    ua, ub = _unpack(rep_bits), _unpack(kp_bits)
    ham = (ua.sum(-1)[:, :, None] + ub.sum(-1)[:, None, :] - 2.0 * torch.bmm(ua, ub.transpose(1, 2))).int()
    key = torch.where(inside, ham << 16 | torch.arange(K, device=dev, dtype=torch.int32), BIG)
    del ham, inside
    if K == 1:
        key = torch.cat([key, torch.full_like(key, BIG)], -1)
    two = torch.topk(key, 2, dim=-1, largest=False).values
    k1, k2 = two[..., 0], two[..., 1]
    have = k1 < BIG
    d1, j1, d2 = torch.where(have, k1 >> 16, A), torch.where(have, k1 & 0xFFFF, -1), torch.where(k2 < BIG, k2 >> 16, A)
    cand = view & have & (d1 <= max_distance) & (d1.float() < ratio * d2.float())
    ls = torch.arange(L, device=dev, dtype=torch.int32)
    j1c = j1.clamp_min(0).long()
    claim = torch.full((B, K), BIG, dtype=torch.int32, device=dev).scatter_reduce(1, j1c, torch.where(cand, d1 << 16 | ls, BIG), "amin")
    kp_lm = torch.where(claim < BIG, claim & 0xFFFF, -1)
    kept = cand & (kp_lm.gather(1, j1c) == ls)
    state = torch.where(~view, 0, torch.where(~have, 1, torch.where(~cand, 2, torch.where(kept, 4, 3)))).to(torch.uint8)
    proj = torch.where(view[..., None], torch.stack([v, u], -1), -1.0).float()
    mk = torch.where(kept[..., None], kp.gather(1, j1c[..., None].expand(B, L, 2)), -1.0)
    counts = torch.stack([(state == s).sum(1) for s in range(5)], 1).int()
    return proj, state, torch.where(kept, j1, -1), torch.where(state >= 2, d1, A), mk, kp_lm, counts


def _same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_torch_formulation_computes_the_same_outputs():
    """the yardstick's outputs EQUAL mi_localmap_match's on the ragged batch (an item with nothing in view, crowded windows, twins)
    and on the hand-made windows"""
    arrays, scalars = batch_tensors(small_batch())
    assert _same(ops.localmap_match(*arrays, *scalars), torch_match(*arrays, *scalars))
    for name in ("gates", "border-in", "border-out", "radius-in", "radius-out", "tie", "single", "nearest-invalid", "claims", "1x1", "17x37"):
        arrays, scalars = batch_tensors([G.match_scene(name)])
        assert _same(ops.localmap_match(*arrays, *scalars), torch_match(*arrays, *scalars)), name


def test_match_on_256_frames_beats_the_torch_formulation():
    cases = distinct_cases()
    arrays, scalars = batch_tensors(cases, FRAMES // len(cases))
    assert tuple(arrays[0].shape) == (FRAMES, LANDMARKS, 3) and tuple(arrays[6].shape) == (FRAMES, KEYPOINTS, 2)
    hip = time_ms(lambda: ops.localmap_match(*arrays, *scalars))
    ref = time_ms(lambda: torch_match(*arrays, *scalars), iters=3, warmup=1)
    out = ops.localmap_match(*arrays, *scalars)
    assert _same(out, torch_match(*arrays, *scalars))                                        # the same result on the timed tensors
    want = [G.LO.match_vectorised(*G.oracle_args(c)) for c in cases]
    for i, o in enumerate(want):
        G.check_match(tuple(g[i].cpu().numpy() for g in out), o, i)
    window = float(np.mean([o["in_window"][o["lm_state"] > 0].mean() for o in want]))
    c = out[6].float().mean(0).tolist()
    rng = np.random.default_rng(5)
    bits = gpu(rng.integers(-(1 << 31), 1 << 31, (FRAMES, 8, 512, 8), dtype=np.int64).astype(np.int32))
    track_kp = gpu(rng.integers(-1, 512, (FRAMES, 8, 512), dtype=np.int64).astype(np.int32))
    desc = time_ms(lambda: ops.localmap_descriptors(bits, track_kp))
    print(f"{FRAMES} frames x {LANDMARKS} landmarks x {KEYPOINTS} keypoints x {NUM_BITS} bits, radius {RADIUS:.0f} px: HIP mi_localmap_match {hip:.3f} ms "
          f"({FRAMES / hip * 1e3:.0f} frames/s); the torch-on-GPU formulation {ref:.3f} ms ({ref / hip:.1f}x); {window:.1f} keypoints per window; "
          f"landmarks per state {[round(x, 1) for x in c]}; mi_localmap_descriptors on {FRAMES} x 8 x 512 x 512 slots {desc:.3f} ms")
    assert c[3] > 0 and c[4] > 100
    assert hip < ref
