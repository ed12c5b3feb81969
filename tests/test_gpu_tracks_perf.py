"""K28 rate: mi_tracks_build on 256 windows x 8 frames x 512 keypoints x 13 pairs x 512 matches beats a torch-on-GPU
formulation of the same result (min-label propagation by scatter_reduce(amin) with pointer jumping to a fixed point, bincount for
the lengths and the per-frame counts, one sort for the slot order); that the formulation computes mi_tracks_build's outputs is
shown first, on a small ragged batch and on the timed tensors themselves.  mi_tracks_triangulate on the tracks of the same
batch is timed and printed; no earlier path exists to compare it with.  Measured: see DESIGN.md, "K28"."""
import numpy as np
import torch

import test_gpu_tracks as G
from gpu_common import DEV, GPU, gpu, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_track_window

pytestmark = GPU
WINDOWS, FRAMES, KEYPOINTS, LANDMARKS, MAX_LANDMARKS, MIN_VIEWS = 256, 8, 512, 400, 512, 2


def workload(windows=WINDOWS, distinct=8):
    """`distinct` synth_track_window scenes (pair span 2: 13 pairs of 8 frames), repeated: (keypoints, pair_frames, match_ij,
    match_valid, R0, t0) on the GPU"""
    s = [synth_track_window(700 + i, FRAMES, KEYPOINTS, LANDMARKS) for i in range(min(distinct, windows))]
    pick = [i % len(s) for i in range(windows)]
    return [torch.from_numpy(np.ascontiguousarray(np.stack([s[i][k] for i in pick]))).to(DEV) for k in (0, 2, 3, 4, 5, 6)]


def torch_build(keypoints, pair_frames, match_ij, match_valid, kp_valid, min_views, L):
    """mi_tracks_build's six outputs from stock torch ops.  The label loop ends on torch.equal: one host round trip per round."""
    B, F, K, _ = keypoints.shape
    P, M = match_valid.shape[1:]
    N = F * K
    dev = keypoints.device
    a, b = (pair_frames[..., c].long()[:, :, None].expand(B, P, M) for c in (0, 1))
    i, j = match_ij[..., 0].long(), match_ij[..., 1].long()
    act = (match_valid != 0) & (a >= 0) & (a < F) & (b >= 0) & (b < F) & (a != b) & (i >= 0) & (i < K) & (j >= 0) & (j < K)
    u, v = torch.where(act, a * K + i, 0).view(B, -1), torch.where(act, b * K + j, 0).view(B, -1)
    act = act.view(B, -1)
    if kp_valid is not None:
        kv = (kp_valid != 0).view(B, N)
        act = act & kv.gather(1, u) & kv.gather(1, v)
    base = torch.arange(B, device=dev)[:, None] * N
    U, V = (torch.where(act, u, 0) + base).view(-1), (torch.where(act, v, 0) + base).view(-1)      # padding: the self-loop of node 0
    label = torch.arange(B * N, device=dev)
    while True:
        m = torch.minimum(label[U], label[V])
        new = label.scatter_reduce(0, U, m, "amin").scatter_reduce(0, V, m, "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    node = torch.arange(B * N, device=dev)
    frame = (node % N) // K
    count = torch.bincount(label, minlength=B * N)
    per_frame = torch.bincount(label * F + frame, minlength=B * N * F).view(B * N, F)
    root = label == node
    conflict = (per_frame > 1).any(1)
    eligible = (root & ~conflict & (count >= min_views)).view(B, N)
    cnt = count.view(B, N)
    key = torch.where(eligible, (F - cnt) * N + torch.arange(N, device=dev)[None], (F + 1) * N)
    order = key.argsort(1)[:, :L]                                                                 # (length descending, label ascending)
    kept = eligible.gather(1, order)
    slot_of = torch.full((B, N), -1, dtype=torch.long, device=dev)
    slot_of.scatter_(1, order, torch.where(kept, torch.arange(order.shape[1], device=dev)[None].expand_as(order), -1))
    slot = slot_of.view(-1)[label]
    kp_track = torch.where(conflict[label], -2, slot).view(B, F, K).int()
    seen = slot >= 0
    at = ((node // N) * F + frame) * L + slot.clamp_min(0)
    track_kp = torch.full((B * F * L,), -1, dtype=torch.int32, device=dev)
    track_kp[at[seen]] = (node % K).int()[seen]
    track_kp = track_kp.view(B, F, L)
    vis = track_kp >= 0
    track_keypoints = torch.where(vis[..., None], keypoints.gather(2, track_kp.clamp_min(0).long()[..., None].expand(B, F, L, 2)), 0.0)
    lengths = torch.where(kept, cnt.gather(1, order), 0).int()
    track_len = torch.zeros((B, L), dtype=torch.int32, device=dev)
    track_len[:, :lengths.shape[1]] = lengths
    n_el = eligible.sum(1)
    counts = torch.stack([(root & (count >= 2)).view(B, N).sum(1), (root & conflict).view(B, N).sum(1), n_el, n_el.clamp_max(L)], 1).int()
    return track_kp, vis, track_keypoints, track_len, kp_track, counts


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_torch_formulation_computes_the_same_tracks():
    """the yardstick's outputs EQUAL mi_tracks_build's on a ragged batch (conflicts, a cut at L, an all-padding window) and on
    the hand-made windows with reversed pairs, out-of-range indices and a kp_valid"""
    batch = G._ragged_batch()
    stack = lambda k: gpu(np.stack([w[k] for w in batch]))
    a = (stack("keypoints"), stack("pair_frames"), stack("match_ij"), stack("match_valid"))
    for L in (32, 8):
        assert _same(ops.tracks_build(*a, None, 2, L), torch_build(*a, None, 2, L))
    for name in ("padding", "repeats", "chain-conflict", "conflict-via-third", "chain16-reversed", "cut"):
        w = G.build_scene(name)
        a = gpu(w["keypoints"][None], w["pair_frames"][None], w["match_ij"][None], w["match_valid"][None])
        kv = None if w["kp_valid"] is None else gpu(w["kp_valid"][None])
        assert _same(ops.tracks_build(*a, kv, w["min_views"], w["L"]), torch_build(*a, kv, w["min_views"], w["L"])), name


def test_build_on_256_windows_beats_the_torch_formulation():
    kp, pf, ij, mv, R0, t0 = workload()
    assert tuple(ij.shape) == (WINDOWS, 13, KEYPOINTS, 2)
    hip = time_ms(lambda: ops.tracks_build(kp, pf, ij, mv, None, MIN_VIEWS, MAX_LANDMARKS))
    ref = time_ms(lambda: torch_build(kp, pf, ij, mv, None, MIN_VIEWS, MAX_LANDMARKS), iters=5, warmup=2)
    out = ops.tracks_build(kp, pf, ij, mv, None, MIN_VIEWS, MAX_LANDMARKS)
    assert _same(out, torch_build(kp, pf, ij, mv, None, MIN_VIEWS, MAX_LANDMARKS))             # the same result on the timed tensors
    obs = ops.normalise_keypoints(out[2], G.k_inv_gpu())
    tri = time_ms(lambda: ops.tracks_triangulate(R0, t0, obs, out[1], MIN_VIEWS, G.MAX_E2, G.MAX_COS))
    ok = ops.tracks_triangulate(R0, t0, obs, out[1], MIN_VIEWS, G.MAX_E2, G.MAX_COS)[1]
    c = out[5].float().mean(0).tolist()
    print(f"{WINDOWS} windows x {FRAMES} frames x {KEYPOINTS} keypoints x 13 pairs x {KEYPOINTS} matches: HIP mi_tracks_build {hip:.3f} ms "
          f"({WINDOWS / hip * 1e3:.0f} windows/s); the torch-on-GPU formulation {ref:.3f} ms ({ref / hip:.1f}x); mi_tracks_triangulate on its "
          f"{MAX_LANDMARKS} slots {tri:.3f} ms; per window {c[0]:.0f} components, {c[1]:.0f} conflicting, {c[2]:.0f} eligible, "
          f"{float(ok.float().sum(1).mean()):.0f} triangulated")
    assert c[1] > 0 and c[2] > 50 and ok.any()
    assert hip < ref
