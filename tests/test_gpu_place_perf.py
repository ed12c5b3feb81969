"""K26 rate: `mi_place_votes` for one query frame of 512 descriptors against 1 024 keyframes of 512 descriptors of 256 bits --
and for 8 such queries -- beats a torch-on-GPU formulation that is handed the UNPACKED 0 / 1 descriptors for nothing: a
batched matmul, pq + pd - 2 dot, torch.topk(2, largest=False), the vote and the sum.  That the formulation returns the
kernel's votes exactly is asserted on a small shape first and on the timed tensors afterwards.  Both times, the keyframes
per second and the share of `mi_place_select` are printed.  Measured on an MI355X: see DESIGN.md, "K26"."""
import numpy as np
import pytest
import torch

from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_place_descriptors

pytestmark = GPU_PERF
KEYFRAMES, DESCRIPTORS, BITS, MAX_DISTANCE, RATIO = 1024, 512, 256, 64, 0.8


def workload(queries, keyframes=KEYFRAMES, k=DESCRIPTORS, bits=BITS):
    """(db_bits (N, k, W), q_bits (Q, k, W)) on the GPU: query i revisits a keyframe of its own"""
    db = synth_place_descriptors(900, keyframes, k, bits, 0.1, 0.5)[0]
    q = np.stack([_revisit(db, 900 + i, k, bits) for i in range(queries)])
    return torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)


def _revisit(db, seed, k, bits):
    """a revisit of keyframe seed % N of `db`: half of its rows with 10 % of the bits flipped, the rest random"""
    rng = np.random.default_rng(seed)
    rows = db[seed % db.shape[0]].view(np.uint32).copy()
    flips = rng.random((k, bits)) < 0.1
    mask = (flips.reshape(k, bits // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    fresh = rng.integers(0, 1 << 32, size=rows.shape, dtype=np.uint64).astype(np.uint32)
    return np.where((rng.random(k) < 0.5)[:, None], rows ^ mask, fresh)[rng.permutation(k)].view(np.int32)


def unpack(bits):
    """(F, K, W) int32 -> (F, K, 32 W) float32 of 0 / 1"""
    shifts = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(-1) >> shifts) & 1).reshape(bits.shape[0], bits.shape[1], -1).float()


def torch_votes(db_u, q_u, max_distance, ratio):
    """votes (Q, N) from the unpacked descriptors, stock torch ops"""
    pd, out = db_u.sum(-1), []
    for qi in q_u:                                                               # a query at a time: (N, Kq, Kd) floats
        ham = qi.sum(-1)[None, :, None] + pd[:, None, :] - 2.0 * torch.matmul(qi.unsqueeze(0), db_u.transpose(1, 2))
        two = torch.topk(ham, 2, dim=2, largest=False).values
        out.append(((two[..., 0] <= max_distance) & (two[..., 0] < ratio * two[..., 1])).sum(1))
    return torch.stack(out).to(torch.int32)


def test_torch_formulation_returns_the_kernels_votes():
    db, q = workload(2, 40, 96)
    want = ops.place_votes(db, None, q, None, MAX_DISTANCE, RATIO)
    assert torch.equal(torch_votes(unpack(db), unpack(q), MAX_DISTANCE, RATIO), want) and int(want.max()) >= 20


@pytest.mark.parametrize("queries", [1, 8])
def test_hip_votes_beat_torch_on_gpu(queries):
    db, q = workload(queries)
    db_u, q_u = unpack(db), unpack(q)
    hip = time_ms(lambda: ops.place_votes(db, None, q, None, MAX_DISTANCE, RATIO))
    ref = time_ms(lambda: torch_votes(db_u, q_u, MAX_DISTANCE, RATIO))
    votes = ops.place_votes(db, None, q, None, MAX_DISTANCE, RATIO)
    both = time_ms(lambda: ops.place_select(ops.place_votes(db, None, q, None, MAX_DISTANCE, RATIO), 4, 20))
    select = time_ms(lambda: ops.place_select(votes, 4, 20))
    matches = time_ms(lambda: ops.place_votes(db, None, q, None, MAX_DISTANCE, RATIO, want_matches=True))
    pairs = queries * KEYFRAMES * DESCRIPTORS * DESCRIPTORS
    print(f"{queries} x {DESCRIPTORS} descriptors against {KEYFRAMES} keyframes x {DESCRIPTORS}, {BITS} bits: HIP mi_place_votes {hip:.3f} ms "
          f"({queries * KEYFRAMES / hip * 1e3:.0f} keyframes/s, {pairs / hip / 1e9:.2f} T descriptor pairs/s), torch-on-GPU matmul + topk "
          f"{ref:.3f} ms ({ref / hip:.1f}x); with every row's neighbour written {matches:.3f} ms; mi_place_select {select:.3f} ms, "
          f"{select / both:.1%} of votes + select ({both:.3f} ms)")
    assert torch.equal(torch_votes(db_u, q_u, MAX_DISTANCE, RATIO), votes)       # the two timed calls compute the same votes
    # the same shape at 512 bits: twice the MFMA work under the same epilogue, which tells the two apart
    db2, q2 = torch.cat([db, db.flip(2)], 2).contiguous(), torch.cat([q, q.flip(2)], 2).contiguous()
    wide = time_ms(lambda: ops.place_votes(db2, None, q2, None, 2 * MAX_DISTANCE, RATIO))
    print(f"512-bit descriptors, same shape: {wide:.3f} ms ({wide / hip:.2f}x the 256-bit time)")
    assert torch.equal(ops.place_votes(db2, None, q2, None, 2 * MAX_DISTANCE, RATIO), votes)   # every distance doubles: the same votes
    assert hip < ref
