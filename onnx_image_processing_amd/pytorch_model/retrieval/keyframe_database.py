"""KeyframeDatabase -- "which of the keyframes I have already seen is this frame?": the retrieval step loop closure and
relocalisation both start with, between `SparseBAD.forward_bits`, which produces the packed descriptors, and the pose
estimators of `pytorch_model.geometry`, which consume matched keypoints.  A brute-force, exact vote of the query's
descriptors against every stored keyframe (nearest neighbour within a Hamming distance, Lowe's ratio test against the second
nearest) where a host would keep a bag-of-words index (DBoW2) and call cv2.BFMatcher.knnMatch.  K26: `mi_place_votes`,
`mi_place_select`; the semantics are stated in include/mi355x_match.h.  The reference has no counterpart (its roadmap lists
loop closure detection and relocalisation as open)."""
import torch
from torch import nn

from ... import ops


class KeyframeDatabase(nn.Module):
    """capacity keyframes of max_keypoints descriptors of num_bits (256 / 512) bits in preallocated buffers (`bits`
    (capacity, K, num_bits / 32) int32, `valid` (capacity, K) bool, `keypoints` (capacity, K, 2) float32: move them with
    .to(device)) and a host-side `size`.

    add(bits, keypoints) -> the new keyframes' indices; query(bits, keypoints, exclude_recent=0) -> (cand_index (Q, C),
    cand_votes (Q, C), votes (Q, size)); match(bits, keypoints, cand_index) -> (keypoints_query (Q * C, Kq, 2), keypoints_db
    (Q * C, Kq, 2), valid (Q * C, Kq)), what RelativePoseEstimator, TwoViewPoseEstimator, HomographyEstimator and, with the
    depth frames, RgbdPoseEstimator take.  A descriptor is valid where its keypoint's first coordinate is >= 0 (top-k's
    convention for empty slots).

    max_distance: the largest Hamming distance of a vote (None: num_bits // 4); ratio: nearest < ratio * second nearest;
    min_votes: fewer votes make no candidate; num_candidates: C."""

    def __init__(self, capacity: int, max_keypoints: int, num_bits: int = 256, max_distance: int | None = None, ratio: float = 0.8,
                 min_votes: int = 20, num_candidates: int = 4) -> None:
        super().__init__()
        if not 1 <= capacity <= ops.PLACE_MAX_KEYFRAMES:
            raise ValueError(f"capacity must be in 1 .. {ops.PLACE_MAX_KEYFRAMES}, got {capacity}")
        if not 1 <= max_keypoints <= ops.PLACE_MAX_DESCRIPTORS:
            raise ValueError(f"max_keypoints must be in 1 .. {ops.PLACE_MAX_DESCRIPTORS}, got {max_keypoints}")
        if num_bits not in (256, 512):
            raise ValueError(f"num_bits must be 256 or 512, got {num_bits}")
        if max_distance is None:
            max_distance = num_bits // 4
        if not 0 <= max_distance <= num_bits:
            raise ValueError(f"max_distance must be in 0 .. {num_bits}, got {max_distance}")
        if not 0.0 < ratio <= 1.0:
            raise ValueError(f"ratio must be in (0, 1], got {ratio}")
        if min_votes < 0:
            raise ValueError(f"min_votes must not be negative, got {min_votes}")
        if not 1 <= num_candidates <= ops.PLACE_MAX_CANDIDATES:
            raise ValueError(f"num_candidates must be in 1 .. {ops.PLACE_MAX_CANDIDATES}, got {num_candidates}")
        self.capacity, self.max_keypoints, self.num_bits = int(capacity), int(max_keypoints), int(num_bits)
        self.max_distance, self.ratio = int(max_distance), float(ratio)
        self.min_votes, self.num_candidates = int(min_votes), int(num_candidates)
        self.size = 0
        self.register_buffer("bits", torch.zeros((capacity, max_keypoints, num_bits // 32), dtype=torch.int32))
        self.register_buffer("valid", torch.zeros((capacity, max_keypoints), dtype=torch.bool))
        self.register_buffer("keypoints", torch.full((capacity, max_keypoints, 2), -1.0, dtype=torch.float32))

    def reset(self) -> None:
        self.size = 0

    def _frames(self, bits: torch.Tensor, keypoints: torch.Tensor, what: str):
        if bits.dim() != 3 or bits.shape[2] != self.num_bits // 32 or bits.dtype != torch.int32:
            raise RuntimeError(f"{what}: bits must be (frames, K, {self.num_bits // 32}) int32, got {tuple(bits.shape)} {bits.dtype}")
        if tuple(keypoints.shape) != (bits.shape[0], bits.shape[1], 2):
            raise RuntimeError(f"{what}: keypoints must be ({bits.shape[0]}, {bits.shape[1]}, 2), got {tuple(keypoints.shape)}")
        if not bits.is_cuda or not keypoints.is_cuda:
            raise RuntimeError(f"{what}: bits and keypoints must live on the GPU; this package has no CPU path")
        return bits, keypoints.float(), keypoints[..., 0] >= 0

    @torch.no_grad()
    def add(self, bits: torch.Tensor, keypoints: torch.Tensor) -> torch.Tensor:
        b, kp, valid = self._frames(bits, keypoints, "add")
        if b.shape[1] != self.max_keypoints:
            raise RuntimeError(f"add: keyframes hold {self.max_keypoints} keypoints, got {b.shape[1]}")
        count = int(b.shape[0])
        if self.size + count > self.capacity:
            raise RuntimeError(f"add: the database is full ({self.size} of {self.capacity} keyframes, {count} more)")
        lo, hi = self.size, self.size + count
        self.bits[lo:hi] = b
        self.valid[lo:hi] = valid
        self.keypoints[lo:hi] = kp
        self.size = hi
        return torch.arange(lo, hi, dtype=torch.int64, device=self.bits.device)

    @torch.no_grad()
    def query(self, bits: torch.Tensor, keypoints: torch.Tensor, exclude_recent: int = 0):
        b, _, valid = self._frames(bits, keypoints, "query")
        if exclude_recent < 0:
            raise RuntimeError(f"query: exclude_recent must not be negative, got {exclude_recent}")
        if self.size == 0:
            raise RuntimeError("query: the database is empty")
        n, q = self.size, int(b.shape[0])
        votes = ops.place_votes(self.bits[:n], self.valid[:n], b, valid, self.max_distance, self.ratio)
        lo = hi = None
        if exclude_recent > 0:
            lo = torch.full((q,), max(0, n - int(exclude_recent)), dtype=torch.int32, device=b.device)
            hi = torch.full((q,), n, dtype=torch.int32, device=b.device)
        cand_index, cand_votes = ops.place_select(votes, self.num_candidates, self.min_votes, lo, hi)
        return cand_index, cand_votes, votes

    @torch.no_grad()
    def match(self, bits: torch.Tensor, keypoints: torch.Tensor, cand_index: torch.Tensor):
        b, kp, valid = self._frames(bits, keypoints, "match")
        q, kq = int(b.shape[0]), int(b.shape[1])
        if cand_index.dim() != 2 or cand_index.shape[0] != q:
            raise RuntimeError(f"match: cand_index must be ({q}, C), got {tuple(cand_index.shape)}")
        if self.size == 0:
            raise RuntimeError("match: the database is empty")
        n, c = self.size, int(cand_index.shape[1])
        _, nn_index, _, nn_vote = ops.place_votes(self.bits[:n], self.valid[:n], b, valid, self.max_distance, self.ratio,
                                                  frame_index=cand_index, want_matches=True)
        frames = self.keypoints[cand_index.clamp(min=0).long()]                           # (Q, C, Kd, 2)
        picked = torch.gather(frames, 2, nn_index.clamp(min=0).long().unsqueeze(-1).expand(q, c, kq, 2))
        kp_db = torch.where((nn_index >= 0).unsqueeze(-1), picked, torch.full_like(picked, -1.0))
        kp_q = kp.unsqueeze(1).expand(q, c, kq, 2).contiguous()
        return kp_q.view(q * c, kq, 2), kp_db.view(q * c, kq, 2), nn_vote.reshape(q * c, kq)
