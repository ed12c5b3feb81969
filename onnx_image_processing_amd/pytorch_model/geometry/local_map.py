"""LocalMapTracker -- the join between LandmarkTracks and AbsolutePoseEstimator: the tracking thread's step.  Every landmark
gets the descriptor of one of its observations; a new frame with a predicted pose is matched against the landmarks by
projecting each of them and searching a small window round the projection (ORB-SLAM's SearchByProjection in TrackLocalMap),
instead of matching the frame in full against an old keyframe and translating the matches back to landmarks on the host.
K29: `mi_localmap_descriptors`, `mi_localmap_match`; the definitions are stated in include/mi355x_match.h.  The
reference has no counterpart (its roadmap lists tracking against a map as open)."""
import torch
from torch import nn

from ... import ops


class LocalMapTracker(nn.Module):
    """describe(bits, track_kp) -> (rep_bits, rep_frame): bits (B, F, K, W) the packed hard bits of a window's frames (what
    SparseBAD.forward_bits returns per frame), track_kp (B, F, L) as LandmarkTracks returns it; rep_bits (B, L, W): per landmark
    slot the descriptor of the view with the smallest median Hamming distance to the slot's views, rep_frame (B, L): its frame,
    -1 for an empty slot.

    match(points, rep_bits, R, t, keypoints, bits, point_ok=None, radius_px=None) -> (keypoints2d, valid, lm_kp, kp_lm, proj,
    state, counts): points (B, L, 3) and point_ok (B, L) as LandmarkTracks returns them, the pose R (B, 3, 3), t (B, 3) with
    X_camera = R X + t, the frame's keypoints (B, K, 2) in pixel (y, x) order -- a keypoint is valid where its first coordinate
    is >= 0, top-k's convention -- and bits (B, K, W).  keypoints2d (B, L, 2) and valid (B, L) go into
    AbsolutePoseEstimator.forward(points, keypoints2d, valid); lm_kp (B, L): the keypoint a landmark was matched to or -1; kp_lm
    (B, K): the landmark a keypoint was matched to, -1 for the keypoints left over for new landmarks; proj (B, L, 2): the
    projection or (-1, -1); state (B, L): 0 not in view, 1 no keypoint in the window, 2 failed the distance or the ratio test, 3
    lost its keypoint to a nearer landmark, 4 matched; counts (B, 5): landmarks per state.

    forward(points, rep_bits, R_pred, t_pred, keypoints, bits, estimator, point_ok=None) -> (R, t, inlier_mask, ok, lm_kp, kp_lm,
    counts): match at radius_px with the predicted pose, solve with `estimator` (an AbsolutePoseEstimator), and where that is ok
    match again at refine_radius_px with the solved pose and solve again; where the first solve is not ok the predicted pose
    comes back with ok False, and where only the second fails the first solve does.  Unbatched input gives unbatched output.

    K: the 3x3 camera matrix; image_size (height, width); a landmark is searched when it projects inside the image at a depth
    in [min_depth, max_depth]; a match needs a Hamming distance of at most max_distance (None: num_bits // 4) that is below
    ratio times the second nearest in the window."""

    def __init__(self, K: torch.Tensor, image_size, num_bits: int = 256, radius_px: float = 40.0, refine_radius_px: float = 10.0,
                 max_distance: int | None = None, ratio: float = 0.8, min_depth: float = 0.1, max_depth: float = 100.0) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        try:
            height, width = (int(v) for v in image_size)
        except (TypeError, ValueError):
            raise ValueError(f"image_size must be (height, width), got {image_size!r}") from None
        if height < 1 or width < 1:
            raise ValueError(f"image_size must be positive, got {image_size!r}")
        if num_bits not in (256, 512):
            raise ValueError(f"num_bits must be 256 or 512, got {num_bits}")
        for name, value in (("radius_px", radius_px), ("refine_radius_px", refine_radius_px)):
            if not 0 < value < float("inf"):
                raise ValueError(f"{name} must be positive and finite, got {value}")
        if max_distance is None:
            max_distance = num_bits // 4
        if not 0 <= max_distance <= num_bits:
            raise ValueError(f"max_distance must be in 0 .. {num_bits}, got {max_distance}")
        if not 0.0 < ratio <= 1.0:
            raise ValueError(f"ratio must be in (0, 1], got {ratio}")
        if not 0 < min_depth < max_depth < float("inf"):
            raise ValueError(f"need 0 < min_depth < max_depth < inf, got {min_depth} and {max_depth}")
        if not (float(K_f[0, 0]) > 0 and float(K_f[1, 1]) > 0):
            raise ValueError(f"K must have positive focal lengths, got {float(K_f[0, 0])} and {float(K_f[1, 1])}")
        self.register_buffer("K", K_f)
        self.register_buffer("cam", torch.stack([K_f[0, 0], K_f[1, 1], K_f[0, 2], K_f[1, 2]]))
        self.height, self.width, self.num_bits = height, width, int(num_bits)
        self.radius_px, self.refine_radius_px = float(radius_px), float(refine_radius_px)
        self.max_distance, self.ratio = int(max_distance), float(ratio)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)

    @torch.no_grad()
    def describe(self, bits: torch.Tensor, track_kp: torch.Tensor):
        single = bits.dim() == 3
        if single:
            bits, track_kp = bits.unsqueeze(0), track_kp.unsqueeze(0)
        if bits.dim() != 4 or 32 * bits.shape[-1] != self.num_bits:
            raise RuntimeError(f"bits must be (B, F, K, {self.num_bits // 32}) or (F, K, {self.num_bits // 32}), got {tuple(bits.shape)}")
        rep_bits, rep_frame, _ = ops.localmap_descriptors(bits, track_kp)
        return (rep_bits[0], rep_frame[0]) if single else (rep_bits, rep_frame)

    def _match(self, points, rep_bits, R, t, keypoints, bits, point_ok, radius_px):
        if points.dim() != 3 or points.shape[-1] != 3 or keypoints.dim() != 3 or keypoints.shape[-1] != 2:
            raise RuntimeError(f"points must be (B, L, 3) or (L, 3) and keypoints (B, K, 2) or (K, 2), got {tuple(points.shape)} and "
                               f"{tuple(keypoints.shape)}")
        if 32 * rep_bits.shape[-1] != self.num_bits or 32 * bits.shape[-1] != self.num_bits:
            raise RuntimeError(f"descriptors must have {self.num_bits // 32} words, got {tuple(rep_bits.shape)} and {tuple(bits.shape)}")
        cam = self.cam.to(points.device).expand(points.shape[0], 4)
        proj, state, lm_kp, _, match_keypoints, kp_lm, counts = ops.localmap_match(
            points, point_ok, rep_bits, R, t, cam, keypoints, keypoints[..., 0] >= 0, bits, self.height, self.width, self.min_depth,
            self.max_depth, self.radius_px if radius_px is None else float(radius_px), self.max_distance, self.ratio)
        return match_keypoints, state == 4, lm_kp, kp_lm, proj, state, counts

    @torch.no_grad()
    def match(self, points: torch.Tensor, rep_bits: torch.Tensor, R: torch.Tensor, t: torch.Tensor, keypoints: torch.Tensor,
              bits: torch.Tensor, point_ok: torch.Tensor | None = None, radius_px: float | None = None):
        single = points.dim() == 2
        if single:
            points, rep_bits, R, t, keypoints, bits = (a.unsqueeze(0) for a in (points, rep_bits, R, t, keypoints, bits))
            point_ok = None if point_ok is None else point_ok.unsqueeze(0)
        res = self._match(points, rep_bits, R, t, keypoints, bits, point_ok, radius_px)
        return tuple(o[0] for o in res) if single else res

    @torch.no_grad()
    def forward(self, points: torch.Tensor, rep_bits: torch.Tensor, R_pred: torch.Tensor, t_pred: torch.Tensor, keypoints: torch.Tensor,
                bits: torch.Tensor, estimator: nn.Module, point_ok: torch.Tensor | None = None):
        single = points.dim() == 2
        if single:
            points, rep_bits, R_pred, t_pred, keypoints, bits = (a.unsqueeze(0) for a in (points, rep_bits, R_pred, t_pred, keypoints, bits))
            point_ok = None if point_ok is None else point_ok.unsqueeze(0)
        R0, t0 = R_pred.float(), t_pred.float()
        kp2d, valid, lm_kp, kp_lm, _, _, counts = self._match(points, rep_bits, R0, t0, keypoints, bits, point_ok, self.radius_px)
        R1, t1, inl1, _, _, ok1 = estimator(points, kp2d, valid)
        # the second pass: the solved pose where there is one (the predicted pose elsewhere, its results discarded below)
        first = ok1[:, None, None]
        Rs, ts = torch.where(first, R1, R0), torch.where(ok1[:, None], t1, t0)
        kp2d_b, valid_b, lm_kp_b, kp_lm_b, _, _, counts_b = self._match(points, rep_bits, Rs, ts, keypoints, bits, point_ok, self.refine_radius_px)
        R2, t2, inl2, _, _, ok2 = estimator(points, kp2d_b, valid_b)
        second = ok1 & ok2
        R = torch.where(second[:, None, None], R2, Rs)
        t = torch.where(second[:, None], t2, ts)
        inlier = torch.where(second[:, None], inl2, inl1 & ok1[:, None])
        lm_kp = torch.where(second[:, None], lm_kp_b, lm_kp)
        kp_lm = torch.where(second[:, None], kp_lm_b, kp_lm)
        counts = torch.where(second[:, None], counts_b, counts)
        res = (R, t, inlier, ok1, lm_kp, kp_lm, counts)
        return tuple(o[0] for o in res) if single else res
