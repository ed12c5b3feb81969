"""LandmarkTracks -- the join between the matcher and BundleAdjuster: the pairwise matches of a window of frames become
landmark tracks (one column per landmark, one row per frame), the ambiguous tracks are rejected, and every track gets a
point from all the frames that see it.  The host code it replaces is a union-find over the window's keypoints, a gather and
a per-landmark least-squares loop.  K28: `mi_tracks_build`, `mi_tracks_triangulate`; the definitions are stated in
include/mi355x_match.h.  The reference has no counterpart (its roadmap lists map management as open)."""
import math

import torch
from torch import nn

from ... import ops


class LandmarkTracks(nn.Module):
    """forward(keypoints, pair_frames, match_ij, match_valid, R, t, kp_valid=None) -> (points, track_keypoints, visible,
    point_ok, track_kp, kp_track, counts) for a batch of windows: keypoints (B, F, K, 2) in pixel (y, x) order, the order
    MatchExtractionWrapper returns; pair_frames (B, P, 2) integer (a, b): the frame pairs that were matched; match_ij
    (B, P, M, 2) integer (i in a, j in b) and match_valid (B, P, M): what ops.match_pairs(..., want_ij=True),
    ops.mnn_extract(..., return_indices=True) and KeyframeDatabase.match return per pair; kp_valid (B, F, K) or None; poses R
    (B, F, 3, 3), t (B, F, 3) with X_camera = R X + t.  points (B, L, 3), track_keypoints (B, F, L, 2) pixel (y, x), visible
    (B, F, L) -- cleared for a landmark whose triangulation failed -- go into BundleAdjuster.forward with (R, t) unchanged;
    point_ok (B, L); track_kp (B, F, L): the keypoint index or -1; kp_track (B, F, K): the slot of a keypoint, -2 inside a
    conflicting component, -1 otherwise; counts (B, 4): components of at least two keypoints, conflicting, eligible, kept.
    Unbatched input (keypoints (F, K, 2), ...) gives unbatched output.

    A track is a connected component of the matches; one that holds two keypoints of the same frame is ambiguous and
    dropped whole; the longest max_landmarks of those seen in at least min_views frames are kept.  A landmark is
    triangulated from all its views and kept when it lies in front of every one of them, no view is further than
    max_reproj_px from its reprojection and two of its rays are at least min_parallax_deg apart.

    build(keypoints, pair_frames, match_ij, match_valid, kp_valid=None) -> (track_keypoints, visible, track_kp, track_len,
    kp_track, counts) and triangulate(R, t, track_keypoints, visible) -> (points, point_ok, visible_out, e2max_px2,
    cos_parallax) are the two halves."""

    def __init__(self, K: torch.Tensor, max_landmarks: int = 2048, min_views: int = 2, max_reproj_px: float = 3.0,
                 min_parallax_deg: float = 1.0) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        if not 1 <= max_landmarks <= ops.BA_MAX_LANDMARKS:
            raise ValueError(f"max_landmarks must be in 1 .. {ops.BA_MAX_LANDMARKS}, got {max_landmarks}")
        if not 2 <= min_views <= ops.TRACKS_MAX_FRAMES:
            raise ValueError(f"min_views must be in 2 .. {ops.TRACKS_MAX_FRAMES}, got {min_views}")
        if not (max_reproj_px > 0 and max_reproj_px < float("inf")):
            raise ValueError(f"max_reproj_px must be positive and finite, got {max_reproj_px}")
        if not 0 <= min_parallax_deg < 180:
            raise ValueError(f"min_parallax_deg must be in [0, 180), got {min_parallax_deg}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.focal = float((K_f[0, 0] + K_f[1, 1]) / 2)
        if not self.focal > 0:
            raise ValueError(f"K must have a positive mean focal length, got {self.focal}")
        self.max_landmarks = int(max_landmarks)
        self.min_views = int(min_views)
        self.max_reproj_px = float(max_reproj_px)
        self.min_parallax_deg = float(min_parallax_deg)
        self.max_cos = math.cos(math.radians(self.min_parallax_deg))

    @torch.no_grad()
    def build(self, keypoints: torch.Tensor, pair_frames: torch.Tensor, match_ij: torch.Tensor, match_valid: torch.Tensor,
              kp_valid: torch.Tensor | None = None):
        single = keypoints.dim() == 3
        if single:
            keypoints, pair_frames, match_ij, match_valid = (a.unsqueeze(0) for a in (keypoints, pair_frames, match_ij, match_valid))
            kp_valid = None if kp_valid is None else kp_valid.unsqueeze(0)
        if keypoints.dim() != 4 or keypoints.shape[-1] != 2:
            raise RuntimeError(f"keypoints must be (B, F, K, 2) or (F, K, 2), got {tuple(keypoints.shape)}")
        track_kp, vis, track_keypoints, track_len, kp_track, counts = ops.tracks_build(
            keypoints, pair_frames, match_ij, match_valid, kp_valid, self.min_views, self.max_landmarks)
        res = (track_keypoints, vis, track_kp, track_len, kp_track, counts)
        return tuple(o[0] for o in res) if single else res

    @torch.no_grad()
    def triangulate(self, R: torch.Tensor, t: torch.Tensor, track_keypoints: torch.Tensor, visible: torch.Tensor):
        single = track_keypoints.dim() == 3
        if single:
            R, t, track_keypoints, visible = (a.unsqueeze(0) for a in (R, t, track_keypoints, visible))
        if track_keypoints.dim() != 4 or track_keypoints.shape[-1] != 2:
            raise RuntimeError(f"track_keypoints must be (B, F, L, 2) or (F, L, 2), got {tuple(track_keypoints.shape)}")
        obs = ops.normalise_keypoints(track_keypoints, self.K_inv.to(track_keypoints.device))
        points, point_ok, vis_out, e2max, cos_par = ops.tracks_triangulate(
            R, t, obs, visible != 0, self.min_views, (self.max_reproj_px / self.focal) ** 2, self.max_cos)
        res = (points, point_ok, vis_out, e2max * (self.focal * self.focal), cos_par)
        return tuple(o[0] for o in res) if single else res

    def forward(self, keypoints: torch.Tensor, pair_frames: torch.Tensor, match_ij: torch.Tensor, match_valid: torch.Tensor,
                R: torch.Tensor, t: torch.Tensor, kp_valid: torch.Tensor | None = None):
        track_keypoints, vis, track_kp, _, kp_track, counts = self.build(keypoints, pair_frames, match_ij, match_valid, kp_valid)
        points, point_ok, vis_out, _, _ = self.triangulate(R, t, track_keypoints, vis)
        return points, track_keypoints, vis_out, point_ok, track_kp, kp_track, counts
