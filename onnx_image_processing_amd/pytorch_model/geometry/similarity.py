"""SimilarityEstimator -- the alignment of two maps whose units differ: two bundle-adjustment windows of a monocular
sequence, the landmarks round a loop candidate against those round the current keyframe, two sessions of one place, an
estimated trajectory against a reference one.  From 3-D to 3-D landmark correspondences it finds X2 = s R X1 + t by 3-point
RANSAC (ORB-SLAM's Sim3Solver) and moves map 1 into map 2's frame and units.  K30: `mi_sim3_ransac`, `mi_sim3_refit`,
`mi_sim3_apply`; the algorithm is stated in include/mi355x_match_sim3.h.  The reference has no counterpart (its odometry
sample sums unit translations; its `vo/trajectory.py` aligns trajectories on the host)."""
import torch
from torch import nn

from ... import ops

_METRICS = {"reprojection": ops.SIM3_REPROJ, "point": ops.SIM3_POINT}


class SimilarityEstimator(nn.Module):
    """forward(pts1, pts2, valid=None) -> (s, R, t, inlier, count, rmse, ok) for corresponding points (B, N, 3) of two maps
    and an optional (B, N) mask: X2 = s R X1 + t with det R = +1; inlier (B, N) marks the rows within the threshold of that
    similarity, count (B,) their number, rmse (B,) their root-mean-square error in the metric's units; ok is False -- with
    s = 1, R = identity, t = 0, no inliers -- where fewer than 3 rows are valid or no sample explains 3 of them.  (N, 3) points
    give unbatched output.

    metric "reprojection": the points are in the two keyframes' CAMERA frames (landmark_pairs makes them so) and a row is
    scored by its symmetric reprojection error in normalised image coordinates, so that the depth error of a triangulated
    point, large and along its ray, does not decide the inliers; `threshold` is in normalised units, or in pixels when
    `focal` (the focal length in pixels) is given.  metric "point": any frames, a row is scored by |s R X1 + t - X2| and
    `threshold` is in the units of map 2 (for trajectories and world-frame maps); `focal` must be None.
    num_hypotheses 3-point samples are drawn per pair by the counter-based sampler from `seed`; refine_rounds rounds of
    closed-form refit on the inliers follow the selection (no non-linear refinement).

    apply(s, R, t, R_frames, t_frames, points) -> (R_frames', t_frames', points'): map 1 -- frame poses (B, F, 3, 3), (B, F, 3)
    with X_camera = R_k X + t_k and landmarks (B, L, 3); either may be None -- in map 2's frame and units.
    inverse(s, R, t) -> the similarity from map 2 to map 1.  as_pose(s, R, t) -> (R, t / s): the rigid pose under which map-1
    points project as under the similarity, for LocalMapTracker.match (the guided search after a Sim(3)).
    align_trajectory(est_centres, ref_centres, valid=None) -> (s, R, t, rmse): the least-squares similarity over all valid
    rows (no RANSAC) and the root-mean-square distance after it, the ATE of an estimated trajectory.
    landmark_pairs(...) -> (pts1, pts2, valid): see there."""

    def __init__(self, metric: str = "reprojection", threshold: float | None = None, focal: float | None = None,
                 num_hypotheses: int = 128, refine_rounds: int = 3, seed: int = 0) -> None:
        super().__init__()
        if metric not in _METRICS:
            raise ValueError(f"metric must be 'reprojection' or 'point', got {metric!r}")
        if focal is not None and metric != "reprojection":
            raise ValueError("focal belongs to the reprojection metric: a point threshold is in the units of map 2")
        if focal is not None and not 0 < focal < float("inf"):
            raise ValueError(f"focal must be positive and finite, got {focal}")
        if threshold is None:
            if metric != "reprojection":
                raise ValueError("the point metric needs a threshold in the units of map 2")
            threshold = 2.0 if focal is not None else 0.004              # two pixels at a 500-pixel focal length
        if not 0 < threshold < float("inf"):
            raise ValueError(f"threshold must be positive and finite, got {threshold}")
        if num_hypotheses < 1:
            raise ValueError(f"num_hypotheses must be positive, got {num_hypotheses}")
        if not 0 <= refine_rounds <= ops.POSE_MAX_REFINE_ROUNDS:
            raise ValueError(f"refine_rounds must be in 0 .. {ops.POSE_MAX_REFINE_ROUNDS}, got {refine_rounds}")
        self.metric = metric
        self.metric_id = _METRICS[metric]
        self.focal = None if focal is None else float(focal)
        self.threshold = float(threshold)
        self.kernel_threshold = self.threshold / self.focal if self.focal is not None else self.threshold
        self.num_hypotheses = int(num_hypotheses)
        self.refine_rounds = int(refine_rounds)
        self.seed = int(seed)

    @staticmethod
    def _batched(pts1, pts2, valid, what):
        single = pts1.dim() == 2
        if single:
            pts1, pts2 = pts1.unsqueeze(0), pts2.unsqueeze(0)
            valid = None if valid is None else valid.unsqueeze(0)
        if pts1.dim() != 3 or pts1.shape[-1] != 3 or pts1.shape != pts2.shape:
            raise RuntimeError(f"{what}: points must both be (B, N, 3) or (N, 3), got {tuple(pts1.shape)}, {tuple(pts2.shape)}")
        return single, pts1, pts2, valid

    @torch.no_grad()
    def forward(self, pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None = None):
        single, p1, p2, v = self._batched(pts1, pts2, valid, "SimilarityEstimator")
        s, r, t, inlier, _, count, rmse, ok = ops.sim3_ransac(p1, p2, v, self.num_hypotheses, self.kernel_threshold, self.metric_id,
                                                              self.refine_rounds, self.seed)
        if self.focal is not None:
            rmse = rmse * self.focal
        out = (s, r, t, inlier, count, rmse, ok)
        return tuple(x[0] for x in out) if single else out

    @torch.no_grad()
    def apply(self, s: torch.Tensor, R: torch.Tensor, t: torch.Tensor, R_frames: torch.Tensor | None, t_frames: torch.Tensor | None,
              points: torch.Tensor | None):
        single = s.dim() == 0
        if single:
            s, R, t = s.unsqueeze(0), R.unsqueeze(0), t.unsqueeze(0)
            R_frames, t_frames, points = (None if a is None else a.unsqueeze(0) for a in (R_frames, t_frames, points))
        out = ops.sim3_apply(s, R, t, R_frames, t_frames, points)
        return tuple(None if x is None else x[0] for x in out) if single else out

    @staticmethod
    def inverse(s: torch.Tensor, R: torch.Tensor, t: torch.Tensor):
        """X1 = (1 / s) R^T (X2 - t)"""
        si = 1.0 / s
        Rt = R.transpose(-1, -2)
        return si, Rt, -si[..., None] * (Rt @ t[..., None])[..., 0]

    @staticmethod
    def as_pose(s: torch.Tensor, R: torch.Tensor, t: torch.Tensor):
        """(R, t / s): s R X + t and R X + t / s lie on one ray"""
        return R, t / s[..., None]

    @torch.no_grad()
    def align_trajectory(self, est_centres: torch.Tensor, ref_centres: torch.Tensor, valid: torch.Tensor | None = None):
        single, p1, p2, v = self._batched(est_centres, ref_centres, valid, "align_trajectory")
        mask = torch.ones(p1.shape[:2], dtype=torch.bool, device=p1.device) if v is None else v != 0
        s, r, t, _ = ops.sim3_refit(p1, p2, mask)
        moved = s[:, None, None] * (p1.float() @ r.transpose(1, 2)) + t[:, None]
        d2 = ((moved - p2.float()) ** 2).sum(-1) * mask
        rmse = torch.sqrt(d2.sum(1) / mask.sum(1).clamp(min=1))
        out = (s, r, t, rmse)
        return tuple(x[0] for x in out) if single else out

    @staticmethod
    @torch.no_grad()
    def landmark_pairs(match_ij: torch.Tensor, match_valid: torch.Tensor, kp_track1: torch.Tensor, frame1, points1: torch.Tensor,
                       point_ok1: torch.Tensor, R1: torch.Tensor, t1: torch.Tensor, kp_track2: torch.Tensor, frame2,
                       points2: torch.Tensor, point_ok2: torch.Tensor, R2: torch.Tensor, t2: torch.Tensor):
        """Keypoint matches between two keyframes -> the camera-frame landmark pairs of forward(): (pts1, pts2, valid), (B, M, 3)
        twice and (B, M) bool.  match_ij (B, M, 2) integer (i in keyframe 1, j in keyframe 2) and match_valid (B, M): what
        KeyframeDatabase.match or the matcher returns.  Per side: kp_track (B, F, K), points (B, L, 3) and point_ok (B, L) as
        LandmarkTracks returns them for the window the keyframe lies in, `frame` the keyframe's index in that window (an int or
        a (B,) tensor), R (B, F, 3, 3), t (B, F, 3) the window's poses (X_camera = R X + t).  A row is valid when the match is,
        both indices are keypoints and both keypoints belong to landmarks whose point is ok; the other rows are zero.  For two
        windows that share a frame, `frame1` / `frame2` are that frame's indices and match_ij pairs each of its keypoints with
        itself.  Unbatched input (match_ij (M, 2), ...) gives unbatched output.  Plain torch gathers."""
        single = match_ij.dim() == 2
        sides = [[kp_track1, points1, point_ok1, R1, t1], [kp_track2, points2, point_ok2, R2, t2]]
        if single:
            match_ij, match_valid = match_ij.unsqueeze(0), match_valid.unsqueeze(0)
            sides = [[a.unsqueeze(0) for a in side] for side in sides]
        if match_ij.dim() != 3 or match_ij.shape[-1] != 2 or match_valid.shape != match_ij.shape[:2]:
            raise RuntimeError(f"landmark_pairs: match_ij must be (B, M, 2) or (M, 2) with match_valid (B, M) or (M,), got "
                               f"{tuple(match_ij.shape)}, {tuple(match_valid.shape)}")
        b = match_ij.shape[0]
        rows = torch.arange(b, device=match_ij.device)
        valid = match_valid != 0
        out = []
        for side, (kp_track, points, point_ok, R, t), frame in zip((0, 1), sides, (frame1, frame2)):
            if kp_track.dim() != 3 or points.dim() != 3 or R.dim() != 4:
                raise RuntimeError(f"landmark_pairs: side {side + 1} must be kp_track (B, F, K), points (B, L, 3), R (B, F, 3, 3), got "
                                   f"{tuple(kp_track.shape)}, {tuple(points.shape)}, {tuple(R.shape)}")
            f = torch.as_tensor(frame, device=match_ij.device).long().expand(b)
            k, l = kp_track.shape[2], points.shape[1]
            i = match_ij[..., side].long()
            slot = kp_track[rows, f].long().gather(1, i.clamp(0, k - 1))
            valid = valid & (i >= 0) & (i < k) & (slot >= 0) & (slot < l)
            sc = slot.clamp(0, l - 1)
            valid = valid & (point_ok.gather(1, sc) != 0)
            x = points.float().gather(1, sc[..., None].expand(-1, -1, 3))
            out.append(x @ R[rows, f].float().transpose(1, 2) + t[rows, f].float()[:, None])
        pts1, pts2 = (torch.where(valid[..., None], p, torch.zeros_like(p)).contiguous() for p in out)
        res = (pts1, pts2, valid)
        return tuple(x[0] for x in res) if single else res
