"""HomographyEstimator, PlanarPoseEstimator and TwoViewPoseEstimator -- two-view geometry for the scenes
RelativePoseEstimator's 8-point solve is degenerate on: matched points on a plane, and a camera that only rotates.  The
host calls users would reach for are cv2.findHomography(RANSAC) and cv2.decomposeHomographyMat, and ORB-SLAM's initialiser
for the choice between the essential matrix and the homography.  K24: `mi_homography_ransac`, `mi_homography_pose`,
`mi_two_view_select`; the algorithm and its divergences from OpenCV are in include/mi355x_match.h.  The reference has no
such step."""
import torch
from torch import nn

from ... import ops


def _batched(keypoints1, keypoints2, valid):
    single = keypoints1.dim() == 2
    k1 = keypoints1.unsqueeze(0) if single else keypoints1
    k2 = keypoints2.unsqueeze(0) if single else keypoints2
    v = valid.unsqueeze(0) if (single and valid is not None) else valid
    if k1.dim() != 3 or k1.shape[-1] != 2 or k1.shape != k2.shape:
        raise RuntimeError(f"keypoints must both be (B, N, 2) or (N, 2), got {tuple(keypoints1.shape)}, {tuple(keypoints2.shape)}")
    return single, k1, k2, v


class HomographyEstimator(nn.Module):
    """forward(keypoints1, keypoints2, valid=None) -> (H_pixels, inlier_mask, ok) for matched keypoints (B, N, 2) in pixel
    (y, x) order; `valid` (B, N) selects the real matches of a padded batch.  H_pixels = K H K^-1 (B, 3, 3) maps pixel
    (x, y, 1) of image 1 onto image 2 up to scale, as cv2.findHomography's result does, at unit Frobenius norm of the
    normalised H; inlier_mask (B, N) is the RANSAC inlier set; ok is False, with a zero H, where no sample could be solved
    or fewer than 4 correspondences agree.  (N, 2) input gives unbatched output.

    K: the 3x3 camera matrix.  ransac_threshold is in pixels (OpenCV's ransacReprojThreshold default), applied to the
    SYMMETRIC transfer error after division by (fx + fy) / 2; num_hypotheses 4-point samples are drawn per pair by the
    counter-based sampler from `seed`; refine_rounds rounds of refit-on-inliers follow the selection."""

    def __init__(self, K: torch.Tensor, num_hypotheses: int = 256, ransac_threshold: float = 3.0, refine_rounds: int = 3,
                 seed: int = 0) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        if num_hypotheses < 1:
            raise ValueError(f"num_hypotheses must be positive, got {num_hypotheses}")
        if not ransac_threshold > 0:
            raise ValueError(f"ransac_threshold must be positive, got {ransac_threshold}")
        if not 0 <= refine_rounds <= ops.POSE_MAX_REFINE_ROUNDS:
            raise ValueError(f"refine_rounds must be in 0 .. {ops.POSE_MAX_REFINE_ROUNDS}, got {refine_rounds}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.num_hypotheses = int(num_hypotheses)
        self.ransac_threshold = float(ransac_threshold)
        self.refine_rounds = int(refine_rounds)
        self.seed = int(seed)
        self.focal = float((K_f[0, 0] + K_f[1, 1]) / 2)

    def _ransac(self, k1, k2, v):
        """(normalised points of both views, H, inlier, count) of a batch"""
        k_inv = self.K_inv.to(k1.device)
        p1, p2 = ops.normalise_keypoints(k1, k_inv), ops.normalise_keypoints(k2, k_inv)
        h, inlier, _, count, _ = ops.homography_ransac(p1, p2, v, self.num_hypotheses, self.ransac_threshold / self.focal,
                                                       self.refine_rounds, self.seed)
        return p1, p2, h, inlier, count

    @torch.no_grad()
    def forward(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, valid: torch.Tensor | None = None):
        single, k1, k2, v = _batched(keypoints1, keypoints2, valid)
        _, _, h, inlier, count = self._ransac(k1, k2, v)
        ok = count >= 4
        kd = self.K.to(h.device)
        h_px = torch.where(ok[:, None, None], kd @ h @ self.K_inv.to(h.device), torch.zeros_like(h))
        out = (h_px, inlier & ok[:, None], ok)
        return tuple(x[0] for x in out) if single else out


class PlanarPoseEstimator(HomographyEstimator):
    """forward(keypoints1, keypoints2, valid=None) -> (R (B, 2, 3, 3), t (B, 2, 3), normal (B, 2, 3), count (B, 2),
    pose_mask (B, N), H (B, 3, 3), rotation_only (B,), ok (B,)): HomographyEstimator's RANSAC followed by the decomposition
    of H -- the two leading slots of `mi_homography_pose`, which a plane in front of both cameras leaves equally likely.
    x2 ~ (R + t normal^T) x1 in normalised coordinates: t is the translation in units of the plane's distance to camera 1,
    normal the plane's unit normal in camera 1 (pointing away from it).  H is the normalised homography (not in pixels).
    rotation_only: the two views differ by a rotation alone; then t and normal are zero and both slots hold that rotation.
    ok is False -- R = identity, the rest zero -- where fewer than 4 inliers lie in front of both cameras."""

    @torch.no_grad()
    def forward(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, valid: torch.Tensor | None = None):
        single, k1, k2, v = _batched(keypoints1, keypoints2, valid)
        p1, p2, h, inlier, _ = self._ransac(k1, k2, v)
        r, t, normal, count, pose_mask, rot, ok = ops.homography_pose(h, p1, p2, inlier)
        out = (r[:, :2], t[:, :2], normal[:, :2], count[:, :2], pose_mask, h, rot, ok)
        return tuple(x[0] for x in out) if single else out


class TwoViewPoseEstimator(nn.Module):
    """forward(keypoints1, keypoints2, valid=None) -> (R, t, inlier_mask, model, ok): RelativePoseEstimator (K15) and
    PlanarPoseEstimator (K24) on the same normalised points, and per pair the model `mi_two_view_select` chooses: model
    (B,) int64 is 0 for the essential matrix and 1 for the homography.  x2 ~ R x1 + t with det R = +1 and |t| = 1.

    With model = 0 the outputs are RelativePoseEstimator's, bit for bit.  With model = 1 they are slot 0 of the
    decomposition -- or, with `normal_prior` (3,) given (the expected plane normal in camera 1: (0, 0, 1) for a wall
    faced head-on), the one of the two leading slots whose normal has the larger dot product with it -- with t scaled to
    unit length (zero for a pure rotation) and inlier_mask the RANSAC inliers in front of both cameras under slot 0.

    ransac_threshold / homography_threshold are the two RANSACs' thresholds in pixels and also the scales of the selection
    scores; selection_cut is the share of the two scores' sum the homography's must exceed (0.45: ORB-SLAM's, Mur-Artal et
    al. 2015, section IV); the other arguments are RelativePoseEstimator's."""

    def __init__(self, K: torch.Tensor, num_hypotheses: int = 256, ransac_threshold: float = 1.0,
                 homography_threshold: float = 3.0, refine_rounds: int = 3, distance_threshold: float = 50.0,
                 selection_cut: float = 0.45, normal_prior=None, seed: int = 0) -> None:
        super().__init__()
        from .relative_pose import RelativePoseEstimator
        self.relative = RelativePoseEstimator(K, num_hypotheses, ransac_threshold, refine_rounds, distance_threshold, seed)
        if not homography_threshold > 0:
            raise ValueError(f"homography_threshold must be positive, got {homography_threshold}")
        self.planar = PlanarPoseEstimator(K, num_hypotheses, homography_threshold, refine_rounds, seed)
        if not 0 <= selection_cut <= 1:
            raise ValueError(f"selection_cut must be in 0 .. 1, got {selection_cut}")
        self.selection_cut = float(selection_cut)
        if normal_prior is None:
            self.normal_prior = None
        else:
            prior = torch.as_tensor(normal_prior).float()
            if tuple(prior.shape) != (3,) or not float(prior.norm()) > 0:
                raise ValueError(f"normal_prior must be a non-zero 3-vector, got shape {tuple(prior.shape)}")
            self.register_buffer("normal_prior", prior / prior.norm())

    @torch.no_grad()
    def forward(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, valid: torch.Tensor | None = None):
        single, k1, k2, v = _batched(keypoints1, keypoints2, valid)
        rel, pl = self.relative, self.planar
        k_inv = rel.K_inv.to(k1.device)
        p1, p2 = ops.normalise_keypoints(k1, k_inv), ops.normalise_keypoints(k2, k_inv)
        thr_e, thr_h = rel.ransac_threshold / rel.focal, pl.ransac_threshold / pl.focal
        # K15, exactly as RelativePoseEstimator.forward runs it
        e, inl_e, _, _ = ops.essential_ransac(p1, p2, v, rel.num_hypotheses, thr_e, rel.refine_rounds, rel.seed)
        r_e, t_e, mask_e, _, ok_e = ops.recover_pose(e, p1, p2, inl_e, rel.distance_threshold)
        # K24
        h, inl_h, _, _, _ = ops.homography_ransac(p1, p2, v, pl.num_hypotheses, thr_h, pl.refine_rounds, pl.seed)
        r4, t4, n4, _, mask_h, rot, ok_h = ops.homography_pose(h, p1, p2, inl_h)
        _, _, choice = ops.two_view_select(e, h, p1, p2, v, thr_e, thr_h, self.selection_cut)
        if self.normal_prior is None:
            r_h, t_h = r4[:, 0], t4[:, 0]
        else:
            second = (n4[:, 1] @ self.normal_prior.to(n4.device)) > (n4[:, 0] @ self.normal_prior.to(n4.device))
            r_h = torch.where(second[:, None, None], r4[:, 1], r4[:, 0])
            t_h = torch.where(second[:, None], t4[:, 1], t4[:, 0])
        norm = t_h.norm(dim=1, keepdim=True)
        t_h = torch.where((norm > 0) & ~rot[:, None], t_h / norm.clamp_min(1e-30), torch.zeros_like(t_h))
        out = (torch.where(choice[:, None, None], r_h, r_e), torch.where(choice[:, None], t_h, t_e),
               torch.where(choice[:, None], mask_h, mask_e), choice.long(), torch.where(choice, ok_h, ok_e))
        return tuple(x[0] for x in out) if single else out
