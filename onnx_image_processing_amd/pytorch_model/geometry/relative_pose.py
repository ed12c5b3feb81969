"""RelativePoseEstimator and triangulate_points -- the GPU form of reference pytorch_model/vo/pose_estimation.py:53-162
(estimate_pose_ransac, triangulate_points), which runs OpenCV on the host one pair at a time.  K15: `mi_essential_ransac`,
`mi_recover_pose`, `mi_triangulate`; the algorithm and its divergences from OpenCV are in include/mi355x_match.h."""
import torch
from torch import nn

from ... import ops


class RelativePoseEstimator(nn.Module):
    """forward(keypoints1, keypoints2, valid=None) -> (R, t, inlier_mask, E, ok) for matched keypoints (B, N, 2) in pixel
    (y, x) order, the order MatchExtractionWrapper returns and estimate_pose_ransac takes; `valid` (B, N) selects the real
    matches of a padded batch.  x2 ~ R x1 + t with det R = +1 and |t| = 1 (OpenCV's convention); inlier_mask is the RANSAC
    inlier set AND the depth test of the pose recovery (:113); ok is False -- with R = identity, t = 0 -- where fewer than 5
    correspondences survive (:109, where the reference returns None).  (N, 2) input gives unbatched output.

    K: the 3x3 camera matrix.  ransac_threshold is in pixels and is divided by (fx + fy) / 2 as cv2.findEssentialMat does;
    num_hypotheses 8-point samples are drawn per pair by the counter-based sampler from `seed`; refine_rounds rounds of
    refit-on-inliers follow the selection; distance_threshold is cv2.recoverPose's depth cut."""

    def __init__(self, K: torch.Tensor, num_hypotheses: int = 256, ransac_threshold: float = 1.0, refine_rounds: int = 3,
                 distance_threshold: float = 50.0, seed: int = 0) -> None:
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
        if not distance_threshold > 0:
            raise ValueError(f"distance_threshold must be positive, got {distance_threshold}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.num_hypotheses = int(num_hypotheses)
        self.ransac_threshold = float(ransac_threshold)
        self.refine_rounds = int(refine_rounds)
        self.distance_threshold = float(distance_threshold)
        self.seed = int(seed)
        self.focal = float((K_f[0, 0] + K_f[1, 1]) / 2)

    @torch.no_grad()
    def forward(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, valid: torch.Tensor | None = None):
        single = keypoints1.dim() == 2
        k1 = keypoints1.unsqueeze(0) if single else keypoints1
        k2 = keypoints2.unsqueeze(0) if single else keypoints2
        v = valid.unsqueeze(0) if (single and valid is not None) else valid
        if k1.dim() != 3 or k1.shape[-1] != 2 or k1.shape != k2.shape:
            raise RuntimeError(f"keypoints must both be (B, N, 2) or (N, 2), got {tuple(keypoints1.shape)}, {tuple(keypoints2.shape)}")
        k_inv = self.K_inv.to(k1.device)
        p1, p2 = ops.normalise_keypoints(k1, k_inv), ops.normalise_keypoints(k2, k_inv)
        e, inlier, _, _ = ops.essential_ransac(p1, p2, v, self.num_hypotheses, self.ransac_threshold / self.focal,
                                               self.refine_rounds, self.seed)
        r, t, pose_mask, _, ok = ops.recover_pose(e, p1, p2, inlier, self.distance_threshold)
        out = (r, t, pose_mask, e, ok)
        return tuple(x[0] for x in out) if single else out


@torch.no_grad()
def triangulate_points(keypoints1: torch.Tensor, keypoints2: torch.Tensor, R1: torch.Tensor, t1: torch.Tensor,
                       R2: torch.Tensor, t2: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """Reference triangulate_points (:118-162) on torch tensors: keypoints (B, N, 2) / (N, 2) in pixel (y, x), camera poses
    R (.., 3, 3), t (.., 3) or (.., 3, 1), K (3, 3) -> points (B, N, 3) / (N, 3); a point whose homogeneous coordinate
    vanishes stays at the origin."""
    single = keypoints1.dim() == 2
    k1 = (keypoints1.unsqueeze(0) if single else keypoints1).float()
    k2 = (keypoints2.unsqueeze(0) if single else keypoints2).float()
    b = k1.shape[0]
    dev = k1.device
    Kd = K.double().to(dev)

    def proj(R, t):
        # K [R | t] in float64 (36 products per pose), rounded to float32 once: the entries reach the focal length in size,
        # and a float32 product would put a second rounding into what the reference forms in float64
        rt = torch.cat([R.double().to(dev).reshape(-1, 3, 3), t.double().to(dev).reshape(-1, 3, 1)], dim=2)
        return (Kd @ rt).float().expand(b, 3, 4).contiguous()

    pts, _ = ops.triangulate(proj(R1, t1), proj(R2, t2), k1.flip(-1), k2.flip(-1))
    return pts[0] if single else pts
