"""AbsolutePoseEstimator -- the camera pose from 3-D to 2-D matches, the case between RelativePoseEstimator (2-D to 2-D, a
translation of unit length) and RgbdPoseEstimator (3-D to 3-D, depth needed at the keypoint in both frames): 3-D points on
one side, the pixels they are seen at on the other.  A frame whose depth has holes at the matched corners, a colour-only
frame against the points of a TsdfVolume, a new frame against triangulated landmarks.  Batched P3P RANSAC with MSAC
selection and Gauss-Newton local optimisation, the device counterpart of cv2.solvePnPRansac.  K23:
`mi_normalise_keypoints`, `mi_pnp_ransac`; the algorithm is stated in include/mi355x_match.h.  The reference has no
counterpart (its odometry sample sums unit translations)."""
import torch
from torch import nn

from ... import ops


class AbsolutePoseEstimator(nn.Module):
    """forward(points3d, keypoints2d, valid=None) -> (R, t, inlier_mask, rmse_px, info, ok) for points3d (B, N, 3) in the
    model frame and keypoints2d (B, N, 2), the pixels they are matched to, in (y, x) order, the order MatchExtractionWrapper
    returns; `valid` (B, N) selects the real matches of a padded batch.  X_camera = R X_model + t with det R = +1 and t in
    the units of the points; inlier_mask marks the matches that reproject within ransac_threshold pixels of their keypoint,
    rmse_px is their root-mean-square reprojection distance in pixels (of the mean focal length), info (B, 6, 6) the
    Gauss-Newton information matrix J^T J of the pose over the inliers in (rotation, translation) order and normalised image
    units; ok is False -- with R = identity, t = 0, no inliers, info = 0 -- where fewer than 4 matches are valid or no sample
    explains 4 of them.  (N, 3) points with (N, 2) keypoints give unbatched output.

    K: the 3x3 camera matrix.  num_hypotheses 4-point samples are drawn per pair by the counter-based sampler from `seed`
    (three rows solve, the fourth picks among the solutions); ransac_threshold is the inlier distance in pixels, divided by
    (fx + fy) / 2 for the kernels; refine_rounds rounds of refit-on-inliers follow the selection."""

    def __init__(self, K: torch.Tensor, num_hypotheses: int = 128, ransac_threshold: float = 2.0, refine_rounds: int = 3,
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
        self.focal = float((K_f[0, 0] + K_f[1, 1]) / 2)
        if not self.focal > 0:
            raise ValueError(f"K must have a positive mean focal length, got {self.focal}")
        self.num_hypotheses = int(num_hypotheses)
        self.ransac_threshold = float(ransac_threshold)
        self.refine_rounds = int(refine_rounds)
        self.seed = int(seed)

    def _solve(self, x: torch.Tensor, kp: torch.Tensor, v: torch.Tensor | None):
        pts2 = ops.normalise_keypoints(kp, self.K_inv.to(kp.device))
        r, t, inlier, _, _, rmse, info, ok = ops.pnp_ransac(x, pts2, v, self.num_hypotheses, self.ransac_threshold / self.focal,
                                                            self.refine_rounds, self.seed)
        return r, t, inlier, rmse * self.focal, info, ok

    @torch.no_grad()
    def forward(self, points3d: torch.Tensor, keypoints2d: torch.Tensor, valid: torch.Tensor | None = None):
        single = keypoints2d.dim() == 2
        x = points3d.unsqueeze(0) if single else points3d
        kp = keypoints2d.unsqueeze(0) if single else keypoints2d
        v = valid.unsqueeze(0) if (single and valid is not None) else valid
        if x.dim() != 3 or x.shape[-1] != 3 or kp.dim() != 3 or kp.shape[-1] != 2 or x.shape[:2] != kp.shape[:2]:
            raise RuntimeError(f"points3d must be (B, N, 3) or (N, 3) and keypoints2d (B, N, 2) or (N, 2), got "
                               f"{tuple(points3d.shape)}, {tuple(keypoints2d.shape)}")
        out = self._solve(x, kp, v)
        return tuple(o[0] for o in out) if single else out

    @torch.no_grad()
    def forward_rgbd(self, keypoints1: torch.Tensor, keypoints2: torch.Tensor, depth1: torch.Tensor,
                     valid: torch.Tensor | None = None, depth_scale: float = 1.0, min_depth: float = 0.1,
                     max_depth: float = 10.0):
        """Matched keypoints (B, N, 2) in pixel (y, x) of two frames and the FIRST frame's depth (B, H, W) or (B, 1, H, W),
        float32 or uint16, aligned to the camera of K: frame 1 is lifted through its depth (`mi_lift_keypoints`), frame 2
        needs none.  Returns forward()'s tuple with X2 = R X1 + t, t in the units of depth * depth_scale -- RgbdPoseEstimator's
        motion from matches whose depth is missing in frame 2."""
        single = keypoints1.dim() == 2
        k1 = keypoints1.unsqueeze(0) if single else keypoints1
        k2 = keypoints2.unsqueeze(0) if single else keypoints2
        v = valid.unsqueeze(0) if (single and valid is not None) else valid
        if k1.dim() != 3 or k1.shape[-1] != 2 or k1.shape != k2.shape:
            raise RuntimeError(f"keypoints must both be (B, N, 2) or (N, 2), got {tuple(keypoints1.shape)}, {tuple(keypoints2.shape)}")
        d = depth1
        if single and d.dim() == 2:
            d = d.unsqueeze(0)
        elif not single and d.dim() == 4 and d.shape[1] == 1:
            d = d[:, 0]
        if d.dim() != 3:
            raise RuntimeError(f"depth1 must be (B, H, W) or (B, 1, H, W), got {tuple(depth1.shape)}")
        x1, v1 = ops.lift_keypoints(k1, d, self.K_inv.to(k1.device), depth_scale, min_depth, max_depth, v)
        out = self._solve(x1, k2, v1)
        return tuple(o[0] for o in out) if single else out
