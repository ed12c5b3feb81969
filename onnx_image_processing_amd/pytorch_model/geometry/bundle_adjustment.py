"""BundleAdjuster -- the joint refinement of a window of camera poses and the landmarks they share: what follows
AbsolutePoseEstimator / RelativePoseEstimator and `LandmarkTracks` (the window's matches as tracks with triangulated
points: this module's arguments) in a visual-odometry back end, and the host call
(g2o, Ceres, cv2.detail.BundleAdjusterReproj) it replaces.  Levenberg-Marquardt on the reprojection error with the
landmarks eliminated by the Schur complement, a Huber loss, a fixed number of iterations, every window of the batch in one
workgroup of one launch.  K25: `mi_normalise_keypoints`, `mi_ba_refine`, `mi_ba_cost`; the algorithm is stated in
include/mi355x_match.h.  The reference has no counterpart (its roadmap lists bundle adjustment as open)."""
import torch
from torch import nn

from ... import ops


class BundleAdjuster(nn.Module):
    """forward(R, t, points, keypoints, visible) -> (R, t, points, visible_out, point_ok, cost0_px2, cost_px2, info, ok) for a
    batch of windows: poses R (B, F, 3, 3), t (B, F, 3) with X_camera = R X + t, landmarks points (B, L, 3), keypoints
    (B, F, L, 2) in pixel (y, x) order, the order MatchExtractionWrapper returns, and visible (B, F, L), True where frame f
    sees landmark l.  The first num_fixed frames are held -- the gauge: 1 for metric input, 2 to pin the scale of monocular
    input, F for structure only.  A landmark seen in fewer than 2 frames takes no part and comes back unchanged with point_ok
    False.  cost0_px2 / cost_px2: the robust cost before and after, in squared pixels of the mean focal length; info
    (B, 6F, 6F): the marginal information of the poses at the result, (rotation, translation) per frame, normalised units;
    ok False -- everything returned unchanged -- where a seen point lies behind its camera at the start or no landmark is
    active.  Unbatched input (R (F, 3, 3), ...) gives unbatched output.

    K: the 3x3 camera matrix.  huber_px: the Huber width in pixels (0: plain squares).  outlier_rounds: after a refinement,
    observations further than outlier_px from their reprojection are cleared from `visible` (visible_out) and the window is
    refined again from the result with plain squares -- ORB-SLAM's local bundle adjustment scheme.  A window that the first
    pass refuses goes through no round: it comes back as it came, `visible_out` = `visible` included.  A window whose
    cleared observations a later pass refuses (no landmark with two views is left) keeps the earlier pass's result
    whole: its state, its cost (the Huber cost of that pass) and the mask that pass ran on."""

    def __init__(self, K: torch.Tensor, iterations: int = 10, huber_px: float = 2.0, num_fixed: int = 1, outlier_rounds: int = 1,
                 outlier_px: float = 3.0) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        if not 1 <= iterations <= ops.BA_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in 1 .. {ops.BA_MAX_ITERATIONS}, got {iterations}")
        if not (huber_px >= 0 and huber_px < float("inf")):
            raise ValueError(f"huber_px must be finite and not negative, got {huber_px}")
        if not 1 <= num_fixed <= ops.BA_MAX_FRAMES:
            raise ValueError(f"num_fixed must be in 1 .. {ops.BA_MAX_FRAMES}, got {num_fixed}")
        if outlier_rounds < 0:
            raise ValueError(f"outlier_rounds must not be negative, got {outlier_rounds}")
        if not outlier_px > 0:
            raise ValueError(f"outlier_px must be positive, got {outlier_px}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        self.focal = float((K_f[0, 0] + K_f[1, 1]) / 2)
        if not self.focal > 0:
            raise ValueError(f"K must have a positive mean focal length, got {self.focal}")
        self.iterations = int(iterations)
        self.huber_px = float(huber_px)
        self.num_fixed = int(num_fixed)
        self.outlier_rounds = int(outlier_rounds)
        self.outlier_px = float(outlier_px)

    @torch.no_grad()
    def forward(self, R: torch.Tensor, t: torch.Tensor, points: torch.Tensor, keypoints: torch.Tensor, visible: torch.Tensor):
        single = keypoints.dim() == 3
        if single:
            R, t, points, keypoints, visible = (a.unsqueeze(0) for a in (R, t, points, keypoints, visible))
        if keypoints.dim() != 4 or keypoints.shape[-1] != 2:
            raise RuntimeError(f"keypoints must be (B, F, L, 2) or (F, L, 2), got {tuple(keypoints.shape)}")
        obs = ops.normalise_keypoints(keypoints, self.K_inv.to(keypoints.device))
        vis = visible != 0
        f2 = self.focal * self.focal
        out = ops.ba_refine(R, t, points, obs, vis, self.num_fixed, self.iterations, self.huber_px / self.focal)
        cost0 = out[4]
        gate = (self.outlier_px / self.focal) ** 2
        for _ in range(self.outlier_rounds):
            # a window is taken through a round only as a whole: where the pass so far was refused, or the pass on the
            # cleared observations is, the window keeps the state, the cost, `ok` AND the mask of the pass that produced them
            e2, _, _ = ops.ba_cost(out[0], out[1], out[2], obs, vis, 0.0)
            cleared = vis & ~(e2 > gate)
            again = ops.ba_refine(out[0], out[1], out[2], obs, cleared, self.num_fixed, self.iterations, 0.0)
            take = out[8] & again[8]
            out = tuple(torch.where(take.view(-1, *([1] * (a.dim() - 1))), b, a) for a, b in zip(out, again))
            vis = torch.where(take.view(-1, 1, 1), cleared, vis)
        r_o, t_o, x_o, point_ok, _, cost, _, info, ok = out
        res = (r_o, t_o, x_o, vis, point_ok, cost0 * f2, cost * f2, info, ok)
        return tuple(o[0] for o in res) if single else res
