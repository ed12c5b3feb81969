"""PoseGraphOptimizer -- the step that closes a loop: the odometry edges of a trajectory and the loop edges that
KeyframeDatabase and a pose estimator found move every keyframe pose so that all of them agree.  The host call it replaces
is g2o or GTSAM.  Levenberg-Marquardt on the relative-pose residuals, every damped step by a fixed number of block-Jacobi
preconditioned conjugate-gradient trips, a Huber loss, every graph of the batch in one workgroup of one launch.  K27:
`mi_pgo_refine`, `mi_pgo_cost`; the algorithm is stated in include/mi355x_match.h.  The reference has no counterpart (its
roadmap lists loop closure as open)."""
import torch
from torch import nn

from ... import ops


class PoseGraphOptimizer(nn.Module):
    """forward(R, t, edge_index, R_meas, t_meas, information, fixed, edge_valid=None, protected=None) ->
    (R, t, edge_valid_out, chi2, cost0, cost, info, ok) for a batch of graphs: poses R (B, N, 3, 3), t (B, N, 3) with
    X_camera = R X + t; edge_index (B, E, 2) integer (i, j); R_meas (B, E, 3, 3), t_meas (B, E, 3): the measured motion
    X_j = R_meas X_i + t_meas, what RgbdPoseEstimator, DenseRgbdRefiner, DirectRgbdRefiner and
    AbsolutePoseEstimator.forward_rgbd return for (frame 1 = i, frame 2 = j); information (B, E, 6, 6) in (rotation,
    translation) order, the `information` / `info` those modules return; fixed (B, N), True where a node is held (at least one
    per graph: the gauge); edge_valid (B, E), False for padding (None: every edge); protected (B, E), True for edges the
    outlier round never clears -- the odometry (None: no edge is protected).  chi2 (B, E): e^T Omega e of every edge at the
    result; cost0 / cost: the robust cost before and after; info (B, N, 6, 6): the conditional information of each node given
    its neighbours (not the marginal); ok False -- everything returned unchanged -- where a graph has no active edge, no
    fixed node, no free node with an edge, or a cost that is not finite.  Unbatched input gives unbatched output.

    huber: the Huber width on chi = sqrt(chi2) (0: plain squares).  outlier_rounds: after a refinement, edges that are not
    protected and whose chi2 exceeds outlier_chi2 (16.81: the 99 % point of chi-square with 6 degrees of freedom) are cleared
    from `edge_valid` (edge_valid_out) and the graph is refined again from the result with plain squares -- BundleAdjuster's
    two-pass scheme.  A graph that the first pass refuses goes through no round; a graph whose cleared edges a later pass
    refuses keeps the earlier pass's result whole: its state, its cost and the mask that pass ran on.  A long chain with few
    closures needs pcg_iterations of the order of its length."""

    def __init__(self, iterations: int = 10, pcg_iterations: int = 64, huber: float = 3.0, outlier_rounds: int = 1,
                 outlier_chi2: float = 16.81) -> None:
        super().__init__()
        if not 1 <= iterations <= ops.PGO_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in 1 .. {ops.PGO_MAX_ITERATIONS}, got {iterations}")
        if not 1 <= pcg_iterations <= ops.PGO_MAX_PCG:
            raise ValueError(f"pcg_iterations must be in 1 .. {ops.PGO_MAX_PCG}, got {pcg_iterations}")
        if not (huber >= 0 and huber < float("inf")):
            raise ValueError(f"huber must be finite and not negative, got {huber}")
        if outlier_rounds < 0:
            raise ValueError(f"outlier_rounds must not be negative, got {outlier_rounds}")
        if not outlier_chi2 > 0:
            raise ValueError(f"outlier_chi2 must be positive, got {outlier_chi2}")
        self.iterations = int(iterations)
        self.pcg_iterations = int(pcg_iterations)
        self.huber = float(huber)
        self.outlier_rounds = int(outlier_rounds)
        self.outlier_chi2 = float(outlier_chi2)

    @torch.no_grad()
    def forward(self, R: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, R_meas: torch.Tensor, t_meas: torch.Tensor,
                information: torch.Tensor, fixed: torch.Tensor, edge_valid: torch.Tensor | None = None,
                protected: torch.Tensor | None = None):
        single = edge_index.dim() == 2
        if single:
            R, t, edge_index, R_meas, t_meas, information, fixed = (a.unsqueeze(0) for a in (R, t, edge_index, R_meas, t_meas, information, fixed))
            edge_valid = None if edge_valid is None else edge_valid.unsqueeze(0)
            protected = None if protected is None else protected.unsqueeze(0)
        if edge_index.dim() != 3 or edge_index.shape[-1] != 2:
            raise RuntimeError(f"edge_index must be (B, E, 2) or (E, 2), got {tuple(edge_index.shape)}")
        b, e = edge_index.shape[:2]
        valid = torch.ones((b, e), dtype=torch.bool, device=edge_index.device) if edge_valid is None else edge_valid != 0
        keep = torch.zeros_like(valid) if protected is None else protected != 0
        if tuple(valid.shape) != (b, e) or tuple(keep.shape) != (b, e):
            raise RuntimeError(f"edge_valid and protected must be ({b}, {e}), got {tuple(valid.shape)} and {tuple(keep.shape)}")
        edges = (edge_index, R_meas, t_meas, information)
        out = ops.pgo_refine(R, t, *edges, fixed, valid, self.iterations, self.pcg_iterations, self.huber)
        cost0 = out[3]
        for _ in range(self.outlier_rounds):
            # a graph is taken through a round only as a whole (BundleAdjuster's rule): where the pass so far was refused, or
            # the pass on the cleared edges is, it keeps the state, the cost, `ok` AND the mask of the pass that produced them
            cleared = valid & ~((out[2] > self.outlier_chi2) & ~keep)
            again = ops.pgo_refine(out[0], out[1], *edges, fixed, cleared, self.iterations, self.pcg_iterations, 0.0)
            take = out[7] & again[7]
            out = tuple(torch.where(take.view(-1, *([1] * (a.dim() - 1))), b2, a) for a, b2 in zip(out, again))
            valid = torch.where(take.view(-1, 1), cleared, valid)
        r_o, t_o, chi2, _, cost, _, info, ok = out
        res = (r_o, t_o, valid, chi2, cost0, cost, info, ok)
        return tuple(o[0] for o in res) if single else res
