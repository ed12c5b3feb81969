"""SimilarityGraphOptimizer -- the step that closes a MONOCULAR loop: a Sim(3) loop constraint from SimilarityEstimator, and
the odometry / covisibility edges of the trajectory, move and rescale every keyframe so that all of them agree, and
`correct` carries the landmarks along.  PoseGraphOptimizer with a scale per node: the unit of a monocular map drifts, the
loop measures by how much, and only nodes that carry a scale can spread that over the trajectory.  The host call it
replaces is ORB-SLAM's OptimizeEssentialGraph (g2o's VertexSim3Expmap / EdgeSim3) and the map correction after it.  K31:
`mi_simgraph_refine`, `mi_simgraph_cost`, `mi_simgraph_correct`; the algorithm is stated in
include/mi355x_match_simgraph.h.  The reference has no counterpart (its roadmap lists loop closure as open)."""
import torch
from torch import nn

from ... import ops


class SimilarityGraphOptimizer(nn.Module):
    """forward(s, R, t, edge_index, s_meas, R_meas, t_meas, information, fixed, edge_valid=None, protected=None) ->
    (s, R, t, edge_valid_out, chi2, cost0, cost, info, ok) for a batch of graphs: node states s (B, N) (None: ones), R (B, N, 3,
    3), t (B, N, 3) with X_camera = s R X + t; edge_index (B, E, 2) integer (i, j); s_meas (B, E), R_meas (B, E, 3, 3), t_meas
    (B, E, 3): the measured similarity X_j = s_meas R_meas X_i + t_meas, what SimilarityEstimator returns for (frame 1 = i,
    frame 2 = j) and what edges_from_state gives for the edges taken from the current poses; information (B, E, 7, 7) in
    (rotation, translation, log-scale) order (information_from_pose pads a pose estimator's 6x6); fixed (B, N), True where a
    node is held with all its 7 degrees of freedom (at least one per graph: the gauge); edge_valid (B, E), False for padding
    (None: every edge); protected (B, E), True for edges the outlier round never clears -- the odometry (None: no edge is
    protected).  chi2 (B, E): e^T Omega e of every edge at the result; cost0 / cost: the robust cost before and after; info
    (B, N, 7, 7): the conditional information of each node given its neighbours (not the marginal); ok False -- everything
    returned unchanged -- where a graph has no active edge, no fixed node, no free node with an edge, or a cost that is not
    finite (a node scale that is not positive).  Unbatched input gives unbatched output.

    huber, outlier_rounds: PoseGraphOptimizer's, with outlier_chi2 = 18.48, the 99 % point of chi-square with 7 degrees of
    freedom: after a refinement, edges that are not protected and whose chi2 exceeds it are cleared and the graph is refined
    again from the result with plain squares; a graph goes through a round only as a whole, and one that a pass refuses keeps
    the earlier pass's state, cost and mask.

    edges_from_state(R, t, edge_index, s=None) -> (s_meas, R_meas, t_meas): the relative similarities of the current poses.
    information_from_pose(info6, scale_weight) -> (..., 7, 7).
    correct(R_old, t_old, s, R, t, points, ref) -> (R_out, t_out, points_out): the metric map after the optimisation."""

    def __init__(self, iterations: int = 10, pcg_iterations: int = 64, huber: float = 3.0, outlier_rounds: int = 1,
                 outlier_chi2: float = 18.48) -> None:
        super().__init__()
        if not 1 <= iterations <= ops.SIMGRAPH_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in 1 .. {ops.SIMGRAPH_MAX_ITERATIONS}, got {iterations}")
        if not 1 <= pcg_iterations <= ops.SIMGRAPH_MAX_PCG:
            raise ValueError(f"pcg_iterations must be in 1 .. {ops.SIMGRAPH_MAX_PCG}, got {pcg_iterations}")
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
    def forward(self, s: torch.Tensor | None, R: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s_meas: torch.Tensor,
                R_meas: torch.Tensor, t_meas: torch.Tensor, information: torch.Tensor, fixed: torch.Tensor,
                edge_valid: torch.Tensor | None = None, protected: torch.Tensor | None = None):
        single = edge_index.dim() == 2
        if s is None:
            s = torch.ones(t.shape[:-1], dtype=torch.float32, device=t.device)
        if single:
            s, R, t, edge_index, s_meas, R_meas, t_meas, information, fixed = (
                a.unsqueeze(0) for a in (s, R, t, edge_index, s_meas, R_meas, t_meas, information, fixed))
            edge_valid = None if edge_valid is None else edge_valid.unsqueeze(0)
            protected = None if protected is None else protected.unsqueeze(0)
        if edge_index.dim() != 3 or edge_index.shape[-1] != 2:
            raise RuntimeError(f"edge_index must be (B, E, 2) or (E, 2), got {tuple(edge_index.shape)}")
        b, e = edge_index.shape[:2]
        valid = torch.ones((b, e), dtype=torch.bool, device=edge_index.device) if edge_valid is None else edge_valid != 0
        keep = torch.zeros_like(valid) if protected is None else protected != 0
        if tuple(valid.shape) != (b, e) or tuple(keep.shape) != (b, e):
            raise RuntimeError(f"edge_valid and protected must be ({b}, {e}), got {tuple(valid.shape)} and {tuple(keep.shape)}")
        edges = (edge_index, s_meas, R_meas, t_meas, information)
        out = ops.simgraph_refine(s, R, t, *edges, fixed, valid, self.iterations, self.pcg_iterations, self.huber)
        cost0 = out[4]
        for _ in range(self.outlier_rounds):
            # PoseGraphOptimizer's rule: a graph is taken through a round only as a whole; where the pass so far was refused,
            # or the pass on the cleared edges is, it keeps the state, the cost, `ok` AND the mask of the pass that produced them
            cleared = valid & ~((out[3] > self.outlier_chi2) & ~keep)
            again = ops.simgraph_refine(out[0], out[1], out[2], *edges, fixed, cleared, self.iterations, self.pcg_iterations, 0.0)
            take = out[8] & again[8]
            out = tuple(torch.where(take.view(-1, *([1] * (a.dim() - 1))), b2, a) for a, b2 in zip(out, again))
            valid = torch.where(take.view(-1, 1), cleared, valid)
        s_o, r_o, t_o, chi2, _, cost, _, info, ok = out
        res = (s_o, r_o, t_o, valid, chi2, cost0, cost, info, ok)
        return tuple(o[0] for o in res) if single else res

    @staticmethod
    @torch.no_grad()
    def edges_from_state(R: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s: torch.Tensor | None = None):
        """(s_meas, R_meas, t_meas) of the edges (i, j) from the current state: s_z = s_j / s_i, R_z = R_j R_i^T,
        t_z = t_j - s_z R_z t_i, so that X_j = s_z R_z X_i + t_z -- the odometry / covisibility edges of an essential graph,
        scale 1 for metric poses (s = None).  float64 in torch, rounded to float32 once.  An index outside [0, N) gives NaN
        (an inactive edge).  (B, ...) or unbatched."""
        R64, t64 = R.double(), t.double()
        s64 = torch.ones(t.shape[:-1], dtype=torch.float64, device=t.device) if s is None else s.double()
        n = R.shape[-3]
        idx = edge_index.long()
        inside = ((idx >= 0) & (idx < n)).all(-1)
        i, j = idx[..., 0].clamp(0, n - 1), idx[..., 1].clamp(0, n - 1)

        def pick(a, k):                                     # a (..., N, *tail), k (..., E) -> (..., E, *tail)
            tail = a.shape[k.dim():]
            return torch.gather(a, k.dim() - 1, k.reshape(*k.shape, *([1] * len(tail))).expand(*k.shape, *tail))
        Ri, Rj, ti, tj, si, sj = pick(R64, i), pick(R64, j), pick(t64, i), pick(t64, j), pick(s64, i), pick(s64, j)
        zs = sj / si
        zr = Rj @ Ri.transpose(-1, -2)
        zt = tj - zs[..., None] * (zr @ ti[..., None])[..., 0]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=t.device)
        zs, zr, zt = torch.where(inside, zs, nan), torch.where(inside[..., None, None], zr, nan), torch.where(inside[..., None], zt, nan)
        return zs.float(), zr.float(), zt.float()

    @staticmethod
    def information_from_pose(info6: torch.Tensor, scale_weight):
        """A (..., 6, 6) information matrix in (rotation, translation) order, what the pose estimators and refiners return,
        padded to (..., 7, 7) with `scale_weight` (a number or a (...) tensor: 1 / sigma^2 of the log-scale) on the new
        diagonal element and zeros beside it: an edge that says nothing about the scale beyond that weight."""
        out = torch.zeros(*info6.shape[:-2], 7, 7, dtype=info6.dtype, device=info6.device)
        out[..., :6, :6] = info6
        out[..., 6, 6] = torch.as_tensor(scale_weight, dtype=info6.dtype, device=info6.device)
        return out

    @staticmethod
    @torch.no_grad()
    def correct(R_old: torch.Tensor | None, t_old: torch.Tensor | None, s: torch.Tensor | None, R: torch.Tensor | None,
                t: torch.Tensor | None, points: torch.Tensor | None = None, ref: torch.Tensor | None = None):
        """`mi_simgraph_correct`: metric poses R_old (B, N, 3, 3), t_old (B, N, 3) before, the optimised state s (B, N), R, t,
        landmarks points (B, L, 3) and the keyframe ref (B, L) each is attached to -> (R_out, t_out, points_out): R', t' / s' and
        every landmark where its reference keyframe sees it as before, depths in the new unit -- what BundleAdjuster takes
        next.  The poses or the landmarks may be None.  Unbatched input gives unbatched output."""
        lead = s if s is not None else points
        single = lead is not None and lead.dim() == (1 if s is not None else 2)
        if single:
            R_old, t_old, s, R, t, points, ref = (None if a is None else a.unsqueeze(0) for a in (R_old, t_old, s, R, t, points, ref))
        out = ops.simgraph_correct(R_old, t_old, s, R, t, points, ref)
        return tuple(None if x is None else x[0] for x in out) if single else out
