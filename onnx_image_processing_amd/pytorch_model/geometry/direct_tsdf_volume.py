"""DirectTsdfVolume -- TsdfVolume with gray values in the model: a second volume of (gray, gweight) records is fused beside the
signed distance, the raycast returns the model's intensity map as well, and tracking hands (vertex, normal, intensity) to the
joint refinement of DirectRgbdRefiner in place of the depth-only ICP, so that a textured wall, floor or table top no longer
freezes frame-to-model tracking.  The extracted mesh and point cloud carry a gray value per vertex.  K22:
`mi_tsdf_gray_reset`, `mi_tsdf_integrate_gray`, `mi_tsdf_sample_gray`.  The algorithms are stated in include/mi355x_match.h.
The reference has no counterpart."""
import math

import torch

from ... import ops
from .tsdf_volume import TsdfVolume


class DirectTsdfVolume(TsdfVolume):
    """TsdfVolume's constructor, and photo_weight and intensity_threshold as in DirectRgbdRefiner (the weight of one gray level
    in the depth's unit, 0 turns the term off and gives TsdfVolume's tracking; residuals above the threshold, in gray levels,
    are dropped).  The buffer `intensity` (batch, NZ, NY, NX, 2) float32 holds the (gray, gweight) records beside `volume`.
    Gray frames are float32 or uint8 (FrameIngest's outputs) of the depth's shape, in the depth's camera.

    reset()                                    both volumes empty
    integrate(depth, gray, R, t, active=None)  TsdfVolume.integrate's shapes; `volume` gets its bits, `intensity` the running
                                               mean of the gray value in the truncation band of every seen surface, in one pass
    raycast(R, t, size=None)                   -> (vertex, normal, intensity), each (B, H, W, 4): the parent's raycast and the
                                               intensity volume gathered at its vertices, `ops.intensity_maps`' layout with
                                               zero gradients (a frame 1 for `ops.rgbd_refine`)
    track(depth, gray, R_pred, t_pred)         -> (R, t, information, rmse, count, rmse_photo, count_photo, ok): the raycast at
                                               the prediction against the live frame's surfel and intensity maps, refined from
                                               the identity by `ops.rgbd_refine`, composed onto the prediction
    forward(depth, gray, R_pred, t_pred)       track, then integrate at the tracked pose where ok; the same outputs
    extract_surface(...) / extract_points(...) the parent's tuple with intensity (B, MV) float32 and intensity_valid (B, MV) bool
                                               appended: the intensity volume gathered at the world vertices

    Everything runs on the current stream without a synchronisation and is capturable, except an extraction without
    capacities, as in the parent."""

    def __init__(self, *args, photo_weight: float = 0.003, intensity_threshold: float = 30.0, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        if not (photo_weight >= 0 and math.isfinite(photo_weight)):
            raise ValueError(f"photo_weight must be finite and not negative, got {photo_weight}")
        if not (intensity_threshold > 0 and math.isfinite(intensity_threshold)):
            raise ValueError(f"intensity_threshold must be positive and finite, got {intensity_threshold}")
        self.photo_weight = float(photo_weight)
        self.intensity_threshold = float(intensity_threshold)
        self.register_buffer("intensity", torch.zeros_like(self.volume))                 # empty: what reset() writes

    def _gray_like(self, gray: torch.Tensor, depth: torch.Tensor) -> None:
        if gray.shape != depth.shape:
            raise RuntimeError(f"gray must have depth's shape {tuple(depth.shape)}, got {tuple(gray.shape)}")
        self._on_gpu(depth, "depth")
        self._on_gpu(gray, "gray")

    @torch.no_grad()
    def reset(self) -> None:
        super().reset()
        ops.tsdf_gray_reset(self.intensity)

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, gray: torch.Tensor, R: torch.Tensor, t: torch.Tensor,
                  active: torch.Tensor | None = None) -> None:
        if depth.dim() not in (3, 4) or depth.shape[0] != self.batch:
            raise RuntimeError(f"depth must have shape ({self.batch}, H, W) or ({self.batch}, F, H, W), got {tuple(depth.shape)}")
        self._gray_like(gray, depth)
        d, g = (depth.unsqueeze(1), gray.unsqueeze(1)) if depth.dim() == 3 else (depth, gray)
        f = int(d.shape[1])
        ops.tsdf_integrate_gray(self.volume, self.intensity, d, g, R.reshape(self.batch, f, 3, 3), t.reshape(self.batch, f, 3),
                                self.camera, self.origin, self.voxel_size, self.truncation, self.max_weight, self.depth_scale,
                                self.min_depth, self.max_depth, None if active is None else active.reshape(self.batch, f))

    @torch.no_grad()
    def raycast(self, R: torch.Tensor, t: torch.Tensor, size=None):
        r, tt = R.reshape(self.batch, 3, 3), t.reshape(self.batch, 3)
        vertex, normal = super().raycast(r, tt, size)
        return vertex, normal, ops.tsdf_sample_gray(self.intensity, vertex, self.origin, self.voxel_size, r, tt)

    @torch.no_grad()
    def track(self, depth: torch.Tensor, gray: torch.Tensor, R_pred: torch.Tensor, t_pred: torch.Tensor):
        if depth.dim() != 3 or depth.shape[0] != self.batch:
            raise RuntimeError(f"depth must have shape ({self.batch}, H, W), got {tuple(depth.shape)}")
        self._gray_like(gray, depth)
        b, dev = self.batch, depth.device
        r_pred, t_pred = R_pred.reshape(b, 3, 3).float().contiguous(), t_pred.reshape(b, 3).float().contiguous()
        model = self.raycast(r_pred, t_pred, (int(depth.shape[1]), int(depth.shape[2])))
        live = (*ops.surfel_maps(depth, self.K_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump),
                ops.intensity_maps(gray))
        eye = torch.eye(3, device=dev).expand(b, 3, 3).contiguous()
        r_i, t_i, info, rmse, count, rmse_photo, count_photo, _, ok = ops.rgbd_refine(
            model, live, eye, torch.zeros((b, 3), device=dev), self.camera, self.schedule, self.distance_threshold,
            self.angle_threshold, self.photo_weight, self.intensity_threshold, self.min_correspondences)
        r, t = ops.pose_compose(r_i, t_i, r_pred, t_pred)
        return r, t, info, rmse, count, rmse_photo, count_photo, ok

    def _vertex_gray(self, vertices: torch.Tensor):
        rec = ops.tsdf_sample_gray(self.intensity, vertices, self.origin, self.voxel_size)
        return rec[..., 0], rec[..., 3] != 0

    @torch.no_grad()
    def extract_surface(self, max_vertices: int | None = None, max_triangles: int | None = None, min_weight: float = 1.0):
        out = super().extract_surface(max_vertices, max_triangles, min_weight)
        return (*out, *self._vertex_gray(out[0]))

    @torch.no_grad()
    def extract_points(self, max_points: int | None = None, min_weight: float = 1.0):
        out = super().extract_points(max_points, min_weight)
        return (*out, *self._vertex_gray(out[0]))

    @torch.no_grad()
    def forward(self, depth: torch.Tensor, gray: torch.Tensor, R_pred: torch.Tensor, t_pred: torch.Tensor):
        out = self.track(depth, gray, R_pred, t_pred)
        self.integrate(depth, gray, out[0], out[1], out[7])
        return out
