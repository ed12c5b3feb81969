"""TsdfVolume -- the fused model of an RGB-D odometry: depth frames integrated into a truncated signed distance volume, the
volume raycast at a predicted pose into a synthetic surfel map, and that map handed to the point-to-plane ICP of
DenseRgbdRefiner in place of a single noisy depth frame (frame-to-model tracking).  K19: `mi_tsdf_reset`,
`mi_tsdf_integrate`, `mi_tsdf_raycast`, `mi_pose_compose`; K20 takes the fused surface out as a triangle mesh or a point cloud:
`mi_tsdf_surface`.  The algorithms are stated in include/mi355x_match.h.  The reference has no counterpart."""
import math

import torch
from torch import nn

from ... import ops


class TsdfVolume(nn.Module):
    """`batch` volumes of dims = (NX, NY, NZ) voxels of voxel_size, the corner of voxel (0, 0, 0) at origin (x, y, z), kept as
    the buffer `volume` (batch, NZ, NY, NX, 2) float32 of (tsdf, weight) records.  Poses are world (the volume's frame) to
    camera, X_c = R X_w + t, the convention of RgbdPoseEstimator / DenseRgbdRefiner with the volume as frame 1.  Depth frames
    are float32 or uint16, ALREADY aligned to the camera of K (DepthAlignment); depth_scale turns a depth value into the unit
    of voxel_size, pixels outside [min_depth, max_depth] are ignored.

    reset()                              every voxel empty: (1, 0)
    integrate(depth, R, t, active=None)  depth (B, H, W) with R (B, 3, 3), t (B, 3), or (B, F, H, W) with (B, F, 3, 3), (B, F, 3):
                                         the frames fused in order in one pass over the volume; active (B,) / (B, F) bool on
                                         the GPU leaves frames out without a synchronisation
    raycast(R, t, size=None)             -> (vertex, normal), each (B, H, W, 4) in the camera frame, `ops.surfel_maps`' layout;
                                         size = (H, W) defaults to the constructor's
    track(depth, R_pred, t_pred)         -> (R, t, information, rmse, count, ok): the raycast at the prediction against the
                                         surfel maps of depth (B, H, W), refined from the identity by `ops.icp_refine` with the
                                         gates of DenseRgbdRefiner, composed onto the prediction.  ok is False -- with the
                                         pose before the failed step -- where the system was degenerate (an empty volume
                                         returns the prediction)
    forward(depth, R_pred, t_pred)       track, then integrate at the tracked pose where ok; the same outputs
    extract_surface(max_vertices=None, max_triangles=None, min_weight=1.0)
                                         -> (vertices, normals, triangles, counts): the fused surface as an indexed triangle
                                         mesh in the world frame (K20, marching tetrahedra)
    extract_points(max_points=None, min_weight=1.0)
                                         -> (points, normals, counts): the mesh's vertices alone, a point cloud

    truncation defaults to 4 voxels; max_weight caps the running mean's memory; the raycast samples every step_fraction (at
    most 1) of the truncation.  Everything runs on the current stream without a synchronisation and is capturable, except an
    extraction without capacities, which reads the counts back once to size its outputs."""

    def __init__(self, K: torch.Tensor, dims, voxel_size: float, origin, truncation: float | None = None, max_weight: float = 64.0,
                 step_fraction: float = 0.5, depth_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                 batch: int = 1, size=None, schedule=((4, 4), (2, 4), (1, 6)), distance_threshold: float = 0.1,
                 angle_threshold_deg: float = 30.0, normal_max_jump: float = 0.1, min_correspondences: int = 64) -> None:
        super().__init__()
        K_f = torch.as_tensor(K).float()
        if tuple(K_f.shape) != (3, 3):
            raise ValueError(f"K must be a 3x3 camera matrix, got shape {tuple(K_f.shape)}")
        try:
            nx, ny, nz = (int(d) for d in dims)
            ox, oy, oz = (float(o) for o in origin)
        except (TypeError, ValueError):
            raise ValueError(f"dims and origin must be 3 values each, got {dims!r} and {origin!r}") from None
        if min(nx, ny, nz) < 2:
            raise ValueError(f"every dimension must be at least 2 voxels, got {(nx, ny, nz)}")
        if not 1 <= int(batch) <= 65535 or int(batch) * nx * ny * nz >= 2 ** 31:
            raise ValueError(f"need 1 <= batch <= 65535 and batch * voxels < 2^31, got batch {batch} of {(nx, ny, nz)}")
        if not all(math.isfinite(o) for o in (ox, oy, oz)):
            raise ValueError(f"origin must be finite, got {origin}")
        if not (voxel_size > 0 and math.isfinite(voxel_size)):
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        truncation = 4.0 * voxel_size if truncation is None else truncation
        if not (truncation > 0 and math.isfinite(truncation)):
            raise ValueError(f"truncation must be positive, got {truncation}")
        if not (max_weight > 0 and math.isfinite(max_weight)):
            raise ValueError(f"max_weight must be positive, got {max_weight}")
        if not 0 < step_fraction <= 1:
            raise ValueError(f"step_fraction must be in (0, 1], got {step_fraction}")
        if not depth_scale > 0:
            raise ValueError(f"depth_scale must be positive, got {depth_scale}")
        if not min_depth > 0 or not max_depth >= min_depth or not math.isfinite(max_depth):
            raise ValueError(f"need 0 < min_depth <= max_depth, got {min_depth}, {max_depth}")
        if size is not None and (len(tuple(size)) != 2 or min(int(s) for s in size) < 3):
            raise ValueError(f"size must be (H, W) with H, W >= 3, got {size}")
        try:
            sched = tuple((int(s), int(i)) for s, i in schedule)
        except (TypeError, ValueError):
            raise ValueError(f"schedule must be a sequence of (stride, iterations) pairs, got {schedule!r}") from None
        if not 1 <= len(sched) <= ops.ICP_MAX_STAGES:
            raise ValueError(f"schedule needs 1 .. {ops.ICP_MAX_STAGES} stages, got {len(sched)}")
        if any(s not in ops.ICP_STRIDES or i < 0 for s, i in sched):
            raise ValueError(f"every stage needs a stride in {ops.ICP_STRIDES} and iterations >= 0, got {sched}")
        if sum(i for _, i in sched) > ops.ICP_MAX_ITERATIONS:
            raise ValueError(f"at most {ops.ICP_MAX_ITERATIONS} iterations in all, got {sum(i for _, i in sched)}")
        if not distance_threshold > 0:
            raise ValueError(f"distance_threshold must be positive, got {distance_threshold}")
        if not 0 < angle_threshold_deg <= 180:
            raise ValueError(f"angle_threshold_deg must be in (0, 180], got {angle_threshold_deg}")
        if not normal_max_jump > 0:
            raise ValueError(f"normal_max_jump must be positive, got {normal_max_jump}")
        if min_correspondences < 1:
            raise ValueError(f"min_correspondences must be positive, got {min_correspondences}")
        self.register_buffer("K", K_f)
        self.register_buffer("K_inv", torch.linalg.inv(K_f.cpu()).to(K_f.device))
        volume = torch.zeros((int(batch), nz, ny, nx, 2), dtype=torch.float32)
        volume[..., 0] = 1.0                                         # empty: what reset() writes
        self.register_buffer("volume", volume)
        self.camera = (float(K_f[0, 0]), float(K_f[1, 1]), float(K_f[0, 2]), float(K_f[1, 2]))
        self.dims = (nx, ny, nz)
        self.batch = int(batch)
        self.origin = (ox, oy, oz)
        self.voxel_size = float(voxel_size)
        self.truncation = float(truncation)
        self.max_weight = float(max_weight)
        self.step_fraction = float(step_fraction)
        self.depth_scale = float(depth_scale)
        self.min_depth = float(min_depth)
        self.max_depth = float(max_depth)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.schedule = sched
        self.distance_threshold = float(distance_threshold)
        self.angle_threshold = math.radians(float(angle_threshold_deg))
        self.normal_max_jump = float(normal_max_jump)
        self.min_correspondences = int(min_correspondences)

    def _on_gpu(self, x: torch.Tensor, what: str) -> None:
        if not x.is_cuda or not self.volume.is_cuda:
            dev = x.device if not x.is_cuda else self.volume.device
            raise RuntimeError(f"TsdfVolume: {what} and the volume must live on the GPU (got device {dev}); this package has no "
                               f"CPU path")

    @torch.no_grad()
    def reset(self) -> None:
        self._on_gpu(self.volume, "the volume")
        ops.tsdf_reset(self.volume)

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, R: torch.Tensor, t: torch.Tensor, active: torch.Tensor | None = None) -> None:
        if depth.dim() not in (3, 4) or depth.shape[0] != self.batch:
            raise RuntimeError(f"depth must have shape ({self.batch}, H, W) or ({self.batch}, F, H, W), got {tuple(depth.shape)}")
        self._on_gpu(depth, "depth")
        d = depth.unsqueeze(1) if depth.dim() == 3 else depth
        f = int(d.shape[1])
        ops.tsdf_integrate(self.volume, d, R.reshape(self.batch, f, 3, 3), t.reshape(self.batch, f, 3), self.camera, self.origin,
                           self.voxel_size, self.truncation, self.max_weight, self.depth_scale, self.min_depth, self.max_depth,
                           None if active is None else active.reshape(self.batch, f))

    @torch.no_grad()
    def raycast(self, R: torch.Tensor, t: torch.Tensor, size=None):
        self._on_gpu(R, "the pose")
        size = self.size if size is None else size
        if size is None:
            raise RuntimeError("raycast needs size = (H, W): none was given here or to the constructor")
        return ops.tsdf_raycast(self.volume, R.reshape(self.batch, 3, 3), t.reshape(self.batch, 3), self.K_inv, size, self.origin,
                                self.voxel_size, self.truncation, self.step_fraction, self.min_depth, self.max_depth)

    @torch.no_grad()
    def track(self, depth: torch.Tensor, R_pred: torch.Tensor, t_pred: torch.Tensor):
        if depth.dim() != 3 or depth.shape[0] != self.batch:
            raise RuntimeError(f"depth must have shape ({self.batch}, H, W), got {tuple(depth.shape)}")
        self._on_gpu(depth, "depth")
        b, dev = self.batch, depth.device
        r_pred, t_pred = R_pred.reshape(b, 3, 3).float().contiguous(), t_pred.reshape(b, 3).float().contiguous()
        model = self.raycast(r_pred, t_pred, (int(depth.shape[1]), int(depth.shape[2])))
        live = ops.surfel_maps(depth, self.K_inv, self.depth_scale, self.min_depth, self.max_depth, self.normal_max_jump)
        eye = torch.eye(3, device=dev).expand(b, 3, 3).contiguous()
        r_i, t_i, info, rmse, count, _, ok = ops.icp_refine(model, live, eye, torch.zeros((b, 3), device=dev), self.camera,
                                                            self.schedule, self.distance_threshold, self.angle_threshold,
                                                            self.min_correspondences)
        r, t = ops.pose_compose(r_i, t_i, r_pred, t_pred)
        return r, t, info, rmse, count, ok

    def _capacities(self, max_vertices, max_triangles, min_weight: float, triangles: bool):
        """the capacities as given, or -- where one is None -- the exact totals from the sizing pass: ONE host round trip.  The
        sizing pass allocates its own workspace (a byte per voxel), as the extraction after it does again."""
        # extract_points passes triangles=False and max_triangles=None: no triangle capacity is wanted, so 0 without a sizing pass
        if max_vertices is not None and (max_triangles is not None or not triangles):
            return int(max_vertices), int(max_triangles or 0)
        counts = ops.tsdf_surface_counts(self.volume, min_weight).max(dim=0).values.tolist()      # synchronises
        return (counts[0] if max_vertices is None else int(max_vertices),
                counts[1] if max_triangles is None else int(max_triangles))

    @torch.no_grad()
    def extract_surface(self, max_vertices: int | None = None, max_triangles: int | None = None, min_weight: float = 1.0):
        """K20, `mi_tsdf_surface`: the fused surface as an indexed triangle mesh -> (vertices (B, MV, 4) float32 (x, y, z, 1) in
        the world frame, normals (B, MV, 4) (unit, towards free space, 1; zeros where the gradient is not available), triangles
        (B, MT, 3) int32 vertex ids, counts (B, 2) int32 = the true (vertices, triangles) of every volume).  Volume b's mesh is
        the first counts[b, 0] vertices and counts[b, 1] triangles; the rows after them are zeros and (-1, -1, -1).  A voxel
        counts as observed from weight >= min_weight.
        With both capacities given it runs on the current stream without a synchronisation and is capturable; counts above a
        capacity mean an incomplete mesh.  With a capacity None it first runs the sizing pass and reads the counts back -- one
        host synchronisation -- so that the arrays hold exactly the largest volume's mesh."""
        self._on_gpu(self.volume, "the volume")
        mv, mt = self._capacities(max_vertices, max_triangles, min_weight, True)
        return ops.tsdf_surface(self.volume, self.origin, self.voxel_size, mv, mt, min_weight)

    @torch.no_grad()
    def extract_points(self, max_points: int | None = None, min_weight: float = 1.0):
        """The vertices of `extract_surface` on their own -> (points (B, MP, 4), normals (B, MP, 4), counts (B, 2)); no triangle
        is formed.  max_points None: the sizing pass and one host synchronisation, as above.  The cloud of volume b is
        points[b, :counts[b, 0], :3]: `ops.voxel_downsample_batch` (VoxelDownsampling, K12) takes the list of these slices."""
        self._on_gpu(self.volume, "the volume")
        mp, _ = self._capacities(max_points, None, min_weight, False)
        points, normals, _, counts = ops.tsdf_surface(self.volume, self.origin, self.voxel_size, mp, 0, min_weight, triangles=False)
        return points, normals, counts

    @torch.no_grad()
    def forward(self, depth: torch.Tensor, R_pred: torch.Tensor, t_pred: torch.Tensor):
        out = self.track(depth, R_pred, t_pred)
        self.integrate(depth, out[0], out[1], out[5])
        return out
