"""Undistorter and StereoRectifier -- a real lens to the ideal pinhole camera every other module assumes: the sampling map of a
camera, the remap of frames through it, the undistortion of keypoints, the rectifying rotations of a stereo rig.  K34:
`mi_rectify_map`, `mi_rectify_remap`, `mi_rectify_points`, `mi_rectify_stereo_rig`; the arithmetic is stated in
include/mi355x_match_rectify.h.  The reference has no module for it: its camera wrapper receives the intrinsic matrix and the
distortion coefficients from the device and keeps fx, fy, cx, cy only (pytorch_model/vo/camera.py); a host calls
cv2.initUndistortRectifyMap, cv2.remap, cv2.undistortPoints and cv2.stereoRectify on the CPU."""
import torch
from torch import nn

from ... import ops


def _matrix(value, what: str) -> torch.Tensor:
    m = torch.as_tensor(value, dtype=torch.float64, device="cpu")
    if tuple(m.shape) != (3, 3):
        raise ValueError(f"{what} must be a 3x3 matrix, got shape {tuple(m.shape)}")
    return m.clone()


def _size(value, what: str):
    h, w = (int(v) for v in value)
    if not (1 <= h <= ops.RECTIFY_MAX_DIM and 1 <= w <= ops.RECTIFY_MAX_DIM):
        raise ValueError(f"{what} must be (height, width) in 1 .. {ops.RECTIFY_MAX_DIM}, got {tuple(value)}")
    return h, w


class Undistorter(nn.Module):
    """forward(frames) -> the frames as the ideal camera `new_camera_matrix` (default: camera_matrix) sees them after `rotation`
    (default: none): frames (B, H, W) or (B, 1, H, W), uint8, uint16 or float32 -- what FrameIngest returns, or depth counts --,
    with (H, W) = size; the output has out_size (default: size).  The map is built once, in the constructor, on `device`.
    dist_coeffs: OpenCV's 4, 5 or 8 for model="pinhole" (k1 k2 p1 p2 [k3 [k4 k5 k6]]), k1 .. k4 for model="fisheye"
    (Kannala-Brandt).  interpolation "linear" (uint16 frames are always sampled "nearest") or "nearest"; a tap outside the source
    reads border_value.
    .map (h, w, 2) int32 and .mask (h, w) bool, True where every tap of a pixel lies inside the source.
    .points(keypoints, normalised=True): keypoints (B, n, 2) or (n, 2) in pixel (y, x) order, as the detectors return them ->
    (points, ok): normalised (x, y) of the rectified camera, as ops.normalise_keypoints gives for an ideal one, or with
    normalised=False its pixels in (y, x) order; (0, 0) where ok is False."""

    def __init__(self, camera_matrix, dist_coeffs, size, model: str = "pinhole", new_camera_matrix=None, rotation=None, out_size=None,
                 interpolation: str = "linear", border_value: float = 0.0, iterations: int = 10, max_residual_px: float = 0.5,
                 device="cuda") -> None:
        super().__init__()
        self.model = ops.rectify_model(model)
        self.camera_matrix = _matrix(camera_matrix, "camera_matrix")
        self.new_camera_matrix = self.camera_matrix.clone() if new_camera_matrix is None else _matrix(new_camera_matrix, "new_camera_matrix")
        self.rotation = None if rotation is None else _matrix(rotation, "rotation")
        self.dist_coeffs = torch.tensor(list(ops.rectify_coeffs(dist_coeffs, self.model)), dtype=torch.float64)
        self.size, self.out_size = _size(size, "size"), _size(size if out_size is None else out_size, "out_size")
        if interpolation not in ("linear", "nearest"):
            raise ValueError(f"interpolation must be 'linear' or 'nearest', got {interpolation!r}")
        if not 1 <= iterations <= ops.RECTIFY_MAX_ITERATIONS:
            raise ValueError(f"iterations must be in 1 .. {ops.RECTIFY_MAX_ITERATIONS}, got {iterations}")
        if not max_residual_px > 0:
            raise ValueError(f"max_residual_px must be positive, got {max_residual_px}")
        self.interpolation = ops.RECTIFY_LINEAR if interpolation == "linear" else ops.RECTIFY_NEAREST
        self.border_value, self.iterations, self.max_residual_px = float(border_value), int(iterations), float(max_residual_px)
        map_, mask = ops.rectify_map(self.camera_matrix, self.dist_coeffs, self.size, self.new_camera_matrix, self.out_size, self.rotation,
                                     self.model, device)
        self.register_buffer("map", map_)
        self.register_buffer("mask", mask.view(torch.bool))

    @torch.no_grad()
    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        if tuple(frames.shape[-2:]) != self.size:
            raise RuntimeError(f"the frames must be {self.size} high and wide, got {tuple(frames.shape)}")
        nearest = frames.dtype == torch.uint16 or self.interpolation == ops.RECTIFY_NEAREST
        return ops.rectify_remap(frames, self.map, ops.RECTIFY_NEAREST if nearest else ops.RECTIFY_LINEAR, self.border_value)

    @torch.no_grad()
    def points(self, keypoints: torch.Tensor, normalised: bool = True):
        single = keypoints.dim() == 2
        kp = keypoints.unsqueeze(0) if single else keypoints
        if kp.dim() != 3 or kp.shape[-1] != 2:
            raise RuntimeError(f"keypoints must be (B, n, 2) or (n, 2), got {tuple(keypoints.shape)}")
        if not kp.is_cuda:
            raise RuntimeError(f"keypoints must live on the GPU (got device {kp.device}); this package has no CPU path")
        out, ok = ops.rectify_points(kp.float().flip(-1).contiguous(), self.camera_matrix, self.dist_coeffs, self.rotation,
                                     None if normalised else self.new_camera_matrix, self.model, self.iterations, self.max_residual_px)
        if not normalised:
            out = out.flip(-1)
        return (out[0], ok[0]) if single else (out, ok)


class StereoRectifier(nn.Module):
    """forward(left, right) -> the rectified pair StereoMatcher takes: a scene point lies on one row of both outputs, at
    x_right = x_left - d with d >= 0.  k1, d1 / k2, d2: camera matrix and distortion coefficients of the left / right camera;
    R, T: X2 = R X1 + T, camera 1 on the left; size (height, width) of the raw frames, out_size of the rectified ones (default:
    size).  .r1, .r2, .k_new (3 x 3 float64), .baseline = |T|, .fb = f * baseline (what StereoMatcher.depth and ops.stereo_depth
    want, in T's unit), .left and .right (the two Undistorters, with their .mask and .points)."""

    def __init__(self, k1, d1, k2, d2, R, T, size, model: str = "pinhole", out_size=None, interpolation: str = "linear",
                 border_value: float = 0.0, device="cuda") -> None:
        super().__init__()
        out = _size(size if out_size is None else out_size, "out_size")
        t = torch.as_tensor(T, dtype=torch.float64, device="cpu").reshape(-1)
        if t.numel() != 3:
            raise ValueError(f"T must have 3 elements, got {t.numel()}")
        try:
            self.r1, self.r2, self.k_new, self.baseline, self.fb = ops.rectify_stereo_rig(_matrix(k1, "k1"), _matrix(k2, "k2"), _matrix(R, "R"), t, out)
        except RuntimeError as e:
            raise ValueError(f"the rig cannot be rectified (no baseline, a swapped or vertical rig, or values that are not finite): {e}") from None
        self.left = Undistorter(k1, d1, size, model, self.k_new, self.r1, out, interpolation, border_value, device=device)
        self.right = Undistorter(k2, d2, size, model, self.k_new, self.r2, out, interpolation, border_value, device=device)

    @torch.no_grad()
    def forward(self, left: torch.Tensor, right: torch.Tensor):
        return self.left(left), self.right(right)
