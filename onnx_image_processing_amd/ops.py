"""Functional layer over the C ABI: shape checks, output/workspace allocation, launch.

Everything here is asynchronous on torch's current HIP stream.  Outputs are fresh torch
tensors on the input's device (the reference's ownership convention); workspaces come from
torch's caching allocator, so a steady-state step performs no hipMalloc.
"""
from __future__ import annotations

import torch

from . import _native as N
from .distributed import RECORD_FIELDS, tag_record

F32 = torch.float32


U8 = torch.uint8


def convert_u8(image: torch.Tensor) -> torch.Tensor:
    """uint8 device tensor -> float32 of the same shape (`mi_convert_u8_f32`): what the reference's hosts do on the CPU
    before calling the model (sample/visual_odometry.py:65-92)."""
    src = image.contiguous()
    out = torch.empty(src.shape, dtype=F32, device=src.device)
    if src.numel():
        N.call("mi_convert_u8_f32", N.dev(src, U8, "image"), src.numel(), out.data_ptr(), N.stream_ptr())
    return out


class ImagePair:
    """image1 / image2 of a matcher (two equally shaped (B,1,H,W) batches) as ONE batch of 2B images, batch a first, for
    the front-end entry points that take two base pointers (`mi_corner_response_pair`, `mi_sparse_bad_pair`,
    `mi_angle_at_keypoints_pair`, `mi_sparse_bad_oriented_pair`): nothing is concatenated, every stage is one launch
    for both images, and what follows (NMS, top-k, ...) runs on ordinary (2B, ...) tensors.  Accepted wherever those four
    ops take `image`."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor):
        if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
            raise RuntimeError(f"image batches differ: {tuple(a.shape)} {a.dtype} {a.device} vs {tuple(b.shape)} {b.dtype} {b.device}")
        self.a, self.b = a, b

    @property
    def device(self):
        return self.a.device

    @property
    def dtype(self):
        return self.a.dtype

    @property
    def shape(self):
        return torch.Size((2 * self.a.shape[0],) + tuple(self.a.shape[1:]))


def _images(image, what: str, keep_u8: bool = False):
    """(N,1,H,W) image batch as a contiguous float32 tensor.  uint8 frames (the u8 ingest path): kept as they are for
    the entry points that have a uint8 form (keep_u8), converted on the device for the others.  An ImagePair comes
    back as an ImagePair of two such tensors."""
    if isinstance(image, ImagePair):
        return ImagePair(_images(image.a, what, keep_u8), _images(image.b, what, keep_u8))
    if image.dim() != 4 or image.shape[1] != 1:
        raise RuntimeError(f"{what} must have shape (N, 1, H, W), got {tuple(image.shape)}")
    if image.dtype == U8:
        return image.contiguous() if keep_u8 else convert_u8(image)
    return image.float().contiguous()


def _workspace(query: str, *args, device, refusal: str | None = None):
    """The library workspace of one call, sized by the `*_workspace_bytes` entry `query`(*args) -> (int64 tensor of
    ceil(bytes / 16) * 2 words, bytes).  The library is told the queried count, not the rounded one.  A size of 0 means
    the request is outside what the entry point covers: RuntimeError(refusal) for the ops that have a refusal text."""
    wbytes = int(getattr(N.library_of(query), query)(*args))
    if wbytes == 0 and refusal is not None:
        raise RuntimeError(refusal)
    return torch.empty(((wbytes + 15) // 16 * 2,), dtype=torch.int64, device=device), wbytes


TILE_COUNTER_BYTES = N.MI_TILE_COUNTER_BYTES

# Sinkhorn solver flags handed to mi_sinkhorn_dots / mi_match_pairs (include/mi355x_match.h, "co-residency"):
# 0 = MI_SOLVER_DEFAULT; MI_SOLVER_MULTI_LAUNCH for a process that shares its GPU with long-running foreign kernels;
# MI_SOLVER_NO_FORK keeps the >= 64-pair Sinkhorn on the caller's stream (no helper streams, no events, no tuning).
# A preference of this Python layer (the C library has no process-wide switch); results are identical either way.
MI_SOLVER_DEFAULT, MI_SOLVER_MULTI_LAUNCH, MI_SOLVER_NO_FORK = N.MI_SOLVER_DEFAULT, N.MI_SOLVER_MULTI_LAUNCH, N.MI_SOLVER_NO_FORK
# (not a preference: sinkhorn_bits sets it by itself when the descriptors have fewer than 1024 bits, which is what lets
# mi_sinkhorn_dots' row kernel read the uint16 dot products as fp16 denormals)
MI_SOLVER_DOTS_BELOW_1024 = N.MI_SOLVER_DOTS_BELOW_1024
_solver_flags = MI_SOLVER_DEFAULT


def set_solver_flags(flags: int) -> None:
    global _solver_flags
    if not isinstance(flags, int) or flags & ~(MI_SOLVER_MULTI_LAUNCH | MI_SOLVER_NO_FORK):
        raise ValueError("solver flags must be MI_SOLVER_DEFAULT (0) or an OR of MI_SOLVER_MULTI_LAUNCH (1) and "
                         f"MI_SOLVER_NO_FORK (2), got {flags}")
    _solver_flags = int(flags)


MI_SCHEDULE_UNDECIDED, MI_SCHEDULE_CALLER_HELPER, MI_SCHEDULE_TWO_HELPERS, MI_SCHEDULE_UNSPLIT = (
    N.MI_SCHEDULE_UNDECIDED, N.MI_SCHEDULE_CALLER_HELPER, N.MI_SCHEDULE_TWO_HELPERS, N.MI_SCHEDULE_UNSPLIT)


def sinkhorn_schedule(batch: int, n: int, m: int, iterations: int) -> int:
    """The stream schedule in force for mi_sinkhorn_dots calls of this shape on torch's current stream
    (`mi_sinkhorn_dots_schedule`): MI_SCHEDULE_UNDECIDED until the tuner has decided or a schedule is pinned."""
    return int(N.load().mi_sinkhorn_dots_schedule(N.stream_ptr(), int(batch), int(n), int(m), int(iterations)))


def set_sinkhorn_schedule(schedule: int) -> None:
    """Pin a stream schedule for torch's current stream, or MI_SCHEDULE_UNDECIDED to start tuning over
    (`mi_sinkhorn_dots_set_schedule`)."""
    N.check(N.load().mi_sinkhorn_dots_set_schedule(N.stream_ptr(), int(schedule)), "mi_sinkhorn_dots_set_schedule")


def corner_response(image: torch.Tensor, block_size: int) -> torch.Tensor:
    img = _images(image, "image", keep_u8=True)
    n, _, h, w = img.shape
    out = torch.empty(img.shape, dtype=F32, device=img.device)
    u8 = img.dtype == U8
    # K1's ticket counters: a fresh block per call from the caching allocator (stream-ordered: no sharing between
    # streams, nothing cached per stream); the library clears it on the stream before the kernel draws from it
    ctr = torch.empty(TILE_COUNTER_BYTES // 4, dtype=torch.int32, device=img.device)
    if isinstance(img, ImagePair):
        N.call("mi_corner_response_pair", N.dev(img.a, U8 if u8 else F32, "image"), N.dev(img.b, U8 if u8 else F32, "image"),
               int(u8), n // 2, h, w, int(block_size), N.dev(out, F32, "score"), ctr.data_ptr(), N.stream_ptr())
        return out
    N.call("mi_corner_response_balanced", N.dev(img, U8 if u8 else F32, "image"), int(u8), n, h, w, int(block_size),
           N.dev(out, F32, "score"), ctr.data_ptr(), N.stream_ptr())
    return out


def _score_maps(scores: torch.Tensor) -> torch.Tensor:
    if scores.dim() != 3:
        raise RuntimeError(f"scores must have shape (B, H, W), got {tuple(scores.shape)}")
    return scores.float().contiguous()


def nms_mask(scores: torch.Tensor, radius: int) -> torch.Tensor:
    s = _score_maps(scores)
    b, h, w = s.shape
    mask = torch.empty_like(s)
    N.call("mi_nms_mask", N.dev(s, F32, "scores"), b, h, w, int(radius), N.dev(mask, F32, "mask"), N.stream_ptr())
    return mask


def candidate_layout(h: int, w: int) -> tuple[int, int]:
    """(segments per image, slots per segment) of the K2 candidate buffer."""
    import ctypes
    seg, cap = ctypes.c_int(0), ctypes.c_int(0)
    N.check(N.load().mi_candidate_layout(int(h), int(w), ctypes.byref(seg), ctypes.byref(cap)), "mi_candidate_layout")
    return seg.value, cap.value


def _candidate_buffers(b: int, h: int, w: int, device):
    seg, cap = candidate_layout(h, w)
    cand = torch.empty((b, seg, cap), dtype=torch.int64, device=device)
    count = torch.empty((b, seg), dtype=torch.int32, device=device)      # fully written by K2
    return cand, count, seg, cap


def _topk_from_candidates(cand, count, seg, cap, b, h, w, k):
    if h * w < k:
        raise RuntimeError(f"selected index k out of range (k={k} > H*W={h * w})")  # torch.topk's failure mode
    kpts = torch.empty((b, k, 2), dtype=F32, device=cand.device)
    ksc = torch.empty((b, k), dtype=F32, device=cand.device)
    N.call("mi_topk_keypoints", cand.data_ptr(), count.data_ptr(), seg, cap, b, w, int(k), kpts.data_ptr(),
           ksc.data_ptr(), N.stream_ptr())
    return kpts, ksc


def nms_topk(scores: torch.Tensor, radius: int, k: int, score_threshold: float = 0.0, border_margin: int = 0):
    """Fused NMS + border + threshold + top-k (the mask is never materialised)."""
    s = _score_maps(scores)
    b, h, w = s.shape
    cand, count, seg, cap = _candidate_buffers(b, h, w, s.device)
    N.call("mi_nms_candidates", N.dev(s, F32, "scores"), b, h, w, int(radius), float(score_threshold),
           int(border_margin), cand.data_ptr(), count.data_ptr(), N.stream_ptr())
    return _topk_from_candidates(cand, count, seg, cap, b, h, w, k)


def select_topk(scores: torch.Tensor, mask: torch.Tensor, k: int, score_threshold: float = 0.0,
                border_margin: int = 0):
    s = _score_maps(scores)
    mk = _score_maps(mask)
    if mk.shape != s.shape:
        raise RuntimeError(f"nms_mask shape {tuple(mk.shape)} != scores shape {tuple(s.shape)}")
    b, h, w = s.shape
    cand, count, seg, cap = _candidate_buffers(b, h, w, s.device)
    N.call("mi_select_candidates", N.dev(s, F32, "scores"), N.dev(mk, F32, "nms_mask"), b, h, w,
           float(score_threshold), int(border_margin), cand.data_ptr(), count.data_ptr(), N.stream_ptr())
    return _topk_from_candidates(cand, count, seg, cap, b, h, w, k)


def bad_plan(pair_geom: torch.Tensor, pair_thr: torch.Tensor) -> torch.Tensor:
    """Device-resident fast-path plan for a pair table (built once; see mi_bad_plan_build)."""
    p = pair_geom.numel()
    nbytes = int(N.load().mi_bad_plan_bytes(p))
    plan = torch.empty(((nbytes + 15) // 16 * 2,), dtype=torch.int64, device=pair_geom.device)
    N.call("mi_bad_plan_build", N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"), p,
           plan.data_ptr(), N.stream_ptr())
    return plan


def sparse_bad(image: torch.Tensor, keypoints: torch.Tensor, pair_geom: torch.Tensor, pair_thr: torch.Tensor,
               mode: int, temperature: float, normalize: bool, want_desc: bool = True, want_bits: bool = False,
               plan: torch.Tensor | None = None):
    img = _images(image, "image", keep_u8=True)
    n, _, h, w = img.shape
    if keypoints.dim() != 3 or keypoints.shape[0] != n or keypoints.shape[2] != 2:
        raise RuntimeError(f"keypoints must have shape ({n}, K, 2), got {tuple(keypoints.shape)}")
    kp = keypoints.float().contiguous()
    k = kp.shape[1]
    p = pair_geom.numel()
    desc = torch.empty((n, k, p), dtype=F32, device=img.device) if want_desc else None
    bits = torch.empty((n, k, p // 32), dtype=torch.int32, device=img.device) if want_bits else None
    u8 = img.dtype == U8
    if isinstance(img, ImagePair):
        N.call("mi_sparse_bad_pair", N.dev(img.a, U8 if u8 else F32, "image"), N.dev(img.b, U8 if u8 else F32, "image"),
               int(u8), n // 2, h, w, N.dev(kp, F32, "keypoints"), k,
               N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"), p, int(mode),
               float(temperature), int(bool(normalize)), desc.data_ptr() if want_desc else None,
               bits.data_ptr() if want_bits else None, plan.data_ptr() if plan is not None else None,
               torch.empty((n * k,), dtype=torch.uint8, device=img.device).data_ptr() if plan is not None else None,
               N.stream_ptr())
        return desc, bits
    N.call("mi_sparse_bad_u8" if u8 else "mi_sparse_bad", N.dev(img, U8 if u8 else F32, "image"), n, h, w,
           N.dev(kp, F32, "keypoints"), k,
           N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"), p, int(mode),
           float(temperature), int(bool(normalize)), desc.data_ptr() if want_desc else None,
           bits.data_ptr() if want_bits else None, plan.data_ptr() if plan is not None else None,
           torch.empty((n * k,), dtype=torch.uint8, device=img.device).data_ptr() if plan is not None else None,
           N.stream_ptr())
    return desc, bits


def bad_dense(image: torch.Tensor, pair_geom: torch.Tensor, pair_thr: torch.Tensor, mode: int,
              temperature: float) -> torch.Tensor:
    img = _images(image, "x")
    n, _, h, w = img.shape
    p = pair_geom.numel()
    out = torch.empty((n, p, h, w), dtype=F32, device=img.device)
    N.call("mi_bad_dense", N.dev(img, F32, "x"), n, h, w, N.dev(pair_geom, torch.int32, "pair_geom"),
           N.dev(pair_thr, F32, "pair_thr"), p, int(mode), float(temperature), out.data_ptr(), N.stream_ptr())
    return out


def bad_dense_oriented(image: torch.Tensor, orientation: torch.Tensor, pair_geom: torch.Tensor, pair_thr: torch.Tensor,
                       mode: int, temperature: float) -> torch.Tensor:
    img = _images(image, "x")
    n, _, h, w = img.shape
    ori = orientation.float().contiguous()
    if tuple(ori.shape) != (n, 1, h, w):
        raise RuntimeError(f"orientation must have shape ({n}, 1, {h}, {w}), got {tuple(ori.shape)}")
    p = pair_geom.numel()
    out = torch.empty((n, p, h, w), dtype=F32, device=img.device)
    N.call("mi_bad_dense_oriented", N.dev(img, F32, "x"), N.dev(ori, F32, "orientation"), n, h, w,
           N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"), p, int(mode),
           float(temperature), out.data_ptr(), N.stream_ptr())
    return out


def gather_descriptors(descriptor_map: torch.Tensor, keypoints: torch.Tensor, bilinear: bool) -> torch.Tensor:
    if descriptor_map.dim() != 4 or keypoints.dim() != 3 or keypoints.shape[0] != descriptor_map.shape[0]:
        raise RuntimeError(f"expected (B,D,H,W) and (B,N,2), got {tuple(descriptor_map.shape)} {tuple(keypoints.shape)}")
    dm = descriptor_map.float().contiguous()
    kp = keypoints.float().contiguous()
    b, d, h, w = dm.shape
    out = torch.empty((b, kp.shape[1], d), dtype=F32, device=dm.device)
    N.call("mi_gather_descriptors", N.dev(dm, F32, "descriptor_map"), b, d, h, w, N.dev(kp, F32, "keypoints"),
           kp.shape[1], int(bool(bilinear)), out.data_ptr(), N.stream_ptr())
    return out


def angle_map(image: torch.Tensor, moment_kernels: torch.Tensor, patch_size: int) -> torch.Tensor:
    img = _images(image, "image")
    n, _, h, w = img.shape
    out = torch.empty_like(img)
    N.call("mi_angle_map", N.dev(img, F32, "image"), n, h, w, int(patch_size),
           N.dev(moment_kernels.contiguous(), F32, "moment_kernels"), out.data_ptr(), N.stream_ptr())
    return out


def angle_at_keypoints(image: torch.Tensor, keypoints: torch.Tensor, moment_kernels: torch.Tensor,
                       patch_size: int) -> torch.Tensor:
    img = _images(image, "image")
    n, _, h, w = img.shape
    kp = keypoints.float().contiguous()
    theta = torch.empty((n, kp.shape[1]), dtype=F32, device=img.device)
    if isinstance(img, ImagePair):
        N.call("mi_angle_at_keypoints_pair", N.dev(img.a, F32, "image"), N.dev(img.b, F32, "image"), n // 2, h, w,
               N.dev(kp, F32, "keypoints"), kp.shape[1], int(patch_size),
               N.dev(moment_kernels.contiguous(), F32, "moment_kernels"), theta.data_ptr(), N.stream_ptr())
        return theta
    N.call("mi_angle_at_keypoints", N.dev(img, F32, "image"), n, h, w, N.dev(kp, F32, "keypoints"), kp.shape[1],
           int(patch_size), N.dev(moment_kernels.contiguous(), F32, "moment_kernels"), theta.data_ptr(),
           N.stream_ptr())
    return theta


def sparse_bad_oriented(image: torch.Tensor, keypoints: torch.Tensor, orientation: torch.Tensor,
                        pair_geom: torch.Tensor, pair_thr: torch.Tensor, mode: int, temperature: float,
                        normalize: bool, want_desc: bool = True, want_bits: bool = False, bilinear: bool = False,
                        max_reach: float = 0.0):
    """orientation: dense map (B,1,H,W) -- the reference's argument -- or per-keypoint angles (B,K).
    bilinear: sampling_mode="bilinear" of the box-mean maps instead of "nearest".
    max_reach: upper bound of |pair offset| + box radius over the table in pixels (0 = unknown: the 60-pixel window)."""
    img = _images(image, "image")
    n, _, h, w = img.shape
    if keypoints.dim() != 3 or keypoints.shape[0] != n or keypoints.shape[2] != 2:
        raise RuntimeError(f"keypoints must have shape ({n}, K, 2), got {tuple(keypoints.shape)}")
    kp = keypoints.float().contiguous()
    k = kp.shape[1]
    ang = orientation.float().contiguous()
    if ang.dim() == 4 and tuple(ang.shape) == (n, 1, h, w):
        amap, akp = N.dev(ang, F32, "orientation"), None
    elif ang.dim() == 2 and tuple(ang.shape) == (n, k):
        amap, akp = None, N.dev(ang, F32, "orientation")
    else:
        raise RuntimeError(f"orientation must be ({n}, 1, {h}, {w}) or ({n}, {k}), got {tuple(ang.shape)}")
    p = pair_geom.numel()
    desc = torch.empty((n, k, p), dtype=F32, device=img.device) if want_desc else None
    bits = torch.empty((n, k, p // 32), dtype=torch.int32, device=img.device) if want_bits else None
    status = torch.empty((n, k), dtype=torch.uint8, device=img.device)      # int32-table fast path bookkeeping
    if isinstance(img, ImagePair):
        if akp is None:
            raise RuntimeError("an ImagePair takes per-keypoint angles (2B, K), not a dense orientation map")
        N.call("mi_sparse_bad_oriented_pair", N.dev(img.a, F32, "image"), N.dev(img.b, F32, "image"), n // 2, h, w,
               N.dev(kp, F32, "keypoints"), k, akp, N.dev(pair_geom, torch.int32, "pair_geom"),
               N.dev(pair_thr, F32, "pair_thr"), p, int(mode), float(temperature), int(bool(normalize)),
               int(bool(bilinear)), float(max_reach), desc.data_ptr() if want_desc else None,
               bits.data_ptr() if want_bits else None, status.data_ptr(), N.stream_ptr())
        return desc, bits
    N.call("mi_sparse_bad_oriented", N.dev(img, F32, "image"), n, h, w, N.dev(kp, F32, "keypoints"), k, amap, akp,
           N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"), p, int(mode),
           float(temperature), int(bool(normalize)), int(bool(bilinear)), float(max_reach),
           desc.data_ptr() if want_desc else None, bits.data_ptr() if want_bits else None, status.data_ptr(),
           N.stream_ptr())
    return desc, bits


def _pitch(m: int) -> int:
    return (m + 3) // 4 * 4


def cost_logscores_bits(bits1: torch.Tensor, bits2: torch.Tensor, normalized: bool, epsilon: float):
    b, n, words = bits1.shape
    m = bits2.shape[1]
    pitch = _pitch(m)
    z = torch.empty((b, n, pitch), dtype=F32, device=bits1.device)
    N.call("mi_cost_logscores_bits", N.dev(bits1, torch.int32, "bits1"), N.dev(bits2, torch.int32, "bits2"), b, n, m,
           words * 32, int(bool(normalized)), float(epsilon), z.data_ptr(), pitch, N.stream_ptr())
    return z, pitch


def cost_logscores_f32(desc1: torch.Tensor, desc2: torch.Tensor, distance: int, epsilon: float):
    if desc1.dim() != 3 or desc2.dim() != 3 or desc1.shape[0] != desc2.shape[0] or desc1.shape[2] != desc2.shape[2]:
        raise RuntimeError(f"descriptor shapes do not match: {tuple(desc1.shape)} vs {tuple(desc2.shape)}")
    d1 = desc1.float().contiguous()
    d2 = desc2.float().contiguous()
    b, n, d = d1.shape
    m = d2.shape[1]
    pitch = _pitch(m)
    z = torch.empty((b, n, pitch), dtype=F32, device=d1.device)
    N.call("mi_cost_logscores_f32", N.dev(d1, F32, "desc1"), N.dev(d2, F32, "desc2"), b, n, m, d, int(distance),
           float(epsilon), z.data_ptr(), pitch, N.stream_ptr())
    return z, pitch


def sinkhorn(z: torch.Tensor, m: int, pitch: int, dustbin_logscore: float, iterations: int,
             return_duals: bool = False, use_workspace: bool = True, want_p: bool = True):
    """want_p=False: duals only (P is not written); returns (None, u, v)."""
    b, n, _ = z.shape
    u = torch.empty((b, n + 1), dtype=F32, device=z.device)
    v = torch.empty((b, m + 1), dtype=F32, device=z.device)
    p = torch.empty((b, n + 1, m + 1), dtype=F32, device=z.device) if want_p else None
    # no workspace (by choice, or M > 1024 where the query answers 0): the two-pass form
    work, wbytes = _workspace("mi_sinkhorn_workspace_bytes", b, n, m, device=z.device) if use_workspace else (None, 0)
    N.call("mi_sinkhorn", N.dev(z, F32, "z"), b, n, m, pitch, float(dustbin_logscore), int(iterations),
           u.data_ptr(), v.data_ptr(), p.data_ptr() if p is not None else None,
           work.data_ptr() if wbytes else None, wbytes, N.stream_ptr())
    return (p, u, v) if (return_duals or not want_p) else p


DOTS_MIN_EPSILON = N.MI_DOTS_MIN_EPSILON      # below it the clamped fp32-Z form runs


def dots_supported(b: int, n: int, m: int, epsilon: float = 1.0) -> bool:
    return epsilon >= DOTS_MIN_EPSILON and int(N.load().mi_sinkhorn_dots_workspace_bytes(b, n, m)) > 0


class DotsState(tuple):
    """The state tuple of sinkhorn_bits(return_state=True) -- (dots, row_info, col_info, pitch, (workspace, status word
    address)) -- which also remembers the descriptors' bit count: below 1024 bits every dot product is below 1024, and
    mnn_from_duals_dots may vouch for that (MI_SOLVER_DOTS_BELOW_1024).  A slice or a hand-built tuple carries no count
    and nothing is vouched for."""
    num_bits = None


def sinkhorn_bits(bits1: torch.Tensor, bits2: torch.Tensor, normalized: bool, epsilon: float, unused_score: float,
                  iterations: int, return_duals: bool = False, want_p: bool = True, return_state: bool = False):
    """Cost + Sinkhorn for packed hard-bit descriptors (B,N,D/32),(B,M,D/32) int32 -> P (B,N+1,M+1),
    uint16 dot-product form (M <= 1024; half the bytes per iteration).  return_state: also the
    (dots, row_info, col_info, pitch, (workspace, status word address)) the duals refer to (for mnn_from_duals_dots;
    the workspace is kept alive because the call's status word lives in it)."""
    b, n, words = bits1.shape
    m = bits2.shape[1]
    dev = bits1.device
    work, wbytes = (_workspace("mi_sinkhorn_dots_workspace_bytes", b, n, m, device=dev) if epsilon >= DOTS_MIN_EPSILON
                    else (None, 0))
    if wbytes == 0:
        if return_state or not want_p:
            raise RuntimeError(f"the dot-product Sinkhorn form supports M <= 1024 and epsilon >= {DOTS_MIN_EPSILON}, "
                               f"got M = {m}, epsilon = {epsilon}")
        z, pitch = cost_logscores_bits(bits1, bits2, normalized, epsilon)
        return sinkhorn(z, m, pitch, -unused_score / epsilon, iterations, return_duals=return_duals)
    pitch = (m + 7) // 8 * 8
    dots = torch.empty((b, n, pitch), dtype=torch.int16, device=dev)
    row_info = torch.empty((b, n, 2), dtype=F32, device=dev)
    col_info = torch.empty((b, m, 2), dtype=F32, device=dev)
    N.call("mi_cost_dots_bits", N.dev(bits1, torch.int32, "bits1"), N.dev(bits2, torch.int32, "bits2"), b, n, m,
           words * 32, int(bool(normalized)), dots.data_ptr(), pitch, row_info.data_ptr(), col_info.data_ptr(),
           N.stream_ptr())
    u = torch.empty((b, n + 1), dtype=F32, device=dev)
    v = torch.empty((b, m + 1), dtype=F32, device=dev)
    p = torch.empty((b, n + 1, m + 1), dtype=F32, device=dev) if want_p else None
    N.call("mi_sinkhorn_dots", dots.data_ptr(), row_info.data_ptr(), col_info.data_ptr(), b, n, m, pitch,
           float(epsilon), float(unused_score), 1.0 if normalized else float(words * 32), int(iterations),
           u.data_ptr(), v.data_ptr(), p.data_ptr() if p is not None else None, work.data_ptr(), wbytes,
           _solver_flags | (MI_SOLVER_DOTS_BELOW_1024 if words * 32 < 1024 else 0), N.stream_ptr())
    if return_state:
        status = N.load().mi_sinkhorn_dots_status_word(work.data_ptr(), b, n, m)
        state = DotsState((dots, row_info, col_info, pitch, (work, status)))
        state.num_bits = words * 32
        return p, u, v, state
    return (p, u, v) if (return_duals or not want_p) else p


def match_filters(p: torch.Tensor, ratio_threshold: float, dustbin_margin: float):
    """In-place outlier filters on P (B,N+1,M+1) -> (P, valid (B,N) bool)."""
    b, n1, m1 = p.shape
    valid = torch.empty((b, n1 - 1), dtype=torch.bool, device=p.device)       # the kernel writes 0/1 bytes
    N.call("mi_match_filters", N.dev(p, F32, "P"), b, n1 - 1, m1 - 1, float(ratio_threshold), float(dustbin_margin),
           valid.data_ptr(), N.stream_ptr())
    return p, valid


def match_filter_masks(p: torch.Tensor, has_dustbin: bool, ratio_threshold: float, dustbin_margin: float) -> torch.Tensor:
    """Masks of the two outlier tests, P untouched: P (B,N+1,M+1) with has_dustbin, else the core (B,N,M) -> (B,N) bool."""
    pp = p.float().contiguous()
    b, n, m = pp.shape[0], pp.shape[1] - int(has_dustbin), pp.shape[2] - int(has_dustbin)
    valid = torch.empty((b, n), dtype=torch.bool, device=pp.device)
    N.call("mi_match_filter_masks", N.dev(pp, F32, "P"), b, n, m, int(has_dustbin), float(ratio_threshold),
           float(dustbin_margin), valid.data_ptr(), N.stream_ptr())
    return valid


def mnn_extract(p: torch.Tensor, kpts1: torch.Tensor, kpts2: torch.Tensor, max_matches: int, threshold: float,
                return_indices: bool = False):
    if p.dim() != 3:
        raise RuntimeError(f"P must have shape (B, N+1, M+1), got {tuple(p.shape)}")
    pp = p.float().contiguous()
    k1 = kpts1.float().contiguous()
    k2 = kpts2.float().contiguous()
    b, n, m = pp.shape[0], k1.shape[1], k2.shape[1]
    if pp.shape[1] != n + 1 or pp.shape[2] != m + 1:
        raise RuntimeError(f"P shape {tuple(pp.shape)} does not match keypoints ({n}, {m})")
    dev = pp.device
    row_best = torch.empty((b, n), dtype=torch.int64, device=dev)
    col_best = torch.empty((b, m), dtype=torch.int64, device=dev)
    mk1 = torch.empty((b, max_matches, 2), dtype=F32, device=dev)
    mk2 = torch.empty((b, max_matches, 2), dtype=F32, device=dev)
    sc = torch.empty((b, max_matches), dtype=F32, device=dev)
    valid = torch.empty((b, max_matches), dtype=torch.bool, device=dev)          # the kernel writes 0/1 bytes
    ij = torch.empty((b, max_matches, 2), dtype=torch.int32, device=dev)
    N.call("mi_mnn_extract", N.dev(pp, F32, "P"), b, n, m, N.dev(k1, F32, "keypoints1"), N.dev(k2, F32, "keypoints2"),
           int(max_matches), float(threshold), row_best.data_ptr(), col_best.data_ptr(), mk1.data_ptr(),
           mk2.data_ptr(), sc.data_ptr(), valid.data_ptr(), ij.data_ptr(), N.stream_ptr())
    out = (mk1, mk2, sc, valid)
    return out + (ij,) if return_indices else out


def mnn_duals_supported(b: int, n: int, m: int) -> bool:
    return int(N.load().mi_mnn_duals_workspace_bytes(b, n, m)) > 0


def _mnn_record_outputs(b, max_matches, dev):
    """(record (B, Mx, 6) float32, valid (B, Mx) bool, match_ij (B, Mx, 2) int32) for the _records entries."""
    return (torch.empty((b, max_matches, RECORD_FIELDS), dtype=F32, device=dev),
            torch.empty((b, max_matches), dtype=torch.bool, device=dev),          # the kernel writes 0/1 bytes
            torch.empty((b, max_matches, 2), dtype=torch.int32, device=dev))


def _mnn_record_views(rec, valid, ij, return_indices):
    """mk1, mk2, scores as views of the record the select kernel wrote, and valid tagged as that record's own
    (distributed.pack_records then hands the record back instead of packing it again)."""
    tag_record(rec, valid)
    out = (rec[..., 0:2], rec[..., 2:4], rec[..., 4], valid)
    return out + (ij,) if return_indices else out


def mnn_from_duals(z: torch.Tensor, m: int, pitch: int, u: torch.Tensor, v: torch.Tensor, kpts1: torch.Tensor,
                   kpts2: torch.Tensor, max_matches: int, threshold: float, return_indices: bool = False):
    """mnn_extract(P) with P = exp(Z + u + v) evaluated on the fly (P never written)."""
    b, n, _ = z.shape
    k1, k2 = kpts1.float().contiguous(), kpts2.float().contiguous()
    work, wbytes = _workspace("mi_mnn_duals_workspace_bytes", b, n, m, device=z.device,
                              refusal=f"mnn_from_duals supports N <= 4096 and M <= 1024, got ({n}, {m})")
    rec, valid, ij = _mnn_record_outputs(b, max_matches, z.device)
    N.call("mi_mnn_from_duals_records", N.dev(z, F32, "z"), b, n, m, pitch, N.dev(u, F32, "u"), N.dev(v, F32, "v"),
           N.dev(k1, F32, "keypoints1"), N.dev(k2, F32, "keypoints2"), int(max_matches), float(threshold),
           work.data_ptr(), wbytes, rec.data_ptr(), valid.data_ptr(), ij.data_ptr(), N.stream_ptr())
    return _mnn_record_views(rec, valid, ij, return_indices)


def mnn_from_duals_dots(state, m: int, epsilon: float, u: torch.Tensor, v: torch.Tensor, kpts1: torch.Tensor,
                        kpts2: torch.Tensor, max_matches: int, threshold: float, return_indices: bool = False,
                        dots_below_1024: bool | None = None):
    """dots_below_1024: vouch that every dot product is below 1024 (the kernel then multiplies the uint16 in one mixed-
    precision instruction; the same matches bit for bit).  None: decided from the bit count a DotsState carries."""
    dots, row_info, col_info, pitch = state[:4]
    status = state[4][1] if len(state) > 4 else None          # the producing Sinkhorn call's status word (device address)
    if dots_below_1024 is None:
        num_bits = getattr(state, "num_bits", None)
        dots_below_1024 = num_bits is not None and num_bits < 1024
    b, n, _ = dots.shape
    k1, k2 = kpts1.float().contiguous(), kpts2.float().contiguous()
    work, wbytes = _workspace("mi_mnn_duals_workspace_bytes", b, n, m, device=dots.device,
                              refusal=f"mnn_from_duals_dots supports N <= 4096 and M <= 1024, got ({n}, {m})")
    rec, valid, ij = _mnn_record_outputs(b, max_matches, dots.device)
    N.call("mi_mnn_from_duals_dots_records", dots.data_ptr(), row_info.data_ptr(), col_info.data_ptr(), b, n, m, pitch,
           float(epsilon), N.dev(u, F32, "u"), N.dev(v, F32, "v"), N.dev(k1, F32, "keypoints1"),
           N.dev(k2, F32, "keypoints2"), int(max_matches), float(threshold), work.data_ptr(), wbytes, status,
           MI_SOLVER_DOTS_BELOW_1024 if dots_below_1024 else 0, rec.data_ptr(), valid.data_ptr(), ij.data_ptr(),
           N.stream_ptr())
    return _mnn_record_views(rec, valid, ij, return_indices)


# ---- AKAZE (detector/akaze.py) ------------------------------------------------------------------

def akaze_diffuse(image: torch.Tensor, iterations: int, kappa: float, dt: float = 0.25) -> torch.Tensor:
    """NonLinearDiffusion.forward: `iterations` explicit steps, ping-ponging two buffers."""
    img = _images(image, "image")
    n, _, h, w = img.shape
    if iterations <= 0:
        return img
    bufs = [torch.empty_like(img), torch.empty_like(img) if iterations > 1 else None]
    cur = img
    for i in range(int(iterations)):
        dst = bufs[i & 1]
        N.call("mi_akaze_diffuse", N.dev(cur, F32, "image"), n, h, w, float(kappa), float(dt), dst.data_ptr(),
               N.stream_ptr())
        cur = dst
    return cur


def akaze_scale(image: torch.Tensor, iterations: int, kappa: float, dt: float, threshold: float, nms_size: int,
                scores_out: torch.Tensor | None = None, image_out: torch.Tensor | None = None):
    """One AKAZE scale in one launch: (diffused image, Hessian score map) = (NonLinearDiffusion(image),
    HessianDetector(diffused)); `mi_akaze_scale`."""
    img = _images(image, "image")
    n, _, h, w = img.shape
    out = image_out if image_out is not None else torch.empty_like(img)
    scores = scores_out if scores_out is not None else torch.empty_like(img)
    fused = bool(N.load().mi_akaze_scale_fused(int(iterations), int(nms_size)))
    tmp = None if fused or iterations <= 1 else torch.empty_like(img)
    N.call("mi_akaze_scale", N.dev(img, F32, "image"), n, h, w, int(iterations), float(kappa), float(dt), float(threshold),
           int(nms_size), N.dev(out, F32, "image_out"), N.dev(scores, F32, "scores"), tmp.data_ptr() if tmp is not None else None,
           N.stream_ptr())
    return out, scores


def akaze_scale_sets(image1: torch.Tensor, image2: torch.Tensor, iterations: int, kappa: float, dt: float, threshold: float,
                     nms_size: int, scores_out: torch.Tensor, image_out: torch.Tensor):
    """The first AKAZE scale of two equally shaped batches in one launch (`mi_akaze_scale_sets`): image_out / scores_out
    (2N,1,H,W) receive batch 1 then batch 2."""
    a, b = _images(image1, "image1"), _images(image2, "image2")
    if a.shape != b.shape:
        raise RuntimeError(f"image shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    n, _, h, w = a.shape
    if tuple(image_out.shape) != (2 * n, 1, h, w) or tuple(scores_out.shape) != (2 * n, 1, h, w):
        raise RuntimeError("image_out / scores_out must be (2N,1,H,W)")
    fused = bool(N.load().mi_akaze_scale_fused(int(iterations), int(nms_size)))
    tmp = None if fused or iterations <= 1 else torch.empty_like(a)
    N.call("mi_akaze_scale_sets", N.dev(a, F32, "image1"), N.dev(b, F32, "image2"), n, h, w, int(iterations), float(kappa),
           float(dt), float(threshold), int(nms_size), N.dev(image_out, F32, "image_out"), N.dev(scores_out, F32, "scores"),
           tmp.data_ptr() if tmp is not None else None, N.stream_ptr())
    return image_out, scores_out


AKAZE_KAPPA_MIN, AKAZE_KAPPA_MAX = N.MI_AKAZE_KAPPA_MIN, N.MI_AKAZE_KAPPA_MAX


def akaze_kappa_fused(kappa: float) -> bool:
    """kappa inside the range the fused scale kernels accept (their exactly rounded division helpers are verified for
    it); outside, the modules run the per-step kernels (IEEE operators)."""
    return AKAZE_KAPPA_MIN <= float(kappa) <= AKAZE_KAPPA_MAX


def akaze_attain(scale_scores: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """(S,N,1,H,W) per-scale maps + their maximum -> attain (N,1,H,W) uint8, bit s = scale s reaches it (the general-
    parameter route of AKAZE.detect_select; elementwise torch ops on the device)."""
    bits = torch.zeros(scores.shape, dtype=torch.int32, device=scores.device)
    for s in range(scale_scores.shape[0]):
        bits |= (scale_scores[s] == scores).to(torch.int32) << s
    return bits.to(U8)


def akaze_scale_select(image: torch.Tensor, iterations: int, kappa: float, dt: float, threshold: float, nms_size: int,
                       prev_scores: torch.Tensor | None, image_out: torch.Tensor | None = None):
    """The last AKAZE scale with the selection across scales folded in (`mi_akaze_scale_select`): (diffused image,
    best = max over prev_scores (S-1,N,1,H,W) and this scale's score map, attain (N,1,H,W) uint8: bit s = scale s
    reaches best)."""
    img = _images(image, "image")
    n, _, h, w = img.shape
    num_prev = 0 if prev_scores is None else int(prev_scores.shape[0])
    if num_prev > 7:
        raise RuntimeError(f"at most 8 scales, got {num_prev + 1}")
    if num_prev and tuple(prev_scores.shape[1:]) != (n, 1, h, w):
        raise RuntimeError(f"prev_scores must be (S-1,{n},1,{h},{w}), got {tuple(prev_scores.shape)}")
    out = image_out if image_out is not None else torch.empty_like(img)
    best = torch.empty_like(img)
    attain = torch.empty((n, 1, h, w), dtype=U8, device=img.device)
    fused = bool(N.load().mi_akaze_scale_fused(int(iterations), int(nms_size)))
    tmp = None if fused or iterations <= 1 else torch.empty_like(img)
    N.call("mi_akaze_scale_select", N.dev(img, F32, "image"), n, h, w, int(iterations), float(kappa), float(dt),
           float(threshold), int(nms_size), N.dev(out, F32, "image_out"),
           N.dev(prev_scores, F32, "prev_scores") if num_prev else None, num_prev, best.data_ptr(), attain.data_ptr(),
           tmp.data_ptr() if tmp is not None else None, N.stream_ptr())
    return out, best, attain


def akaze_orientation_from_attain(attain: torch.Tensor, scale_theta: torch.Tensor, keypoints: torch.Tensor) -> torch.Tensor:
    n, _, h, w = attain.shape
    s = int(scale_theta.shape[0])
    kp = keypoints.float().contiguous()
    k = kp.shape[1]
    theta = torch.empty((n, k), dtype=F32, device=attain.device)
    N.call("mi_akaze_orientation_from_attain", N.dev(attain, U8, "attain"), N.dev(scale_theta, F32, "scale_theta"), s, n,
           h, w, N.dev(kp, F32, "keypoints"), k, theta.data_ptr(), N.stream_ptr())
    return theta


def akaze_orientation_select(scale_images: torch.Tensor, attain: torch.Tensor, keypoints: torch.Tensor,
                             moment_kernels: torch.Tensor, patch_size: int) -> torch.Tensor:
    """AKAZE.forward's orientation at keypoints in one launch (`mi_akaze_orientation_select`): scale_images (S,N,1,H,W)
    stacked diffused images, attain (N,1,H,W) uint8 from akaze_scale_select."""
    s, n, _, h, w = scale_images.shape
    kp = keypoints.float().contiguous()
    k = kp.shape[1]
    theta = torch.empty((n, k), dtype=F32, device=attain.device)
    N.call("mi_akaze_orientation_select", N.dev(scale_images, F32, "scale_images"), n * h * w, s,
           N.dev(attain, U8, "attain"), n, h, w, N.dev(kp, F32, "keypoints"), k, int(patch_size),
           N.dev(moment_kernels.float().contiguous(), F32, "moment_kernels"), theta.data_ptr(), N.stream_ptr())
    return theta


def akaze_hessian_scores(image: torch.Tensor, threshold: float, nms_size: int,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    img = _images(image, "image")
    n, _, h, w = img.shape
    if out is None:
        out = torch.empty_like(img)
    N.call("mi_akaze_hessian_scores", N.dev(img, F32, "image"), n, h, w, float(threshold), int(nms_size),
           N.dev(out, F32, "scores"), N.stream_ptr())
    return out


def akaze_combine(scale_scores: torch.Tensor, scale_orientations: torch.Tensor | None):
    """(S,N,1,H,W) stacks -> (scores, orientations) of AKAZE.forward; orientations None -> scores only."""
    s, n, _, h, w = scale_scores.shape
    scores = torch.empty((n, 1, h, w), dtype=F32, device=scale_scores.device)
    oris = torch.empty_like(scores) if scale_orientations is not None else None
    N.call("mi_akaze_combine", N.dev(scale_scores, F32, "scale_scores"),
           N.opt(scale_orientations, F32, "scale_orientations"),
           s, n, h, w, scores.data_ptr(), oris.data_ptr() if oris is not None else None, N.stream_ptr())
    return scores, oris


def akaze_orientation_at_keypoints(scale_scores: torch.Tensor, scale_theta: torch.Tensor,
                                   keypoints: torch.Tensor) -> torch.Tensor:
    s, n, _, h, w = scale_scores.shape
    kp = keypoints.float().contiguous()
    k = kp.shape[1]
    theta = torch.empty((n, k), dtype=F32, device=scale_scores.device)
    N.call("mi_akaze_orientation_at_keypoints", N.dev(scale_scores, F32, "scale_scores"),
           N.dev(scale_theta, F32, "scale_theta"), s, n, h, w, N.dev(kp, F32, "keypoints"), k, theta.data_ptr(),
           N.stream_ptr())
    return theta


# ---- essential-matrix head (geometry/essential_matrix_estimator.py) ---------------------------------

def _validity_bytes(valid: torch.Tensor | None) -> torch.Tensor | None:
    """A validity mask as the uint8 array the C ABI reads; a bool tensor is VIEWED (one byte per element, 0 / 1): no copy
    kernel on the per-pair path."""
    if valid is None:
        return None
    if valid.dtype == torch.bool:
        return valid.contiguous().view(torch.uint8)
    return (valid != 0).contiguous().view(torch.uint8)


def essential_matrix(p: torch.Tensor, pts1_n: torch.Tensor, pts2_n: torch.Tensor, valid1: torch.Tensor | None,
                     valid2: torch.Tensor | None, top_k: int, n_iter: int, n_iter_manifold: int,
                     banded: bool = True) -> torch.Tensor:
    """P (B,N+1,M+1), normalised points (B,N,2)/(B,M,2) as (x,y), optional validity (B,N)/(B,M) -> E (B,3,3).
    banded: the two-launch form on a workspace (top_k <= 4); False: the single-launch dense form."""
    if p.dim() != 3:
        raise RuntimeError(f"P must have shape (B, N+1, M+1), got {tuple(p.shape)}")
    pp = p.float().contiguous()
    b, n, m = pp.shape[0], pp.shape[1] - 1, pp.shape[2] - 1
    q1, q2 = pts1_n.float().contiguous(), pts2_n.float().contiguous()
    if tuple(q1.shape) != (b, n, 2) or tuple(q2.shape) != (b, m, 2):
        raise RuntimeError(f"points must be ({b},{n},2) and ({b},{m},2), got {tuple(q1.shape)}, {tuple(q2.shape)}")
    if (valid1 is None) != (valid2 is None):
        raise RuntimeError("valid1 and valid2 must be given together")
    v1, v2 = _validity_bytes(valid1), _validity_bytes(valid2)
    e = torch.empty((b, 3, 3), dtype=F32, device=pp.device)
    # no workspace (by choice, or top_k > 4 where the query answers 0): the single-launch dense form
    work, wbytes = (_workspace("mi_essential_matrix_workspace_bytes", b, n, m, int(top_k), device=pp.device) if banded
                    else (None, 0))
    N.call("mi_essential_matrix", N.dev(pp, F32, "P"), b, n, m, N.dev(q1, F32, "pts1"), N.dev(q2, F32, "pts2"),
           N.opt(v1, U8, "valid1"), N.opt(v2, U8, "valid2"), int(top_k), int(n_iter), int(n_iter_manifold),
           e.data_ptr(), work.data_ptr() if wbytes else None, wbytes, N.stream_ptr())
    return e


def essential_matrix_dots(state, m: int, epsilon: float, u: torch.Tensor, v: torch.Tensor, pts1_n: torch.Tensor,
                          pts2_n: torch.Tensor, valid1: torch.Tensor | None, valid2: torch.Tensor | None, top_k: int,
                          n_iter: int, n_iter_manifold: int, banded: bool = True) -> torch.Tensor:
    """essential_matrix() without a materialised P (`mi_essential_matrix_dots`): `state` = the (dots, row_info, col_info,
    pitch, ...) tuple of sinkhorn_bits(return_state=True), u / v its duals.  Same E bit for bit as essential_matrix on
    the P that solve would have written."""
    dots, row_info, col_info, pitch = state[:4]
    b, n = dots.shape[0], dots.shape[1]
    q1, q2 = pts1_n.float().contiguous(), pts2_n.float().contiguous()
    if tuple(q1.shape) != (b, n, 2) or tuple(q2.shape) != (b, m, 2):
        raise RuntimeError(f"points must be ({b},{n},2) and ({b},{m},2), got {tuple(q1.shape)}, {tuple(q2.shape)}")
    if (valid1 is None) != (valid2 is None):
        raise RuntimeError("valid1 and valid2 must be given together")
    v1, v2 = _validity_bytes(valid1), _validity_bytes(valid2)
    e = torch.empty((b, 3, 3), dtype=F32, device=dots.device)
    work, wbytes = (_workspace("mi_essential_matrix_workspace_bytes", b, n, m, int(top_k), device=dots.device) if banded
                    else (None, 0))
    N.call("mi_essential_matrix_dots", dots.data_ptr(), row_info.data_ptr(), col_info.data_ptr(), int(pitch), float(epsilon),
           N.dev(u, F32, "u"), N.dev(v, F32, "v"), b, n, m, N.dev(q1, F32, "pts1"), N.dev(q2, F32, "pts2"),
           N.opt(v1, U8, "valid1"), N.opt(v2, U8, "valid2"), int(top_k), int(n_iter), int(n_iter_manifold),
           e.data_ptr(), work.data_ptr() if wbytes else None, wbytes, N.stream_ptr())
    return e


# ---- FAST / DoG detectors (detector/fast.py, detector/dog.py) -----------------------------------------

def fast_score(image: torch.Tensor, threshold: float) -> torch.Tensor:
    img = _images(image, "image")
    n, _, h, w = img.shape
    out = torch.empty_like(img)
    N.call("mi_fast_score", N.dev(img, F32, "image"), n, h, w, float(threshold), out.data_ptr(), N.stream_ptr())
    return out


def dog_responses(image: torch.Tensor, weights_1d: torch.Tensor, want_maps: bool = True, want_score: bool = False):
    """weights_1d (S, ks): 1-D factors of the normalised Gaussians -> DoG maps (N, S-1, H, W) and/or the
    score map max_s |DoG_s| (N, 1, H, W)."""
    img = _images(image, "image")
    n, _, h, w = img.shape
    s, ks = weights_1d.shape
    out = torch.empty((n, s - 1, h, w), dtype=F32, device=img.device) if want_maps else None
    score = torch.empty((n, 1, h, w), dtype=F32, device=img.device) if want_score else None
    N.call("mi_dog_responses", N.dev(img, F32, "image"), n, h, w, N.dev(weights_1d.contiguous(), F32, "weights_1d"), s,
           ks, out.data_ptr() if out is not None else None, score.data_ptr() if score is not None else None,
           N.stream_ptr())
    return out, score


def normalise_keypoints(keypoints: torch.Tensor, k_inv: torch.Tensor) -> torch.Tensor:
    """(..., 2) pixel keypoints (y, x) -> (..., 2) normalised (x, y) = K^-1 [x, y, 1] (first two rows)."""
    kp = keypoints.float().contiguous()
    ki = k_inv.float().contiguous()
    out = torch.empty_like(kp)
    N.call("mi_normalise_keypoints", N.dev(kp, F32, "keypoints"), kp.numel() // 2, N.dev(ki, F32, "K_inv"),
           out.data_ptr(), N.stream_ptr())
    return out


def core_maxima(p: torch.Tensor):
    """P (B,N+1,M+1) -> (row maxima (B,N), column maxima (B,M)) of the core P[:, :N, :M]."""
    pp = p.float().contiguous()
    b, n, m = pp.shape[0], pp.shape[1] - 1, pp.shape[2] - 1
    r = torch.empty((b, n), dtype=F32, device=pp.device)
    c = torch.empty((b, m), dtype=F32, device=pp.device)
    N.call("mi_core_maxima", N.dev(pp, F32, "P"), b, n, m, r.data_ptr(), c.data_ptr(), N.stream_ptr())
    return r, c


def match_pairs(image1: torch.Tensor, image2: torch.Tensor, *, block_size: int, nms_radius: int, max_keypoints: int,
                score_threshold: float, border_margin: int, pair_geom: torch.Tensor, pair_thr: torch.Tensor,
                plan: torch.Tensor | None, normalize_descriptors: bool, epsilon: float, unused_score: float,
                sinkhorn_iterations: int, max_matches: int, match_threshold: float, want_ij: bool = False):
    """The whole path in ONE C-ABI call (`mi_match_pairs`): what MatchExtractionWrapper(ShiTomasiSparseBADSinkhornMatcher)
    computes for hard-binarised descriptors and the L2 cost, bit-identical to the module path.
    -> (keypoints1, keypoints2, matched1, matched2, scores, valid[, match_ij])."""
    u8 = image1.dtype == U8 and image2.dtype == U8           # both uint8: the u8 ingest form; otherwise float32
    a, b2 = _images(image1, "image1", keep_u8=u8), _images(image2, "image2", keep_u8=u8)
    if a.shape != b2.shape:
        raise RuntimeError(f"image shapes differ: {tuple(a.shape)} vs {tuple(b2.shape)}")
    n, _, h, w = a.shape
    dev = a.device
    prm = N.MatchParams(int(block_size), int(nms_radius), int(max_keypoints), float(score_threshold), int(border_margin),
                        int(pair_geom.numel()), N.dev(pair_geom, torch.int32, "pair_geom"), N.dev(pair_thr, F32, "pair_thr"),
                        plan.data_ptr() if plan is not None else None, int(bool(normalize_descriptors)), float(epsilon),
                        float(unused_score), int(sinkhorn_iterations), int(max_matches), float(match_threshold),
                        _solver_flags)
    import ctypes
    work, wbytes = _workspace("mi_match_pairs_workspace_bytes", n, h, w, ctypes.byref(prm), device=dev,
                              refusal="mi_match_pairs does not cover these parameters (K <= 1024, P % 64 == 0, odd block size ...)")
    k, mx = int(max_keypoints), int(max_matches)
    kp1 = torch.empty((n, k, 2), dtype=F32, device=dev)
    kp2 = torch.empty((n, k, 2), dtype=F32, device=dev)
    mk1 = torch.empty((n, mx, 2), dtype=F32, device=dev)
    mk2 = torch.empty((n, mx, 2), dtype=F32, device=dev)
    sc = torch.empty((n, mx), dtype=F32, device=dev)
    valid = torch.empty((n, mx), dtype=torch.bool, device=dev)
    ij = torch.empty((n, mx, 2), dtype=torch.int32, device=dev) if want_ij else None
    N.call("mi_match_pairs_u8" if u8 else "mi_match_pairs", N.dev(a, U8 if u8 else F32, "image1"),
           N.dev(b2, U8 if u8 else F32, "image2"), n, h, w, ctypes.byref(prm), kp1.data_ptr(),
           kp2.data_ptr(), mk1.data_ptr(), mk2.data_ptr(), sc.data_ptr(), valid.data_ptr(),
           ij.data_ptr() if ij is not None else None, work.data_ptr(), wbytes, N.stream_ptr())
    out = (kp1, kp2, mk1, mk2, sc, valid)
    return out + (ij,) if want_ij else out


# ---- K12 voxel downsampling (pointcloud/voxel_downsampling.py) ----------------------------------------------------

def _leaf_array(leaf_size, batch: int, device) -> torch.Tensor:
    """One float32 leaf per cloud on `device`.  A device tensor stays on the device (0-dim or one value: broadcast; else
    one per cloud) -- never read back; a CPU tensor, a Python number or a sequence of numbers becomes a fill / copy."""
    if isinstance(leaf_size, torch.Tensor):
        if leaf_size.is_cuda:
            lf = leaf_size.to(device=device, dtype=F32).reshape(-1)
            if lf.numel() == 1:
                return lf.expand(batch).contiguous() if batch > 1 else lf.contiguous()
            if lf.numel() != batch:
                raise RuntimeError(f"leaf_size has {lf.numel()} values for {batch} clouds")
            return lf.contiguous()
        leaf_size = leaf_size.reshape(-1).tolist()
        if len(leaf_size) == 1:
            leaf_size = leaf_size[0]
    if isinstance(leaf_size, (list, tuple)):
        if len(leaf_size) != batch:
            raise RuntimeError(f"leaf_size has {len(leaf_size)} values for {batch} clouds")
        return torch.tensor([float(x) for x in leaf_size], dtype=F32).to(device)
    return torch.full((batch,), float(leaf_size), dtype=F32, device=device)


def _voxel_launch(pts: torch.Tensor, offsets: torch.Tensor, batch: int, leaf: torch.Tensor):
    total, d = pts.shape
    if d < 3:
        raise RuntimeError(f"points must have at least 3 columns, got {d}")
    if total >= 2 ** 31:
        raise RuntimeError(f"{total} points: at most 2^31 - 1 per call")
    dev = pts.device
    out = torch.empty((total, d), dtype=F32, device=dev)
    mask = torch.empty((total,), dtype=torch.bool, device=dev)
    counts = torch.empty((batch,), dtype=torch.int64, device=dev)
    work, wbytes = _workspace("mi_voxel_downsample_workspace_bytes", batch, total, d, device=dev)
    N.call("mi_voxel_downsample", pts.data_ptr() if total else None, N.dev(offsets, torch.int64, "offsets"), batch, total,
           d, N.dev(leaf, F32, "leaf_size"), out.data_ptr() if total else None, mask.data_ptr() if total else None,
           counts.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return out, mask, counts


def voxel_downsample(points: torch.Tensor, leaf_size) -> tuple[torch.Tensor, torch.Tensor]:
    """VoxelDownsampling.forward (`mi_voxel_downsample`, one cloud): points (N, D) float32 on the GPU, D >= 3;
    leaf_size a 0-dim / one-value tensor (a device tensor is read on the device) or a number.  Returns (output_points
    (N, D): the voxel means in ascending key order then zero rows, mask (N,) bool).  N = 0 returns the reference's
    (points.clone(), empty mask).  Capturable into a hipGraph when leaf_size is a device tensor or a number."""
    pts = points.contiguous()
    N.dev(pts, F32, "points")
    if pts.dim() != 2:
        raise RuntimeError(f"points must have shape (N, D), got {tuple(pts.shape)}")
    if pts.shape[1] < 3:
        raise RuntimeError(f"points must have at least 3 columns, got {pts.shape[1]}")
    if pts.shape[0] == 0:
        return pts.clone(), torch.ones(0, dtype=torch.bool, device=pts.device)
    offsets = torch.arange(2, dtype=torch.int64, device=pts.device) * pts.shape[0]      # [0, N] without a host copy
    out, mask, _ = _voxel_launch(pts, offsets, 1, _leaf_array(leaf_size, 1, pts.device))
    return out, mask


def voxel_downsample_batch(clouds, leaf_sizes, offsets: torch.Tensor | None = None):
    """B clouds in one `mi_voxel_downsample` call.  clouds: a list of (N_i, D) float32 GPU tensors (empty ones allowed),
    or one packed (total, D) tensor together with `offsets` (B+1 int64: cloud b = rows offsets[b] .. offsets[b+1]-1;
    on the device it is used as it is).  leaf_sizes: one leaf for all clouds or one per cloud (numbers, a CPU tensor
    or a device tensor read on the device).  Returns (output_points (total, D), mask (total,) bool, counts (B,) int64,
    offsets (B+1,) int64 on the device): cloud b's rows of the two outputs are what voxel_downsample returns for it."""
    if isinstance(clouds, torch.Tensor):
        if offsets is None:
            raise RuntimeError("a packed (total, D) tensor needs offsets")
        pts = clouds.contiguous()
        N.dev(pts, F32, "points")
        offs = offsets.to(device=pts.device, dtype=torch.int64).contiguous()
        batch = offs.numel() - 1
    else:
        clouds = list(clouds)
        if not clouds:
            raise RuntimeError("voxel_downsample_batch needs at least one cloud")
        for k, c in enumerate(clouds):
            N.dev(c.contiguous(), F32, f"clouds[{k}]")
            if c.dim() != 2 or c.shape[1] != clouds[0].shape[1]:
                raise RuntimeError(f"clouds[{k}] must have shape (N, {clouds[0].shape[1]}), got {tuple(c.shape)}")
        pts = torch.cat([c.contiguous() for c in clouds], 0)
        sizes = [0] + [int(c.shape[0]) for c in clouds]
        acc = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
        offs = acc.to(pts.device)
        batch = len(clouds)
    if pts.dim() != 2:
        raise RuntimeError(f"points must have shape (total, D), got {tuple(pts.shape)}")
    if batch < 1:
        raise RuntimeError("offsets must have at least 2 entries")
    out, mask, counts = _voxel_launch(pts, offs, batch, _leaf_array(leaf_sizes, batch, pts.device))
    return out, mask, counts, offs


# ---- K13 depth front end (depth/depth2pointcloud.py, depth2pointcloud_with_normal.py, depth_align.py) -------------

U16 = torch.uint16


def _depth_frames(depth: torch.Tensor, u_tab: torch.Tensor, v_tab: torch.Tensor, what: str):
    """(contiguous depth, is_u16, batch, h, w, batched, trailing_one) for depth of shape (H, W), (H, W, 1), (B, H, W) or
    (B, H, W, 1), H and W being the lengths of the two tables."""
    if not depth.is_cuda:
        raise RuntimeError(f"{what}: depth must live on the GPU (got device {depth.device}); this package has no CPU path")
    if depth.dtype not in (F32, U16):
        raise RuntimeError(f"{what}: depth must be float32 or uint16, got {depth.dtype}")
    N.dev(u_tab, F32, "u_tab")
    N.dev(v_tab, F32, "v_tab")
    h, w = v_tab.numel(), u_tab.numel()
    shape = tuple(depth.shape)
    if shape == (h, w):
        batched, one = False, False
    elif shape == (h, w, 1):
        batched, one = False, True
    elif len(shape) == 3 and shape[1:] == (h, w):
        batched, one = True, False
    elif len(shape) == 4 and shape[1:] == (h, w, 1):
        batched, one = True, True
    else:
        raise RuntimeError(f"{what}: depth must have shape ({h}, {w}), ({h}, {w}, 1), (B, {h}, {w}) or (B, {h}, {w}, 1), "
                           f"got {shape}")
    batch = shape[0] if batched else 1
    if h < 1 or w < 1 or batch < 1:
        raise RuntimeError(f"{what}: empty depth batch {shape}")
    if batch * h * w >= 2 ** 31:
        raise RuntimeError(f"{what}: {batch * h * w} pixels: at most 2^31 - 1 per call")
    return depth.contiguous(), int(depth.dtype == U16), batch, h, w, batched, one


def depth_to_points(depth: torch.Tensor, u_tab: torch.Tensor, v_tab: torch.Tensor, z_scale: float, normals: bool = False):
    """DepthToPointCloud(.WithNormal).forward for a batch of frames in one launch (`mi_depth_to_points`).  depth: float32
    or uint16 on the GPU, (H, W), (H, W, 1), (B, H, W) or (B, H, W, 1); u_tab (W,), v_tab (H,) float32 on the GPU and
    z_scale: the columns of the reference's `uv` buffer.  Returns points (H, W, 3) / (B, H, W, 3) = depth * (u_tab[x],
    v_tab[y], z_scale), the reference's bits, and with normals=True also the unit normals of the same shape.  Current
    stream, no synchronisation, capturable."""
    d, is_u16, batch, h, w, batched, _ = _depth_frames(depth, u_tab, v_tab, "depth_to_points")
    shape = (batch, h, w, 3) if batched else (h, w, 3)
    pts = torch.empty(shape, dtype=F32, device=d.device)
    nrm = torch.empty(shape, dtype=F32, device=d.device) if normals else None
    N.call("mi_depth_to_points", d.data_ptr(), is_u16, batch, h, w, u_tab.data_ptr(), v_tab.data_ptr(), float(z_scale),
           pts.data_ptr(), nrm.data_ptr() if normals else None, N.stream_ptr())
    return (pts, nrm) if normals else pts


def depth_align(depth: torch.Tensor, u_tab: torch.Tensor, v_tab: torch.Tensor, z_scale: float, rgb_cx: float, rgb_cy: float,
                rgb_fx: float, rgb_fy: float, rotation: torch.Tensor, translation: torch.Tensor) -> torch.Tensor:
    """DepthAlignment.forward for a batch of frames (`mi_depth_align`): depth as for depth_to_points with the DEPTH
    camera's tables; rotation (3, 3) used as p @ rotation and translation (3,), float32 on the GPU.  Returns the depth
    re-rendered in the colour camera's frame, float32, in depth's shape: per target pixel the minimum over all sources
    whose 2x2 splat covers it, 0 where none does (include/mi355x_match.h lists the divergences from the reference).
    Current stream, no synchronisation, capturable."""
    d, is_u16, batch, h, w, _, _ = _depth_frames(depth, u_tab, v_tab, "depth_align")
    rot, tr = rotation.contiguous(), translation.contiguous()
    N.dev(rot, F32, "rotation")
    N.dev(tr, F32, "translation")
    if rot.numel() != 9 or tr.numel() != 3:
        raise RuntimeError(f"rotation must have 9 and translation 3 values, got {rot.numel()} and {tr.numel()}")
    out = torch.empty(tuple(depth.shape), dtype=F32, device=d.device)
    N.call("mi_depth_align", d.data_ptr(), is_u16, batch, h, w, u_tab.data_ptr(), v_tab.data_ptr(), float(z_scale),
           float(rgb_cx), float(rgb_cy), float(rgb_fx), float(rgb_fy), rot.data_ptr(), tr.data_ptr(), out.data_ptr(),
           N.stream_ptr())
    return out


# ---- K14 thresholds (threshold/otsu.py, threshold/multi_otsu.py) ------------------------------------------------------

I32 = torch.int32
I64 = torch.int64
_PIX = {U8: N.MI_PIX_U8, U16: N.MI_PIX_U16, I32: N.MI_PIX_I32, F32: N.MI_PIX_F32}
THRESHOLD_MAX_BINS = N.MI_THRESHOLD_MAX_BINS
THRESHOLD_MAX_CLASSES = N.MI_THRESHOLD_MAX_CLASSES


def _threshold_frames(frames: torch.Tensor, what: str):
    """(contiguous frames, MI_PIX_* code, batch, pixels, batched): a tensor of up to two dimensions is one frame, one
    of three or more is a batch along its first dimension."""
    if not frames.is_cuda:
        raise RuntimeError(f"{what}: frames must live on the GPU (got device {frames.device}); this package has no CPU path")
    if frames.dtype not in _PIX:
        raise RuntimeError(f"{what}: frames must be uint8, uint16, int32 or float32, got {frames.dtype}")
    batched = frames.dim() >= 3
    batch = frames.shape[0] if batched else 1
    if frames.numel() == 0:
        raise RuntimeError(f"{what}: empty frames {tuple(frames.shape)}")
    return frames.contiguous(), _PIX[frames.dtype], batch, frames.numel() // batch, batched


def _check_bins(bins: int, what: str) -> int:
    bins = int(bins)
    if bins < 1 or bins > THRESHOLD_MAX_BINS:
        raise ValueError(f"{what}: {bins} bins: between 1 and {THRESHOLD_MAX_BINS}")
    return bins


def _histograms(hist: torch.Tensor, what: str):
    """(contiguous int64 histograms, batch, bins, batched) from (bins,) or (B, bins)"""
    if hist.dim() not in (1, 2):
        raise RuntimeError(f"{what}: hist must have shape (bins,) or (B, bins), got {tuple(hist.shape)}")
    h = hist.contiguous()
    N.dev(h, I64, "hist")
    batched = h.dim() == 2
    batch = h.shape[0] if batched else 1
    if batch < 1:
        raise RuntimeError(f"{what}: empty batch of histograms")
    return h, batch, _check_bins(h.shape[-1], what), batched


def histogram(frames: torch.Tensor, min_val: int, bins: int) -> torch.Tensor:
    """Per-frame histogram (`mi_histogram`): int64 (bins,) for one frame (a tensor of up to two dimensions), (B, bins) for
    a batch (B, ...).  hist[i] counts the pixels whose integer value v (float32: truncated toward zero) has
    v - min_val == i; values outside the range and NaN are not counted.  Exact and bitwise reproducible.  Current
    stream, no synchronisation, capturable."""
    f, code, batch, pixels, batched = _threshold_frames(frames, "histogram")
    bins = _check_bins(bins, "histogram")
    hist = torch.empty((batch, bins) if batched else (bins,), dtype=I64, device=f.device)
    N.call("mi_histogram", f.data_ptr(), code, batch, pixels, int(min_val), bins, hist.data_ptr(), N.stream_ptr())
    return hist


def otsu_threshold(hist: torch.Tensor, min_val: int) -> torch.Tensor:
    """Otsu's threshold of int64 histograms (bins,) / (B, bins) whose bin i holds the value min_val + i
    (`mi_otsu_threshold`): int32 () / (B,), on the device; the reference's float32 score and first-maximum rule."""
    h, batch, bins, batched = _histograms(hist, "otsu_threshold")
    thresh = torch.empty((batch,), dtype=I32, device=h.device)
    N.call("mi_otsu_threshold", h.data_ptr(), batch, bins, int(min_val), thresh.data_ptr(), N.stream_ptr())
    return thresh if batched else thresh.reshape(())


def multi_otsu_combinations(bins: int, n_class: int) -> int:
    """C(bins - 1, n_class - 1), the number of candidates; ValueError outside what `mi_multi_otsu_threshold` takes."""
    import math
    bins, n_class = int(bins), int(n_class)
    if n_class < 2 or n_class > THRESHOLD_MAX_CLASSES:
        raise ValueError(f"n_class must be between 2 and {THRESHOLD_MAX_CLASSES}, got {n_class}")
    if bins < n_class or bins > THRESHOLD_MAX_BINS:
        raise ValueError(f"{bins} bins for {n_class} classes: between n_class and {THRESHOLD_MAX_BINS}")
    combos = math.comb(bins - 1, n_class - 1)
    if combos > 2 ** 31 - 1:
        raise ValueError(f"{combos} threshold combinations ({bins} bins, {n_class} classes): at most 2^31 - 1")
    return combos


def multi_otsu_threshold(hist: torch.Tensor, min_val: int, n_class: int = 3) -> torch.Tensor:
    """The n_class - 1 multi-Otsu thresholds of int64 histograms (bins,) / (B, bins) (`mi_multi_otsu_threshold`): int32
    (n_class - 1,) / (B, n_class - 1), on the device, each the inclusive upper bound of its class.  The fp64 argmax over
    all C(bins - 1, n_class - 1) candidates, the first in itertools.combinations order among equals."""
    h, batch, bins, batched = _histograms(hist, "multi_otsu_threshold")
    multi_otsu_combinations(bins, n_class)
    work, wbytes = _workspace("mi_multi_otsu_workspace_bytes", batch, bins, int(n_class), device=h.device)
    out = torch.empty((batch, n_class - 1) if batched else (n_class - 1,), dtype=I32, device=h.device)
    N.call("mi_multi_otsu_threshold", h.data_ptr(), batch, bins, int(min_val), int(n_class), out.data_ptr(), work.data_ptr(),
           wbytes, N.stream_ptr())
    return out


def threshold_apply(frames: torch.Tensor, thresholds: torch.Tensor, binary=None) -> torch.Tensor:
    """One pass over frames (as for histogram) with int32 thresholds on the device: () / (T,) for one frame, (B,) /
    (B, T) for a batch, T <= 4 (`mi_threshold_apply`).  binary=None: uint8 labels, the number of thresholds t with v > t.
    binary=(low, high, dtype) with one threshold per frame: low where v <= t and high elsewhere, in dtype (uint8, int32 or
    float32): OtsuThreshold's bin_img.  The result has the frames' shape."""
    f, code, batch, pixels, batched = _threshold_frames(frames, "threshold_apply")
    t = thresholds.contiguous()
    N.dev(t, I32, "thresholds")
    if t.numel() % batch != 0 or not 1 <= t.numel() // batch <= THRESHOLD_MAX_CLASSES - 1:
        raise RuntimeError(f"thresholds of shape {tuple(t.shape)} for {batch} frame(s): 1 to {THRESHOLD_MAX_CLASSES - 1} each")
    n_thresh = t.numel() // batch
    if binary is None:
        low, high, dtype = 0, 0, U8
    else:
        low, high, dtype = binary
        if dtype not in (U8, I32, F32):
            raise ValueError(f"bin_img dtype must be uint8, int32 or float32, got {dtype}")
        if n_thresh != 1:
            raise RuntimeError("a two-valued image takes one threshold per frame")
    shape = tuple(frames.shape)
    out = torch.empty(shape or (1,), dtype=dtype, device=f.device)
    N.call("mi_threshold_apply", f.data_ptr(), code, batch, pixels, t.data_ptr(), n_thresh, _PIX[dtype],
           0 if binary is None else 1, int(low), int(high), out.data_ptr(), N.stream_ptr())
    return out if shape else out.reshape(())


def otsu(frames: torch.Tensor, min_val: int, max_val: int, dtype: torch.dtype = I32):
    """OtsuThreshold.forward for one frame or a batch: histogram -> threshold -> two-valued image on the current stream
    with nothing read back in between.  Returns (thresh int32 () / (B,), bin_img in `dtype` with the frames' shape:
    min_val where v <= thresh, max_val elsewhere).  max_val is inclusive: max_val - min_val + 1 bins."""
    if dtype not in (U8, I32, F32):
        raise ValueError(f"bin_img dtype must be uint8, int32 or float32, got {dtype}")
    hist = histogram(frames, min_val, _check_bins(int(max_val) - int(min_val) + 1, "otsu"))
    thresh = otsu_threshold(hist, min_val)
    return thresh, threshold_apply(frames, thresh, binary=(int(min_val), int(max_val), dtype))


# ---- relative pose (K15: vo/pose_estimation.py:53-162 on the GPU) ---------------------------------------------------------

POSE_MAX_N = N.MI_POSE_MAX_N
POSE_MAX_REFINE_ROUNDS = N.MI_POSE_MAX_REFINE_ROUNDS


def _row_pairs(a: torch.Tensor, b: torch.Tensor, valid: torch.Tensor | None, what: str, widths: tuple, limit: int, names: tuple,
               rows: str = "rows"):
    """The two (B, N, widths[i]) float32 arrays of a RANSAC solver and an optional (B, N) mask, as the C ABI reads them."""
    qa, qb = a.float().contiguous(), b.float().contiguous()
    if qa.dim() != 3 or qb.dim() != 3 or (qa.shape[-1], qb.shape[-1]) != widths or qa.shape[:2] != qb.shape[:2]:
        must = f"both be (B, N, {widths[0]})" if widths[0] == widths[1] else f"be (B, N, {widths[0]}) and (B, N, {widths[1]})"
        raise RuntimeError(f"{what}: points must {must}, got {tuple(a.shape)} and {tuple(b.shape)}")
    bsz, n = int(qa.shape[0]), int(qa.shape[1])
    if not 1 <= n <= limit:
        raise RuntimeError(f"{what}: N = {n} {rows}, supported: 1 .. {limit}")
    v = _validity_bytes(valid)
    if v is not None and tuple(v.shape) != (bsz, n):
        raise RuntimeError(f"{what}: the mask must be ({bsz}, {n}), got {tuple(v.shape)}")
    N.dev(qa, F32, names[0]), N.dev(qb, F32, names[1])
    return qa, qb, v, bsz, n


def _correspondences(pts1, pts2, valid, what: str):
    """(B, N, 2) normalised (x, y) points of both views"""
    return _row_pairs(pts1, pts2, valid, what, (2, 2), POSE_MAX_N, ("pts1", "pts2"), "correspondences")


def _hypotheses(entry: str, qa: torch.Tensor, qb: torch.Tensor, v, b: int, n: int, num_hypotheses: int, threshold: float,
                seed: int, floats: tuple):
    """`mi_*_hypotheses` share one signature: -> (models (B, H, *floats), MSAC cost (B, H) float32, count (B, H) int32)"""
    h = int(num_hypotheses)
    m_h = torch.empty((b, h, *floats), dtype=F32, device=qa.device)
    cost = torch.empty((b, h), dtype=F32, device=qa.device)
    count = torch.empty((b, h), dtype=I32, device=qa.device)
    N.call(entry, qa.data_ptr(), qb.data_ptr(), N.opt(v, U8, "valid"), b, n, h, float(threshold),
           int(seed) & 0xFFFFFFFF, m_h.data_ptr(), cost.data_ptr(), count.data_ptr(), N.stream_ptr())
    return m_h, cost, count


def _pose_outputs(b: int, dev):
    """R (B, 3, 3) and t (B, 3) float32"""
    return torch.empty((b, 3, 3), dtype=F32, device=dev), torch.empty((b, 3), dtype=F32, device=dev)


def _ransac_outputs(b: int, n: int, dev):
    """what every `mi_*_ransac` reports: inlier (B, N) uint8, best_h (B,) int32, count (B,) int32"""
    return (torch.empty((b, n), dtype=U8, device=dev), torch.empty((b,), dtype=I32, device=dev),
            torch.empty((b,), dtype=I32, device=dev))


def _ransac(entry: str, what: str, rows, num_hypotheses: int, threshold: float, refine_rounds: int, seed: int, outputs: tuple):
    """`mi_*_ransac` share one signature around their outputs (given in the ABI's order); rows: what _row_pairs returned"""
    qa, qb, v, b, n = rows
    h = int(num_hypotheses)
    work, wbytes = _workspace(f"{entry}_workspace_bytes", b, n, h, device=qa.device,
                              refusal=f"{what}: unsupported request (batch {b}, N {n}, {h} hypotheses)")
    N.call(entry, qa.data_ptr(), qb.data_ptr(), N.opt(v, U8, "valid"), b, n, h, float(threshold), int(refine_rounds),
           int(seed) & 0xFFFFFFFF, *(o.data_ptr() for o in outputs), work.data_ptr(), wbytes, N.stream_ptr())


def _matrix_refit(entry: str, what: str, pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor):
    """`mi_essential_refit` / `mi_homography_refit`: a 3 x 3 matrix over the masked correspondences -> (matrix, ok bool)"""
    q1, q2, v, b, n = _correspondences(pts1, pts2, mask, what)
    if v is None:
        raise RuntimeError(f"{what} needs a mask")
    mat = torch.empty((b, 3, 3), dtype=F32, device=q1.device)
    ok = torch.empty((b,), dtype=U8, device=q1.device)
    N.call(entry, q1.data_ptr(), q2.data_ptr(), N.dev(v, U8, "mask"), b, n, mat.data_ptr(), ok.data_ptr(), N.stream_ptr())
    return mat, ok.view(torch.bool)


def essential_hypotheses(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int,
                         threshold: float, seed: int = 0):
    """`mi_essential_hypotheses`: H 8-point hypotheses per pair from the counter-based sampler, each scored on every valid
    correspondence -> (E_h (B, H, 3, 3), MSAC cost (B, H) float32, inlier count (B, H) int32)."""
    return _hypotheses("mi_essential_hypotheses", *_correspondences(pts1, pts2, valid, "essential_hypotheses"), num_hypotheses,
                       threshold, seed, (3, 3))


def essential_refit(pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor):
    """`mi_essential_refit`: the linear 8-point E over the masked correspondences -> (E (B, 3, 3), ok (B,) bool)."""
    return _matrix_refit("mi_essential_refit", "essential_refit", pts1, pts2, mask)


def essential_ransac(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int,
                     threshold: float, refine_rounds: int = 3, seed: int = 0):
    """`mi_essential_ransac`: hypotheses, MSAC selection and refine_rounds rounds of refit-and-rescore in two launches ->
    (E (B, 3, 3), inlier (B, N) bool, best_h (B,) int32, count (B,) int32)."""
    rows = _correspondences(pts1, pts2, valid, "essential_ransac")
    b, n, dev = rows[3], rows[4], rows[0].device
    e = torch.empty((b, 3, 3), dtype=F32, device=dev)
    inlier, best_h, count = _ransac_outputs(b, n, dev)
    _ransac("mi_essential_ransac", "essential_ransac", rows, num_hypotheses, threshold, refine_rounds, seed,
            (e, inlier, best_h, count))
    return e, inlier.view(torch.bool), best_h, count


def recover_pose(e: torch.Tensor, pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor | None,
                 distance_threshold: float = 50.0):
    """`mi_recover_pose`: (R (B, 3, 3), t (B, 3), pose_mask (B, N) bool, count (B,) int32, ok (B,) bool) with
    x2 ~ R x1 + t, det R = +1, |t| = 1; identity / zero where fewer than 5 correspondences pass the depth test."""
    q1, q2, v, b, n = _correspondences(pts1, pts2, mask, "recover_pose")
    ee = e.float().contiguous()
    if tuple(ee.shape) != (b, 3, 3):
        raise RuntimeError(f"recover_pose: E must be ({b}, 3, 3), got {tuple(e.shape)}")
    r, t = _pose_outputs(b, q1.device)
    pose_mask = torch.empty((b, n), dtype=U8, device=q1.device)
    count = torch.empty((b,), dtype=I32, device=q1.device)
    ok = torch.empty((b,), dtype=U8, device=q1.device)
    N.call("mi_recover_pose", N.dev(ee, F32, "E"), q1.data_ptr(), q2.data_ptr(), N.opt(v, U8, "mask"),
           b, n, float(distance_threshold), r.data_ptr(), t.data_ptr(), pose_mask.data_ptr(), count.data_ptr(), ok.data_ptr(),
           N.stream_ptr())
    return r, t, pose_mask.view(torch.bool), count, ok.view(torch.bool)


def triangulate(proj1: torch.Tensor, proj2: torch.Tensor, pts1: torch.Tensor, pts2: torch.Tensor):
    """`mi_triangulate`: two-view DLT of (B, N, 2) points (x, y) under projection matrices (B, 3, 4) ->
    (points (B, N, 3), finite (B, N) bool); zeros where the homogeneous coordinate vanishes."""
    q1, q2 = pts1.float().contiguous(), pts2.float().contiguous()
    p1, p2 = proj1.float().contiguous(), proj2.float().contiguous()
    if q1.dim() != 3 or q1.shape[-1] != 2 or q1.shape != q2.shape or q1.shape[1] < 1:
        raise RuntimeError(f"triangulate: points must both be (B, N, 2), got {tuple(pts1.shape)} and {tuple(pts2.shape)}")
    b, n = int(q1.shape[0]), int(q1.shape[1])
    if tuple(p1.shape) != (b, 3, 4) or tuple(p2.shape) != (b, 3, 4):
        raise RuntimeError(f"triangulate: projection matrices must be ({b}, 3, 4), got {tuple(proj1.shape)}, {tuple(proj2.shape)}")
    out = torch.empty((b, n, 3), dtype=F32, device=q1.device)
    finite = torch.empty((b, n), dtype=U8, device=q1.device)
    N.call("mi_triangulate", N.dev(p1, F32, "proj1"), N.dev(p2, F32, "proj2"), N.dev(q1, F32, "pts1"), N.dev(q2, F32, "pts2"),
           b, n, out.data_ptr(), finite.data_ptr(), N.stream_ptr())
    return out, finite.view(torch.bool)


# ---- K17 metric RGB-D pose (include/mi355x_match.h, "metric RGB-D pose") ---------------------------------------------------

RIGID_MAX_N = N.MI_RIGID_MAX_N


def lift_keypoints(keypoints: torch.Tensor, depth: torch.Tensor, k_inv: torch.Tensor, z_scale: float = 1.0,
                   min_depth: float = 0.1, max_depth: float = 10.0, valid: torch.Tensor | None = None):
    """`mi_lift_keypoints`: keypoints (B, N, 2) in pixel (y, x) and depth (B, H, W), float32 or uint16, aligned to the camera
    of k_inv (3, 3) -> (points (B, N, 3) float32 = depth at the nearest pixel times the keypoint's ray, valid (B, N) bool).
    A row is valid when `valid` (optional, (B, N)) selects it, its pixel is inside the frame and min_depth <= depth *
    z_scale <= max_depth; the other rows are zero.  Current stream, no synchronisation, capturable."""
    if not depth.is_cuda:
        raise RuntimeError(f"lift_keypoints: depth must live on the GPU (got device {depth.device}); this package has no CPU path")
    if depth.dtype not in (F32, U16):
        raise RuntimeError(f"lift_keypoints: depth must be float32 or uint16, got {depth.dtype}")
    kp = keypoints.float().contiguous()
    if kp.dim() != 3 or kp.shape[-1] != 2 or kp.shape[1] < 1:
        raise RuntimeError(f"lift_keypoints: keypoints must be (B, N, 2), got {tuple(keypoints.shape)}")
    b, n = int(kp.shape[0]), int(kp.shape[1])
    if depth.dim() != 3 or depth.shape[0] != b or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise RuntimeError(f"lift_keypoints: depth must be ({b}, H, W), got {tuple(depth.shape)}")
    if not min_depth > 0 or not max_depth >= min_depth or not z_scale > 0:
        raise RuntimeError(f"lift_keypoints: need 0 < min_depth <= max_depth and z_scale > 0, got {min_depth}, {max_depth}, {z_scale}")
    d = depth.contiguous()
    ki = k_inv.float().contiguous()
    if tuple(ki.shape) != (3, 3):
        raise RuntimeError(f"lift_keypoints: K_inv must be (3, 3), got {tuple(k_inv.shape)}")
    v = _validity_bytes(valid)
    if v is not None and tuple(v.shape) != (b, n):
        raise RuntimeError(f"lift_keypoints: the mask must be ({b}, {n}), got {tuple(v.shape)}")
    pts = torch.empty((b, n, 3), dtype=F32, device=d.device)
    ok = torch.empty((b, n), dtype=U8, device=d.device)
    N.call("mi_lift_keypoints", N.dev(kp, F32, "keypoints"), d.data_ptr(), int(d.dtype == U16), b, n, int(d.shape[1]),
           int(d.shape[2]), N.dev(ki, F32, "K_inv"), float(z_scale), float(min_depth), float(max_depth),
           N.opt(v, U8, "valid"), pts.data_ptr(), ok.data_ptr(), N.stream_ptr())
    return pts, ok.view(torch.bool)


def _point_pairs(pts1, pts2, valid, what: str):
    """(B, N, 3) points of both frames"""
    return _row_pairs(pts1, pts2, valid, what, (3, 3), RIGID_MAX_N, ("pts1", "pts2"))


def rigid_hypotheses(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int,
                     threshold: float, seed: int = 0):
    """`mi_rigid_hypotheses`: H 3-point rigid motions per pair from the counter-based sampler, each scored on every valid
    row -> (rt_h (B, H, 12): R row-major then t, MSAC cost (B, H) float32, inlier count (B, H) int32)."""
    return _hypotheses("mi_rigid_hypotheses", *_point_pairs(pts1, pts2, valid, "rigid_hypotheses"), num_hypotheses, threshold, seed,
                       (12,))


def rigid_refit(pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor):
    """`mi_rigid_refit`: Horn's closed-form motion over the masked rows -> (R (B, 3, 3), t (B, 3), ok (B,) bool)."""
    q1, q2, v, b, n = _point_pairs(pts1, pts2, mask, "rigid_refit")
    if v is None:
        raise RuntimeError("rigid_refit needs a mask")
    r, t = _pose_outputs(b, q1.device)
    ok = torch.empty((b,), dtype=U8, device=q1.device)
    N.call("mi_rigid_refit", q1.data_ptr(), q2.data_ptr(), N.dev(v, U8, "mask"), b, n, r.data_ptr(), t.data_ptr(),
           ok.data_ptr(), N.stream_ptr())
    return r, t, ok.view(torch.bool)


def rigid_ransac(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int, threshold: float,
                 refine_rounds: int = 3, seed: int = 0):
    """`mi_rigid_ransac`: hypotheses, MSAC selection and refine_rounds rounds of refit-and-rescore in two launches ->
    (R (B, 3, 3), t (B, 3), inlier (B, N) bool, best_h (B,) int32, count (B,) int32, rmse (B,) float32, ok (B,) bool)."""
    rows = _point_pairs(pts1, pts2, valid, "rigid_ransac")
    b, n, dev = rows[3], rows[4], rows[0].device
    r, t = _pose_outputs(b, dev)
    inlier, best_h, count = _ransac_outputs(b, n, dev)
    rmse = torch.empty((b,), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    _ransac("mi_rigid_ransac", "rigid_ransac", rows, num_hypotheses, threshold, refine_rounds, seed,
            (r, t, inlier, best_h, count, rmse, ok))
    return r, t, inlier.view(torch.bool), best_h, count, rmse, ok.view(torch.bool)


# ---- K30 similarity alignment (include/mi355x_match_sim3.h) -----------------------------------------------------------------

SIM3_MAX_N = N.SIM3_CONSTANTS["MI_SIM3_MAX_N"]
SIM3_POINT, SIM3_REPROJ = N.SIM3_CONSTANTS["MI_SIM3_POINT"], N.SIM3_CONSTANTS["MI_SIM3_REPROJ"]


def _sim3_pairs(pts1, pts2, valid, what: str, metric: int | None = None):
    """(B, N, 3) points of both maps"""
    if metric is not None and metric not in (SIM3_POINT, SIM3_REPROJ):
        raise RuntimeError(f"{what}: metric must be SIM3_POINT ({SIM3_POINT}) or SIM3_REPROJ ({SIM3_REPROJ}), got {metric}")
    return _row_pairs(pts1, pts2, valid, what, (3, 3), SIM3_MAX_N, ("pts1", "pts2"))


def sim3_hypotheses(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int, threshold: float,
                    metric: int = SIM3_REPROJ, seed: int = 0):
    """`mi_sim3_hypotheses`: H 3-point similarities X2 = s R X1 + t per pair from the counter-based sampler, each scored on
    every valid row under `metric` -> (srt_h (B, H, 13): R row-major, t, s; MSAC cost (B, H) float32, inlier count (B, H)
    int32)."""
    qa, qb, v, b, n = _sim3_pairs(pts1, pts2, valid, "sim3_hypotheses", metric)
    h = int(num_hypotheses)
    m_h = torch.empty((b, h, 13), dtype=F32, device=qa.device)
    cost = torch.empty((b, h), dtype=F32, device=qa.device)
    count = torch.empty((b, h), dtype=I32, device=qa.device)
    N.call("mi_sim3_hypotheses", qa.data_ptr(), qb.data_ptr(), N.opt(v, U8, "valid"), b, n, h, float(threshold), int(metric),
           int(seed) & 0xFFFFFFFF, m_h.data_ptr(), cost.data_ptr(), count.data_ptr(), N.stream_ptr())
    return m_h, cost, count


def sim3_refit(pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor):
    """`mi_sim3_refit`: Horn's rotation and Umeyama's scale over the masked rows -> (s (B,), R (B, 3, 3), t (B, 3), ok (B,)
    bool)."""
    q1, q2, v, b, n = _sim3_pairs(pts1, pts2, mask, "sim3_refit")
    if v is None:
        raise RuntimeError("sim3_refit needs a mask")
    r, t = _pose_outputs(b, q1.device)
    s = torch.empty((b,), dtype=F32, device=q1.device)
    ok = torch.empty((b,), dtype=U8, device=q1.device)
    N.call("mi_sim3_refit", q1.data_ptr(), q2.data_ptr(), N.dev(v, U8, "mask"), b, n, s.data_ptr(), r.data_ptr(), t.data_ptr(),
           ok.data_ptr(), N.stream_ptr())
    return s, r, t, ok.view(torch.bool)


def sim3_ransac(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int, threshold: float,
                metric: int = SIM3_REPROJ, refine_rounds: int = 3, seed: int = 0):
    """`mi_sim3_ransac`: hypotheses, MSAC selection and refine_rounds rounds of refit-and-rescore in two launches ->
    (s (B,), R (B, 3, 3), t (B, 3), inlier (B, N) bool, best_h (B,) int32, count (B,) int32, rmse (B,) float32 in the metric's
    units, ok (B,) bool)."""
    qa, qb, v, b, n = _sim3_pairs(pts1, pts2, valid, "sim3_ransac", metric)
    dev, h = qa.device, int(num_hypotheses)
    r, t = _pose_outputs(b, dev)
    s = torch.empty((b,), dtype=F32, device=dev)
    inlier, best_h, count = _ransac_outputs(b, n, dev)
    rmse = torch.empty((b,), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    work, wbytes = _workspace("mi_sim3_ransac_workspace_bytes", b, n, h, device=dev,
                              refusal=f"sim3_ransac: unsupported request (batch {b}, N {n}, {h} hypotheses)")
    N.call("mi_sim3_ransac", qa.data_ptr(), qb.data_ptr(), N.opt(v, U8, "valid"), b, n, h, float(threshold), int(metric),
           int(refine_rounds), int(seed) & 0xFFFFFFFF, s.data_ptr(), r.data_ptr(), t.data_ptr(), inlier.data_ptr(),
           best_h.data_ptr(), count.data_ptr(), rmse.data_ptr(), ok.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return s, r, t, inlier.view(torch.bool), best_h, count, rmse, ok.view(torch.bool)


def sim3_apply(s: torch.Tensor, r: torch.Tensor, t: torch.Tensor, r_frames: torch.Tensor | None, t_frames: torch.Tensor | None,
               points: torch.Tensor | None):
    """`mi_sim3_apply`: map 1 moved into map 2's frame and units by (s (B,), R (B, 3, 3), t (B, 3)): frame poses r_frames
    (B, F, 3, 3), t_frames (B, F, 3) (X_c = R_k X + t_k) and landmarks points (B, L, 3) -> (r_out, t_out, points_out) with
    R_k' = R_k R^T, t_k' = s t_k - R_k' t, X' = s R X + t, float64 rounded once.  The poses or the points may be None (then
    None comes back), not both."""
    ss, rr, tt = s.float().contiguous(), r.float().contiguous(), t.float().contiguous()
    if ss.dim() != 1 or ss.shape[0] < 1 or tuple(rr.shape) != (ss.shape[0], 3, 3) or tuple(tt.shape) != (ss.shape[0], 3):
        raise RuntimeError(f"sim3_apply: s, R, t must be (B,), (B, 3, 3), (B, 3), got {tuple(s.shape)}, {tuple(r.shape)}, {tuple(t.shape)}")
    b, dev = int(ss.shape[0]), ss.device
    if (r_frames is None) != (t_frames is None):
        raise RuntimeError("sim3_apply: r_frames and t_frames must be given together")
    if r_frames is None and points is None:
        raise RuntimeError("sim3_apply needs frame poses or points")
    f = l = 0
    rk = tk = x = r_out = t_out = x_out = None
    if r_frames is not None:
        rk, tk = r_frames.float().contiguous(), t_frames.float().contiguous()
        if rk.dim() != 4 or tuple(rk.shape[::3]) != (b, 3) or rk.shape[2] != 3 or tuple(tk.shape) != (b, rk.shape[1], 3):
            raise RuntimeError(f"sim3_apply: frame poses must be ({b}, F, 3, 3) and ({b}, F, 3), got {tuple(r_frames.shape)}, "
                               f"{tuple(t_frames.shape)}")
        f = int(rk.shape[1])
    if points is not None:
        x = points.float().contiguous()
        if x.dim() != 3 or x.shape[0] != b or x.shape[2] != 3:
            raise RuntimeError(f"sim3_apply: points must be ({b}, L, 3), got {tuple(points.shape)}")
        l = int(x.shape[1])
    if f + l < 1:
        raise RuntimeError("sim3_apply: no frame and no point to move")
    if f:
        r_out, t_out = torch.empty_like(rk), torch.empty_like(tk)
    if l:
        x_out = torch.empty_like(x)
    N.call("mi_sim3_apply", N.dev(ss, F32, "s"), N.dev(rr, F32, "R"), N.dev(tt, F32, "t"), b, f, l,
           N.dev(rk, F32, "r_frames") if f else None, N.dev(tk, F32, "t_frames") if f else None,
           N.dev(x, F32, "points") if l else None, r_out.data_ptr() if f else None, t_out.data_ptr() if f else None,
           x_out.data_ptr() if l else None, N.stream_ptr())
    if r_frames is not None and not f:
        r_out, t_out = torch.empty_like(rk), torch.empty_like(tk)
    if points is not None and not l:
        x_out = torch.empty_like(x)
    return r_out, t_out, x_out


# ---- K23 absolute pose (include/mi355x_match.h, "absolute pose") ------------------------------------------------------------

PNP_MAX_N = N.MI_PNP_MAX_N


def _model_matches(pts3, pts2, valid, what: str):
    """(B, N, 3) model points and (B, N, 2) normalised (x, y) image points"""
    return _row_pairs(pts3, pts2, valid, what, (3, 2), PNP_MAX_N, ("pts3", "pts2"))


def pnp_hypotheses(pts3: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int, threshold: float,
                   seed: int = 0):
    """`mi_pnp_hypotheses`: H P3P poses per pair from the counter-based sampler (three rows solve, a fourth picks the
    candidate), each scored on every valid row by its reprojection distance in normalised units -> (rt_h (B, H, 12): R
    row-major then t, MSAC cost (B, H) float32, inlier count (B, H) int32)."""
    return _hypotheses("mi_pnp_hypotheses", *_model_matches(pts3, pts2, valid, "pnp_hypotheses"), num_hypotheses, threshold, seed,
                       (12,))


def pnp_refit(pts3: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor, r0: torch.Tensor, t0: torch.Tensor):
    """`mi_pnp_refit`: a fixed number of reprojection Gauss-Newton iterations over the masked rows from the pose r0 (B, 3, 3),
    t0 (B, 3) -> (R (B, 3, 3), t (B, 3), info (B, 6, 6) = J^T J at the result in (omega, tau) order, ok (B,) bool); where ok
    is False the pose is (r0, t0) and info zero."""
    q3, q2, v, b, n = _model_matches(pts3, pts2, mask, "pnp_refit")
    if v is None:
        raise RuntimeError("pnp_refit needs a mask")
    ra, ta = r0.float().contiguous(), t0.float().contiguous()
    if tuple(ra.shape) != (b, 3, 3) or tuple(ta.shape) != (b, 3):
        raise RuntimeError(f"pnp_refit: the starting pose must be ({b}, 3, 3) and ({b}, 3), got {tuple(r0.shape)} and {tuple(t0.shape)}")
    r, t = _pose_outputs(b, q3.device)
    info = torch.empty((b, 6, 6), dtype=F32, device=q3.device)
    ok = torch.empty((b,), dtype=U8, device=q3.device)
    N.call("mi_pnp_refit", q3.data_ptr(), q2.data_ptr(), N.dev(v, U8, "mask"), N.dev(ra, F32, "r0"), N.dev(ta, F32, "t0"), b, n,
           r.data_ptr(), t.data_ptr(), info.data_ptr(), ok.data_ptr(), N.stream_ptr())
    return r, t, info, ok.view(torch.bool)


def pnp_ransac(pts3: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int, threshold: float,
               refine_rounds: int = 3, seed: int = 0):
    """`mi_pnp_ransac`: hypotheses, MSAC selection and refine_rounds rounds of refit-and-rescore in two launches ->
    (R (B, 3, 3), t (B, 3), inlier (B, N) bool, best_h (B,) int32, count (B,) int32, rmse (B,) float32 in normalised units,
    info (B, 6, 6) float32, ok (B,) bool)."""
    rows = _model_matches(pts3, pts2, valid, "pnp_ransac")
    b, n, dev = rows[3], rows[4], rows[0].device
    r, t = _pose_outputs(b, dev)
    inlier, best_h, count = _ransac_outputs(b, n, dev)
    rmse = torch.empty((b,), dtype=F32, device=dev)
    info = torch.empty((b, 6, 6), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    _ransac("mi_pnp_ransac", "pnp_ransac", rows, num_hypotheses, threshold, refine_rounds, seed,
            (r, t, inlier, best_h, count, rmse, info, ok))
    return r, t, inlier.view(torch.bool), best_h, count, rmse, info, ok.view(torch.bool)


# ---- K24 planar two-view pose (include/mi355x_match.h, "planar two-view pose") ----------------------------------------------


def homography_hypotheses(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int,
                          threshold: float, seed: int = 0):
    """`mi_homography_hypotheses`: H 4-point homographies per pair from the counter-based sampler, each scored on every valid
    correspondence by its symmetric transfer error -> (H_h (B, H, 3, 3), MSAC cost (B, H) float32, inlier count (B, H) int32)."""
    return _hypotheses("mi_homography_hypotheses", *_correspondences(pts1, pts2, valid, "homography_hypotheses"), num_hypotheses,
                       threshold, seed, (3, 3))


def homography_refit(pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor):
    """`mi_homography_refit`: the normalised DLT homography over the masked correspondences -> (H (B, 3, 3), ok (B,) bool)."""
    return _matrix_refit("mi_homography_refit", "homography_refit", pts1, pts2, mask)


def homography_ransac(pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None, num_hypotheses: int,
                      threshold: float, refine_rounds: int = 3, seed: int = 0):
    """`mi_homography_ransac`: hypotheses, MSAC selection and refine_rounds rounds of refit-and-rescore in two launches ->
    (H (B, 3, 3), inlier (B, N) bool, best_h (B,) int32, count (B,) int32, MSAC cost (B,) float32)."""
    rows = _correspondences(pts1, pts2, valid, "homography_ransac")
    b, n, dev = rows[3], rows[4], rows[0].device
    hm = torch.empty((b, 3, 3), dtype=F32, device=dev)
    inlier, best_h, count = _ransac_outputs(b, n, dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    _ransac("mi_homography_ransac", "homography_ransac", rows, num_hypotheses, threshold, refine_rounds, seed,
            (hm, inlier, best_h, count, cost))
    return hm, inlier.view(torch.bool), best_h, count, cost


def homography_pose(h: torch.Tensor, pts1: torch.Tensor, pts2: torch.Tensor, mask: torch.Tensor | None):
    """`mi_homography_pose`: the four (R, t, normal) candidates of each homography, sorted by the number of masked rows in
    front of both cameras -> (R (B, 4, 3, 3), t (B, 4, 3) in units of the plane's distance, normal (B, 4, 3), count (B, 4)
    int32, pose_mask (B, N) bool: the rows passing under slot 0, rotation_only (B,) bool, ok (B,) bool)."""
    q1, q2, v, b, n = _correspondences(pts1, pts2, mask, "homography_pose")
    hh = h.float().contiguous()
    if tuple(hh.shape) != (b, 3, 3):
        raise RuntimeError(f"homography_pose: H must be ({b}, 3, 3), got {tuple(h.shape)}")
    r = torch.empty((b, 4, 3, 3), dtype=F32, device=q1.device)
    t = torch.empty((b, 4, 3), dtype=F32, device=q1.device)
    normal = torch.empty((b, 4, 3), dtype=F32, device=q1.device)
    count = torch.empty((b, 4), dtype=I32, device=q1.device)
    pose_mask = torch.empty((b, n), dtype=U8, device=q1.device)
    rot = torch.empty((b,), dtype=U8, device=q1.device)
    ok = torch.empty((b,), dtype=U8, device=q1.device)
    N.call("mi_homography_pose", N.dev(hh, F32, "H"), q1.data_ptr(), q2.data_ptr(), N.opt(v, U8, "mask"),
           b, n, r.data_ptr(), t.data_ptr(), normal.data_ptr(), count.data_ptr(), pose_mask.data_ptr(), rot.data_ptr(),
           ok.data_ptr(), N.stream_ptr())
    return r, t, normal, count, pose_mask.view(torch.bool), rot.view(torch.bool), ok.view(torch.bool)


def two_view_select(e: torch.Tensor, h: torch.Tensor, pts1: torch.Tensor, pts2: torch.Tensor, valid: torch.Tensor | None,
                    threshold_e: float, threshold_h: float, cut: float = 0.45):
    """`mi_two_view_select`: the truncated-residual scores of an essential matrix and a homography on the valid
    correspondences and the choice between them -> (score_e (B,) float32, score_h (B,) float32, choice (B,) bool: True for
    the homography, score_h > cut * (score_e + score_h))."""
    q1, q2, v, b, n = _correspondences(pts1, pts2, valid, "two_view_select")
    ee, hh = e.float().contiguous(), h.float().contiguous()
    if tuple(ee.shape) != (b, 3, 3) or tuple(hh.shape) != (b, 3, 3):
        raise RuntimeError(f"two_view_select: E and H must be ({b}, 3, 3), got {tuple(e.shape)} and {tuple(h.shape)}")
    se = torch.empty((b,), dtype=F32, device=q1.device)
    sh = torch.empty((b,), dtype=F32, device=q1.device)
    choice = torch.empty((b,), dtype=U8, device=q1.device)
    N.call("mi_two_view_select", N.dev(ee, F32, "E"), N.dev(hh, F32, "H"), q1.data_ptr(), q2.data_ptr(),
           N.opt(v, U8, "valid"), b, n, float(threshold_e), float(threshold_h), float(cut),
           se.data_ptr(), sh.data_ptr(), choice.data_ptr(), N.stream_ptr())
    return se, sh, choice.view(torch.bool)


# ---- K25 windowed bundle adjustment (include/mi355x_match.h, "windowed bundle adjustment") -----------------------------------

BA_MAX_FRAMES = N.MI_BA_MAX_FRAMES
BA_MAX_LANDMARKS = N.MI_BA_MAX_LANDMARKS
BA_MAX_ITERATIONS = N.MI_BA_MAX_ITERATIONS


def _ba_window(r: torch.Tensor, t: torch.Tensor, points: torch.Tensor, obs: torch.Tensor, vis: torch.Tensor, huber: float, what: str):
    """The state and the observations of a batch of windows as the C ABI reads them: r (B, F, 3, 3), t (B, F, 3), points
    (B, L, 3), obs (B, F, L, 2) normalised (u, v), vis (B, F, L)."""
    rr, tt, xx, oo = (a.float().contiguous() for a in (r, t, points, obs))
    if rr.dim() != 4 or tuple(rr.shape[2:]) != (3, 3) or xx.dim() != 3 or xx.shape[-1] != 3:
        raise RuntimeError(f"{what}: poses must be (B, F, 3, 3) and points (B, L, 3), got {tuple(r.shape)} and {tuple(points.shape)}")
    b, f, l = int(rr.shape[0]), int(rr.shape[1]), int(xx.shape[1])
    if tuple(tt.shape) != (b, f, 3) or xx.shape[0] != b or tuple(oo.shape) != (b, f, l, 2) or tuple(vis.shape) != (b, f, l):
        raise RuntimeError(f"{what}: expected t ({b}, {f}, 3), points ({b}, {l}, 3), obs ({b}, {f}, {l}, 2) and vis ({b}, {f}, {l}), got "
                           f"{tuple(t.shape)}, {tuple(points.shape)}, {tuple(obs.shape)} and {tuple(vis.shape)}")
    if not 2 <= f <= BA_MAX_FRAMES or not 1 <= l <= BA_MAX_LANDMARKS or b < 1:
        raise RuntimeError(f"{what}: F = {f} frames and L = {l} landmarks, supported: 2 .. {BA_MAX_FRAMES} and 1 .. {BA_MAX_LANDMARKS}")
    if not (huber >= 0 and huber < float("inf")):
        raise RuntimeError(f"{what}: huber must be finite and not negative, got {huber}")
    vv = _validity_bytes(vis)
    ptrs = (N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), N.dev(xx, F32, "points"), N.dev(oo, F32, "obs"), N.dev(vv, U8, "vis"))
    return ptrs, (rr, tt, xx, oo, vv), b, f, l


def ba_cost(r: torch.Tensor, t: torch.Tensor, points: torch.Tensor, obs: torch.Tensor, vis: torch.Tensor, huber: float = 0.0):
    """`mi_ba_cost`: the reprojection cost of a batch of windows -> (e2 (B, F, L) float32: the squared normalised distance of
    every seen observation of an active landmark, 0 elsewhere; cost (B,) float32; active (B, L) bool: seen in >= 2 frames)."""
    ptrs, keep, b, f, l = _ba_window(r, t, points, obs, vis, huber, "ba_cost")
    dev = keep[0].device
    e2 = torch.empty((b, f, l), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    active = torch.empty((b, l), dtype=U8, device=dev)
    N.call("mi_ba_cost", *ptrs, b, f, l, float(huber), e2.data_ptr(), cost.data_ptr(), active.data_ptr(), N.stream_ptr())
    return e2, cost, active.view(torch.bool)


def _ba_fixed(num_fixed: int, f: int, what: str) -> int:
    if not 1 <= int(num_fixed) <= f:
        raise RuntimeError(f"{what}: num_fixed must be in 1 .. {f}, got {num_fixed}")
    return int(num_fixed)


def ba_linearise(r: torch.Tensor, t: torch.Tensor, points: torch.Tensor, obs: torch.Tensor, vis: torch.Tensor, num_fixed: int = 1,
                 huber: float = 0.0):
    """`mi_ba_linearise`: one undamped linearisation with the landmarks eliminated -> (S (B, 6F, 6F) float32, the marginal
    information of the window's poses in (omega, tau) order per frame, zero for the first num_fixed frames; b (B, 6F); cost (B,))."""
    ptrs, keep, b, f, l = _ba_window(r, t, points, obs, vis, huber, "ba_linearise")
    nf = _ba_fixed(num_fixed, f, "ba_linearise")
    dev = keep[0].device
    s = torch.empty((b, 6 * f, 6 * f), dtype=F32, device=dev)
    rhs = torch.empty((b, 6 * f), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    work, wbytes = _workspace("mi_ba_workspace_bytes", b, f, l, device=dev)
    N.call("mi_ba_linearise", *ptrs, b, f, l, nf, float(huber), s.data_ptr(), rhs.data_ptr(), cost.data_ptr(), work.data_ptr(), wbytes,
           N.stream_ptr())
    return s, rhs, cost


def ba_refine(r: torch.Tensor, t: torch.Tensor, points: torch.Tensor, obs: torch.Tensor, vis: torch.Tensor, num_fixed: int = 1,
              iterations: int = 10, huber: float = 0.0):
    """`mi_ba_refine`: `iterations` Levenberg-Marquardt iterations on every window in one launch -> (R (B, F, 3, 3), t (B, F, 3),
    points (B, L, 3), point_ok (B, L) bool, cost0 (B,), cost (B,), accepted (B,) int32, info (B, 6F, 6F), ok (B,) bool).  The
    first num_fixed frames and the landmarks seen in fewer than 2 frames come back unchanged; where ok is False (a point
    behind a camera at the start, or no active landmark) everything does."""
    ptrs, keep, b, f, l = _ba_window(r, t, points, obs, vis, huber, "ba_refine")
    nf = _ba_fixed(num_fixed, f, "ba_refine")
    if not 1 <= int(iterations) <= BA_MAX_ITERATIONS:
        raise RuntimeError(f"ba_refine: iterations must be in 1 .. {BA_MAX_ITERATIONS}, got {iterations}")
    dev = keep[0].device
    ro = torch.empty((b, f, 3, 3), dtype=F32, device=dev)
    to = torch.empty((b, f, 3), dtype=F32, device=dev)
    xo = torch.empty((b, l, 3), dtype=F32, device=dev)
    point_ok = torch.empty((b, l), dtype=U8, device=dev)
    cost0 = torch.empty((b,), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    accepted = torch.empty((b,), dtype=I32, device=dev)
    info = torch.empty((b, 6 * f, 6 * f), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    work, wbytes = _workspace("mi_ba_workspace_bytes", b, f, l, device=dev)
    N.call("mi_ba_refine", *ptrs, b, f, l, nf, int(iterations), float(huber), ro.data_ptr(), to.data_ptr(), xo.data_ptr(),
           point_ok.data_ptr(), cost0.data_ptr(), cost.data_ptr(), accepted.data_ptr(), info.data_ptr(), ok.data_ptr(),
           work.data_ptr(), wbytes, N.stream_ptr())
    return ro, to, xo, point_ok.view(torch.bool), cost0, cost, accepted, info, ok.view(torch.bool)


# ---- K27 pose-graph optimisation (include/mi355x_match.h, "pose-graph optimisation") -----------------------------------------

PGO_MAX_NODES = N.MI_PGO_MAX_NODES
PGO_MAX_EDGES = N.MI_PGO_MAX_EDGES
PGO_MAX_ITERATIONS = N.MI_PGO_MAX_ITERATIONS
PGO_MAX_PCG = N.MI_PGO_MAX_PCG


def _pgo_graph(r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, r_meas: torch.Tensor, t_meas: torch.Tensor,
               information: torch.Tensor, edge_valid: torch.Tensor | None, huber: float, what: str, fixed: torch.Tensor | None = None):
    """The state and the edges of a batch of graphs as the C ABI reads them: r (B, N, 3, 3), t (B, N, 3), edge_index (B, E, 2),
    r_meas (B, E, 3, 3), t_meas (B, E, 3), information (B, E, 6, 6), edge_valid (B, E) or None (every edge); fixed (B, N) where the entry takes it (its pointer is then the last of `ptrs`)."""
    rr, tt, zr, zt, om = (a.float().contiguous() for a in (r, t, r_meas, t_meas, information))
    if rr.dim() != 4 or tuple(rr.shape[2:]) != (3, 3) or edge_index.dim() != 3 or edge_index.shape[-1] != 2:
        raise RuntimeError(f"{what}: poses must be (B, N, 3, 3) and edge_index (B, E, 2), got {tuple(r.shape)} and {tuple(edge_index.shape)}")
    b, n, e = int(rr.shape[0]), int(rr.shape[1]), int(edge_index.shape[1])
    if edge_valid is None:
        edge_valid = torch.ones((b, e), dtype=torch.bool, device=rr.device)
    if (tuple(tt.shape) != (b, n, 3) or edge_index.shape[0] != b or tuple(zr.shape) != (b, e, 3, 3) or tuple(zt.shape) != (b, e, 3)
            or tuple(om.shape) != (b, e, 6, 6) or tuple(edge_valid.shape) != (b, e)):
        raise RuntimeError(f"{what}: expected t ({b}, {n}, 3), r_meas ({b}, {e}, 3, 3), t_meas ({b}, {e}, 3), information ({b}, {e}, 6, 6) "
                           f"and edge_valid ({b}, {e}), got {tuple(t.shape)}, {tuple(r_meas.shape)}, {tuple(t_meas.shape)}, "
                           f"{tuple(information.shape)} and {tuple(edge_valid.shape)}")
    if not 2 <= n <= PGO_MAX_NODES or not 1 <= e <= PGO_MAX_EDGES or b < 1:
        raise RuntimeError(f"{what}: N = {n} nodes and E = {e} edges, supported: 2 .. {PGO_MAX_NODES} and 1 .. {PGO_MAX_EDGES}")
    if not (huber >= 0 and huber < float("inf")):
        raise RuntimeError(f"{what}: huber must be finite and not negative, got {huber}")
    if fixed is not None and tuple(fixed.shape) != (b, n):
        raise RuntimeError(f"{what}: fixed must be ({b}, {n}), got {tuple(fixed.shape)}")
    ei = edge_index.to(I32).contiguous()
    ev, fx = _validity_bytes(edge_valid), _validity_bytes(fixed)
    ptrs = (N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), N.dev(ei, I32, "edge_index"), N.dev(zr, F32, "r_meas"), N.dev(zt, F32, "t_meas"),
            N.dev(om, F32, "information"), N.dev(ev, U8, "edge_valid")) + (() if fx is None else (N.dev(fx, U8, "fixed"),))
    return ptrs, (rr, tt, ei, zr, zt, om, ev, fx), b, n, e


def pgo_cost(r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, r_meas: torch.Tensor, t_meas: torch.Tensor,
             information: torch.Tensor, edge_valid: torch.Tensor | None = None, huber: float = 0.0):
    """`mi_pgo_cost`: the cost of a batch of pose graphs -> (chi2 (B, E) float32: e^T Omega e of every active edge, 0 elsewhere;
    cost (B,) float32; active (B, E) bool)."""
    ptrs, keep, b, n, e = _pgo_graph(r, t, edge_index, r_meas, t_meas, information, edge_valid, huber, "pgo_cost")
    dev = keep[0].device
    chi2 = torch.empty((b, e), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    active = torch.empty((b, e), dtype=U8, device=dev)
    N.call("mi_pgo_cost", *ptrs, b, n, e, float(huber), chi2.data_ptr(), cost.data_ptr(), active.data_ptr(), N.stream_ptr())
    return chi2, cost, active.view(torch.bool)


def pgo_linearise(r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, r_meas: torch.Tensor, t_meas: torch.Tensor,
                  information: torch.Tensor, fixed: torch.Tensor, edge_valid: torch.Tensor | None = None, huber: float = 0.0):
    """`mi_pgo_linearise`: one undamped linearisation -> (diag (B, N, 6, 6): the diagonal blocks, zero for fixed and edgeless
    nodes; off (B, E, 6, 6): the (i, j) block of every edge, zero for inactive edges and edges at a fixed node; g (B, N, 6);
    cost (B,))."""
    ptrs, keep, b, n, e = _pgo_graph(r, t, edge_index, r_meas, t_meas, information, edge_valid, huber, "pgo_linearise", fixed)
    dev = keep[0].device
    diag = torch.empty((b, n, 6, 6), dtype=F32, device=dev)
    off = torch.empty((b, e, 6, 6), dtype=F32, device=dev)
    g = torch.empty((b, n, 6), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    work, wbytes = _workspace("mi_pgo_workspace_bytes", b, n, e, device=dev)
    N.call("mi_pgo_linearise", *ptrs, b, n, e, float(huber), diag.data_ptr(), off.data_ptr(), g.data_ptr(),
           cost.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return diag, off, g, cost


def pgo_refine(r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, r_meas: torch.Tensor, t_meas: torch.Tensor,
               information: torch.Tensor, fixed: torch.Tensor, edge_valid: torch.Tensor | None = None, iterations: int = 10,
               pcg_iterations: int = 64, huber: float = 0.0):
    """`mi_pgo_refine`: `iterations` Levenberg-Marquardt iterations of `pcg_iterations` conjugate-gradient trips each on every
    graph in one launch -> (R (B, N, 3, 3), t (B, N, 3), chi2 (B, E), cost0 (B,), cost (B,), accepted (B,) int32, info
    (B, N, 6, 6): each node's conditional information given its neighbours, ok (B,) bool).  Fixed nodes and nodes without an
    active edge come back unchanged; where ok is False (no active edge, no fixed node, no free node with an edge, or a cost
    that is not finite) everything does."""
    if not 1 <= int(iterations) <= PGO_MAX_ITERATIONS:
        raise RuntimeError(f"pgo_refine: iterations must be in 1 .. {PGO_MAX_ITERATIONS}, got {iterations}")
    if not 1 <= int(pcg_iterations) <= PGO_MAX_PCG:
        raise RuntimeError(f"pgo_refine: pcg_iterations must be in 1 .. {PGO_MAX_PCG}, got {pcg_iterations}")
    ptrs, keep, b, n, e = _pgo_graph(r, t, edge_index, r_meas, t_meas, information, edge_valid, huber, "pgo_refine", fixed)
    dev = keep[0].device
    ro = torch.empty((b, n, 3, 3), dtype=F32, device=dev)
    to = torch.empty((b, n, 3), dtype=F32, device=dev)
    chi2 = torch.empty((b, e), dtype=F32, device=dev)
    cost0 = torch.empty((b,), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    accepted = torch.empty((b,), dtype=I32, device=dev)
    info = torch.empty((b, n, 6, 6), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    work, wbytes = _workspace("mi_pgo_workspace_bytes", b, n, e, device=dev)
    N.call("mi_pgo_refine", *ptrs, b, n, e, int(iterations), int(pcg_iterations), float(huber), ro.data_ptr(),
           to.data_ptr(), chi2.data_ptr(), cost0.data_ptr(), cost.data_ptr(), accepted.data_ptr(), info.data_ptr(), ok.data_ptr(),
           work.data_ptr(), wbytes, N.stream_ptr())
    return ro, to, chi2, cost0, cost, accepted, info, ok.view(torch.bool)


# ---- K31 Sim(3) pose-graph optimisation (include/mi355x_match_simgraph.h) ----------------------------------------------------

SIMGRAPH_MAX_NODES = N.SIMGRAPH_CONSTANTS["MI_SIMGRAPH_MAX_NODES"]
SIMGRAPH_MAX_EDGES = N.SIMGRAPH_CONSTANTS["MI_SIMGRAPH_MAX_EDGES"]
SIMGRAPH_MAX_ITERATIONS = N.SIMGRAPH_CONSTANTS["MI_SIMGRAPH_MAX_ITERATIONS"]
SIMGRAPH_MAX_PCG = N.SIMGRAPH_CONSTANTS["MI_SIMGRAPH_MAX_PCG"]


def _simgraph_graph(s: torch.Tensor, r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s_meas: torch.Tensor,
                    r_meas: torch.Tensor, t_meas: torch.Tensor, information: torch.Tensor, edge_valid: torch.Tensor | None, huber: float,
                    what: str, fixed: torch.Tensor | None = None):
    """The state and the edges of a batch of similarity graphs as the C ABI reads them: s (B, N), r (B, N, 3, 3), t (B, N, 3),
    edge_index (B, E, 2), s_meas (B, E), r_meas (B, E, 3, 3), t_meas (B, E, 3), information (B, E, 7, 7), edge_valid (B, E) or
    None (every edge); fixed (B, N) where the entry takes it (its pointer is then the last of `ptrs`)."""
    ss, rr, tt, zs, zr, zt, om = (a.float().contiguous() for a in (s, r, t, s_meas, r_meas, t_meas, information))
    if rr.dim() != 4 or tuple(rr.shape[2:]) != (3, 3) or edge_index.dim() != 3 or edge_index.shape[-1] != 2:
        raise RuntimeError(f"{what}: rotations must be (B, N, 3, 3) and edge_index (B, E, 2), got {tuple(r.shape)} and {tuple(edge_index.shape)}")
    b, n, e = int(rr.shape[0]), int(rr.shape[1]), int(edge_index.shape[1])
    if edge_valid is None:
        edge_valid = torch.ones((b, e), dtype=torch.bool, device=rr.device)
    if (tuple(ss.shape) != (b, n) or tuple(tt.shape) != (b, n, 3) or edge_index.shape[0] != b or tuple(zs.shape) != (b, e)
            or tuple(zr.shape) != (b, e, 3, 3) or tuple(zt.shape) != (b, e, 3) or tuple(om.shape) != (b, e, 7, 7)
            or tuple(edge_valid.shape) != (b, e)):
        raise RuntimeError(f"{what}: expected s ({b}, {n}), t ({b}, {n}, 3), s_meas ({b}, {e}), r_meas ({b}, {e}, 3, 3), t_meas ({b}, {e}, 3), "
                           f"information ({b}, {e}, 7, 7) and edge_valid ({b}, {e}), got {tuple(s.shape)}, {tuple(t.shape)}, "
                           f"{tuple(s_meas.shape)}, {tuple(r_meas.shape)}, {tuple(t_meas.shape)}, {tuple(information.shape)} and "
                           f"{tuple(edge_valid.shape)}")
    if not 2 <= n <= SIMGRAPH_MAX_NODES or not 1 <= e <= SIMGRAPH_MAX_EDGES or b < 1:
        raise RuntimeError(f"{what}: N = {n} nodes and E = {e} edges, supported: 2 .. {SIMGRAPH_MAX_NODES} and 1 .. {SIMGRAPH_MAX_EDGES}")
    if not (huber >= 0 and huber < float("inf")):
        raise RuntimeError(f"{what}: huber must be finite and not negative, got {huber}")
    if fixed is not None and tuple(fixed.shape) != (b, n):
        raise RuntimeError(f"{what}: fixed must be ({b}, {n}), got {tuple(fixed.shape)}")
    ei = edge_index.to(I32).contiguous()
    ev, fx = _validity_bytes(edge_valid), _validity_bytes(fixed)
    ptrs = (N.dev(ss, F32, "s"), N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), N.dev(ei, I32, "edge_index"), N.dev(zs, F32, "s_meas"),
            N.dev(zr, F32, "r_meas"), N.dev(zt, F32, "t_meas"), N.dev(om, F32, "information"),
            N.dev(ev, U8, "edge_valid")) + (() if fx is None else (N.dev(fx, U8, "fixed"),))
    return ptrs, (ss, rr, tt, ei, zs, zr, zt, om, ev, fx), b, n, e


def simgraph_cost(s: torch.Tensor, r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s_meas: torch.Tensor,
                  r_meas: torch.Tensor, t_meas: torch.Tensor, information: torch.Tensor, edge_valid: torch.Tensor | None = None,
                  huber: float = 0.0):
    """`mi_simgraph_cost`: the cost of a batch of similarity graphs -> (chi2 (B, E) float32: e^T Omega e of every active edge, 0
    elsewhere; cost (B,) float32; active (B, E) bool)."""
    ptrs, keep, b, n, e = _simgraph_graph(s, r, t, edge_index, s_meas, r_meas, t_meas, information, edge_valid, huber, "simgraph_cost")
    dev = keep[0].device
    chi2 = torch.empty((b, e), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    active = torch.empty((b, e), dtype=U8, device=dev)
    N.call("mi_simgraph_cost", *ptrs, b, n, e, float(huber), chi2.data_ptr(), cost.data_ptr(), active.data_ptr(), N.stream_ptr())
    return chi2, cost, active.view(torch.bool)


def simgraph_linearise(s: torch.Tensor, r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s_meas: torch.Tensor,
                       r_meas: torch.Tensor, t_meas: torch.Tensor, information: torch.Tensor, fixed: torch.Tensor,
                       edge_valid: torch.Tensor | None = None, huber: float = 0.0):
    """`mi_simgraph_linearise`: one undamped linearisation -> (diag (B, N, 7, 7): the diagonal blocks, zero for fixed and
    edgeless nodes; off (B, E, 7, 7): the (i, j) block of every edge, zero for inactive edges and edges at a fixed node; g
    (B, N, 7); cost (B,))."""
    ptrs, keep, b, n, e = _simgraph_graph(s, r, t, edge_index, s_meas, r_meas, t_meas, information, edge_valid, huber,
                                          "simgraph_linearise", fixed)
    dev = keep[0].device
    diag = torch.empty((b, n, 7, 7), dtype=F32, device=dev)
    off = torch.empty((b, e, 7, 7), dtype=F32, device=dev)
    g = torch.empty((b, n, 7), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    work, wbytes = _workspace("mi_simgraph_workspace_bytes", b, n, e, device=dev)
    N.call("mi_simgraph_linearise", *ptrs, b, n, e, float(huber), diag.data_ptr(), off.data_ptr(), g.data_ptr(),
           cost.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return diag, off, g, cost


def simgraph_refine(s: torch.Tensor, r: torch.Tensor, t: torch.Tensor, edge_index: torch.Tensor, s_meas: torch.Tensor,
                    r_meas: torch.Tensor, t_meas: torch.Tensor, information: torch.Tensor, fixed: torch.Tensor,
                    edge_valid: torch.Tensor | None = None, iterations: int = 10, pcg_iterations: int = 64, huber: float = 0.0):
    """`mi_simgraph_refine`: `iterations` Levenberg-Marquardt iterations of `pcg_iterations` conjugate-gradient trips each on
    every graph in one launch -> (s (B, N), R (B, N, 3, 3), t (B, N, 3), chi2 (B, E), cost0 (B,), cost (B,), accepted (B,) int32,
    info (B, N, 7, 7): each node's conditional information given its neighbours, ok (B,) bool).  Fixed nodes and nodes without
    an active edge come back unchanged; where ok is False (no active edge, no fixed node, no free node with an edge, or a cost
    that is not finite -- a node scale that is not positive among the causes) everything does."""
    if not 1 <= int(iterations) <= SIMGRAPH_MAX_ITERATIONS:
        raise RuntimeError(f"simgraph_refine: iterations must be in 1 .. {SIMGRAPH_MAX_ITERATIONS}, got {iterations}")
    if not 1 <= int(pcg_iterations) <= SIMGRAPH_MAX_PCG:
        raise RuntimeError(f"simgraph_refine: pcg_iterations must be in 1 .. {SIMGRAPH_MAX_PCG}, got {pcg_iterations}")
    ptrs, keep, b, n, e = _simgraph_graph(s, r, t, edge_index, s_meas, r_meas, t_meas, information, edge_valid, huber,
                                          "simgraph_refine", fixed)
    dev = keep[0].device
    so = torch.empty((b, n), dtype=F32, device=dev)
    ro = torch.empty((b, n, 3, 3), dtype=F32, device=dev)
    to = torch.empty((b, n, 3), dtype=F32, device=dev)
    chi2 = torch.empty((b, e), dtype=F32, device=dev)
    cost0 = torch.empty((b,), dtype=F32, device=dev)
    cost = torch.empty((b,), dtype=F32, device=dev)
    accepted = torch.empty((b,), dtype=I32, device=dev)
    info = torch.empty((b, n, 7, 7), dtype=F32, device=dev)
    ok = torch.empty((b,), dtype=U8, device=dev)
    work, wbytes = _workspace("mi_simgraph_workspace_bytes", b, n, e, device=dev)
    N.call("mi_simgraph_refine", *ptrs, b, n, e, int(iterations), int(pcg_iterations), float(huber), so.data_ptr(), ro.data_ptr(),
           to.data_ptr(), chi2.data_ptr(), cost0.data_ptr(), cost.data_ptr(), accepted.data_ptr(), info.data_ptr(), ok.data_ptr(),
           work.data_ptr(), wbytes, N.stream_ptr())
    return so, ro, to, chi2, cost0, cost, accepted, info, ok.view(torch.bool)


def simgraph_correct(r_old: torch.Tensor | None, t_old: torch.Tensor | None, s: torch.Tensor | None, r: torch.Tensor | None,
                     t: torch.Tensor | None, points: torch.Tensor | None, ref: torch.Tensor | None):
    """`mi_simgraph_correct`: the map correction after a Sim(3) graph optimisation.  r_old (B, N, 3, 3), t_old (B, N, 3): the
    metric keyframe poses before; s (B, N), r, t: the optimised state; points (B, L, 3) with ref (B, L) integer: landmarks and
    the keyframe each is attached to -> (r_out, t_out, points_out): the metric poses (R', t' / s') and the landmarks
    R'^T ((R_old X + t_old) - t') / s', float64 rounded once; a landmark whose ref is outside [0, N) is copied.  The five pose
    arrays or the two landmark arrays may be None (then None comes back for them), not both."""
    poses, marks = (r_old, t_old, s, r, t), (points, ref)
    if any(a is None for a in poses) != all(a is None for a in poses) or (points is None) != (ref is None):
        raise RuntimeError("simgraph_correct: r_old, t_old, s, r, t are given together or not at all, and so are points and ref")
    if poses[0] is None and points is None:
        raise RuntimeError("simgraph_correct needs poses or points")
    b = int((s if s is not None else points).shape[0])
    n = l = 0
    ro = to = so = rn = tn = x = rf = r_out = t_out = x_out = None
    if s is not None:
        ro, to, so, rn, tn = (a.float().contiguous() for a in poses)
        n = int(so.shape[1]) if so.dim() == 2 else -1
        if n < 0 or any(tuple(a.shape) != (b, n, 3, 3) for a in (ro, rn)) or any(tuple(a.shape) != (b, n, 3) for a in (to, tn)):
            raise RuntimeError(f"simgraph_correct: poses must be (B, N, 3, 3), (B, N, 3), (B, N), (B, N, 3, 3), (B, N, 3), got "
                               f"{[tuple(a.shape) for a in poses]}")
    if points is not None:
        x, rf = points.float().contiguous(), ref.to(I32).contiguous()
        if x.dim() != 3 or x.shape[0] != b or x.shape[2] != 3 or tuple(rf.shape) != tuple(x.shape[:2]):
            raise RuntimeError(f"simgraph_correct: points must be ({b}, L, 3) and ref ({b}, L), got {tuple(points.shape)}, {tuple(ref.shape)}")
        l = int(x.shape[1])
    if b < 1 or n + l < 1:
        raise RuntimeError("simgraph_correct: no pose and no point to correct")
    if n:
        r_out, t_out = torch.empty_like(rn), torch.empty_like(tn)
    if l:
        x_out = torch.empty_like(x)
    on = lambda a, dt, what: N.opt(a if (a is None or a.numel()) else None, dt, what)
    N.call("mi_simgraph_correct", on(ro, F32, "r_old"), on(to, F32, "t_old"), on(so, F32, "s"), on(rn, F32, "r"), on(tn, F32, "t"),
           on(x, F32, "points"), on(rf, I32, "ref"), b, n, l, N.opt(r_out, F32, "r_out"), N.opt(t_out, F32, "t_out"),
           N.opt(x_out, F32, "points_out"), N.stream_ptr())
    return r_out, t_out, x_out


# ---- K28 landmark tracks (include/mi355x_match.h, "landmark tracks") ---------------------------------------------------------

TRACKS_MAX_FRAMES = N.MI_TRACKS_MAX_FRAMES
TRACKS_MAX_KEYPOINTS = N.MI_TRACKS_MAX_KEYPOINTS
TRACKS_MAX_PAIRS = N.MI_TRACKS_MAX_PAIRS
TRACKS_MAX_MATCHES = N.MI_TRACKS_MAX_MATCHES


def _tracks_views(min_views: int, f: int, what: str) -> int:
    if not 2 <= int(min_views) <= f:
        raise RuntimeError(f"{what}: min_views must be in 2 .. {f}, got {min_views}")
    return int(min_views)


def tracks_build(keypoints: torch.Tensor, pair_frames: torch.Tensor, match_ij: torch.Tensor, match_valid: torch.Tensor,
                 kp_valid: torch.Tensor | None = None, min_views: int = 2, landmarks: int = 2048):
    """`mi_tracks_build`: the pairwise matches of a batch of windows -> landmark tracks.  keypoints (B, F, K, 2) float32, copied
    and never interpreted; pair_frames (B, P, 2) integer (a, b); match_ij (B, P, M, 2) integer (i in a, j in b); match_valid
    (B, P, M); kp_valid (B, F, K) or None (every keypoint) -> (track_kp (B, F, L) int32: keypoint index or -1, vis (B, F, L)
    bool, track_keypoints (B, F, L, 2) float32, track_len (B, L) int32, kp_track (B, F, K) int32: slot, -2 for a conflicting
    component's node, -1 otherwise, counts (B, 4) int32: components of >= 2 nodes, conflicting, eligible, kept)."""
    kk = keypoints.float().contiguous()
    if kk.dim() != 4 or kk.shape[-1] != 2 or pair_frames.dim() != 3 or pair_frames.shape[-1] != 2 or match_ij.dim() != 4 or match_ij.shape[-1] != 2:
        raise RuntimeError(f"tracks_build: keypoints must be (B, F, K, 2), pair_frames (B, P, 2) and match_ij (B, P, M, 2), got "
                           f"{tuple(keypoints.shape)}, {tuple(pair_frames.shape)} and {tuple(match_ij.shape)}")
    b, f, k = (int(v) for v in kk.shape[:3])
    p, m = int(match_ij.shape[1]), int(match_ij.shape[2])
    if (tuple(pair_frames.shape) != (b, p, 2) or match_ij.shape[0] != b or tuple(match_valid.shape) != (b, p, m)
            or (kp_valid is not None and tuple(kp_valid.shape) != (b, f, k))):
        raise RuntimeError(f"tracks_build: expected pair_frames ({b}, {p}, 2), match_ij ({b}, {p}, {m}, 2), match_valid ({b}, {p}, {m}) and "
                           f"kp_valid ({b}, {f}, {k}) or None, got {tuple(pair_frames.shape)}, {tuple(match_ij.shape)}, "
                           f"{tuple(match_valid.shape)} and {None if kp_valid is None else tuple(kp_valid.shape)}")
    l = int(landmarks)
    if (b < 1 or not 2 <= f <= TRACKS_MAX_FRAMES or not 1 <= k <= TRACKS_MAX_KEYPOINTS or not 1 <= p <= TRACKS_MAX_PAIRS
            or not 1 <= m <= TRACKS_MAX_MATCHES or not 1 <= l <= BA_MAX_LANDMARKS):
        raise RuntimeError(f"tracks_build: F = {f} frames, K = {k} keypoints, P = {p} pairs, M = {m} matches and L = {l} landmarks, supported: "
                           f"2 .. {TRACKS_MAX_FRAMES}, 1 .. {TRACKS_MAX_KEYPOINTS}, 1 .. {TRACKS_MAX_PAIRS}, 1 .. {TRACKS_MAX_MATCHES} and "
                           f"1 .. {BA_MAX_LANDMARKS}")
    mv = _tracks_views(min_views, f, "tracks_build")
    pf, ij = pair_frames.to(I32).contiguous(), match_ij.to(I32).contiguous()
    mval, kval = _validity_bytes(match_valid), _validity_bytes(kp_valid)
    ptrs = (N.dev(pf, I32, "pair_frames"), N.dev(ij, I32, "match_ij"), N.dev(mval, U8, "match_valid"), N.opt(kval, U8, "kp_valid"),
            N.dev(kk, F32, "keypoints"))
    dev = kk.device
    track_kp = torch.empty((b, f, l), dtype=I32, device=dev)
    vis = torch.empty((b, f, l), dtype=U8, device=dev)
    track_keypoints = torch.empty((b, f, l, 2), dtype=F32, device=dev)
    track_len = torch.empty((b, l), dtype=I32, device=dev)
    kp_track = torch.empty((b, f, k), dtype=I32, device=dev)
    counts = torch.empty((b, 4), dtype=I32, device=dev)
    work, wbytes = _workspace("mi_tracks_workspace_bytes", b, f, k, p, m, l, device=dev)
    N.call("mi_tracks_build", *ptrs, b, f, k, p, m, mv, l, track_kp.data_ptr(), vis.data_ptr(), track_keypoints.data_ptr(),
           track_len.data_ptr(), kp_track.data_ptr(), counts.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return track_kp, vis.view(torch.bool), track_keypoints, track_len, kp_track, counts


def tracks_triangulate(r: torch.Tensor, t: torch.Tensor, obs: torch.Tensor, vis: torch.Tensor, min_views: int = 2,
                       max_e2: float = 1e-4, max_cos: float = 1.0):
    """`mi_tracks_triangulate`: the N-view triangulation of every landmark slot of a batch of windows.  r (B, F, 3, 3), t
    (B, F, 3) with X_c = R X + t, obs (B, F, L, 2) normalised (x, y), vis (B, F, L) -> (points (B, L, 3) float32, point_ok
    (B, L) bool, vis_out (B, F, L) bool: vis where point_ok, e2max (B, L): the largest squared normalised reprojection
    distance, cos_par (B, L): the cosine of the largest parallax angle between two seeing frames)."""
    rr, tt, oo = (a.float().contiguous() for a in (r, t, obs))
    if rr.dim() != 4 or tuple(rr.shape[2:]) != (3, 3) or oo.dim() != 4 or oo.shape[-1] != 2:
        raise RuntimeError(f"tracks_triangulate: poses must be (B, F, 3, 3) and obs (B, F, L, 2), got {tuple(r.shape)} and {tuple(obs.shape)}")
    b, f, l = int(rr.shape[0]), int(rr.shape[1]), int(oo.shape[2])
    if tuple(tt.shape) != (b, f, 3) or tuple(oo.shape) != (b, f, l, 2) or tuple(vis.shape) != (b, f, l):
        raise RuntimeError(f"tracks_triangulate: expected t ({b}, {f}, 3), obs ({b}, {f}, {l}, 2) and vis ({b}, {f}, {l}), got "
                           f"{tuple(t.shape)}, {tuple(obs.shape)} and {tuple(vis.shape)}")
    if b < 1 or not 2 <= f <= TRACKS_MAX_FRAMES or not 1 <= l <= BA_MAX_LANDMARKS:
        raise RuntimeError(f"tracks_triangulate: F = {f} frames and L = {l} landmarks, supported: 2 .. {TRACKS_MAX_FRAMES} and 1 .. {BA_MAX_LANDMARKS}")
    mv = _tracks_views(min_views, f, "tracks_triangulate")
    if not (0 < max_e2 < float("inf")) or not (-1 < max_cos <= 1):
        raise RuntimeError(f"tracks_triangulate: max_e2 must be positive and finite and max_cos in (-1, 1], got {max_e2} and {max_cos}")
    vv = _validity_bytes(vis)
    ptrs = (N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), N.dev(oo, F32, "obs"), N.dev(vv, U8, "vis"))
    dev = rr.device
    points = torch.empty((b, l, 3), dtype=F32, device=dev)
    point_ok = torch.empty((b, l), dtype=U8, device=dev)
    vis_out = torch.empty((b, f, l), dtype=U8, device=dev)
    e2max = torch.empty((b, l), dtype=F32, device=dev)
    cos_par = torch.empty((b, l), dtype=F32, device=dev)
    N.call("mi_tracks_triangulate", *ptrs, b, f, l, mv, float(max_e2), float(max_cos), points.data_ptr(), point_ok.data_ptr(),
           vis_out.data_ptr(), e2max.data_ptr(), cos_par.data_ptr(), N.stream_ptr())
    return points, point_ok.view(torch.bool), vis_out.view(torch.bool), e2max, cos_par


# ---- K29 local-map tracking (include/mi355x_match.h, "local-map tracking") ---------------------------------------------------

LOCALMAP_MAX_LANDMARKS = N.MI_LOCALMAP_MAX_LANDMARKS
LOCALMAP_MAX_KEYPOINTS = N.MI_LOCALMAP_MAX_KEYPOINTS
LOCALMAP_MAX_FRAMES = N.MI_LOCALMAP_MAX_FRAMES


def _localmap_bits(bits: torch.Tensor, lead: int, what: str):
    """Packed descriptors (..., W) int32 -- as `forward_bits` returns them -- or uint32 with `lead` leading dimensions, W = 8 or
    16, as the C ABI reads them: (int32 tensor, W)."""
    if bits.dim() != lead + 1 or bits.dtype not in (torch.int32, torch.uint32):
        raise RuntimeError(f"{what} must be {lead + 1}-dimensional packed descriptors (..., W) int32, got {tuple(bits.shape)} {bits.dtype}")
    b = bits.contiguous()
    if b.dtype != I32:
        b = b.view(I32)
    if int(b.shape[-1]) not in (8, 16):
        raise RuntimeError(f"{what}: {32 * int(b.shape[-1])}-bit descriptors, supported: 256 and 512")
    return b, int(b.shape[-1])


def localmap_descriptors(bits: torch.Tensor, track_kp: torch.Tensor):
    """`mi_localmap_descriptors`: a representative descriptor per landmark slot.  bits (B, F, K, W) packed hard bits of the
    window's frames, track_kp (B, F, L) integer as tracks_build returns it (anything outside 0 .. K - 1: not seen) ->
    (rep_bits (B, L, W) int32: the words of the view whose median Hamming distance to the slot's views is smallest, the
    lowest frame on a tie; rep_frame (B, L) int32: its frame, -1 for a slot nobody sees; rep_median (B, L) int32: that median,
    num_bits + 1 for a slot nobody sees)."""
    bb, w = _localmap_bits(bits, 3, "localmap_descriptors: bits")
    b, f, k = (int(v) for v in bb.shape[:3])
    if track_kp.dim() != 3 or tuple(track_kp.shape[:2]) != (b, f):
        raise RuntimeError(f"localmap_descriptors: expected track_kp ({b}, {f}, L), got {tuple(track_kp.shape)}")
    l = int(track_kp.shape[2])
    if b < 1 or not 1 <= f <= LOCALMAP_MAX_FRAMES or not 1 <= k <= LOCALMAP_MAX_KEYPOINTS or not 1 <= l <= LOCALMAP_MAX_LANDMARKS:
        raise RuntimeError(f"localmap_descriptors: F = {f} frames, K = {k} keypoints and L = {l} landmarks, supported: 1 .. {LOCALMAP_MAX_FRAMES}, "
                           f"1 .. {LOCALMAP_MAX_KEYPOINTS} and 1 .. {LOCALMAP_MAX_LANDMARKS}")
    tk = track_kp.to(I32).contiguous()
    ptrs = (N.dev(bb, I32, "bits"), N.dev(tk, I32, "track_kp"))
    dev = bb.device
    rep_bits = torch.empty((b, l, w), dtype=I32, device=dev)
    rep_frame = torch.empty((b, l), dtype=I32, device=dev)
    rep_median = torch.empty((b, l), dtype=I32, device=dev)
    N.call("mi_localmap_descriptors", *ptrs, b, f, k, l, 32 * w, rep_bits.data_ptr(), rep_frame.data_ptr(), rep_median.data_ptr(),
           N.stream_ptr())
    return rep_bits, rep_frame, rep_median


def localmap_match(points: torch.Tensor, point_valid: torch.Tensor | None, rep_bits: torch.Tensor, r: torch.Tensor, t: torch.Tensor,
                   cam: torch.Tensor, kp: torch.Tensor, kp_valid: torch.Tensor | None, kp_bits: torch.Tensor, height: int, width: int,
                   min_depth: float, max_depth: float, radius: float, max_distance: int, ratio: float):
    """`mi_localmap_match`: one frame per batch item against that item's landmarks, each searched inside a window round its
    projection.  points (B, L, 3), point_valid (B, L) or None, rep_bits (B, L, W), the predicted pose r (B, 3, 3), t (B, 3) with
    X_c = R X + t, cam (B, 4) = fx, fy, cx, cy, kp (B, K, 2) pixel (y, x), kp_valid (B, K) or None, kp_bits (B, K, W) ->
    (proj (B, L, 2) float32 pixel (y, x) or (-1, -1), lm_state (B, L) uint8: 0 not in view, 1 empty window, 2 failed the distance
    or ratio test, 3 lost its keypoint, 4 kept; lm_kp (B, L) int32; lm_distance (B, L) int32; match_keypoints (B, L, 2) float32;
    kp_lm (B, K) int32; counts (B, 5) int32)."""
    xx, rr, tt, cc, kk = (a.float().contiguous() for a in (points, r, t, cam, kp))
    if xx.dim() != 3 or xx.shape[-1] != 3 or kk.dim() != 3 or kk.shape[-1] != 2:
        raise RuntimeError(f"localmap_match: points must be (B, L, 3) and kp (B, K, 2), got {tuple(points.shape)} and {tuple(kp.shape)}")
    b, l, k = int(xx.shape[0]), int(xx.shape[1]), int(kk.shape[1])
    rb, w = _localmap_bits(rep_bits, 2, "localmap_match: rep_bits")
    kb, kw = _localmap_bits(kp_bits, 2, "localmap_match: kp_bits")
    if (tuple(rb.shape) != (b, l, w) or tuple(kb.shape) != (b, k, w) or kw != w or tuple(rr.shape) != (b, 3, 3) or tuple(tt.shape) != (b, 3)
            or tuple(cc.shape) != (b, 4) or kk.shape[0] != b or (point_valid is not None and tuple(point_valid.shape) != (b, l))
            or (kp_valid is not None and tuple(kp_valid.shape) != (b, k))):
        raise RuntimeError(f"localmap_match: expected rep_bits ({b}, {l}, W), r ({b}, 3, 3), t ({b}, 3), cam ({b}, 4), kp ({b}, {k}, 2), kp_bits "
                           f"({b}, {k}, W) and masks ({b}, {l}) / ({b}, {k}) or None, got {tuple(rep_bits.shape)}, {tuple(r.shape)}, {tuple(t.shape)}, "
                           f"{tuple(cam.shape)}, {tuple(kp.shape)}, {tuple(kp_bits.shape)}, {None if point_valid is None else tuple(point_valid.shape)} "
                           f"and {None if kp_valid is None else tuple(kp_valid.shape)}")
    if b < 1 or b > 65535 or not 1 <= l <= LOCALMAP_MAX_LANDMARKS or not 1 <= k <= LOCALMAP_MAX_KEYPOINTS:
        raise RuntimeError(f"localmap_match: B = {b}, L = {l} landmarks and K = {k} keypoints, supported: 1 .. 65535, 1 .. {LOCALMAP_MAX_LANDMARKS} "
                           f"and 1 .. {LOCALMAP_MAX_KEYPOINTS}")
    inf = float("inf")
    if not (0 < min_depth < max_depth < inf) or not (0 < radius < inf) or not 0 <= int(max_distance) <= 32 * w or not (0 < ratio <= 1) \
            or int(height) < 1 or int(width) < 1:
        raise RuntimeError(f"localmap_match: need 0 < min_depth < max_depth < inf, 0 < radius < inf, 0 <= max_distance <= {32 * w}, 0 < ratio <= 1 "
                           f"and height, width >= 1, got {min_depth}, {max_depth}, {radius}, {max_distance}, {ratio}, {height}, {width}")
    pv, kv = _validity_bytes(point_valid), _validity_bytes(kp_valid)
    ptrs = (N.dev(xx, F32, "points"), N.opt(pv, U8, "point_valid"), N.dev(rb, I32, "rep_bits"), N.dev(rr, F32, "r"), N.dev(tt, F32, "t"),
            N.dev(cc, F32, "cam"), N.dev(kk, F32, "kp"), N.opt(kv, U8, "kp_valid"), N.dev(kb, I32, "kp_bits"))
    dev = xx.device
    proj = torch.empty((b, l, 2), dtype=F32, device=dev)
    lm_state = torch.empty((b, l), dtype=U8, device=dev)
    lm_kp = torch.empty((b, l), dtype=I32, device=dev)
    lm_distance = torch.empty((b, l), dtype=I32, device=dev)
    match_keypoints = torch.empty((b, l, 2), dtype=F32, device=dev)
    kp_lm = torch.empty((b, k), dtype=I32, device=dev)
    counts = torch.empty((b, 5), dtype=I32, device=dev)
    N.call("mi_localmap_match", *ptrs, b, l, k, 32 * w, int(height), int(width), float(min_depth), float(max_depth), float(radius),
           int(max_distance), float(ratio), proj.data_ptr(), lm_state.data_ptr(), lm_kp.data_ptr(), lm_distance.data_ptr(),
           match_keypoints.data_ptr(), kp_lm.data_ptr(), counts.data_ptr(), N.stream_ptr())
    return proj, lm_state, lm_kp, lm_distance, match_keypoints, kp_lm, counts


# ---- K26 loop-closure retrieval (include/mi355x_match.h, "loop-closure retrieval") -------------------------------------------

PLACE_MAX_DESCRIPTORS = N.MI_PLACE_MAX_DESCRIPTORS
PLACE_MAX_KEYFRAMES = N.MI_PLACE_MAX_KEYFRAMES
PLACE_MAX_CANDIDATES = N.MI_PLACE_MAX_CANDIDATES


def _place_bits(bits: torch.Tensor, valid: torch.Tensor | None, what: str):
    """Packed descriptors (frames, K, W) int32 -- as `forward_bits` returns them -- or uint32, W = 8 or 16, and their validity
    (frames, K) or None, as the C ABI reads them."""
    if bits.dim() != 3 or bits.dtype not in (torch.int32, torch.uint32):
        raise RuntimeError(f"{what}: packed descriptors must be (frames, K, W) int32, got {tuple(bits.shape)} {bits.dtype}")
    b = bits.contiguous()
    if b.dtype != torch.int32:
        b = b.view(torch.int32)
    frames, k, words = (int(s) for s in b.shape)
    if words not in (8, 16):
        raise RuntimeError(f"{what}: {32 * words}-bit descriptors, supported: 256 and 512")
    if frames < 1 or not 1 <= k <= PLACE_MAX_DESCRIPTORS:
        raise RuntimeError(f"{what}: {frames} frames of {k} descriptors, supported: >= 1 and 1 .. {PLACE_MAX_DESCRIPTORS}")
    if valid is not None and tuple(valid.shape) != (frames, k):
        raise RuntimeError(f"{what}: expected a validity mask ({frames}, {k}), got {tuple(valid.shape)}")
    return b, _validity_bytes(valid), frames, k, words


def place_votes(db_bits: torch.Tensor, db_valid: torch.Tensor | None, q_bits: torch.Tensor, q_valid: torch.Tensor | None,
                max_distance: int, ratio: float, frame_index: torch.Tensor | None = None, want_matches: bool = False):
    """`mi_place_votes`: every query frame's descriptors against the keyframes of a database -> votes (Q, S) int32, the number
    of query descriptors whose nearest database descriptor is within max_distance bits and passes the ratio test against the
    second nearest.  db_bits (N, Kd, W), q_bits (Q, Kq, W) packed hard bits, validity (N, Kd) / (Q, Kq) or None.  frame_index
    None: S = N, slot s is keyframe s; otherwise (Q, S) int32, the keyframe each slot scores, -1 = an empty slot.
    want_matches: -> (votes, nn_index (Q, S, Kq) int32, nn_distance (Q, S, Kq) int32, nn_vote (Q, S, Kq) bool)."""
    db, dbv, n, kd, words = _place_bits(db_bits, db_valid, "place_votes: database")
    qb, qv, q, kq, qwords = _place_bits(q_bits, q_valid, "place_votes: query")
    if qwords != words:
        raise RuntimeError(f"place_votes: the database holds {32 * words}-bit descriptors, the query {32 * qwords}-bit ones")
    if n > PLACE_MAX_KEYFRAMES or q > 65535:
        raise RuntimeError(f"place_votes: {n} keyframes and {q} queries, supported: <= {PLACE_MAX_KEYFRAMES} and <= 65535")
    if not 0 <= int(max_distance) <= 32 * words:
        raise RuntimeError(f"place_votes: max_distance must be in 0 .. {32 * words}, got {max_distance}")
    if not 0.0 < float(ratio) <= 1.0:
        raise RuntimeError(f"place_votes: ratio must be in (0, 1], got {ratio}")
    slots, fi = n, None
    if frame_index is not None:
        if frame_index.dim() != 2 or frame_index.shape[0] != q or frame_index.shape[1] < 1:
            raise RuntimeError(f"place_votes: frame_index must be ({q}, S), got {tuple(frame_index.shape)}")
        fi = frame_index.to(I32).contiguous()
        slots = int(fi.shape[1])
    ptrs = [N.dev(db, I32, "db_bits"), N.opt(dbv, U8, "db_valid"), n, kd, N.dev(qb, I32, "q_bits"),
            N.opt(qv, U8, "q_valid"), q, kq, N.opt(fi, I32, "frame_index"),
            slots, 32 * words, int(max_distance), float(ratio)]
    dev = db.device
    votes = torch.empty((q, slots), dtype=I32, device=dev)
    if not want_matches:
        N.call("mi_place_votes", *ptrs, votes.data_ptr(), None, None, None, N.stream_ptr())
        return votes
    nn_index = torch.empty((q, slots, kq), dtype=I32, device=dev)
    nn_distance = torch.empty((q, slots, kq), dtype=I32, device=dev)
    nn_vote = torch.empty((q, slots, kq), dtype=U8, device=dev)
    N.call("mi_place_votes", *ptrs, votes.data_ptr(), nn_index.data_ptr(), nn_distance.data_ptr(), nn_vote.data_ptr(), N.stream_ptr())
    return votes, nn_index, nn_distance, nn_vote.view(torch.bool)


def place_select(votes: torch.Tensor, num_candidates: int, min_votes: int, excl_lo: torch.Tensor | None = None,
                 excl_hi: torch.Tensor | None = None):
    """`mi_place_select`: votes (Q, N) int32 -> (cand_index (Q, C) int32, cand_votes (Q, C) int32): per query the keyframes
    with votes >= min_votes outside [excl_lo[q], excl_hi[q]), by (votes descending, index ascending); -1 / 0 in empty places."""
    if votes.dim() != 2 or votes.dtype != I32:
        raise RuntimeError(f"place_select: votes must be (Q, N) int32, got {tuple(votes.shape)} {votes.dtype}")
    v = votes.contiguous()
    q, n = int(v.shape[0]), int(v.shape[1])
    if q < 1 or not 1 <= n <= PLACE_MAX_KEYFRAMES:
        raise RuntimeError(f"place_select: {q} queries and {n} keyframes, supported: >= 1 and 1 .. {PLACE_MAX_KEYFRAMES}")
    if not 1 <= int(num_candidates) <= PLACE_MAX_CANDIDATES:
        raise RuntimeError(f"place_select: num_candidates must be in 1 .. {PLACE_MAX_CANDIDATES}, got {num_candidates}")
    if (excl_lo is None) != (excl_hi is None):
        raise RuntimeError("place_select: excl_lo and excl_hi come together")
    lo = hi = None
    if excl_lo is not None:
        if tuple(excl_lo.shape) != (q,) or tuple(excl_hi.shape) != (q,):
            raise RuntimeError(f"place_select: excl_lo and excl_hi must be ({q},), got {tuple(excl_lo.shape)} and {tuple(excl_hi.shape)}")
        lo, hi = excl_lo.to(I32).contiguous(), excl_hi.to(I32).contiguous()
    ptr = N.dev(v, I32, "votes")
    cand_index = torch.empty((q, int(num_candidates)), dtype=I32, device=v.device)
    cand_votes = torch.empty((q, int(num_candidates)), dtype=I32, device=v.device)
    N.call("mi_place_select", ptr, q, n, N.opt(lo, I32, "excl_lo"),
           N.opt(hi, I32, "excl_hi"), int(min_votes), int(num_candidates), cand_index.data_ptr(),
           cand_votes.data_ptr(), N.stream_ptr())
    return cand_index, cand_votes


# ---- K18 dense RGB-D refinement (include/mi355x_match.h, "dense RGB-D refinement") ------------------------------------------

ICP_MAX_STAGES = N.MI_ICP_MAX_STAGES
ICP_MAX_ITERATIONS = N.MI_ICP_MAX_ITERATIONS
ICP_STRIDES = (1, 2, 4, 8)
ICP_SUMS = 29


def surfel_maps(depth: torch.Tensor, k_inv: torch.Tensor, z_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                normal_max_jump: float = 0.1):
    """`mi_surfel_maps`: depth (B, H, W), float32 or uint16, aligned to the camera of k_inv (3, 3) -> (vertex, normal), each
    (B, H, W, 4) float32: the camera-frame point and the camera-facing surface normal of every pixel, with 1 / 0 in the
    fourth component for valid / invalid (invalid records are zero).  Current stream, no synchronisation, capturable."""
    if not depth.is_cuda:
        raise RuntimeError(f"surfel_maps: depth must live on the GPU (got device {depth.device}); this package has no CPU path")
    if depth.dtype not in (F32, U16):
        raise RuntimeError(f"surfel_maps: depth must be float32 or uint16, got {depth.dtype}")
    if depth.dim() != 3 or depth.shape[1] < 3 or depth.shape[2] < 3 or depth.shape[0] < 1:
        raise RuntimeError(f"surfel_maps: depth must be (B, H, W) with H, W >= 3, got {tuple(depth.shape)}")
    if not min_depth > 0 or not max_depth >= min_depth or not z_scale > 0 or not normal_max_jump > 0:
        raise RuntimeError(f"surfel_maps: need 0 < min_depth <= max_depth, z_scale > 0 and normal_max_jump > 0, got {min_depth}, "
                           f"{max_depth}, {z_scale}, {normal_max_jump}")
    d = depth.contiguous()
    ki = k_inv.float().contiguous()
    if tuple(ki.shape) != (3, 3):
        raise RuntimeError(f"surfel_maps: K_inv must be (3, 3), got {tuple(k_inv.shape)}")
    b, h, w = (int(x) for x in d.shape)
    vertex = torch.empty((b, h, w, 4), dtype=F32, device=d.device)
    normal = torch.empty((b, h, w, 4), dtype=F32, device=d.device)
    N.call("mi_surfel_maps", d.data_ptr(), int(d.dtype == U16), b, h, w, N.dev(ki, F32, "K_inv"), float(z_scale), float(min_depth),
           float(max_depth), float(normal_max_jump), vertex.data_ptr(), normal.data_ptr(), N.stream_ptr())
    return vertex, normal


def _rgbd_inputs(named_maps, r: torch.Tensor, t: torch.Tensor, camera, what: str, workspace: str):
    """The checks and conversions every dense linearisation / refinement shares.  named_maps: [(name, (B, H, W, 4) float32
    map)]; workspace: the entry that sizes the call's workspace (`mi_icp_workspace_bytes` or `mi_rgbd_workspace_bytes`)."""
    first = named_maps[0][1]
    if not first.is_cuda:
        raise RuntimeError(f"{what}: the maps must live on the GPU (got device {first.device}); this package has no CPU path")
    if first.dim() != 4 or first.shape[-1] != 4 or any(x.shape != first.shape or x.dtype != F32 for _, x in named_maps):
        raise RuntimeError(f"{what}: the maps must be float32 (B, H, W, 4) of one shape, got "
                           + ", ".join(f"{n} {x.dtype} {tuple(x.shape)}" for n, x in named_maps))
    b, h, w = int(first.shape[0]), int(first.shape[1]), int(first.shape[2])
    rr, tt = r.float().contiguous(), t.float().contiguous()
    if tuple(rr.shape) != (b, 3, 3) or tuple(tt.shape) != (b, 3):
        raise RuntimeError(f"{what}: the pose must be ({b}, 3, 3) and ({b}, 3), got {tuple(r.shape)} and {tuple(t.shape)}")
    keep = tuple(x.contiguous() for _, x in named_maps)
    maps = tuple(N.dev(x, F32, n) for (n, _), x in zip(named_maps, keep))
    cam = tuple(float(x) for x in camera)
    if len(cam) != 4:
        raise RuntimeError(f"{what}: camera must be (fx, fy, cx, cy), got {camera!r}")
    work, wbytes = _workspace(workspace, b, h, w, device=first.device, refusal=f"{what}: unsupported request (batch {b}, {h} x {w})")
    return keep, maps, rr, tt, cam, b, h, w, work, wbytes


def _surfel_named(maps1, maps2):
    (v1, n1), (v2, n2) = maps1, maps2
    return [("vertex1", v1), ("normal1", n1), ("vertex2", v2), ("normal2", n2)]


def _icp_schedule(schedule, what: str):
    """schedule of (stride, iterations) stages -> (strides, iterations, stages): the two c_int32 arrays as the pointers the
    C ABI takes (each keeps its array alive) and their length"""
    import ctypes
    sched = [(int(s), int(i)) for s, i in schedule]
    if not 1 <= len(sched) <= ICP_MAX_STAGES:
        raise RuntimeError(f"{what}: the schedule needs 1 .. {ICP_MAX_STAGES} stages, got {len(sched)}")
    strides = (ctypes.c_int32 * len(sched))(*[s for s, _ in sched])
    iters = (ctypes.c_int32 * len(sched))(*[i for _, i in sched])
    return ctypes.cast(strides, ctypes.c_void_p), ctypes.cast(iters, ctypes.c_void_p), len(sched)


def _refine_outputs(b: int, dev):
    """the outputs every refinement has: r, t, information, rmse, count, steps, ok (uint8)"""
    return (torch.empty((b, 3, 3), dtype=F32, device=dev), torch.empty((b, 3), dtype=F32, device=dev),
            torch.empty((b, 6, 6), dtype=F32, device=dev), torch.empty((b,), dtype=F32, device=dev),
            torch.empty((b,), dtype=I32, device=dev), torch.empty((b,), dtype=I32, device=dev), torch.empty((b,), dtype=U8, device=dev))


def icp_linearise(maps1, maps2, r: torch.Tensor, t: torch.Tensor, camera, stride: int = 1, distance_threshold: float = 0.1,
                  angle_threshold: float = 0.5235987755982988):
    """`mi_icp_linearise`: one point-to-plane linearisation of frame 1's surfels (maps1 = (vertex, normal) of `surfel_maps`)
    against frame 2's at the pose r (B, 3, 3), t (B, 3), camera = (fx, fy, cx, cy), over every stride-th source pixel ->
    sums (B, 29) float64: A's upper triangle row-major (21), b (6), sum r^2, count.  angle_threshold in radians."""
    keep, maps, rr, tt, cam, b, h, w, work, wbytes = _rgbd_inputs(_surfel_named(maps1, maps2), r, t, camera, "icp_linearise",
                                                                  "mi_icp_workspace_bytes")
    sums = torch.empty((b, ICP_SUMS), dtype=torch.float64, device=rr.device)
    N.call("mi_icp_linearise", *maps, N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), b, h, w, *cam, int(stride),
           float(distance_threshold), float(angle_threshold), sums.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return sums


def icp_refine(maps1, maps2, r0: torch.Tensor, t0: torch.Tensor, camera, schedule=((4, 4), (2, 4), (1, 6)),
               distance_threshold: float = 0.1, angle_threshold: float = 0.5235987755982988, min_correspondences: int = 64):
    """`mi_icp_refine`: projective point-to-plane ICP from (r0, t0) over the schedule's (stride, iterations) stages ->
    (R (B, 3, 3), t (B, 3), information (B, 6, 6) float32, rmse (B,) float32, count (B,) int32, steps (B,) int32,
    ok (B,) bool).  X2 = R X1 + t.  A pair whose system is degenerate keeps the pose before the failed solve, ok = False."""
    keep, maps, rr, tt, cam, b, h, w, work, wbytes = _rgbd_inputs(_surfel_named(maps1, maps2), r0, t0, camera, "icp_refine",
                                                                  "mi_icp_workspace_bytes")
    strides, iters, stages = _icp_schedule(schedule, "icp_refine")
    r, t, info, rmse, count, steps, ok = _refine_outputs(b, rr.device)
    N.call("mi_icp_refine", *maps, N.dev(rr, F32, "r0"), N.dev(tt, F32, "t0"), b, h, w, *cam, strides, iters, stages,
           float(distance_threshold), float(angle_threshold), int(min_correspondences), r.data_ptr(), t.data_ptr(), info.data_ptr(),
           rmse.data_ptr(), count.data_ptr(), steps.data_ptr(), ok.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return r, t, info, rmse, count, steps, ok.view(torch.bool)


# ---- K21 direct RGB-D refinement (include/mi355x_match.h, "direct RGB-D refinement") -----------------------------------------

def intensity_maps(gray: torch.Tensor):
    """`mi_intensity_maps`: gray frames (B, H, W), uint8 or float32 (`ingest_frames`' outputs) -> (B, H, W, 4) float32: the
    gray value, its central differences in x and y and 1 / 0 for valid / invalid (interior pixels with finite values;
    invalid records are zero).  Current stream, no synchronisation, capturable."""
    if not gray.is_cuda:
        raise RuntimeError(f"intensity_maps: gray must live on the GPU (got device {gray.device}); this package has no CPU path")
    if gray.dtype not in (F32, U8):
        raise RuntimeError(f"intensity_maps: gray must be float32 or uint8, got {gray.dtype}")
    if gray.dim() != 3 or gray.shape[1] < 3 or gray.shape[2] < 3 or gray.shape[0] < 1:
        raise RuntimeError(f"intensity_maps: gray must be (B, H, W) with H, W >= 3, got {tuple(gray.shape)}")
    g = gray.contiguous()
    b, h, w = (int(x) for x in g.shape)
    out = torch.empty((b, h, w, 4), dtype=F32, device=g.device)
    N.call("mi_intensity_maps", g.data_ptr(), int(g.dtype == U8), b, h, w, out.data_ptr(), N.stream_ptr())
    return out


def photo_linearise(vertex1: torch.Tensor, intensity1: torch.Tensor, vertex2: torch.Tensor, intensity2: torch.Tensor,
                    r: torch.Tensor, t: torch.Tensor, camera, stride: int = 1, distance_threshold: float = 0.1,
                    intensity_threshold: float = 30.0):
    """`mi_photo_linearise`: one photometric linearisation of frame 1's pixels (its `surfel_maps` vertex map and
    `intensity_maps` map) against frame 2's at the pose r (B, 3, 3), t (B, 3), camera = (fx, fy, cx, cy), over every
    stride-th source pixel -> sums (B, 29) float64 in `icp_linearise`'s layout.  distance_threshold is the occlusion gate
    on depth, intensity_threshold the gate on the residual in gray levels."""
    named = [("vertex1", vertex1), ("intensity1", intensity1), ("vertex2", vertex2), ("intensity2", intensity2)]
    keep, maps, rr, tt, cam, b, h, w, work, wbytes = _rgbd_inputs(named, r, t, camera, "photo_linearise", "mi_rgbd_workspace_bytes")
    sums = torch.empty((b, ICP_SUMS), dtype=torch.float64, device=rr.device)
    N.call("mi_photo_linearise", *maps, N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), b, h, w, *cam, int(stride),
           float(distance_threshold), float(intensity_threshold), sums.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return sums


def rgbd_refine(maps1, maps2, r0: torch.Tensor, t0: torch.Tensor, camera, schedule=((4, 4), (2, 4), (1, 6)),
                distance_threshold: float = 0.1, angle_threshold: float = 0.5235987755982988, photo_weight: float = 0.003,
                intensity_threshold: float = 30.0, min_correspondences: int = 64):
    """`mi_rgbd_refine`: `icp_refine` with a photometric term joined to every step.  maps1, maps2 = (vertex, normal,
    intensity) of `surfel_maps` and `intensity_maps` -> (R (B, 3, 3), t (B, 3), information (B, 6, 6) float32 of the joint
    system, rmse (B,) float32 and count (B,) int32 of the geometric term, rmse_photo (B,) float32 and count_photo (B,) int32
    of the photometric term, steps (B,) int32, ok (B,) bool).  photo_weight is the depth's unit per gray level; 0 gives
    `icp_refine`'s bits."""
    names = ("vertex", "normal", "intensity")
    if len(maps1) != 3 or len(maps2) != 3:
        raise RuntimeError("rgbd_refine: maps1 and maps2 must each be (vertex, normal, intensity)")
    named = [(f"{n}{i}", x) for i, maps in ((1, maps1), (2, maps2)) for n, x in zip(names, maps)]
    keep, maps, rr, tt, cam, b, h, w, work, wbytes = _rgbd_inputs(named, r0, t0, camera, "rgbd_refine", "mi_rgbd_workspace_bytes")
    strides, iters, stages = _icp_schedule(schedule, "rgbd_refine")
    r, t, info, rmse, count, steps, ok = _refine_outputs(b, rr.device)
    rmse_photo = torch.empty((b,), dtype=F32, device=rr.device)
    count_photo = torch.empty((b,), dtype=I32, device=rr.device)
    N.call("mi_rgbd_refine", *maps, N.dev(rr, F32, "r0"), N.dev(tt, F32, "t0"), b, h, w, *cam, strides, iters, stages,
           float(distance_threshold), float(angle_threshold), float(photo_weight), float(intensity_threshold),
           int(min_correspondences), r.data_ptr(), t.data_ptr(), info.data_ptr(), rmse.data_ptr(), count.data_ptr(),
           rmse_photo.data_ptr(), count_photo.data_ptr(), steps.data_ptr(), ok.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return r, t, info, rmse, count, rmse_photo, count_photo, steps, ok.view(torch.bool)


# ---- K19 TSDF fusion (include/mi355x_match.h, "TSDF fusion") ------------------------------------------------------------------

def _tsdf_volume(volume: torch.Tensor, what: str):
    if not volume.is_cuda:
        raise RuntimeError(f"{what}: the volume must live on the GPU (got device {volume.device}); this package has no CPU path")
    if volume.dtype != F32 or volume.dim() != 5 or volume.shape[-1] != 2 or min(volume.shape[:4]) < 1 or min(volume.shape[1:4]) < 2:
        raise RuntimeError(f"{what}: the volume must be float32 (B, NZ, NY, NX, 2) with NZ, NY, NX >= 2, got {volume.dtype} "
                           f"{tuple(volume.shape)}")
    return N.dev(volume, F32, "volume"), tuple(int(x) for x in volume.shape[:4])


def _tsdf_grid(origin, voxel_size: float, truncation: float, what: str):
    o = tuple(float(x) for x in origin)
    if len(o) != 3 or not voxel_size > 0 or not truncation > 0:
        raise RuntimeError(f"{what}: need an origin of 3 values, voxel_size > 0 and truncation > 0, got {origin}, {voxel_size}, "
                           f"{truncation}")
    return (*o, float(voxel_size), float(truncation))


def tsdf_reset(volume: torch.Tensor) -> torch.Tensor:
    """`mi_tsdf_reset`: (tsdf, weight) = (1, 0) into every voxel of volume (B, NZ, NY, NX, 2) float32, in place."""
    ptr, dims = _tsdf_volume(volume, "tsdf_reset")
    N.call("mi_tsdf_reset", ptr, *dims, N.stream_ptr())
    return volume


def tsdf_integrate(volume: torch.Tensor, depth: torch.Tensor, r: torch.Tensor, t: torch.Tensor, camera, origin, voxel_size: float,
                   truncation: float, max_weight: float = 64.0, z_scale: float = 1.0, min_depth: float = 0.1,
                   max_depth: float = 10.0, active: torch.Tensor | None = None) -> torch.Tensor:
    """`mi_tsdf_integrate`: depth (B, F, H, W), float32 or uint16, aligned to camera = (fx, fy, cx, cy), with the world-to-camera
    poses r (B, F, 3, 3), t (B, F, 3), fused into volume (B, NZ, NY, NX, 2) in place, the frames in order, in one pass over the
    volume.  active (B, F) bool / uint8 on the GPU (None: every frame) is read by the kernel: no synchronisation."""
    ptr, dims = _tsdf_volume(volume, "tsdf_integrate")
    if not depth.is_cuda:
        raise RuntimeError(f"tsdf_integrate: depth must live on the GPU (got device {depth.device}); this package has no CPU path")
    if depth.dtype not in (F32, U16):
        raise RuntimeError(f"tsdf_integrate: depth must be float32 or uint16, got {depth.dtype}")
    b = dims[0]
    if depth.dim() != 4 or depth.shape[0] != b or depth.shape[1] < 1 or depth.shape[2] < 3 or depth.shape[3] < 3:
        raise RuntimeError(f"tsdf_integrate: depth must be ({b}, F, H, W) with F >= 1 and H, W >= 3, got {tuple(depth.shape)}")
    d = depth.contiguous()
    f, h, w = (int(x) for x in d.shape[1:])
    rr, tt = r.float().contiguous(), t.float().contiguous()
    if tuple(rr.shape) != (b, f, 3, 3) or tuple(tt.shape) != (b, f, 3):
        raise RuntimeError(f"tsdf_integrate: the poses must be ({b}, {f}, 3, 3) and ({b}, {f}, 3), got {tuple(r.shape)} and "
                           f"{tuple(t.shape)}")
    act = None
    if active is not None:
        if active.dtype not in (torch.bool, U8) or tuple(active.shape) != (b, f):
            raise RuntimeError(f"tsdf_integrate: active must be bool or uint8 ({b}, {f}), got {active.dtype} {tuple(active.shape)}")
        act = active.contiguous().view(U8)
    grid = _tsdf_grid(origin, voxel_size, truncation, "tsdf_integrate")
    fx, fy, cx, cy = (float(x) for x in camera)
    N.call("mi_tsdf_integrate", ptr, *dims, *grid, float(max_weight), d.data_ptr(), int(d.dtype == U16), f, h, w, fx, fy, cx, cy,
           float(z_scale), float(min_depth), float(max_depth), N.dev(rr, F32, "r"), N.dev(tt, F32, "t"),
           N.opt(act, U8, "active"), N.stream_ptr())
    return volume


def tsdf_raycast(volume: torch.Tensor, r: torch.Tensor, t: torch.Tensor, k_inv: torch.Tensor, size, origin, voxel_size: float,
                 truncation: float, step_fraction: float = 0.5, min_depth: float = 0.1, max_depth: float = 10.0):
    """`mi_tsdf_raycast`: volume (B, NZ, NY, NX, 2) seen from the world-to-camera poses r (B, 3, 3), t (B, 3) through the camera
    of k_inv (3, 3) at size = (H, W) -> (vertex, normal), each (B, H, W, 4) float32 in the camera frame, in `surfel_maps`'
    layout: what `icp_linearise` / `icp_refine` take as maps1."""
    ptr, dims = _tsdf_volume(volume, "tsdf_raycast")
    b = dims[0]
    h, w = (int(x) for x in size)
    if h < 3 or w < 3:
        raise RuntimeError(f"tsdf_raycast: size must be (H, W) with H, W >= 3, got {size}")
    rr, tt = r.float().contiguous(), t.float().contiguous()
    if tuple(rr.shape) != (b, 3, 3) or tuple(tt.shape) != (b, 3):
        raise RuntimeError(f"tsdf_raycast: the pose must be ({b}, 3, 3) and ({b}, 3), got {tuple(r.shape)} and {tuple(t.shape)}")
    ki = k_inv.float().contiguous()
    if tuple(ki.shape) != (3, 3):
        raise RuntimeError(f"tsdf_raycast: K_inv must be (3, 3), got {tuple(k_inv.shape)}")
    grid = _tsdf_grid(origin, voxel_size, truncation, "tsdf_raycast")
    vertex = torch.empty((b, h, w, 4), dtype=F32, device=volume.device)
    normal = torch.empty((b, h, w, 4), dtype=F32, device=volume.device)
    N.call("mi_tsdf_raycast", ptr, *dims, *grid, float(step_fraction), N.dev(rr, F32, "r"), N.dev(tt, F32, "t"), h, w,
           N.dev(ki, F32, "K_inv"), float(min_depth), float(max_depth), vertex.data_ptr(), normal.data_ptr(), N.stream_ptr())
    return vertex, normal


def pose_compose(ra: torch.Tensor, ta: torch.Tensor, rb: torch.Tensor, tb: torch.Tensor):
    """`mi_pose_compose`: (ra, ta) o (rb, tb) = (ra rb, ra tb + ta) per item, (B, 3, 3) and (B, 3) float32, formed in float64 and
    rounded once."""
    if not ra.is_cuda:
        raise RuntimeError(f"pose_compose: the poses must live on the GPU (got device {ra.device}); this package has no CPU path")
    a, at, c, ct = (x.float().contiguous() for x in (ra, ta, rb, tb))
    b = int(a.shape[0]) if a.dim() == 3 else 0
    if b < 1 or any(tuple(x.shape) != (b, 3, 3) for x in (a, c)) or any(tuple(x.shape) != (b, 3) for x in (at, ct)):
        raise RuntimeError(f"pose_compose: the poses must be (B, 3, 3) and (B, 3), got {tuple(ra.shape)}, {tuple(ta.shape)}, "
                           f"{tuple(rb.shape)}, {tuple(tb.shape)}")
    r = torch.empty((b, 3, 3), dtype=F32, device=a.device)
    t = torch.empty((b, 3), dtype=F32, device=a.device)
    N.call("mi_pose_compose", N.dev(a, F32, "ra"), N.dev(at, F32, "ta"), N.dev(c, F32, "rb"), N.dev(ct, F32, "tb"), b,
           r.data_ptr(), t.data_ptr(), N.stream_ptr())
    return r, t


# ---- K20 TSDF surface extraction (include/mi355x_match.h, "TSDF surface extraction") --------------------------------------------

def _tsdf_surface_call(volume: torch.Tensor, origin, voxel_size: float, min_weight: float, max_vertices: int, max_triangles: int,
                       normals: bool, triangles: bool, what: str):
    ptr, dims = _tsdf_volume(volume, what)
    o = tuple(float(x) for x in origin)
    if len(o) != 3 or not voxel_size > 0 or not min_weight > 0:
        raise RuntimeError(f"{what}: need an origin of 3 values, voxel_size > 0 and min_weight > 0, got {origin}, {voxel_size}, "
                           f"{min_weight}")
    mv, mt = int(max_vertices), int(max_triangles)
    if mv < 0 or mt < 0:
        raise RuntimeError(f"{what}: the capacities must not be negative, got {max_vertices} and {max_triangles}")
    b, dev = dims[0], volume.device
    work, wbytes = _workspace("mi_tsdf_surface_workspace_bytes", *dims, device=dev,
                              refusal=f"{what}: unsupported volume {tuple(volume.shape)}: vertex ids need 12 * NZ * NY * NX < 2^31")
    counts = torch.empty((b, 2), dtype=torch.int32, device=dev)
    vertex = torch.empty((b, mv, 4), dtype=F32, device=dev) if mv else None
    normal = torch.empty((b, mv, 4), dtype=F32, device=dev) if mv and normals else None
    tris = torch.empty((b, mt, 3), dtype=torch.int32, device=dev) if mt and triangles else None
    N.call("mi_tsdf_surface", ptr, *dims, *o, float(voxel_size), float(min_weight), mv, mt if tris is not None else 0,
           vertex.data_ptr() if vertex is not None else None, normal.data_ptr() if normal is not None else None,
           tris.data_ptr() if tris is not None else None, counts.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return vertex, normal, tris, counts


def tsdf_surface(volume: torch.Tensor, origin, voxel_size: float, max_vertices: int, max_triangles: int, min_weight: float = 1.0,
                 normals: bool = True, triangles: bool = True):
    """`mi_tsdf_surface`: the zero level set of volume (B, NZ, NY, NX, 2) by marching tetrahedra -> (vertex (B, max_vertices, 4)
    float32 in the world frame, normal likewise or None, triangles (B, max_triangles, 3) int32 or None, counts (B, 2) int32 =
    the true (vertices, triangles) of every volume, which may exceed the capacities).  Rows past the counts are zeros and
    (-1, -1, -1).  triangles=False forms no triangle (a point cloud); the counts still hold both totals.  No synchronisation."""
    vertex, normal, tris, counts = _tsdf_surface_call(volume, origin, voxel_size, min_weight, max_vertices, max_triangles, normals,
                                                      triangles, "tsdf_surface")
    b, dev = int(volume.shape[0]), volume.device
    if vertex is None:                                           # a capacity of 0: empty arrays, nothing to write
        vertex = torch.empty((b, 0, 4), dtype=F32, device=dev)
        normal = torch.empty((b, 0, 4), dtype=F32, device=dev) if normals else None
    if tris is None and triangles:
        tris = torch.empty((b, 0, 3), dtype=torch.int32, device=dev)
    return vertex, normal, tris, counts


def tsdf_surface_counts(volume: torch.Tensor, min_weight: float = 1.0) -> torch.Tensor:
    """The sizing pass of `mi_tsdf_surface`: (B, 2) int32 on the device, the (vertices, triangles) a full call would produce.
    The counts depend on neither the origin nor the voxel size."""
    return _tsdf_surface_call(volume, (0.0, 0.0, 0.0), 1.0, min_weight, 0, 0, False, False, "tsdf_surface_counts")[3]


# ---- K22 TSDF intensity (include/mi355x_match.h, "TSDF intensity") ---------------------------------------------------------------

def _tsdf_intensity(intensity: torch.Tensor, dims, what: str) -> int:
    if not intensity.is_cuda:
        raise RuntimeError(f"{what}: the intensity volume must live on the GPU (got device {intensity.device}); this package has "
                           f"no CPU path")
    if intensity.dtype != F32 or tuple(intensity.shape) != (*dims, 2):
        raise RuntimeError(f"{what}: the intensity volume must be float32 {(*dims, 2)}, the volume's shape, got {intensity.dtype} "
                           f"{tuple(intensity.shape)}")
    return N.dev(intensity, F32, "intensity volume")


def tsdf_gray_reset(intensity: torch.Tensor) -> torch.Tensor:
    """`mi_tsdf_gray_reset`: (gray, gweight) = (0, 0) into every record of intensity (B, NZ, NY, NX, 2) float32, in place."""
    ptr, dims = _tsdf_volume(intensity, "tsdf_gray_reset")
    N.call("mi_tsdf_gray_reset", ptr, *dims, N.stream_ptr())
    return intensity


def tsdf_integrate_gray(volume: torch.Tensor, intensity: torch.Tensor, depth: torch.Tensor, gray: torch.Tensor, r: torch.Tensor,
                        t: torch.Tensor, camera, origin, voxel_size: float, truncation: float, max_weight: float = 64.0,
                        z_scale: float = 1.0, min_depth: float = 0.1, max_depth: float = 10.0,
                        active: torch.Tensor | None = None):
    """`mi_tsdf_integrate_gray`: `tsdf_integrate` with gray (B, F, H, W), float32 or uint8, beside depth (B, F, H, W): volume gets
    `tsdf_integrate`'s bits and intensity (B, NZ, NY, NX, 2), records of (gray, gweight), the running mean of the gray value at
    every voxel inside the truncation band of a seen surface, both in place in one pass -> (volume, intensity)."""
    ptr, dims = _tsdf_volume(volume, "tsdf_integrate_gray")
    iptr = _tsdf_intensity(intensity, dims, "tsdf_integrate_gray")
    if not depth.is_cuda or not gray.is_cuda:
        dev = depth.device if not depth.is_cuda else gray.device
        raise RuntimeError(f"tsdf_integrate_gray: depth and gray must live on the GPU (got device {dev}); this package has no CPU "
                           f"path")
    if depth.dtype not in (F32, U16):
        raise RuntimeError(f"tsdf_integrate_gray: depth must be float32 or uint16, got {depth.dtype}")
    if gray.dtype not in (F32, U8):
        raise RuntimeError(f"tsdf_integrate_gray: gray must be float32 or uint8, got {gray.dtype}")
    b = dims[0]
    if depth.dim() != 4 or depth.shape[0] != b or depth.shape[1] < 1 or depth.shape[2] < 3 or depth.shape[3] < 3:
        raise RuntimeError(f"tsdf_integrate_gray: depth must be ({b}, F, H, W) with F >= 1 and H, W >= 3, got {tuple(depth.shape)}")
    if gray.shape != depth.shape:
        raise RuntimeError(f"tsdf_integrate_gray: gray must have depth's shape {tuple(depth.shape)}, got {tuple(gray.shape)}")
    d, g = depth.contiguous(), gray.contiguous()
    f, h, w = (int(x) for x in d.shape[1:])
    rr, tt = r.float().contiguous(), t.float().contiguous()
    if tuple(rr.shape) != (b, f, 3, 3) or tuple(tt.shape) != (b, f, 3):
        raise RuntimeError(f"tsdf_integrate_gray: the poses must be ({b}, {f}, 3, 3) and ({b}, {f}, 3), got {tuple(r.shape)} and "
                           f"{tuple(t.shape)}")
    act = None
    if active is not None:
        if active.dtype not in (torch.bool, U8) or tuple(active.shape) != (b, f):
            raise RuntimeError(f"tsdf_integrate_gray: active must be bool or uint8 ({b}, {f}), got {active.dtype} "
                               f"{tuple(active.shape)}")
        act = active.contiguous().view(U8)
    grid = _tsdf_grid(origin, voxel_size, truncation, "tsdf_integrate_gray")
    fx, fy, cx, cy = (float(x) for x in camera)
    N.call("mi_tsdf_integrate_gray", ptr, iptr, *dims, *grid, float(max_weight), d.data_ptr(), int(d.dtype == U16), g.data_ptr(),
           int(g.dtype == U8), f, h, w, fx, fy, cx, cy, float(z_scale), float(min_depth), float(max_depth), N.dev(rr, F32, "r"),
           N.dev(tt, F32, "t"), N.opt(act, U8, "active"), N.stream_ptr())
    return volume, intensity


def tsdf_sample_gray(intensity: torch.Tensor, points: torch.Tensor, origin, voxel_size: float, r: torch.Tensor | None = None,
                     t: torch.Tensor | None = None) -> torch.Tensor:
    """`mi_tsdf_sample_gray`: the intensity volume (B, NZ, NY, NX, 2) gathered at points (B, ..., 4) float32 records (x, y, z, f)
    -> records of the same shape in `intensity_maps`' layout, (I, 0, 0, 1) or zeros: the weight-normalised trilinear blend
    over the observed corners of the point's cell.  With a world-to-camera pose r (B, 3, 3), t (B, 3) the points are in the
    camera's frame (a raycast's vertex map gives the model's intensity map, `rgbd_refine`'s maps1[2]); without, world points
    (the vertices of `tsdf_surface`)."""
    ptr, dims = _tsdf_volume(intensity, "tsdf_sample_gray")
    b = dims[0]
    if not points.is_cuda:
        raise RuntimeError(f"tsdf_sample_gray: the points must live on the GPU (got device {points.device}); this package has no "
                           f"CPU path")
    if points.dtype != F32 or points.dim() < 3 or points.shape[0] != b or points.shape[-1] != 4:
        raise RuntimeError(f"tsdf_sample_gray: the points must be float32 ({b}, N, 4) or ({b}, H, W, 4), got {points.dtype} "
                           f"{tuple(points.shape)}")
    if (r is None) != (t is None):
        raise RuntimeError("tsdf_sample_gray: give both r and t, or neither")
    o = tuple(float(x) for x in origin)
    if len(o) != 3 or not voxel_size > 0:
        raise RuntimeError(f"tsdf_sample_gray: need an origin of 3 values and voxel_size > 0, got {origin}, {voxel_size}")
    pts = points.contiguous()
    n = pts.numel() // (4 * b)
    rp = tp = None
    if r is not None:
        rr, tt = r.float().contiguous(), t.float().contiguous()
        if tuple(rr.shape) != (b, 3, 3) or tuple(tt.shape) != (b, 3):
            raise RuntimeError(f"tsdf_sample_gray: the pose must be ({b}, 3, 3) and ({b}, 3), got {tuple(r.shape)} and "
                               f"{tuple(t.shape)}")
        rp, tp = N.dev(rr, F32, "r"), N.dev(tt, F32, "t")
    out = torch.empty_like(pts)
    if n == 0:                                                   # no point (a capacity of 0): nothing to write
        return out
    N.call("mi_tsdf_sample_gray", ptr, *dims, *o, float(voxel_size), N.dev(pts, F32, "points"), n, rp, tp, out.data_ptr(),
           N.stream_ptr())
    return out


# ---- K16 frame ingest (sample/visual_odometry.py:65-92 load_image_from_array) ------------------------------------------

INGEST_MAX_DIM = N.MI_INGEST_MAX_DIM
_CHANNEL_ORDERS = {"bgr": N.MI_INGEST_BGR, "rgb": N.MI_INGEST_RGB}


def ingest_frames(frames: torch.Tensor, height: int, width: int, *, channel_order: str = "bgr",
                  out_dtype: torch.dtype = U8) -> torch.Tensor:
    """Colour camera frames -> gray model frames in one launch (`mi_ingest_frames`): what the reference's hosts do on the
    CPU with cv2.cvtColor(BGR2GRAY) + cv2.resize(INTER_LINEAR) + astype(float32), in the integer arithmetic the header
    states.  frames: uint8 (B, Hs, Ws, C) or (Hs, Ws, C) with C in {1, 3, 4} (HWC; the 4th channel is ignored); a view
    whose pixels are dense and whose rows / frames are pitched (a crop, a padded camera buffer) goes in by its strides
    without a copy, anything else is made contiguous first.  -> (B, 1, height, width) of out_dtype (torch.uint8 for the
    `_u8` entry points, torch.float32 holding the same values for the others)."""
    if channel_order not in _CHANNEL_ORDERS:
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    if out_dtype not in (U8, F32):
        raise ValueError(f"out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    if frames.dim() != 4 or frames.shape[-1] not in (1, 3, 4):
        raise RuntimeError(f"frames must have shape (B, Hs, Ws, C) or (Hs, Ws, C) with C in (1, 3, 4), got {tuple(frames.shape)}")
    if not frames.is_cuda:
        raise RuntimeError(f"frames must live on the GPU (got device {frames.device}); this package has no CPU path")
    if frames.dtype != U8:
        raise RuntimeError(f"frames must be torch.uint8, got {frames.dtype}")
    b, hs, ws, c = frames.shape
    height, width = int(height), int(width)
    if min(b, hs, ws, height, width) < 1 or max(b, hs, ws, height, width) > INGEST_MAX_DIM:
        raise RuntimeError(f"frame extents must be in 1 .. {INGEST_MAX_DIM}, got {tuple(frames.shape)} -> ({height}, {width})")
    pitched = (frames.stride(3) == 1 and frames.stride(2) == c and frames.stride(1) >= ws * c
               and frames.stride(0) >= hs * frames.stride(1))
    if not pitched:
        frames = frames.contiguous()
    out = torch.empty((b, 1, height, width), dtype=out_dtype, device=frames.device)
    N.call("mi_ingest_frames", frames.data_ptr(), b, hs, ws, c, frames.stride(1), frames.stride(0),
           _CHANNEL_ORDERS[channel_order], out.data_ptr(), int(out_dtype == F32), height, width, N.stream_ptr())
    return out


# ---- K32 feature tracking (include/mi355x_match_flow.h) -----------------------------------------------------------------------

FLOW_MAX_LEVELS, FLOW_MAX_RADIUS, FLOW_MAX_K = (N.FLOW_CONSTANTS[k] for k in ("MI_FLOW_MAX_LEVELS", "MI_FLOW_MAX_RADIUS", "MI_FLOW_MAX_K"))
FLOW_MAX_ITERATIONS, FLOW_MAX_CELLS = N.FLOW_CONSTANTS["MI_FLOW_MAX_ITERATIONS"], N.FLOW_CONSTANTS["MI_FLOW_MAX_CELLS"]
FLOW_OK, FLOW_PADDING, FLOW_FLAT, FLOW_LEFT = (N.FLOW_CONSTANTS[k] for k in ("MI_FLOW_OK", "MI_FLOW_PADDING", "MI_FLOW_FLAT", "MI_FLOW_LEFT"))


class FlowPyramid:
    """The pyramid block of `mi_flow_pyramid`: `data` (the library's layout, float32 behind an int64 workspace tensor) and
    the request it was built for.  level(l) is a (B, h_l, w_l) float32 view of it."""

    def __init__(self, data: torch.Tensor, batch: int, h: int, w: int, levels: int) -> None:
        self.data, self.batch, self.h, self.w, self.levels = data, batch, h, w, levels

    def level(self, l: int) -> torch.Tensor:
        if not 0 <= l < self.levels:
            raise IndexError(f"level {l} of a {self.levels}-level pyramid")
        off, h, w = 0, self.h, self.w
        for _ in range(l):
            off = (off + self.batch * h * w * 4 + 255) // 256 * 256
            h, w = (h + 1) // 2, (w + 1) // 2
        return self.data.view(F32)[off // 4: off // 4 + self.batch * h * w].view(self.batch, h, w)


def flow_pyramid(frames: torch.Tensor, levels: int) -> FlowPyramid:
    """`mi_flow_pyramid`: gray frames (B, H, W) or (B, 1, H, W), uint8 or float32 (the outputs of ingest_frames), to the
    `levels`-level cv2.pyrDown pyramid the tracker reads."""
    if not frames.is_cuda:
        raise RuntimeError(f"flow_pyramid: frames must live on the GPU (got device {frames.device}); this package has no CPU path")
    if frames.dtype not in (U8, F32):
        raise RuntimeError(f"flow_pyramid: frames must be uint8 or float32, got {frames.dtype}")
    if frames.dim() == 4 and frames.shape[1] == 1:
        frames = frames[:, 0]
    if frames.dim() != 3 or frames.numel() == 0:
        raise RuntimeError(f"flow_pyramid: frames must be (B, H, W) or (B, 1, H, W), got {tuple(frames.shape)}")
    src = frames.contiguous()
    b, h, w = (int(v) for v in src.shape)
    data, nbytes = _workspace("mi_flow_pyramid_bytes", b, h, w, int(levels), device=src.device,
                              refusal=f"flow_pyramid: unsupported request (batch {b}, {h} x {w}, {levels} levels: 1 .. {FLOW_MAX_LEVELS} "
                                      "levels, the top level at least 5 x 5)")
    N.call("mi_flow_pyramid", src.data_ptr(), int(src.dtype == U8), b, h, w, int(levels), data.data_ptr(), nbytes, N.stream_ptr())
    return FlowPyramid(data, b, h, w, int(levels))


def _flow_keypoints(t: torch.Tensor, what: str, batch: int | None = None):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU (got device {t.device}); this package has no CPU path")
    q = t.float().contiguous()
    if q.dim() != 3 or q.shape[2] != 2 or (batch is not None and q.shape[0] != batch) or q.shape[1] < 1:
        raise RuntimeError(f"{what} must be (B, K, 2) (y, x) pixel coordinates, got {tuple(t.shape)}")
    return q


def flow_track(pyr1: FlowPyramid, pyr2: FlowPyramid, keypoints1: torch.Tensor, guess: torch.Tensor | None = None, radius: int = 7,
               max_iterations: int = 30, epsilon: float = 0.01, min_eigen: float = 1e-3):
    """`mi_flow_track`: keypoints1 (B, K, 2) (y, x) of frame 1 followed into frame 2 by pyramidal Lucas-Kanade ->
    (keypoints2 (B, K, 2), status (B, K) bool, code (B, K) uint8 FLOW_OK / FLOW_PADDING / FLOW_FLAT / FLOW_LEFT, residual
    (B, K) mean |e| at level 0, iterations (B, K) int32).  guess (B, K, 2): a predicted displacement (dy, dx) or None."""
    if (pyr1.batch, pyr1.h, pyr1.w, pyr1.levels) != (pyr2.batch, pyr2.h, pyr2.w, pyr2.levels):
        raise RuntimeError("flow_track: the two pyramids differ in batch, size or levels")
    kp = _flow_keypoints(keypoints1, "flow_track: keypoints1", pyr1.batch)
    g = None if guess is None else _flow_keypoints(guess, "flow_track: guess", pyr1.batch)
    if g is not None and g.shape != kp.shape:
        raise RuntimeError(f"flow_track: guess must be {tuple(kp.shape)}, got {tuple(g.shape)}")
    b, k, dev = pyr1.batch, int(kp.shape[1]), kp.device
    kp2 = torch.empty((b, k, 2), dtype=F32, device=dev)
    status, code = torch.empty((b, k), dtype=U8, device=dev), torch.empty((b, k), dtype=U8, device=dev)
    residual = torch.empty((b, k), dtype=F32, device=dev)
    iterations = torch.empty((b, k), dtype=I32, device=dev)
    N.call("mi_flow_track", pyr1.data.data_ptr(), pyr2.data.data_ptr(), kp.data_ptr(), N.opt(g, F32, "guess"), b, pyr1.h, pyr1.w,
           pyr1.levels, k, int(radius), int(max_iterations), float(epsilon), float(min_eigen), kp2.data_ptr(), status.data_ptr(),
           code.data_ptr(), residual.data_ptr(), iterations.data_ptr(), N.stream_ptr())
    return kp2, status.view(torch.bool), code, residual, iterations


def flow_check(keypoints1: torch.Tensor, keypoints_back: torch.Tensor, status_fwd: torch.Tensor, status_bwd: torch.Tensor,
               max_distance: float):
    """`mi_flow_check`: the forward-backward test -> (status (B, K) bool, fb_distance (B, K) float32, +inf where either
    track was lost)."""
    kp = _flow_keypoints(keypoints1, "flow_check: keypoints1")
    back = _flow_keypoints(keypoints_back, "flow_check: keypoints_back", int(kp.shape[0]))
    sf, sb = _validity_bytes(status_fwd), _validity_bytes(status_bwd)
    b, k = int(kp.shape[0]), int(kp.shape[1])
    if back.shape != kp.shape or tuple(sf.shape) != (b, k) or tuple(sb.shape) != (b, k):
        raise RuntimeError(f"flow_check: keypoints must both be ({b}, {k}, 2) and the statuses ({b}, {k})")
    status = torch.empty((b, k), dtype=U8, device=kp.device)
    fb = torch.empty((b, k), dtype=F32, device=kp.device)
    N.call("mi_flow_check", kp.data_ptr(), back.data_ptr(), N.dev(sf, U8, "status_fwd"), N.dev(sb, U8, "status_bwd"), b, k,
           float(max_distance), status.data_ptr(), fb.data_ptr(), N.stream_ptr())
    return status.view(torch.bool), fb


def flow_replenish(keypoints: torch.Tensor, status: torch.Tensor, candidates: torch.Tensor, cand_count: torch.Tensor | None, h: int,
                   w: int, cell: int = 16):
    """`mi_flow_replenish`: lost slots (status 0) of keypoints (B, K, 2) refilled from score-descending candidates
    (B, C, 2), the first cand_count[b] (B,) int32 of them real (None: all), one per cell of cell x cell pixels that holds no
    live keypoint -> (keypoints_out (B, K, 2), is_new (B, K) bool, counts (B, 3) int32: live, accepted, filled)."""
    kp = _flow_keypoints(keypoints, "flow_replenish: keypoints")
    b, k = int(kp.shape[0]), int(kp.shape[1])
    cand = _flow_keypoints(candidates, "flow_replenish: candidates", b)
    st = _validity_bytes(status)
    if tuple(st.shape) != (b, k):
        raise RuntimeError(f"flow_replenish: status must be ({b}, {k}), got {tuple(st.shape)}")
    n_cand = int(cand.shape[1])
    if cand_count is None:
        cand_count = torch.full((b,), n_cand, dtype=I32, device=kp.device)
    cc = cand_count.to(I32).contiguous()
    if tuple(cc.shape) != (b,):
        raise RuntimeError(f"flow_replenish: cand_count must be ({b},), got {tuple(cc.shape)}")
    out = torch.empty((b, k, 2), dtype=F32, device=kp.device)
    is_new = torch.empty((b, k), dtype=U8, device=kp.device)
    counts = torch.empty((b, 3), dtype=I32, device=kp.device)
    N.call("mi_flow_replenish", kp.data_ptr(), N.dev(st, U8, "status"), cand.data_ptr(), N.dev(cc, I32, "cand_count"), b, k, n_cand,
           int(h), int(w), int(cell), out.data_ptr(), is_new.data_ptr(), counts.data_ptr(), N.stream_ptr())
    return out, is_new.view(torch.bool), counts


# ---- K33 stereo depth (include/mi355x_match_stereo.h) -------------------------------------------------------------------------

STEREO_OK, STEREO_NOT_UNIQUE, STEREO_LR = (N.STEREO_CONSTANTS[k] for k in ("MI_STEREO_OK", "MI_STEREO_NOT_UNIQUE", "MI_STEREO_LR"))
STEREO_DISPARITIES = (64, 128, 256)
I16, U16, I64 = torch.int16, torch.uint16, torch.int64


def _stereo_frames(t: torch.Tensor, what: str, dtypes, shape=None):
    """(B, H, W) or (B, 1, H, W) on the GPU, of one of `dtypes`, contiguous; `shape`: the (B, H, W) it must have"""
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU (got device {t.device}); this package has no CPU path")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.numel() == 0 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{what} must be {'(B, H, W) or (B, 1, H, W)' if shape is None else tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def stereo_census(gray: torch.Tensor) -> torch.Tensor:
    """`mi_stereo_census`: gray frames (B, H, W) or (B, 1, H, W), uint8 or float32 (the outputs of ingest_frames) -> the 9 x 7
    census words (B, H, W), 62 bits each in an int64 tensor (torch has no arithmetic on uint64; the bits are the library's)."""
    g = _stereo_frames(gray, "stereo_census: gray", (U8, F32))
    b, h, w = (int(v) for v in g.shape)
    census = torch.empty((b, h, w), dtype=I64, device=g.device)
    N.call("mi_stereo_census", g.data_ptr(), int(g.dtype == U8), b, h, w, census.data_ptr(), N.stream_ptr())
    return census


def stereo_aggregate(census_left: torch.Tensor, census_right: torch.Tensor, max_disparity: int = 128, paths: int = 8, p1: int = 10,
                     p2: int = 120) -> torch.Tensor:
    """`mi_stereo_aggregate`: the census words of a rectified pair -> the semi-global sums S (B, H, W, max_disparity) uint16
    over `paths` (4 or 8) directions with the penalties 0 <= p1 <= p2 <= 255.  max_disparity is 64, 128 or 256."""
    cl = _stereo_frames(census_left, "stereo_aggregate: census_left", (I64,))
    cr = _stereo_frames(census_right, "stereo_aggregate: census_right", (I64,), cl.shape)
    b, h, w = (int(v) for v in cl.shape)
    d = int(max_disparity)
    volume = torch.empty((b, h, w, d if d > 0 else 1), dtype=U16, device=cl.device)
    work, wbytes = _workspace("mi_stereo_workspace_bytes", b, h, w, d, int(paths), device=cl.device)
    N.call("mi_stereo_aggregate", cl.data_ptr(), cr.data_ptr(), b, h, w, d, int(paths), int(p1), int(p2), volume.data_ptr(),
           work.data_ptr() if wbytes else None, wbytes, N.stream_ptr())
    return volume


def stereo_select(volume: torch.Tensor, uniqueness: int = 10, lr_max_diff: int = 1, want_right: bool = True):
    """`mi_stereo_select`: S (B, H, W, D) uint16 -> (disparity (B, H, W) float32, -1 on a rejected pixel; disparity_right
    (B, H, W) int16, or None with want_right=False, which needs lr_max_diff < 0; code (B, H, W) uint8: STEREO_OK,
    STEREO_NOT_UNIQUE, STEREO_LR)."""
    if not want_right and lr_max_diff >= 0:
        raise ValueError("stereo_select: the left-right test (lr_max_diff >= 0) needs the right view's disparities")
    if not volume.is_cuda:
        raise RuntimeError(f"stereo_select: volume must live on the GPU (got device {volume.device}); this package has no CPU path")
    if volume.dtype != U16 or volume.dim() != 4 or volume.numel() == 0:
        raise RuntimeError(f"stereo_select: volume must be (B, H, W, D) uint16, got {tuple(volume.shape)} {volume.dtype}")
    v = volume.contiguous()
    b, h, w, d = (int(x) for x in v.shape)
    disparity = torch.empty((b, h, w), dtype=F32, device=v.device)
    right = torch.empty((b, h, w), dtype=I16, device=v.device) if want_right else None
    code = torch.empty((b, h, w), dtype=U8, device=v.device)
    N.call("mi_stereo_select", v.data_ptr(), b, h, w, d, int(uniqueness), int(lr_max_diff), disparity.data_ptr(),
           None if right is None else right.data_ptr(), code.data_ptr(), N.stream_ptr())
    return disparity, right, code


def stereo_depth(disparity: torch.Tensor, fb: float, min_disparity: float = 0.5) -> torch.Tensor:
    """`mi_stereo_depth`: disparity (B, H, W) or (B, 1, H, W) float32 -> depth of the same shape, fb / disparity where
    disparity >= min_disparity and 0 elsewhere; fb = fx * baseline in the unit the depth is wanted in."""
    d = _stereo_frames(disparity, "stereo_depth: disparity", (F32,))
    b, h, w = (int(v) for v in d.shape)
    depth = torch.empty((b, h, w), dtype=F32, device=d.device)
    N.call("mi_stereo_depth", d.data_ptr(), b, h, w, float(fb), float(min_disparity), depth.data_ptr(), N.stream_ptr())
    return depth.view(disparity.shape)


# ---- K34 camera rectification (include/mi355x_match_rectify.h) ----------------------------------------------------------------

RECTIFY_PINHOLE, RECTIFY_FISHEYE = N.RECTIFY_CONSTANTS["MI_RECTIFY_PINHOLE"], N.RECTIFY_CONSTANTS["MI_RECTIFY_FISHEYE"]
RECTIFY_NEAREST, RECTIFY_LINEAR = N.RECTIFY_CONSTANTS["MI_RECTIFY_NEAREST"], N.RECTIFY_CONSTANTS["MI_RECTIFY_LINEAR"]
RECTIFY_OUTSIDE, RECTIFY_SUBPIXEL_BITS = N.RECTIFY_CONSTANTS["MI_RECTIFY_OUTSIDE"], N.RECTIFY_CONSTANTS["MI_RECTIFY_SUBPIXEL_BITS"]
RECTIFY_MAX_ITERATIONS, RECTIFY_MAX_DIM = N.RECTIFY_CONSTANTS["MI_RECTIFY_MAX_ITERATIONS"], N.RECTIFY_CONSTANTS["MI_RECTIFY_MAX_DIM"]
RECTIFY_MODELS = {"pinhole": RECTIFY_PINHOLE, "fisheye": RECTIFY_FISHEYE}
_RECTIFY_TYPES = {U8: N.RECTIFY_CONSTANTS["MI_RECTIFY_U8"], U16: N.RECTIFY_CONSTANTS["MI_RECTIFY_U16"], F32: N.RECTIFY_CONSTANTS["MI_RECTIFY_F32"]}


def _rectify_doubles(values, count: int, what: str):
    """a host array of `count` doubles for the C ABI from a tensor, an array or a nested list; None stays None (NULL)"""
    if values is None:
        return None
    flat = torch.as_tensor(values, dtype=torch.float64, device="cpu").reshape(-1)
    if flat.numel() != count:
        raise ValueError(f"{what} must have {count} elements, got {flat.numel()}")
    return (N.c_double * count)(*flat.tolist())


def rectify_model(model) -> int:
    """"pinhole" / "fisheye" or the constant itself -> RECTIFY_PINHOLE / RECTIFY_FISHEYE"""
    if model in RECTIFY_MODELS:
        return RECTIFY_MODELS[model]
    if model in RECTIFY_MODELS.values() and not isinstance(model, str):
        return int(model)
    raise ValueError(f"model must be 'pinhole' or 'fisheye', got {model!r}")


def rectify_coeffs(dist_coeffs, model: int):
    """distortion coefficients as the entries take them: MI_RECTIFY_COEFFS doubles.  Pinhole: OpenCV's 4, 5 or 8
    (k1 k2 p1 p2 [k3 [k4 k5 k6]]), None for none; fisheye: k1 .. k4.  The missing ones are 0."""
    flat = [] if dist_coeffs is None else torch.as_tensor(dist_coeffs, dtype=torch.float64, device="cpu").reshape(-1).tolist()
    legal = (0, 4, 5, 8) if model == RECTIFY_PINHOLE else (0, 4, 8)
    if len(flat) not in legal:
        raise ValueError(f"dist_coeffs must have one of {legal} elements for this model, got {len(flat)}")
    return _rectify_doubles(flat + [0.0] * (8 - len(flat)), 8, "dist_coeffs")


def rectify_map(camera_matrix, dist_coeffs, size, new_camera_matrix, out_size=None, rotation=None, model="pinhole", device="cuda",
                want_mask: bool = True):
    """`mi_rectify_map`: the sampling map of one camera, cv2.initUndistortRectifyMap's counterpart.  size = (height, width) of the
    source frames, out_size that of the rectified ones (default: size); the cameras, coefficients and rotation are host values
    (tensors, arrays or lists).  -> (map (h, w, 2) int32: source x, y in 1/32 pixel or RECTIFY_OUTSIDE; mask (h, w) uint8, 1
    where every tap lies inside the source, or None with want_mask=False), on `device`."""
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"rectify_map: the map must live on the GPU (got device {device}); this package has no CPU path")
    m = rectify_model(model)
    (sh, sw), (h, w) = (int(v) for v in size), (int(v) for v in (out_size or size))
    out = torch.empty((max(h, 1), max(w, 1), 2), dtype=torch.int32, device=device)
    mask = torch.empty((max(h, 1), max(w, 1)), dtype=U8, device=device) if want_mask else None
    N.call("mi_rectify_map", m, _rectify_doubles(camera_matrix, 9, "camera_matrix"), rectify_coeffs(dist_coeffs, m),
           _rectify_doubles(rotation, 9, "rotation"), _rectify_doubles(new_camera_matrix, 9, "new_camera_matrix"), sh, sw, h, w,
           out.data_ptr(), None if mask is None else mask.data_ptr(), N.stream_ptr())
    return out, mask


def rectify_remap(frames: torch.Tensor, map: torch.Tensor, interpolation: int | None = None, border_value: float = 0.0) -> torch.Tensor:
    """`mi_rectify_remap`: frames (B, H, W) or (B, 1, H, W), uint8, uint16 or float32, through one map (h, w, 2) int32 of
    rectify_map -> (B, h, w) or (B, 1, h, w) of the same type, cv2.remap for a batch.  interpolation: RECTIFY_LINEAR (the
    default for uint8 and float32) or RECTIFY_NEAREST (the default for uint16, which has no LINEAR: depth is not blended); a
    tap outside the source reads border_value."""
    src = _stereo_frames(frames, "rectify_remap: frames", (U8, U16, F32))
    if not map.is_cuda:
        raise RuntimeError(f"rectify_remap: map must live on the GPU (got device {map.device}); this package has no CPU path")
    if map.dtype != torch.int32 or map.dim() != 3 or map.shape[2] != 2 or map.numel() == 0:
        raise RuntimeError(f"rectify_remap: map must be (h, w, 2) int32, got {tuple(map.shape)} {map.dtype}")
    mp = map.contiguous()
    b, sh, sw = (int(v) for v in src.shape)
    h, w = int(mp.shape[0]), int(mp.shape[1])
    if interpolation is None:
        interpolation = RECTIFY_NEAREST if src.dtype == U16 else RECTIFY_LINEAR
    dst = torch.empty((b, h, w), dtype=src.dtype, device=src.device)
    N.call("mi_rectify_remap", src.data_ptr(), _RECTIFY_TYPES[src.dtype], b, sh, sw, mp.data_ptr(), h, w, int(interpolation),
           float(border_value), dst.data_ptr(), N.stream_ptr())
    return dst.view(b, 1, h, w) if frames.dim() == 4 else dst


def rectify_points(pts: torch.Tensor, camera_matrix, dist_coeffs, rotation=None, new_camera_matrix=None, model="pinhole",
                   iterations: int = 10, max_residual_px: float = 0.5):
    """`mi_rectify_points`: raw pixel coordinates (B, n, 2) float32 in (x, y) order -> (out (B, n, 2) float32, ok (B, n) bool),
    cv2.undistortPoints for a batch.  out is normalised (x, y) after `rotation` when new_camera_matrix is None -- what the pose
    estimators take --, else pixels of that camera; (0, 0) where ok is False (no undistorted point reproduces the input within
    max_residual_px, a value is not finite, the point is behind the rectified camera, or beyond the fisheye model's limit)."""
    if not pts.is_cuda:
        raise RuntimeError(f"rectify_points: pts must live on the GPU (got device {pts.device}); this package has no CPU path")
    if pts.dtype != F32 or pts.dim() != 3 or pts.shape[2] != 2 or pts.numel() == 0:
        raise RuntimeError(f"rectify_points: pts must be (B, n, 2) float32, got {tuple(pts.shape)} {pts.dtype}")
    m = rectify_model(model)
    p = pts.contiguous()
    b, n = int(p.shape[0]), int(p.shape[1])
    out = torch.empty((b, n, 2), dtype=F32, device=p.device)
    ok = torch.empty((b, n), dtype=U8, device=p.device)
    N.call("mi_rectify_points", p.data_ptr(), b, n, m, _rectify_doubles(camera_matrix, 9, "camera_matrix"), rectify_coeffs(dist_coeffs, m),
           _rectify_doubles(rotation, 9, "rotation"), _rectify_doubles(new_camera_matrix, 9, "new_camera_matrix"), int(iterations),
           float(max_residual_px), out.data_ptr(), ok.data_ptr(), N.stream_ptr())
    return out, ok.view(torch.bool)


def rectify_stereo_rig(k1, k2, rotation, translation, size):
    """`mi_rectify_stereo_rig` (host only, no GPU): two cameras with X2 = R X1 + t, camera 1 on the left, and the output size
    (height, width) -> (r1, r2, k_new: (3, 3) float64 CPU tensors; baseline; fb = f * baseline, what stereo_depth wants),
    cv2.stereoRectify without trigonometry.  Map the left camera with (k1, dist1, r1, k_new), the right with (k2, dist2, r2, k_new)."""
    h, w = (int(v) for v in size)
    r1, r2, k_new = ((N.c_double * 9)() for _ in range(3))
    baseline, fb = N.c_double(), N.c_double()
    N.call("mi_rectify_stereo_rig", _rectify_doubles(k1, 9, "k1"), _rectify_doubles(k2, 9, "k2"), _rectify_doubles(rotation, 9, "rotation"),
           _rectify_doubles(translation, 3, "translation"), h, w, r1, r2, k_new, N.ctypes.byref(baseline), N.ctypes.byref(fb))
    return tuple(torch.tensor(list(a), dtype=torch.float64).view(3, 3) for a in (r1, r2, k_new)) + (baseline.value, fb.value)


# ---- K35 disparity post-filters (include/mi355x_match_filter.h) ---------------------------------------------------------------

FILTER_SPECKLE, FILTER_NO_LABEL = N.FILTER_CONSTANTS["MI_FILTER_SPECKLE"], N.FILTER_CONSTANTS["MI_FILTER_NO_LABEL"]
FILTER_MEDIANS = (3, 5)
_FILTER_TYPES = {U8: N.FILTER_CONSTANTS["MI_FILTER_U8"], F32: N.FILTER_CONSTANTS["MI_FILTER_F32"]}


def filter_components(values: torch.Tensor, min_valid: float, max_diff: float, want_sizes: bool = True):
    """`mi_filter_components`: frames (B, H, W) or (B, 1, H, W), uint8 (a class map) or float32 -> (labels int32 of the same shape:
    the smallest y * W + x of the pixel's 4-connected component, FILTER_NO_LABEL on an invalid pixel; sizes int32: the pixel count
    of its component, 0 on an invalid pixel, or None with want_sizes=False).  A pixel is valid iff value >= min_valid; two
    neighbours are joined iff both are valid and |a - b| <= max_diff."""
    v = _stereo_frames(values, "filter_components: values", (U8, F32))
    b, h, w = (int(x) for x in v.shape)
    labels = torch.empty((b, h, w), dtype=I32, device=v.device)
    sizes = torch.empty((b, h, w), dtype=I32, device=v.device) if want_sizes else None
    work, wbytes = _workspace("mi_filter_workspace_bytes", b, h, w, device=v.device,
                              refusal=f"filter_components: {b} frames of {h} x {w} are outside what mi_filter_components covers")
    N.call("mi_filter_components", v.data_ptr(), _FILTER_TYPES[v.dtype], b, h, w, float(min_valid), float(max_diff), labels.data_ptr(),
           None if sizes is None else sizes.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return labels.view(values.shape), None if sizes is None else sizes.view(values.shape)


def filter_speckle(x: torch.Tensor, max_size: int, max_diff: float, min_valid: float = 0.0, invalid_value: float = -1.0,
                   want_removed: bool = False):
    """`mi_filter_speckle`: float32 frames (B, H, W) or (B, 1, H, W) -> the frames with every component of at most max_size
    pixels, and every invalid pixel, set to invalid_value (cv2.filterSpeckles on float disparities); with want_removed also the
    byte map of the VALID pixels that were dropped.  For depth frames: min_valid = min_depth, invalid_value = 0.0."""
    v = _stereo_frames(x, "filter_speckle: x", (F32,))
    b, h, w = (int(s) for s in v.shape)
    out = torch.empty((b, h, w), dtype=F32, device=v.device)
    removed = torch.empty((b, h, w), dtype=U8, device=v.device) if want_removed else None
    work, wbytes = _workspace("mi_filter_workspace_bytes", b, h, w, device=v.device,
                              refusal=f"filter_speckle: {b} frames of {h} x {w} are outside what mi_filter_speckle covers")
    N.call("mi_filter_speckle", v.data_ptr(), b, h, w, float(min_valid), float(max_diff), int(max_size), float(invalid_value), out.data_ptr(),
           None if removed is None else removed.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return (out.view(x.shape), removed.view(x.shape)) if want_removed else out.view(x.shape)


def filter_median(x: torch.Tensor, k: int = 3, min_valid: float = 0.0, invalid_value: float = -1.0) -> torch.Tensor:
    """`mi_filter_median`: float32 frames (B, H, W) or (B, 1, H, W) -> the k x k (3 or 5) median over the VALID taps of the
    window (replicate border), invalid_value where the centre is invalid: it does not fill holes."""
    v = _stereo_frames(x, "filter_median: x", (F32,))
    b, h, w = (int(s) for s in v.shape)
    out = torch.empty((b, h, w), dtype=F32, device=v.device)
    N.call("mi_filter_median", v.data_ptr(), b, h, w, int(k), float(min_valid), float(invalid_value), out.data_ptr(), N.stream_ptr())
    return out.view(x.shape)
