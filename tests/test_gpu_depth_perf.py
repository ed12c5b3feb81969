"""K13 rates: each of the three HIP depth operations on 16 frames of 480x640 in one call beats a torch-on-GPU formulation
of the same operation written here from stock ops, run frame by frame as the reference's modules work: a broadcast
multiply (points); F.conv2d + normalise on top of it (points + normals); back-project, p @ R + t, project and either four
index_put_ + minimum (the reference's form) or one scatter_reduce_('amin') over the four splats (alignment: both are
timed, the faster one is the yardstick and the test prints which)."""
import numpy as np
import torch
import torch.nn.functional as F

from test_depth_host import align_oracle, tables_oracle
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_depth_frame

pytestmark = GPU_PERF
H, W, FRAMES = 480, 640, 16
DEPTH_CAM = (1.0, W, H, 319.5, 239.5, 525.0, 525.0)
# a colour camera with the wider field of view: the torch formulation indexes out of range otherwise, as the reference does
RGB = (322.0, 241.0, 470.0, 471.0)
ROT = [[0.99997753, -0.0029759, -0.00600796], [0.00299993, 0.99998754, 0.0039909], [0.00599601, -0.00400884, 0.99997398]]
TRANS = [0.025, 0.0, 0.0]
SOBEL_V = [[1, 0, -1], [2, 0, -2], [1, 0, -1]]
SOBEL_H = [[1, 2, 1], [0, 0, 0], [-1, -2, -1]]


def torch_points(depth, uv):
    """depth (H, W, 1), uv (H, W, 3)"""
    return depth * uv


def torch_points_normals(depth, uv, sobel_v, sobel_h, minus_one):
    pcd = depth * uv
    nchw = pcd.permute(2, 0, 1).unsqueeze(0)
    dx = F.conv2d(nchw, sobel_v, padding=1)
    dy = F.conv2d(nchw, sobel_h, padding=1)
    vec = torch.cat([dx, dy, minus_one], dim=1).squeeze(0).permute(1, 2, 0)
    return pcd, vec / torch.sqrt(torch.sum(vec ** 2, dim=2, keepdim=True))


def _torch_project(depth, uv, rot, trans, rgb):
    h, w = depth.shape[:2]
    q = (depth * uv) @ rot + trans
    z = q[:, :, 2]
    px = q[:, :, 0] / z * rgb[2] + rgb[0]
    py = q[:, :, 1] / z * rgb[3] + rgb[1]
    off = (z == 0) | (px < 0) | (px >= w) | (py < 0) | (py >= h)
    px = torch.where(off, 0.0, px).reshape(-1)
    py = torch.where(off, 0.0, py).reshape(-1)
    return (px - 0.5).long(), (px + 0.5).long(), (py - 0.5).long(), (py + 0.5).long()


def torch_align_index_put(depth, uv, rot, trans, rgb):
    """the reference's forward: four non-accumulating index_put_ and their minimum"""
    x0, x1, y0, y1 = _torch_project(depth, uv, rot, trans, rgb)
    val = depth.reshape(-1)
    flat = depth[:, :, 0]
    out = None
    for ty in (y0, y1):
        for tx in (x0, x1):
            a = torch.full_like(flat, 10000.0)
            a[ty, tx] = val
            out = a if out is None else torch.minimum(out, a)
    return torch.where(out == 10000.0, 0.0, out)


def torch_align_scatter(depth, uv, rot, trans, rgb):
    """the same with one scatter_reduce_('amin') over the four splats (minimum over all writers, as the HIP path)"""
    h, w = depth.shape[:2]
    x0, x1, y0, y1 = _torch_project(depth, uv, rot, trans, rgb)
    idx = torch.cat([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1])
    out = torch.full((h * w,), 10000.0, device=depth.device).scatter_reduce_(0, idx, depth.reshape(-1).repeat(4), "amin")
    return torch.where(out == 10000.0, 0.0, out).reshape(h, w)


def workload(frames=FRAMES, seed=500):
    """(depth (frames, H, W) on the GPU, tables, torch-side constants); checks on the host that no source indexes out
    of range in the torch formulation (a device-side fault otherwise)."""
    u, v, zs = tables_oracle(*DEPTH_CAM)
    host = np.stack([synth_depth_frame(seed + i, H, W) for i in range(frames)])
    for d in host[:2]:
        align_oracle(d, u, v, zs, RGB, ROT, TRANS, with_clean=True)          # asserts the index range
    uv = np.stack([np.broadcast_to(u[None, :], (H, W)), np.broadcast_to(v[:, None], (H, W)), np.full((H, W), zs, np.float32)], -1)
    t = dict(depth=torch.from_numpy(host).to(DEV), u=torch.from_numpy(u).to(DEV), v=torch.from_numpy(v).to(DEV), zs=float(zs),
             uv=torch.from_numpy(np.ascontiguousarray(uv)).to(DEV), rot=torch.tensor(ROT, device=DEV),
             trans=torch.tensor(TRANS, device=DEV),
             sobel_v=torch.tensor(SOBEL_V, dtype=torch.float32, device=DEV).expand(1, 3, 3, 3).contiguous(),
             sobel_h=torch.tensor(SOBEL_H, dtype=torch.float32, device=DEV).expand(1, 3, 3, 3).contiguous(),
             minus_one=torch.full((1, 1, H, W), -1.0, device=DEV))
    return t


def operations(t):
    """name -> (hip callable, {torch formulation name: callable}) on the workload's frames"""
    d = t["depth"]
    per_frame = [d[i].reshape(H, W, 1) for i in range(d.shape[0])]
    return {
        "points": (lambda: ops.depth_to_points(d, t["u"], t["v"], t["zs"]),
                   {"broadcast multiply": lambda: [torch_points(f, t["uv"]) for f in per_frame]}),
        "points+normals": (lambda: ops.depth_to_points(d, t["u"], t["v"], t["zs"], normals=True),
                           {"conv2d + normalise": lambda: [torch_points_normals(f, t["uv"], t["sobel_v"], t["sobel_h"], t["minus_one"])
                                                           for f in per_frame]}),
        "alignment": (lambda: ops.depth_align(d, t["u"], t["v"], t["zs"], *RGB, t["rot"], t["trans"]),
                      {"4 x index_put_ + minimum": lambda: [torch_align_index_put(f, t["uv"], t["rot"], t["trans"], RGB) for f in per_frame],
                       "scatter_reduce_ amin": lambda: [torch_align_scatter(f, t["uv"], t["rot"], t["trans"], RGB) for f in per_frame]}),
    }


def test_torch_formulations_compute_the_same_thing():
    """the yardsticks are formulations of the same operations: points equal, normals close, scatter alignment equal"""
    t = workload(2)
    d = t["depth"]
    pts, nrm = ops.depth_to_points(d, t["u"], t["v"], t["zs"], normals=True)
    tp, tn = torch_points_normals(d[1].reshape(H, W, 1), t["uv"], t["sobel_v"], t["sobel_h"], t["minus_one"])
    assert torch.equal(tp, pts[1]) and (tn - nrm[1]).abs().max() < 1e-4
    al = ops.depth_align(d, t["u"], t["v"], t["zs"], *RGB, t["rot"], t["trans"])
    ts = torch_align_scatter(d[1].reshape(H, W, 1), t["uv"], t["rot"], t["trans"], RGB)
    tq = torch_align_index_put(d[1].reshape(H, W, 1), t["uv"], t["rot"], t["trans"], RGB)
    assert (ts == al[1]).float().mean() > 0.99 and (tq >= al[1]).float().mean() > 0.99


def test_hip_depth_operations_beat_torch_on_gpu_for_sixteen_frames():
    t = workload()
    failed = []
    for name, (hip_fn, torch_fns) in operations(t).items():
        hip = time_ms(hip_fn)
        refs = {k: time_ms(fn) for k, fn in torch_fns.items()}
        best = min(refs, key=refs.get)
        print(f"{name}: 16 frames HIP {hip:.3f} ms; torch-on-GPU " + ", ".join(f"{k} {v:.3f} ms" for k, v in refs.items())
              + f"; yardstick: {best} ({refs[best] / hip:.1f}x)")
        if not hip < refs[best]:
            failed.append(name)
    assert not failed, failed
