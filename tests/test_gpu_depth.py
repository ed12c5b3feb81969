"""K13 depth front end on the MI355X against the numpy oracles of test_depth_host.py (which reproduce the reference
fixture): points bit for bit, normals within the derived bound at every pixel, alignment equal to the oracle at EVERY
pixel -- also for camera pairs on which the reference raises --, determinism, batching, dirty output buffers, the
modules on the fixture, and the composed depth -> cloud -> voxel path captured into one graph.  Also meant to run
under MI_POISON_EMPTY=1 (conftest.py)."""
import numpy as np
import pytest
import torch

from test_depth_host import (F32, align_cases, align_oracle, camera_args, check_align_against_reference, check_normals,
                             check_points, fixture_depth, golden, points_cases, points_oracle,
                             tables_oracle)
from gpu_common import DEV, GPU, gpu
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_depth_frame

pytestmark = GPU


def _frames(h, w, count, seed, counts=False):
    """count frames of mixed content: plain, with holes, all zero, and with values mi_depth_align silences"""
    out = []
    for i in range(count):
        d = synth_depth_frame(seed + i, h, w, hole_share=(0.0, 0.15, 0.05)[i % 3])
        if counts:
            d = np.round(d.astype(np.float64) * 1000.0)
        if i % 4 == 3:
            d = np.zeros_like(d)
        out.append(d.astype(np.uint16 if counts else F32))
    return np.stack(out)


SIZES = [(1, 1), (1, 77), (45, 1), (37, 53), (5, 130), (9, 128), (480, 640)]


def _camera(scale, h, w):
    return scale, w, h, 0.49 * w + 0.3, 0.52 * h - 0.2, 0.82 * max(w, 8), 0.8 * max(w, 8)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("counts", [False, True], ids=["float32", "uint16"])
def test_points_are_the_oracle_s_bits_and_normals_are_within_the_bound(h, w, counts):
    args = _camera(0.001 if counts else 1.0, h, w)
    u, v, zs = tables_oracle(*args)
    batch = 5 if h * w < 100_000 else 3
    frames = _frames(h, w, batch, 50 + h + w, counts)
    want = points_oracle(frames, u, v, zs)
    tu, tv = gpu(u), gpu(v)
    d = gpu(frames)
    pts = ops.depth_to_points(d, tu, tv, float(zs))
    pts2, nrm = ops.depth_to_points(d, tu, tv, float(zs), normals=True)
    assert pts.shape == (batch, h, w, 3) and nrm.shape == (batch, h, w, 3) and nrm.dtype == torch.float32
    check_points(pts.cpu().numpy(), want, "points only")
    check_points(pts2.cpu().numpy(), want, "points with normals")
    nrm = nrm.cpu().numpy()
    for b in range(batch):
        check_normals(nrm[b], want[b], f"{h}x{w} frame {b}")
        # a frame alone, in each accepted shape, equals its slice of the batch
        for shaped in (d[b], d[b].reshape(h, w, 1), d[b:b + 1], d[b:b + 1].reshape(1, h, w, 1)):
            p1, n1 = ops.depth_to_points(shaped, tu, tv, float(zs), normals=True)
            assert torch.equal(p1.reshape(h, w, 3), pts[b]) and torch.equal(n1.reshape(h, w, 3), torch.from_numpy(nrm[b]).to(DEV))


def test_point_output_shapes():
    u, v, zs = tables_oracle(1.0, 8, 6, 4.0, 3.0, 7.0, 7.5)
    tu, tv = gpu(u), gpu(v)
    for shape, out in (((6, 8), (6, 8, 3)), ((6, 8, 1), (6, 8, 3)), ((3, 6, 8), (3, 6, 8, 3)), ((3, 6, 8, 1), (3, 6, 8, 3))):
        assert ops.depth_to_points(torch.ones(shape, device=DEV), tu, tv, float(zs)).shape == out
        al = ops.depth_align(torch.ones(shape, device=DEV), tu, tv, float(zs), 4.0, 3.0, 7.0, 7.5,
                             torch.eye(3, device=DEV), torch.zeros(3, device=DEV))
        assert al.shape == shape and al.dtype == torch.float32
    with pytest.raises(RuntimeError, match="shape"):
        ops.depth_to_points(torch.ones(8, 6, device=DEV), tu, tv, float(zs))
    with pytest.raises(RuntimeError, match="float32 or uint16"):
        ops.depth_to_points(torch.ones(6, 8, device=DEV, dtype=torch.float64), tu, tv, float(zs))


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    a = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    b = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    c = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (c @ b @ a).astype(F32)


def _align_gpu(frames, u, v, zs, rgb, rot, tr):
    return ops.depth_align(gpu(frames), gpu(u), gpu(v), float(zs), *[float(x) for x in rgb], gpu(np.asarray(rot, F32)),
                           gpu(np.asarray(tr, F32)))


def _check_align_everywhere(frames, u, v, zs, rgb, rot, tr, what):
    got = _align_gpu(frames, u, v, zs, rgb, rot, tr)
    again = _align_gpu(frames, u, v, zs, rgb, rot, tr)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), f"{what}: two runs differ"
    got = got.cpu().numpy()
    for b in range(frames.shape[0]):
        want = align_oracle(frames[b], u, v, zs, rgb, rot, tr)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), \
            f"{what} frame {b}: {int((got[b] != want).sum())} pixels differ from the oracle"
        alone = _align_gpu(frames[b], u, v, zs, rgb, rot, tr).cpu().numpy()
        assert np.array_equal(alone.view(np.uint32), got[b].view(np.uint32)), f"{what} frame {b}: alone != batched"
    return got


def test_alignment_equals_the_oracle_at_every_pixel_of_every_fixture_case():
    g = golden()
    for name in align_cases(g):
        d = fixture_depth(g, name)
        u, v, zs = tables_oracle(*camera_args(g, name))
        rgb, rot, tr = g[f"{name}__rgb"], g[f"{name}__rotation"], g[f"{name}__translation"]
        got = _check_align_everywhere(d[None], u, v, zs, rgb, rot, tr, name)
        _, clean = align_oracle(d, u, v, zs, rgb, rot, tr, with_clean=True)
        check_align_against_reference(got[0], g[f"{name}__aligned"], clean, name)


@pytest.mark.parametrize("counts", [False, True], ids=["float32", "uint16"])
def test_alignment_of_full_frames_with_holes_and_cameras_the_reference_raises_on(counts):
    h, w = 480, 640
    frames = _frames(h, w, 4, 70, counts)
    if not counts:
        frames[1, 100:140, 200:260] = 12000.0          # beyond the fill value: silenced
        frames[1, 300:310, 20:30] = -1.0
        frames[2, 50:60, 50:60] = np.nan
    else:
        frames[1, 100:140, 200:260] = 12000            # counts >= 10000 are silenced as raw values
    scale = 0.001 if counts else 1.0
    u, v, zs = tables_oracle(scale, w, h, 319.5, 239.5, 525.0, 525.0)
    cases = {
        # similar intrinsics: sources land in [w - 0.5, w) / [h - 0.5, h), where the reference raises IndexError
        "similar cameras": ((325.1, 243.7, 520.0, 521.5), _rot(0.01, -0.02, 0.005), (0.025, -0.002, 0.004)),
        "identity": ((319.5, 239.5, 525.0, 525.0), np.eye(3), (0.0, 0.0, 0.0)),
        "narrow colour camera": ((300.0, 250.0, 700.0, 690.0), _rot(-0.03, 0.02, 0.1), (-0.05, 0.01, -0.02)),
        "wide colour camera": ((320.0, 240.0, 470.0, 471.0), _rot(0.004, -0.006, 0.003), (0.025, 0.0, 0.0)),
    }
    for what, (rgb, rot, tr) in cases.items():
        got = _check_align_everywhere(frames, u, v, zs, rgb, rot, tr, what)
        assert (got[0] != 0).mean() > 0.3 and not got[3].any(), what
    # the edge-drop rule was exercised: some source of the first case offers a target in column w or row h
    from test_depth_host import _project
    rgb, rot, tr = cases["similar cameras"]
    d, px, py = _project(frames[0], u, v, zs, rgb, rot, tr)
    live = (px >= 0) & (px < w) & (py >= 0) & (py < h) & (d > 0)
    assert ((np.trunc(px[live] + F32(0.5)) == w) | (np.trunc(py[live] + F32(0.5)) == h)).any()


def test_sources_that_all_leave_the_image_give_zeros():
    h, w = 120, 160
    frames = _frames(h, w, 2, 90)[:2]
    u, v, zs = tables_oracle(1.0, w, h, 80.0, 60.0, 130.0, 130.0)
    for rot, tr in ((np.eye(3), (100.0, 0.0, 0.0)), (_rot(0.0, np.pi, 0.0), (0.0, 0.0, -0.5)), (np.eye(3), (0.0, -50.0, 0.0))):
        got = _check_align_everywhere(frames, u, v, zs, (80.0, 60.0, 120.0, 120.0), rot, tr, "out of frame")
        if tr[0] == 100.0 or tr[1] == -50.0:
            assert not got.any()


def test_dirty_output_buffers_do_not_show():
    """The C entries take outputs of any content: the alignment's fill pass must not assume zeros."""
    h, w, batch = 37, 53, 3
    frames = _frames(h, w, batch, 110)
    args = _camera(1.0, h, w)
    u, v, zs = tables_oracle(*args)
    rgb, rot, tr = (27.0, 18.0, 38.0, 38.5), _rot(0.004, -0.006, 0.003), np.float32([0.025, 0.0, 0.0])
    d, tu, tv, trot, ttr = gpu(frames), gpu(u), gpu(v), gpu(rot), gpu(tr)
    want_p, want_n = ops.depth_to_points(d, tu, tv, float(zs), normals=True)
    want_a = ops.depth_align(d, tu, tv, float(zs), *rgb, trot, ttr)
    assert np.array_equal(want_a[1].cpu().numpy(), align_oracle(frames[1], u, v, zs, rgb, rot, tr))
    for junk in (0.0, float("nan"), -3.0e38, 1e-3, 5.0):
        p = torch.empty((batch, h, w, 3), dtype=torch.float32, device=DEV).fill_(junk)
        n = torch.empty((batch, h, w, 3), dtype=torch.float32, device=DEV).fill_(junk)
        a = torch.empty((batch, h, w), dtype=torch.float32, device=DEV).fill_(junk)
        N.call("mi_depth_to_points", d.data_ptr(), 0, batch, h, w, tu.data_ptr(), tv.data_ptr(), float(zs), p.data_ptr(),
               n.data_ptr(), N.stream_ptr())
        N.call("mi_depth_align", d.data_ptr(), 0, batch, h, w, tu.data_ptr(), tv.data_ptr(), float(zs), *rgb, trot.data_ptr(),
               ttr.data_ptr(), a.data_ptr(), N.stream_ptr())
        for got, want in ((p, want_p), (n, want_n), (a, want_a)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), junk
    a = torch.full((batch, h, w), -1, dtype=torch.int32, device=DEV)            # the sentinel's own bit pattern
    N.call("mi_depth_align", d.data_ptr(), 0, batch, h, w, tu.data_ptr(), tv.data_ptr(), float(zs), *rgb, trot.data_ptr(),
           ttr.data_ptr(), a.data_ptr(), N.stream_ptr())
    assert torch.equal(a, want_a.view(torch.int32))


def test_modules_reproduce_the_reference_fixture():
    from pytorch_model.depth.depth2pointcloud import DepthToPointCloud
    from pytorch_model.depth.depth2pointcloud_with_normal import DepthToPointCloudWithNormal
    from pytorch_model.depth.depth_align import DepthAlignment
    g = golden()
    for name in points_cases(g):
        d = fixture_depth(g, name)
        h, w = d.shape
        args = camera_args(g, name)
        x = gpu(d).reshape(h, w, 1)                                   # what the reference's forward takes
        pts = DepthToPointCloud(*args).to(DEV)(x)
        pts2, nrm = DepthToPointCloudWithNormal(*args).to(DEV)(x)
        assert pts.shape == (h, w, 3) and nrm.shape == (h, w, 3)
        check_points(pts.cpu().numpy(), g[f"{name}__points"], name)
        check_points(pts2.cpu().numpy(), g[f"{name}__points"], name)
        check_normals(nrm.cpu().numpy(), g[f"{name}__points"], name)
        if int(g[f"{name}__millimetres"]):                              # the same frame as uint16 sensor counts
            p16, n16 = DepthToPointCloudWithNormal(*args).to(DEV)(gpu(d.astype(np.uint16)))
            assert torch.equal(p16, pts2) and torch.equal(n16, nrm)
    for name in align_cases(g):
        d = fixture_depth(g, name)
        h, w = d.shape
        args = camera_args(g, name)
        rgb, rot, tr = g[f"{name}__rgb"], g[f"{name}__rotation"], g[f"{name}__translation"]
        model = DepthAlignment(*args, *[float(x) for x in rgb], torch.from_numpy(rot), torch.from_numpy(tr)).to(DEV)
        out = model(gpu(d).reshape(h, w, 1))
        assert out.shape == (h, w, 1)
        u, v, zs = tables_oracle(*args)
        _, clean = align_oracle(d, u, v, zs, rgb, rot, tr, with_clean=True)
        check_align_against_reference(out.reshape(h, w).cpu().numpy(), g[f"{name}__aligned"], clean, name)
        if int(g[f"{name}__millimetres"]):
            assert torch.equal(model(gpu(d.astype(np.uint16))), out.reshape(h, w))


def test_depth_to_voxels_composition_captured_in_one_graph():
    """DepthToPointCloudWithNormal + DepthAlignment + voxel_downsample_batch on 4 frames as one straight-line graph:
    replayed on new depth content it equals the eager result on that content bit for bit."""
    from pytorch_model.depth import DepthAlignment, DepthToPointCloudWithNormal
    h, w, batch = 240, 320, 4
    cam = (1.0, w, h, 159.5, 119.5, 262.5, 262.5)
    pcn = DepthToPointCloudWithNormal(*cam).to(DEV)
    align = DepthAlignment(*cam, 162.0, 121.0, 236.0, 237.0, torch.from_numpy(_rot(0.004, -0.006, 0.003)),
                           torch.tensor([0.025, 0.0, 0.0])).to(DEV)
    offs = (torch.arange(batch + 1, dtype=torch.int64) * (h * w)).to(DEV)
    leaf = torch.full((batch,), 0.02, dtype=torch.float32, device=DEV)

    def run(depth):
        pts, nrm = pcn(depth)
        al = align(depth)
        vox, mask, counts, _ = ops.voxel_downsample_batch(pts.reshape(-1, 3), leaf, offsets=offs)
        return pts, nrm, al, vox, mask, counts

    first = gpu(np.stack([synth_depth_frame(130 + i, h, w, hole_share=0.02 * i) for i in range(batch)]))
    second = gpu(np.stack([synth_depth_frame(140 + i, h, w, hole_share=0.03 * i) for i in range(batch)]))
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, run(first)):
        assert torch.equal(got, want)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(second)
    for got, want in zip(outs, eager):
        assert torch.equal(got, want)
    pts, _, al, vox, mask, counts = eager
    u, v, zs = tables_oracle(*cam)
    check_points(pts.cpu().numpy(), points_oracle(second.cpu().numpy(), u, v, zs), "replayed points")
    assert np.array_equal(al[2].cpu().numpy(), align_oracle(second[2].cpu().numpy(), u, v, zs, (162.0, 121.0, 236.0, 237.0),
                                                            _rot(0.004, -0.006, 0.003), np.float32([0.025, 0, 0])))
    for b in range(batch):
        so, sm = ops.voxel_downsample(pts[b].reshape(-1, 3), 0.02)
        sl = slice(b * h * w, (b + 1) * h * w)
        assert torch.equal(vox[sl], so) and torch.equal(mask[sl], sm) and int(counts[b]) == int(sm.sum())
