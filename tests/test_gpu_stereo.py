"""K33 stereo depth on the GPU against tests/stereo_oracle.py, bit for bit and without a tolerance: the census words as uint64, the
volume as uint16, disparity_right, code, and disparity and depth as float32 bit patterns.  Shapes: (37, 83) at D = 64, (24, 150)
at D = 128, (9, 300) at D = 256 -- more than one workgroup of lines in every direction, no multiple of a wave or a strip -- and
(1, 70), (70, 1), (5, 40) with w < D; 4 and 8 paths, uint8 and float32 gray, a batch of three whose images equal their single
runs; the ends of the penalties and of the uniqueness margin, the left-right test off without a right view, hostile float32
gray, outputs that hold garbage on entry, a repeat, a hipGraph replay, the constant plane through StereoMatcher and the chain
into DepthToPointCloud's kernel and TsdfVolume."""
import numpy as np
import pytest
import torch

import stereo_oracle as SO
from gpu_common import DEV, GPU, gpu, same_bits, twice
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.stereo import StereoMatcher

pytestmark = GPU

KEYS = ("census_left", "census_right", "volume", "disparity", "disparity_right", "code", "depth")
SHAPES = [(37, 83, 64), (24, 150, 128), (9, 300, 256), (1, 70, 64), (70, 1, 64), (5, 40, 64)]
BATCH_SEEDS = (11, 21, 22)
FB, MIN_DISPARITY = 100.0, 0.5


def garbage(shape, dtype):
    """an output buffer that holds 0xA5 bytes on entry"""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t


def run_gpu(left, right, D, paths, p1=SO.P1, p2=SO.P2, uniqueness=SO.UNIQUENESS, lr_max_diff=SO.LR_MAX_DIFF, want_right=True):
    """(B, h, w) numpy views through the five entries of the C ABI, every output pre-filled with garbage -> dict of numpy arrays"""
    l, r = gpu(np.asarray(left), np.asarray(right))
    b, h, w = l.shape
    u8, s = int(l.dtype == torch.uint8), N.stream_ptr()
    cl, cr = garbage((b, h, w), torch.int64), garbage((b, h, w), torch.int64)
    volume = garbage((b, h, w, D), torch.uint16)
    disparity, depth = garbage((b, h, w), torch.float32), garbage((b, h, w), torch.float32)
    dr = garbage((b, h, w), torch.int16) if want_right else None
    code = garbage((b, h, w), torch.uint8)
    N.call("mi_stereo_census", l.data_ptr(), u8, b, h, w, cl.data_ptr(), s)
    N.call("mi_stereo_census", r.data_ptr(), u8, b, h, w, cr.data_ptr(), s)
    N.call("mi_stereo_aggregate", cl.data_ptr(), cr.data_ptr(), b, h, w, D, paths, p1, p2, volume.data_ptr(), None, 0, s)
    N.call("mi_stereo_select", volume.data_ptr(), b, h, w, D, uniqueness, lr_max_diff, disparity.data_ptr(),
           None if dr is None else dr.data_ptr(), code.data_ptr(), s)
    N.call("mi_stereo_depth", disparity.data_ptr(), b, h, w, FB, MIN_DISPARITY, depth.data_ptr(), s)
    torch.cuda.synchronize()
    out = dict(census_left=cl.cpu().numpy().view(np.uint64), census_right=cr.cpu().numpy().view(np.uint64), volume=volume.cpu().numpy(),
               disparity=disparity.cpu().numpy(), code=code.cpu().numpy(), depth=depth.cpu().numpy())
    out["disparity_right"] = None if dr is None else dr.cpu().numpy()
    return out


def same(got, b, want, what):
    """image b of a GPU result against one oracle result, every array byte for byte"""
    for key in KEYS:
        if got[key] is None:
            continue
        g, o = np.ascontiguousarray(got[key][b]), np.ascontiguousarray(want[key])
        assert g.dtype == o.dtype and g.shape == o.shape, (what, key, g.dtype, o.dtype)
        differ = g.view(np.uint8) != o.view(np.uint8)
        assert not differ.any(), f"{what}: {key} differs from the oracle in {int(differ.sum())} bytes of {differ.size}"


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("h,w,D", SHAPES)
def test_every_stage_is_the_oracle_bit_for_bit(h, w, D, paths, u8):
    pairs = [SO.pair(seed, h, w, u8) for seed in BATCH_SEEDS]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    batch = run_gpu(left, right, D, paths)
    for b, seed in enumerate(BATCH_SEEDS):
        same(batch, b, SO.case(seed, h, w, u8, D, paths), (h, w, D, paths, u8, seed))
    alone = run_gpu(left[1:2], right[1:2], D, paths)                          # an image's bits do not depend on its batch
    for key in KEYS:
        assert np.array_equal(alone[key][0].view(np.uint8), batch[key][1].view(np.uint8)), key
    if paths == 8 and u8:
        twice((h, w, D), lambda: tuple(run_gpu(left, right, D, paths)[key] for key in KEYS))


@pytest.mark.parametrize("kw", [dict(p1=0, p2=0), dict(p1=255, p2=255), dict(uniqueness=0), dict(uniqueness=100), dict(lr_max_diff=0),
                                dict(p1=0, p2=255, uniqueness=100, lr_max_diff=5)], ids=str)
def test_the_ends_of_the_parameters(kw):
    for h, w, D in ((24, 90, 64), (9, 150, 128)):
        left, right = SO.pair(12, h, w, True)
        got = run_gpu(left[None], right[None], D, 8, **kw)
        same(got, 0, SO.case(12, h, w, True, D, 8, **kw), (h, w, D, kw))
        if kw.get("uniqueness") == 100:
            assert (got["code"] == SO.NOT_UNIQUE).mean() > 0.9


def test_left_right_test_off_without_a_right_view():
    for h, w, D in ((24, 90, 64), (9, 300, 256)):
        left, right = SO.pair(12, h, w, False)
        want = SO.case(12, h, w, False, D, 8, lr_max_diff=-1)
        none = run_gpu(left[None], right[None], D, 8, lr_max_diff=-1, want_right=False)
        assert none["disparity_right"] is None and not (none["code"] == SO.LR).any()
        same(none, 0, want, (h, w, D, "no right view"))
        same(run_gpu(left[None], right[None], D, 8, lr_max_diff=-1), 0, want, (h, w, D, "right view written, test off"))


@pytest.mark.parametrize("h,w,D", [(37, 83, 64), (5, 40, 64), (9, 150, 128)])
def test_hostile_float_gray(h, w, D):
    """NaN, both infinities and +-1e30 in a tenth of the pixels: the oracle's bits, and every output is a legal value"""
    left, right = SO.hostile_pair(13, h, w)
    got = run_gpu(left[None], right[None], D, 8)
    same(got, 0, SO.run(left, right, D, 8, fb=FB, min_disparity=MIN_DISPARITY), (h, w, D))
    assert got["volume"].max() <= 8 * 319 and got["code"].max() <= SO.LR and np.isfinite(got["depth"]).all()


def test_ops_and_module_give_the_same_bits_as_the_entries():
    left, right = (np.stack([SO.pair(seed, 37, 83, True)[i] for seed in BATCH_SEEDS]) for i in (0, 1))
    want = run_gpu(left, right, 64, 8)
    l, r = gpu(left, right)
    cl, cr = ops.stereo_census(l), ops.stereo_census(r.unsqueeze(1))           # (B, 1, H, W), as ingest_frames returns it
    volume = ops.stereo_aggregate(cl, cr, 64, 8, SO.P1, SO.P2)
    disparity, dr, code = ops.stereo_select(volume, SO.UNIQUENESS, SO.LR_MAX_DIFF)
    depth = ops.stereo_depth(disparity, FB, MIN_DISPARITY)
    got = dict(census_left=cl.cpu().numpy().view(np.uint64), census_right=cr.cpu().numpy().view(np.uint64), volume=volume.cpu().numpy(),
               disparity=disparity.cpu().numpy(), disparity_right=dr.cpu().numpy(), code=code.cpu().numpy(), depth=depth.cpu().numpy())
    for key in KEYS:
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
    m = StereoMatcher(max_disparity=64)
    d2, c2 = m(l.unsqueeze(1), r.unsqueeze(1))
    assert d2.shape == (3, 1, 37, 83) and same_bits((d2[:, 0], c2[:, 0], m.depth(d2, 50.0, 2.0)[:, 0]), (disparity, code, depth))
    assert ops.stereo_select(volume, SO.UNIQUENESS, -1, want_right=False)[1] is None
    with pytest.raises(RuntimeError):
        ops.stereo_aggregate(cl, cr, 96)                                       # MI_E_PARAM, no fall-back


PLANE_CASES = [(0, 8), (5, 8), (17, 8), (30, 8), (30, 4)]


@pytest.mark.parametrize("d0,paths", PLANE_CASES)
def test_constant_plane_through_the_module(d0, paths):
    """the interior of a plane at disparity d0 (rows 3 .. h - 4, columns d0 + 8 .. w - 5): d* = d0 everywhere, accepted, within
    half a pixel; no pixel with x < d0 is accepted; and the module's bits are the oracle's"""
    left, right = SO.plane_pair(0, 21, 90, d0)
    m = StereoMatcher(max_disparity=64, p1=10, p2=120, paths=paths, uniqueness=10, lr_max_diff=1)
    disparity, code = m(gpu(left[None]), gpu(right[None]))
    disparity, code = disparity[0].cpu().numpy(), code[0].cpu().numpy()
    inside = SO.plane_interior(21, 90, d0)
    assert (code[inside] == SO.OK).all() and (np.rint(disparity[inside]) == d0).all() and np.abs(disparity[inside] - d0).max() <= 0.5
    assert (code[:, :d0] != SO.OK).all()                                       # left of d0 the scene point is outside the right view
    want = SO.run(left, right, 64, paths, 10, 120, 10, 1)
    assert np.array_equal(disparity.view(np.uint32), want["disparity"].view(np.uint32)) and np.array_equal(code, want["code"])
    best = m.volume(gpu(left[None]), gpu(right[None]))[0].cpu().numpy().astype(np.int64).argmin(-1)
    assert (best[inside] == d0).all()


def test_chain_into_the_point_cloud_and_the_tsdf_volume():
    """StereoMatcher.depth feeds ops.depth_to_points and TsdfVolume.integrate as a sensor's depth frame does: in the interior of
    a plane at d0 = 17 the points lie between fb / (d0 + 0.5) and fb / (d0 - 0.5), and the volume takes the surface in"""
    from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
    d0, h, w, fx, baseline = 17, 21, 90, 100.0, 0.17
    left, right = SO.plane_pair(0, h, w, d0)
    m = StereoMatcher(max_disparity=64)
    disparity, code = m(gpu(left[None]), gpu(right[None]))
    depth = m.depth(disparity, fx, baseline)
    assert depth.shape == (1, h, w) and depth.dtype == torch.float32
    fb = fx * baseline
    near, far = fb / (d0 + 0.5), fb / (d0 - 0.5)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    u_tab = ((torch.arange(w, dtype=torch.float32) - cx) / fx).to(DEV)
    v_tab = ((torch.arange(h, dtype=torch.float32) - cy) / fx).to(DEV)
    points = ops.depth_to_points(depth, u_tab, v_tab, 1.0)[0].cpu().numpy()
    inside = SO.plane_interior(h, w, d0)
    z = points[..., 2]
    assert (z[inside] >= np.float32(near)).all() and (z[inside] <= np.float32(far)).all()
    rejected = code[0].cpu().numpy() != SO.OK
    assert rejected.any() and not points[rejected].any()                       # a rejected pixel is depth 0: the origin, which every consumer drops
    K = torch.tensor([[fx, 0.0, cx], [0.0, fx, cy], [0.0, 0.0, 1.0]])
    vol = TsdfVolume(K, (32, 16, 16), 0.03, (-0.48, -0.24, 0.76), min_depth=0.1, max_depth=5.0).to(DEV)
    vol.integrate(depth, torch.eye(3, device=DEV)[None], torch.zeros(1, 3, device=DEV))
    tsdf, weight = vol.volume[0, ..., 0].cpu().numpy(), vol.volume[0, ..., 1].cpu().numpy()
    seen = weight > 0
    assert seen.sum() > 500 and (tsdf[seen] > 0).any() and (tsdf[seen] < 0).any()     # voxels in front of the plane and behind it
    zs = np.nonzero(seen & (np.abs(tsdf) < 0.25))[0]                           # the z index of the voxels next to the surface
    assert len(zs) > 0 and 0.76 + zs.min() * 0.03 <= far and near <= 0.76 + (zs.max() + 1) * 0.03


def test_census_aggregate_select_and_depth_replay_from_one_graph():
    sets = [gpu(*SO.pair(seed, 24, 150, True)) for seed in BATCH_SEEDS]
    sets = [(l[None], r[None]) for l, r in sets]
    m = StereoMatcher(max_disparity=128)

    def run(l, r):
        disparity, code = m(l, r)
        return disparity, code, m.depth(disparity, 50.0, 2.0)
    eager = [[x.clone() for x in run(*s)] for s in sets]
    static = [x.clone() for x in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(*static)
    for i in (1, 2, 0):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[i]), i
    want = SO.case(BATCH_SEEDS[0], 24, 150, True, 128, 8)
    assert np.array_equal(out[0][0].cpu().numpy().view(np.uint32), want["disparity"].view(np.uint32))
