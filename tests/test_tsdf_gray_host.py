"""K22 TSDF intensity without a GPU: the host-side argument checks of the three entries (MI_E_* before any launch), the Python
module's constructor and its refusal of CPU tensors, the export through the `pytorch_model` alias, the numpy oracle's own
sanity, and the kernels' arithmetic (csrc/tsdf_gray_math.h) compiled as plain C++ in tests/native/tsdf_gray_host.cpp.

Bounds.  The joint voxel update and the gather are float32 in the header's order, which the oracle's float32 run reproduces
operation by operation: compared bit for bit.
The oracle's own sanity is the experiment the feature rests on: photo_oracle.scene("plane", seed, h, w), frame 1 fused at the
identity into ROOM, frame 2 tracked from the identity as prediction (the true motion is 2.0 deg and 4.5 - 4.8 cm).  K19's
tracking (tsdf_oracle.track) is not ok with 0 steps on all six scenes, in float64 and in float32; direct tracking is ok with 14
steps in both, with equal counts in both.  Its distance from the truth (float64 run; deg, m) and the float32 run's distance
from the float64 run (deg, m):
    (48, 64)    seed 0  1.8643e-2  6.8776e-4   4.0753e-7  7.8572e-9      counts 2452 + 2624
                seed 1  1.2932e-2  7.4820e-4   7.9474e-7  2.8515e-8      counts 2441 + 2651
                seed 2  1.5486e-2  9.1242e-4   3.1529e-6  1.0139e-7      counts 2452 + 2650
    (120, 160)  seed 0  2.4718e-2  8.5116e-4   1.0023e-6  2.0508e-8      counts 15505 + 17123
                seed 1  2.9137e-2  9.4596e-4   3.7049e-6  1.2110e-7      counts 15493 + 17155
                seed 2  2.6599e-2  8.8594e-4   2.8320e-6  9.8842e-8      counts 15509 + 17247
Every raycast hit gets an intensity (0.902 of the pixels at (48, 64), 0.912 at (120, 160)); its median deviation from the frame
that was fused is 1.689 and 1.104 gray levels."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as IO
import photo_oracle as PO
import tsdf_gray_oracle as GO
import tsdf_oracle as TO
from helpers import host_program, run_records as run
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import rgbd_camera

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
# (h, w), seed -> (deg, m) of the float64 oracle from the truth, (deg, m) of the float32 run from the float64 run
TRACK = {((48, 64), 0): (1.8643e-2, 6.8776e-4, 4.0753e-7, 7.8572e-9), ((48, 64), 1): (1.2932e-2, 7.4820e-4, 7.9474e-7, 2.8515e-8),
         ((48, 64), 2): (1.5486e-2, 9.1242e-4, 3.1529e-6, 1.0139e-7), ((120, 160), 0): (2.4718e-2, 8.5116e-4, 1.0023e-6, 2.0508e-8),
         ((120, 160), 1): (2.9137e-2, 9.4596e-4, 3.7049e-6, 1.2110e-7), ((120, 160), 2): (2.6599e-2, 8.8594e-4, 2.8320e-6, 9.8842e-8)}
HITS = {(48, 64): (0.902, 1.689), (120, 160): (0.912, 1.104)}             # share of raycast hits, median |I_model - gray| of them


@pytest.fixture(scope="module")
def lib():
    return N.load()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


def volume_refusals(call):
    """the checks every volume entry shares; call(**kw) overrides batch, nz, ny, nx, ivol"""
    assert call(batch=0) == SHAPE and call(nz=1) == SHAPE and call(ny=1) == SHAPE and call(nx=1) == SHAPE and call(nx=-3) == SHAPE
    assert call(batch=2, nz=1024, ny=1024, nx=1024) == SHAPE and call(batch=8, nz=512, ny=512, nx=1024) == SHAPE    # >= 2^31 voxels
    assert call(batch=65535, nz=32, ny=32, nx=33) == SHAPE and call(batch=65536, nz=2, ny=2, nx=2) == PARAM
    assert call(ivol=None) == NULL


def test_abi_version_is_unchanged(lib):
    assert lib.mi_abi_version() == 3


def test_gray_reset_argument_checks(lib, p):
    f = lib.mi_tsdf_gray_reset

    def call(**kw):
        a = dict(batch=2, nz=56, ny=44, nx=72, ivol=p)
        a.update(kw)
        return f(a["ivol"], a["batch"], a["nz"], a["ny"], a["nx"], None)
    volume_refusals(call)
    assert call(ivol=p + 8) == ALIGN and call(ivol=p + 4) == ALIGN


def test_integrate_gray_argument_checks(lib, p):
    f = lib.mi_tsdf_integrate_gray
    good = [p, p, 2, 56, 44, 72, -2.25, -1.75, 0.5, 0.0625, 0.25, 64.0, p, 0, p, 0, 4, 48, 64, 50.0, 50.0, 32.0, 24.0, 1.0, 0.1, 10.0, p,
            p, None, None]
    for i in (0, 1, 12, 14, 26, 27):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=2, nz=56, ny=44, nx=72, o=(-2.25, -1.75, 0.5), vs=0.0625, trunc=0.25, mw=64.0, vol=p, ivol=p, u16=0, u8=0, frames=4,
                 h=48, w=64, fx=50.0, fy=50.0, cx=32.0, cy=24.0, zs=1.0, lo=0.1, hi=10.0, active=p)
        a.update(kw)
        return f(a["vol"], a["ivol"], a["batch"], a["nz"], a["ny"], a["nx"], *a["o"], a["vs"], a["trunc"], a["mw"], p, a["u16"], p, a["u8"],
                 a["frames"], a["h"], a["w"], a["fx"], a["fy"], a["cx"], a["cy"], a["zs"], a["lo"], a["hi"], p, p, a["active"], None)
    volume_refusals(call)
    assert call(vol=None) == NULL
    assert call(frames=0) == SHAPE and call(frames=-1) == SHAPE and call(h=2) == SHAPE and call(w=2) == SHAPE
    assert call(batch=4, nz=2, ny=2, nx=2, frames=8, h=8192, w=8192) == SHAPE                                 # batch frames h w >= 2^31
    for kw in (dict(o=(NAN, 0.0, 0.0)), dict(o=(0.0, INF, 0.0)), dict(o=(0.0, 0.0, -INF)), dict(vs=0.0), dict(vs=-1.0), dict(vs=NAN),
               dict(vs=INF), dict(trunc=0.0), dict(trunc=INF), dict(trunc=NAN), dict(mw=0.0), dict(mw=-2.0), dict(mw=INF), dict(mw=NAN),
               dict(fx=0.0), dict(fy=INF), dict(cx=NAN), dict(cy=INF), dict(zs=0.0), dict(zs=INF), dict(lo=0.0), dict(lo=NAN),
               dict(hi=0.05), dict(hi=INF)):
        assert call(**kw) == PARAM, kw
    assert call(vol=p + 8) == ALIGN and call(ivol=p + 8) == ALIGN and call(ivol=p + 4, u16=1, u8=1, active=None) == ALIGN


def test_sample_gray_argument_checks(lib, p):
    f = lib.mi_tsdf_sample_gray
    good = [p, 2, 56, 44, 72, -2.25, -1.75, 0.5, 0.0625, p, 3072, p, p, p, None]
    for i in (0, 9, 11, 12, 13):                         # the volume, the points, r without t, t without r, the output
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=2, nz=56, ny=44, nx=72, o=(-2.25, -1.75, 0.5), vs=0.0625, ivol=p, pts=p, n=3072, r=p, t=p, out=p)
        a.update(kw)
        return f(a["ivol"], a["batch"], a["nz"], a["ny"], a["nx"], *a["o"], a["vs"], a["pts"], a["n"], a["r"], a["t"], a["out"], None)
    volume_refusals(call)
    assert call(n=0) == SHAPE and call(n=-5) == SHAPE and call(n=2 ** 30) == SHAPE and call(batch=1, n=2 ** 31 - 1, ivol=None) == NULL
    assert call(batch=4, nz=2, ny=2, nx=2, n=2 ** 29) == SHAPE
    for kw in (dict(o=(NAN, 0.0, 0.0)), dict(o=(0.0, -INF, 0.0)), dict(vs=0.0), dict(vs=-1.0), dict(vs=INF), dict(vs=NAN)):
        assert call(**kw) == PARAM, kw
    assert call(ivol=p + 8) == ALIGN and call(pts=p + 4) == ALIGN and call(out=p + 8) == ALIGN
    assert call(r=None, t=None, out=p + 8) == ALIGN                                     # no pose is a legal request


def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import DirectTsdfVolume, TsdfVolume
    Kt = torch.from_numpy(rgbd_camera(48, 64))
    m = DirectTsdfVolume(Kt, (72, 44, 56), 0.0625, (-2.25, -1.75, 0.5))
    assert isinstance(m, TsdfVolume) and (m.photo_weight, m.intensity_threshold) == (0.003, 30.0)
    assert (m.dims, m.batch, m.voxel_size, m.origin, m.truncation, m.max_weight, m.step_fraction) == \
        ((72, 44, 56), 1, 0.0625, (-2.25, -1.75, 0.5), 0.25, 64.0, 0.5)
    assert tuple(m.intensity.shape) == (1, 56, 44, 72, 2) and m.intensity.dtype == torch.float32
    assert {"volume", "intensity"} <= set(dict(m.named_buffers())) and not bool(m.intensity.any())          # born empty
    assert bool((m.volume[..., 0] == 1).all()) and not bool(m.volume[..., 1].any())
    m3 = DirectTsdfVolume(Kt, (2, 2, 2), 1.0, (0, 0, 0), truncation=0.5, batch=3, size=(48, 64), photo_weight=0.0, intensity_threshold=5)
    assert tuple(m3.intensity.shape) == (3, 2, 2, 2, 2) and m3.photo_weight == 0.0 and m3.intensity_threshold == 5.0
    base = dict(dims=(8, 8, 8), voxel_size=0.1, origin=(0.0, 0.0, 0.0))
    for kw in (dict(photo_weight=-0.001), dict(photo_weight=NAN), dict(photo_weight=INF), dict(intensity_threshold=0.0),
               dict(intensity_threshold=-1.0), dict(intensity_threshold=INF), dict(intensity_threshold=NAN),
               dict(dims=(8, 1, 8)), dict(voxel_size=0.0), dict(truncation=0.0), dict(batch=0), dict(schedule=())):     # and the parent's
        with pytest.raises(ValueError):
            DirectTsdfVolume(Kt, **{**base, **kw})
    eye, zero, depth, gray = torch.eye(3)[None], torch.zeros(1, 3), torch.ones(1, 48, 64), torch.ones(1, 48, 64)
    for call in (m.reset, lambda: m.integrate(depth, gray, eye, zero), lambda: m.raycast(eye, zero, (48, 64)),
                 lambda: m.track(depth, gray, eye, zero), lambda: m(depth, gray, eye, zero), m.extract_surface, m.extract_points):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match=r"\(1, H, W\)"):
        m.integrate(torch.ones(2, 48, 64), torch.ones(2, 48, 64), eye, zero)
    with pytest.raises(RuntimeError, match="depth's shape"):
        m.integrate(depth, torch.ones(1, 48, 63), eye, zero)
    with pytest.raises(RuntimeError, match="depth's shape"):
        m.track(depth, torch.ones(1, 47, 64), eye, zero)
    vol = torch.zeros(1, 4, 4, 4, 2)
    for call in (lambda: ops.tsdf_gray_reset(vol),
                 lambda: ops.tsdf_integrate_gray(vol, vol.clone(), depth[None], gray[None], eye[None], zero[None], (50.0, 50.0, 32.0, 24.0),
                                                 (0, 0, 0), 0.1, 0.4),
                 lambda: ops.tsdf_sample_gray(vol, torch.ones(1, 5, 4), (0, 0, 0), 0.1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import DirectTsdfVolume
    assert DirectTsdfVolume is real.DirectTsdfVolume and "DirectTsdfVolume" in real.__all__
    from pytorch_model.geometry.direct_tsdf_volume import DirectTsdfVolume as again
    assert again is DirectTsdfVolume and issubclass(DirectTsdfVolume, real.TsdfVolume)


# ---- the oracle's own sanity --------------------------------------------------------------------------------------------------------

def test_oracle_integration_basics():
    h, w = 48, 64
    dims, grid = TO.grid_of(TO.ROOM)
    cam = TO.camera(h, w)[0]
    depth, R, t = TO.views(h, w)
    gray = GO.views_gray(h, w)
    empty = GO.reset(dims)
    assert not empty[0].any() and not empty[1].any() and empty[0].shape == (56, 44, 72)
    vol, ivol = GO.fused_room(h, w)
    # the (tsdf, weight) half is tsdf_oracle's; gray lives in the truncation band alone, where it is a mean of the frames' values
    ref = TO.fused_room(h, w)
    assert np.array_equal(vol[0], ref[0]) and np.array_equal(vol[1], ref[1])
    seen = ivol[1] > 0
    assert 0.02 < seen.mean() < 0.5 and not seen[vol[1] == 0].any() and (vol[1][seen] >= ivol[1][seen]).all()
    assert (vol[0][seen] < 1).all() or (np.abs(vol[0][seen]) <= 1).all()
    assert not ivol[0][~seen].any() and gray.min() - 1e-9 <= ivol[0][seen].min() and ivol[0][seen].max() <= gray.max() + 1e-9
    assert (vol[1] > ivol[1]).any()                                                         # free space in front: tsdf alone
    # four frames in one call are four calls of one; a masked frame is a frame left out; NaN gray leaves the record alone
    step = (TO.reset(dims), empty)
    for f in range(4):
        step = GO.integrate(*step, depth[f:f + 1], gray[f:f + 1], R[f:f + 1], t[f:f + 1], cam, grid)
    assert all(np.array_equal(a, b) for x, y in zip(step, (vol, ivol)) for a, b in zip(x, y))
    masked = GO.integrate(TO.reset(dims), empty, depth, gray, R, t, cam, grid, active=[1, 0, 1, 1])
    three = GO.integrate(TO.reset(dims), empty, depth[[0, 2, 3]], gray[[0, 2, 3]], R[[0, 2, 3]], t[[0, 2, 3]], cam, grid)
    assert all(np.array_equal(a, b) for x, y in zip(masked, three) for a, b in zip(x, y))
    blind = GO.integrate(TO.reset(dims), empty, depth, np.full_like(gray, np.nan), R, t, cam, grid)
    assert np.array_equal(blind[0][0], vol[0]) and not blind[1][0].any() and not blind[1][1].any()
    # the float32 run has the float64 run's weights on every voxel
    v32, i32 = GO.fused_room(h, w, dtype=F32)
    assert np.array_equal(i32[1], ivol[1]) and np.array_equal(v32[1], vol[1]) and np.abs(i32[0] - ivol[0]).max() < 1e-3


def test_oracle_sampler_basics():
    dims, grid = TO.grid_of(TO.ROOM)
    ivol = GO.synthetic(dims)
    pts, names = GO.hand_points(dims, grid)
    I, ok = GO.sample(ivol, pts[:, :3], pts[:, 3], grid, dtype=F32)
    row = {n: i for i, n in enumerate(names)}
    want = {"g = 0": True, "g = n - 1": True, "below": False, "above": False, "far outside": False, "nan": False, "inf": False,
            "f = 0": False, "no observed corner": False, "some observed corners": True}
    for name, valid in want.items():
        assert ok[row[name]] == valid, name
    assert ok[row["f = -1"]] == ok[row["f = 2"]] and I[row["f = -1"]] == I[row["f = 2"]]
    assert I[row["g = 0"]] == ivol[0][0, 0, 0] and I[row["g = n - 1"]] == ivol[0][-1, -1, -1]            # a corner voxel's own value
    assert 0.3 < ok[len(names):].mean() < 0.9 and not I[~ok].any()
    # an observed voxel's centre returns its gray value whatever its neighbours hold; a constant volume returns the constant
    k, j, i = np.argwhere(ivol[1] > 0)[1234]
    c = (np.array([i, j, k]) + 0.5) * grid[1] + grid[0].astype(F64)
    I1, ok1 = GO.sample(ivol, c[None], [1.0], grid)
    assert ok1[0] and abs(I1[0] - ivol[0][k, j, i]) < 1e-9
    flat = (np.full_like(ivol[0], 93.0) * (ivol[1] > 0), ivol[1])
    I2, ok2 = GO.sample(flat, pts[:, :3], pts[:, 3], grid)
    assert np.array_equal(ok2, ok) and np.abs(I2[ok2] - 93.0).max() < 1e-9
    # with a pose: the camera-frame points of the world points give the same samples
    R, t = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), np.array([0.5, -0.25, 1.0])     # a quarter turn: exact
    fin = np.isfinite(pts[:, :3]).all(1)
    cam_pts = pts[fin, :3].astype(F64) @ R.T + t
    I3, ok3 = GO.sample(ivol, cam_pts, pts[fin, 3], grid, R, t)
    I4, ok4 = GO.sample(ivol, pts[fin, :3], pts[fin, 3], grid)
    inner = ~np.isin(np.flatnonzero(fin), [row[n] for n in ("g = 0", "g = n - 1", "last x layer", "below", "above")])
    assert np.array_equal(ok3[inner], ok4[inner]) and np.abs(I3 - I4)[inner & ok4].max() < 1e-9


@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_direct_tracking_moves_where_k19_is_frozen(h, w, seed):
    res = {}
    for T in (F64, F32):
        vol, ivol, grid, s = GO.plane_model(seed, h, w, dtype=T)
        R19, t19, o19 = TO.track(vol, grid, s["depth2"], np.eye(3), np.zeros(3), h, w, dtype=T)
        assert not o19["ok"] and o19["steps"] == 0, T                                    # K19: frozen on the plane
        R, t, o = GO.track(vol, ivol, grid, s["depth2"], s["gray2"], np.eye(3), np.zeros(3), h, w, dtype=T)
        assert o["ok"] and o["steps"] == 14, T
        res[T] = (np.asarray(R, F64), np.asarray(t, F64), o)
    (R64, t64, o64), (R32, t32, o32) = res[F64], res[F32]
    assert (o32["count"], o32["count_photo"]) == (o64["count"], o64["count_photo"])
    rot, tr = IO.rotation_angle_deg_small(R64, s["R"]), float(np.abs(t64 - s["t"]).max())
    drot, dtr = IO.rotation_angle_deg_small(R32, R64), float(np.abs(t32 - t64).max())
    print(f"plane {h} x {w} seed {seed}: counts {o64['count']} + {o64['count_photo']}; truth {rot:.4e} deg {tr:.4e} m; float32 from "
          f"float64 {drot:.4e} deg {dtr:.4e} m")
    want = TRACK[(h, w), seed]
    assert rot <= want[0] * 1.001 and tr <= want[1] * 1.001 and drot <= want[2] * 1.01 + 1e-9 and dtr <= want[3] * 1.01 + 1e-10
    assert rot < 0.05 and tr < 2e-3                                                      # of a motion of 2.0 deg and 4.5 - 4.8 cm
    # every raycast hit has an intensity, close to the frame that was fused
    vol, ivol, grid, s = GO.plane_model(seed, h, w)
    maps1, int1 = GO.raycast(vol, ivol, np.eye(3), np.zeros(3), TO.camera(h, w)[1], h, w, grid)
    assert np.array_equal(int1[1], maps1[1]) and abs(maps1[1].mean() - HITS[h, w][0]) < 2e-3
    assert abs(np.median(np.abs(int1[0][..., 0] - s["gray1"])[int1[1]]) - HITS[h, w][1]) < 2e-3 and not int1[0][..., 1:].any()


# ---- the kernels' arithmetic on the host ----------------------------------------------------------------------------------------

# tests/native/tsdf_gray_host.cpp around csrc/tsdf_gray_math.h, compiled as plain C++ (no HIP)
gray_host = host_program("tsdf_gray_host.cpp", hip=False)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def test_native_voxel_update_is_the_float32_oracles(gray_host):
    h, w = 37, 53
    dims, grid = TO.grid_of(TO.ODD)
    cam = TO.camera(h, w)[0]
    depth, R, t = TO.views(h, w)
    depth, gray = depth.copy(), GO.views_gray(h, w).copy()
    depth[2, 18, 26], depth[2, 18, 27], depth[2, 19, 26], depth[2, 19, 27], depth[2, 20, 26] = np.nan, np.inf, 0.0, 0.0999, 10.001
    gray[2, 17, 20:30], gray[2, 21, 26] = np.nan, np.inf
    before = GO.integrate(TO.reset(dims, F32), GO.reset(dims, F32), depth[:2], gray[:2], R[:2], t[:2], cam, grid, max_weight=2.0, dtype=F32)
    after = GO.integrate(*before, depth[2:3], gray[2:3], R[2:3], t[2:3], cam, grid, max_weight=2.0, dtype=F32)
    nx, ny, nz = dims
    vox = [(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)]
    R32, t32 = R[2].astype(F32), t[2].astype(F32)
    proj = run(gray_host, ["project"], [[i, j, k, grid[1], *grid[0], *R32.ravel(), *t32, *cam, w, h] for i, j, k in vox])
    (bt, bw), (bg, bgw) = before
    recs, where = [], []
    for (i, j, k), o in zip(vox, proj):
        if o[0]:
            y, x = int(o[2]), int(o[1])
            recs.append([depth[2, y, x], 1.0, TO.MIN_DEPTH, TO.MAX_DEPTH, o[3], grid[2], 2.0, bt[k, j, i], bw[k, j, i], gray[2, y, x],
                         bg[k, j, i], bgw[k, j, i]])
            where.append((k, j, i))
    assert 0.3 * len(vox) < len(recs) < len(vox)                                    # part of the volume is outside the frame
    out = np.array(run(gray_host, ["fuse"], recs))
    got = [x.copy() for x in (bt, bw, bg, bgw)]
    idx = tuple(np.array(where).T)
    for c, arr in enumerate(got):
        arr[idx] = out[:, 2 + c].astype(F32)
    (at, aw), (ag, agw) = after
    assert same(got[0], at) and same(got[1], aw) and same(got[2], ag) and same(got[3], agw)
    fused, updated = out[:, 0].astype(bool), out[:, 1].astype(bool)
    assert 0 < updated.sum() < fused.sum() < len(out) and not updated[~fused].any()
    assert agw.max() == 2 and (agw != bgw).any() and (ag != bg).any()
    # one by one: (d, z_scale, min, max, qz, truncation, max_weight, tsdf, weight, g, gray, gweight)
    base = [2.0, 1.0, 0.1, 10.0, 2.1, 0.25, 64.0, 0.5, 3.0, 100.0, 40.0, 3.0]

    def case(**kw):
        a = list(base)
        for k, v in kw.items():
            a[dict(d=0, zs=1, qz=4, mw=6, g=9, gw=11)[k]] = v
        return a
    o = run(gray_host, ["fuse"], [case(), case(g=np.nan), case(g=np.inf), case(g=-np.inf), case(d=np.nan), case(qz=2.2501), case(qz=2.25),
                                  case(qz=1.75), case(qz=1.7499), case(gw=64.0), case(d=2000.0, zs=0.001, qz=1.9)])
    mean = F32((F32(40) * F32(3) + F32(100)) / F32(4))
    assert list(o[0]) == [1, 1, o[0][2], 4, mean, 4]
    for r in o[1:4]:                                                                # gray not finite: K19's update alone
        assert list(r) == [1, 0, o[0][2], 4, 40, 3]
    for r in o[4:6]:                                                                # no depth update: nothing at all
        assert list(r) == [0, 0, 0.5, 3, 40, 3]
    assert list(o[6][:2]) == [1, 1] and o[6][4] == mean                             # sdf = -truncation: the band's far end
    assert list(o[7][:2]) == [1, 1] and o[7][4] == mean                             # sdf = +truncation: the band's near end
    assert list(o[8]) == [1, 0, F32((F32(0.5) * F32(3) + F32(1)) / F32(4)), 4, 40, 3]          # free space: tsdf alone
    assert list(o[9][:2]) == [1, 1] and o[9][5] == 64                                # the weight's cap
    assert list(o[10][:2]) == [1, 1] and o[10][4] == mean                            # sdf = 0.1 with a depth scale


def test_native_sampler_is_the_float32_oracles(gray_host, tmp_path):
    from onnx_image_processing_amd.synth import synth_depth_room
    h, w = 37, 53
    ki = TO.camera(h, w)[1]
    _, Rv, tv = TO.views(h, w)
    R32, t32 = Rv[3].astype(F32), tv[3].astype(F32)
    eye = [*np.eye(3).ravel(), 0, 0, 0]
    for spec in (TO.ROOM, TO.ODD, TO.TINY):
        dims, grid = TO.grid_of(spec)
        nx, ny, nz = dims
        path = str(tmp_path / "intensity.bin")
        args = ["sample", path, str(nx), str(ny), str(nz)]
        pts, names = GO.hand_points(dims, grid)
        # hand-placed world points on the synthetic volume, on one with a single observed record, and on an empty one
        one = GO.reset(dims, F32)
        one[0][1, 0, 1], one[1][1, 0, 1] = 77.5, 3.0
        for ivol in (GO.synthetic(dims), one, GO.reset(dims, F32)):
            np.stack(ivol, axis=-1).astype(F32).tofile(path)
            I, ok = GO.sample(ivol, pts[:, :3], pts[:, 3], grid, dtype=F32)
            out = np.array(run(gray_host, args, [[0, *pt, *grid[0], grid[1], *eye] for pt in pts]))
            assert np.array_equal(out[:, 0].astype(bool), ok) and same(out[:, 1], I), spec
            # the same records read as camera-frame points under a pose
            I, ok = GO.sample(ivol, pts[:, :3], pts[:, 3], grid, R32, t32, dtype=F32)
            out = np.array(run(gray_host, args, [[1, *pt, *grid[0], grid[1], *R32.ravel(), *t32] for pt in pts]))
            assert np.array_equal(out[:, 0].astype(bool), ok) and same(out[:, 1], I), spec
        assert GO.sample(one, pts[:, :3], pts[:, 3], grid, dtype=F32)[1].any() and not ok.any()
        # the raycast's vertex map on the fused room: the model's intensity map
        vol, ivol = GO.fused_room(h, w, spec, F32)
        np.stack(ivol, axis=-1).astype(F32).tofile(path)
        maps, (rec, ok) = GO.raycast(vol, ivol, R32, t32, ki, h, w, grid, dtype=F32)
        v = maps[0].reshape(-1, 3)
        out = np.array(run(gray_host, args, [[1, *vv, f, *grid[0], grid[1], *R32.ravel(), *t32] for vv, f in zip(v, maps[1].ravel())]))
        assert np.array_equal(out[:, 0].astype(bool), ok.ravel()) and same(out[:, 1], rec[..., 0].ravel()), spec
        assert ok.any() and not ok[~maps[1]].any()
        if spec is not TO.TINY:
            assert ok.sum() > 0.9 * maps[1].sum()
