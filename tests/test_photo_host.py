"""K21 direct RGB-D refinement without a GPU: the kernels' arithmetic (csrc/photo_math.h) compiled as plain C++ in
tests/native/photo_host.cpp against tests/photo_oracle.py, the host-side argument checks of the four entries (MI_E_* before
any launch), the Python module's constructor and its refusal of CPU tensors, and the oracle's own behaviour on the textured
plane, which is what the feature is for.

Bounds.  Records, footprints, gates, rows and residuals are float32 in the header's order, which numpy's float32 run
reproduces operation by operation: compared bit for bit over a whole 37 x 53 frame.  The joint sums are one float64 multiply
and add per entry in both: equal bits; the solve is compared to the limits of tests/test_icp_host.py (pivot ratio 1e-9
relative, residual |A x + b| <= 1e-9 |b|, x to 1e-12 relative for a well-conditioned system).

The oracle's anchors, float64, default schedule from identity on the textured plane (rotation 2 deg, translation 5 cm):
icp_oracle.refine is frozen at step 0 on every seed; the joint oracle applies all 14 steps and ends at
  (48, 64):   4.619e-3 / 3.032e-3 / 9.901e-4 deg and 6.858e-5 / 3.863e-5 / 3.081e-5 m from the truth (seeds 0 1 2)
  (120, 160): 5.524e-4 / 2.389e-4 / 3.816e-4 deg and 2.474e-5 / 1.517e-5 / 5.606e-6 m
with its smallest pivot ratio 1.2e-2.  tests/test_gpu_direct_rgbd.py builds on these."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as IO
import photo_oracle as PO
from helpers import host_program, run_records as run
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import rgbd_camera

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
ANGLE = float(np.deg2rad(30.0))
# (deg, m) of the float64 joint oracle from the truth, seeds 0 1 2
PLANE_TRUTH = {(48, 64): ((4.619e-3, 6.858e-5), (3.032e-3, 3.863e-5), (9.901e-4, 3.081e-5)),
               (120, 160): ((5.524e-4, 2.474e-5), (2.389e-4, 1.517e-5), (3.816e-4, 5.606e-6))}


# ---- the oracle on the scene the feature is for -------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
def test_oracle_reaches_the_truth_on_the_textured_plane_where_icp_is_frozen(h, w):
    for seed in (0, 1, 2):
        s = PO.scene("plane", seed, h, w)
        k18 = IO.refine(s["maps1"], s["maps2"], np.eye(3), np.zeros(3), s["cam"])
        assert not k18["ok"] and k18["steps"] == 0 and k18["count"] > 0.9 * (h - 2) * (w - 2)
        o = PO.refine_scene(s)
        rot, tr = IO.rotation_angle_deg_small(o["R"], s["R"]), np.abs(o["t"] - s["t"]).max()
        print(f"textured plane {h} x {w} seed {seed}: {rot:.3e} deg {tr:.3e} m from the truth, last step {o['last_step']:.1e}, "
              f"pivot ratio {o['min_ratio']:.1e}, counts {o['count']} + {o['count_photo']}")
        assert o["ok"] and o["steps"] == 14 and o["min_ratio"] > 1e-3 and o["last_step"] < 1e-9
        want = PLANE_TRUTH[(h, w)][seed]
        assert rot <= want[0] * 1.001 and tr <= want[1] * 1.001
        assert np.allclose(o["information"], o["information"].T) and o["count_photo"] > 0.9 * (h - 2) * (w - 2)


def test_oracle_weight_zero_is_icp_and_untextured_plane_stays_frozen():
    s = PO.scene("room", 1, 48, 64)
    a = PO.refine_scene(s, weight=0.0)
    b = IO.refine(s["maps1"], s["maps2"], np.eye(3), np.zeros(3), s["cam"])
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["information"], b["information"])
    assert a["count"] == b["count"] and a["rmse"] == b["rmse"] and a["ok"] and a["count_photo"] == 0 and a["rmse_photo"] == 0.0
    p = PO.scene("plane", 0, 48, 64)
    flat = PO.intensity_maps(np.full((48, 64), 100.0, F32))
    o = PO.refine(p["maps1"], flat, p["maps2"], flat, np.eye(3), np.zeros(3), p["cam"])
    assert not o["ok"] and o["steps"] == 0 and o["count_photo"] > 2000 and o["rmse_photo"] == 0.0
    # rendering: both frames see one texture, so at the truth the residual is interpolation error only, far below the
    # residual at identity
    at_truth = PO.linearise(p["maps1"], p["int1"], p["maps2"], p["int2"], p["R"], p["t"], p["cam"])
    at_identity = PO.linearise(p["maps1"], p["int1"], p["maps2"], p["int2"], np.eye(3), np.zeros(3), p["cam"])
    rms = [np.sqrt(x[27] / x[28]) for x in (at_truth, at_identity)]
    assert at_truth[28] > 0.85 * 48 * 64 and rms[0] < 1.0 and rms[1] > 10 * rms[0]
    u8 = PO.scene("plane", 0, 48, 64, u8=True)
    assert u8["gray1"].dtype == np.uint8 and np.abs(u8["gray1"].astype(F64) - p["gray1"]).max() <= 0.5


# ---- argument checks and the module ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    return N.load()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


def test_intensity_maps_and_workspace_argument_checks(lib, p):
    f, wb = lib.mi_intensity_maps, lib.mi_rgbd_workspace_bytes
    assert f(None, 0, 2, 48, 64, p, None) == NULL and f(p, 0, 2, 48, 64, None, None) == NULL
    assert f(p, 1, 0, 48, 64, p, None) == SHAPE and f(p, 1, 2, 2, 64, p, None) == SHAPE and f(p, 0, 2, 48, 2, p, None) == SHAPE
    assert f(p, 0, 4, 32768, 16384, p, None) == SHAPE and f(p, 0, 65536, 3, 3, p, None) == PARAM
    assert f(p, 0, 2, 48, 64, p + 4, None) == ALIGN
    need = wb(3, 120, 160)
    assert need >= 3 * (12 * 8 + 2 * 10 * 256 + 8) and need % 16 == 0        # poses, 2 x 10 slab records of 256 bytes, two words
    assert need > lib.mi_icp_workspace_bytes(3, 120, 160)
    assert wb(0, 120, 160) == 0 and wb(3, 2, 160) == 0 and wb(3, 120, 2) == 0 and wb(65536, 3, 3) == 0 and wb(4, 32768, 16384) == 0


def test_photo_linearise_argument_checks(lib, p):
    f, need = lib.mi_photo_linearise, lib.mi_rgbd_workspace_bytes(3, 120, 160)
    good = [p, p, p, p, p, p, 3, 120, 160, 125.0, 125.0, 80.0, 60.0, 1, 0.1, 30.0, p, p, need, None]
    for i in (0, 1, 2, 3, 4, 5, 16, 17):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=3, h=120, w=160, fx=125.0, cy=60.0, stride=1, dist=0.1, thr=30.0, ws=p, wbytes=need, v1=p, g2=p)
        a.update(kw)
        return f(a["v1"], p, p, a["g2"], p, p, a["batch"], a["h"], a["w"], a["fx"], 125.0, 80.0, a["cy"], a["stride"], a["dist"],
                 a["thr"], p, a["ws"], a["wbytes"], None)
    assert call(batch=0) == SHAPE and call(h=2) == SHAPE and call(w=0) == SHAPE and call(batch=70000, h=3, w=3) == PARAM
    for s in (0, 3, 5, 16, -1):
        assert call(stride=s) == PARAM, s
    for s in (1, 2, 4, 8):
        assert call(stride=s, wbytes=need - 1) == CAPACITY, s             # every other check passed
    assert call(fx=0.0) == PARAM and call(cy=float("inf")) == PARAM and call(dist=0.0) == PARAM and call(dist=float("nan")) == PARAM
    assert call(thr=0.0) == PARAM and call(thr=-1.0) == PARAM and call(thr=float("inf")) == PARAM and call(thr=float("nan")) == PARAM
    assert call(ws=p + 4) == ALIGN and call(v1=p + 4) == ALIGN and call(g2=p + 8) == ALIGN


def test_rgbd_refine_argument_checks(lib, p):
    f, need = lib.mi_rgbd_refine, lib.mi_rgbd_workspace_bytes(2, 48, 64)

    def arr(*v):
        a = (ctypes.c_int32 * len(v))(*v)
        p_keepalive.append(a)
        return ctypes.cast(a, ctypes.c_void_p)
    st, it = arr(4, 2, 1), arr(4, 4, 6)
    good = [p] * 8 + [2, 48, 64, 50.0, 50.0, 32.0, 24.0, st, it, 3, 0.1, ANGLE, 0.003, 30.0, 64] + [p] * 10 + [need, None]
    for i in list(range(8)) + [15, 16] + list(range(23, 33)):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=2, h=48, st=st, it=it, stages=3, dist=0.1, ang=ANGLE, wt=0.003, thr=30.0, minc=64, ws=p, wbytes=need, g1=p, n2=p)
        a.update(kw)
        return f(p, p, a["g1"], p, a["n2"], p, p, p, a["batch"], a["h"], 64, 50.0, 50.0, 32.0, 24.0, a["st"], a["it"], a["stages"],
                 a["dist"], a["ang"], a["wt"], a["thr"], a["minc"], p, p, p, p, p, p, p, p, p, a["ws"], a["wbytes"], None)
    assert call(wbytes=need - 1) == CAPACITY and call(wbytes=lib.mi_icp_workspace_bytes(2, 48, 64)) == CAPACITY
    assert call(ws=p + 8) == ALIGN and call(g1=p + 4) == ALIGN and call(n2=p + 8) == ALIGN
    assert call(batch=0) == SHAPE and call(h=1) == SHAPE and call(batch=65536) == PARAM
    assert call(stages=0) == PARAM and call(stages=5) == PARAM and call(minc=0) == PARAM
    assert call(st=arr(4, 3, 1)) == PARAM and call(it=arr(4, -1, 6)) == PARAM and call(it=arr(30, 30, 5)) == PARAM
    assert call(it=arr(30, 30, 4), wbytes=0) == CAPACITY and call(it=arr(0, 0, 0), wbytes=0) == CAPACITY
    assert call(dist=float("nan")) == PARAM and call(ang=4.0) == PARAM
    assert call(wt=-0.001) == PARAM and call(wt=float("inf")) == PARAM and call(wt=float("nan")) == PARAM
    assert call(wt=0.0, wbytes=0) == CAPACITY                                                         # weight 0: legal
    assert call(thr=0.0) == PARAM and call(thr=float("inf")) == PARAM and call(thr=float("nan")) == PARAM


def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import DenseRgbdRefiner, DirectRgbdRefiner
    from pytorch_model.geometry.direct_rgbd import DirectRgbdRefiner as again
    assert DirectRgbdRefiner is real.DirectRgbdRefiner and again is DirectRgbdRefiner and "DirectRgbdRefiner" in real.__all__
    Kt = torch.from_numpy(rgbd_camera(48, 64))
    m = DirectRgbdRefiner(Kt)
    assert (m.photo_weight, m.intensity_threshold, m.schedule, m.distance_threshold, m.min_correspondences) == \
        (0.003, 30.0, ((4, 4), (2, 4), (1, 6)), 0.1, 64)
    assert isinstance(m, DenseRgbdRefiner) and m.camera == (50.0, 50.0, 32.0, 24.0)
    assert DirectRgbdRefiner(Kt, photo_weight=0.0).photo_weight == 0.0
    for kw in (dict(photo_weight=-1.0), dict(photo_weight=float("nan")), dict(photo_weight=float("inf")), dict(intensity_threshold=0.0),
               dict(intensity_threshold=float("inf")), dict(intensity_threshold=float("nan")), dict(schedule=((3, 1),)),
               dict(distance_threshold=0.0)):
        with pytest.raises(ValueError):
            DirectRgbdRefiner(Kt, **kw)
    for shape in ((2, 48, 64), (2, 1, 48, 64), (48, 64)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(torch.ones(shape), torch.ones(shape), torch.ones(shape), torch.ones(shape))
    with pytest.raises(RuntimeError, match=r"\(B, H, W\) or \(B, 1, H, W\)"):
        m(torch.ones(2, 48, 64), torch.ones(2, 3, 48, 64), torch.ones(2, 48, 64), torch.ones(2, 3, 48, 64))
    maps = (torch.zeros(1, 48, 64, 4),) * 3
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.intensity_maps(torch.ones(1, 48, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.photo_linearise(*maps, maps[0], torch.eye(3)[None], torch.zeros(1, 3), (50.0, 50.0, 32.0, 24.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rgbd_refine(maps, maps, torch.eye(3)[None], torch.zeros(1, 3), (50.0, 50.0, 32.0, 24.0))


# ---- the kernels' arithmetic on the host ----------------------------------------------------------------------------------------

# tests/native/photo_host.cpp around csrc/photo_math.h, compiled as plain C++ (no HIP)
photo_host = host_program("photo_host.cpp", hip=False)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
def test_native_record_is_the_float32_oracles(photo_host, u8):
    h, w = 37, 53
    g = PO.scene("room", 1, h, w, u8=u8)["gray1"].copy()
    if not u8:
        g[5, 7], g[20, 30], g[h - 2, w - 2] = np.nan, np.inf, -np.inf
    rec, ok = PO.intensity_maps(g, dtype=F32)
    f = g.astype(F32)
    px = [(y, x) for y in range(h) for x in range(w)]

    def at(y, x):
        return f[y, x] if 0 <= y < h and 0 <= x < w else 12345.0       # outside the frame: not read by the kernel

    inner = lambda y, x: 1 <= x <= w - 2 and 1 <= y <= h - 2            # noqa: E731
    out = run(photo_host, "record", [[at(y, x), at(y, x - 1), at(y, x + 1), at(y - 1, x), at(y + 1, x), inner(y, x)] for y, x in px])
    got = np.array(out).reshape(h, w, 4)
    assert np.array_equal(got[..., 0] != 0, ok) and np.array_equal(bits(got[..., 1:]), bits(rec))
    assert not ok[0].any() and not ok[-1].any() and not ok[:, 0].any() and not ok[:, -1].any() and ok[1:-1, 1:-1].mean() > 0.98
    assert not rec[~ok].any()
    if not u8:
        for y, x in ((5, 7), (20, 30), (h - 2, w - 2)):                  # a poked value takes its four neighbours' records
            for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                assert not ok[yy, xx]
        assert ok[5, 9] and ok[7, 7]


def test_native_row_is_the_float32_oracles(photo_host):
    h, w = 37, 53
    s = PO.scene("room", 2, h, w, dtype=F32)
    (v1, vok1), (v2, vok2) = s["maps1"][:2], s["maps2"][:2]
    (rec1, gok1), (rec2, gok2) = s["int1"], s["int2"]
    cam = s["cam"]
    Rp, tp = (x.astype(F32) for x in IO.perturbed(s["R"], s["t"]))
    thr = 8.0                                                            # tight enough for the intensity gate to reject some
    J, r = PO.rows(s["maps1"], s["int1"], s["maps2"], s["int2"], Rp, tp, cam, 1, IO.DIST, thr, dtype=F32)
    src = [(y, x) for y in range(h) for x in range(w) if vok1[y, x] and gok1[y, x]]
    head = lambda y, x: [*Rp.ravel(), *tp, *v1[y, x], rec1[y, x, 0]]     # noqa: E731
    tail = [*cam, w, h, F32(IO.DIST), F32(thr)]
    # pass 1 finds each source pixel's footprint; pass 2 feeds the footprint's records and the nearest vertex
    first = run(photo_host, "row", [[*head(y, x), *([0.0] * 20), *tail] for y, x in src])
    recs = []
    for (y, x), o in zip(src, first):
        if o[0] >= 1:
            x0, y0, nx, ny = (int(z) for z in o[1:5])
            assert 0 <= x0 <= w - 2 and 0 <= y0 <= h - 2 and nx in (x0, x0 + 1) and ny in (y0, y0 + 1)
            four = [[*rec2[y0 + dy, x0 + dx], gok2[y0 + dy, x0 + dx]] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
            recs.append([*head(y, x), *four[0], *four[1], *four[2], *four[3], *v2[ny, nx], vok2[ny, nx], *tail])
    second = run(photo_host, "row", recs)
    out = np.array([o for o in second if o[0] == 2])
    gated = sum(1 for o in second if o[0] == 1)
    assert len(out) == len(r) and len(r) > 0.6 * h * w and len(first) - len(recs) >= 10 and gated > 20
    assert np.array_equal(bits(out[:, 5:11]), bits(J)) and np.array_equal(bits(out[:, 11]), bits(r))
    assert all(not o[5:].any() for o in second if o[0] != 2)             # a rejected sample adds zeros
    loose = PO.rows(s["maps1"], s["int1"], s["maps2"], s["int2"], Rp, tp, cam, 1, IO.DIST, 30.0, dtype=F32)[1]
    assert len(loose) > len(r)                                           # the intensity gate was at work


def test_native_joint_solve_matches_the_oracle(photo_host):
    systems = []
    for kind, seed in (("plane", 0), ("plane", 2), ("room", 1), ("flat", 0)):
        s = PO.scene(kind, seed, 48, 64)
        for stride in (1, 4):
            g = IO.linearise(s["maps1"], s["maps2"], np.eye(3), np.zeros(3), s["cam"], stride)
            ph = PO.linearise(s["maps1"], s["int1"], s["maps2"], s["int2"], np.eye(3), np.zeros(3), s["cam"], stride)
            systems.append((PO.PHOTO_WEIGHT, g, ph))
    (g, ph), (gr, pr) = systems[0][1:], systems[4][1:]                   # the plane, the sphere room
    few_g, few_p = gr.copy(), pr.copy()
    few_g[28], few_p[28] = 40, 23                                        # 63 in all
    enough_g = gr.copy()
    enough_g[28] = 0                                                     # the photometric count alone suffices
    nan_p = pr.copy()
    nan_p[5] = np.nan
    systems += [(0.0, g, ph), (1e-7, g, ph), (PO.PHOTO_WEIGHT, few_g, few_p), (PO.PHOTO_WEIGHT, enough_g, pr), (PO.PHOTO_WEIGHT, gr, nan_p),
                (0.0, gr, nan_p)]
    out = run(photo_host, "joint", [[64, wt, *a, *b] for wt, a, b in systems])
    seen = []
    for (wt, a, b), o in zip(systems, out):
        s = PO.joint(a, b if np.float32(wt) != 0 else None, wt)
        assert np.array_equal(o[8:], s, equal_nan=True)                  # the joint sums: the same float64 operations
        x, ratio = IO.solve(s, 64)
        assert bool(o[0]) == (x is not None)
        seen.append(bool(o[0]))
        if x is None:
            assert not o[2:8].any() and o[1] <= 1e-6
            continue
        assert abs(o[1] - ratio) <= 1e-9 * ratio
        A, rhs = IO.full_matrix(s), s[21:27]
        assert np.abs(A @ o[2:8] + rhs).max() <= 1e-9 * np.abs(rhs).max()
        if ratio > 1e-3:
            assert np.abs(o[2:8] - x).max() <= 1e-12 * np.abs(x).max()
    # the plane is solvable only through the texture: weight 0 and a weight too small to lift the pivots are degenerate
    assert seen == [True] * 8 + [False, False, False, True, False, True]
