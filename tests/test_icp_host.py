"""K18 dense RGB-D refinement without a GPU: the host-side argument checks of the four entries (MI_E_* before any launch),
the Python module's constructor and its refusal of CPU tensors, the export through the `pytorch_model` alias,
synth_depth_room, the numpy oracle's own sanity, and the kernels' arithmetic (csrc/icp_math.h) compiled as plain C++ in
tests/native/icp_host.cpp.

Bounds.  The solve, Exp and the pose update are float64 in both the header and the oracle, in the same order of operations
but for numpy's matrix products: they agree to 1e-12 relative (a few hundred float64 roundings; an ill-conditioned system
multiplies that by its condition number, so it is compared through its residual |A x + b| <= 1e-9 |b|).  The per-pixel row
and the normal are float32 in the header's order, which numpy's float32 run reproduces operation by operation: compared bit
for bit.  The oracle's fixed point: refined from the truth at (48, 64), seeds 0 1 2, the float64 oracle ends within 5.2624e-2
deg and 1.6994e-3 m of the truth (the bias of crease and sphere normals, tests/test_gpu_icp.py) and within 1e-9 of its own
result from identity."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as IO
from helpers import host_program, run_records as run
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
ANGLE = float(np.deg2rad(30.0))


@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


p_keepalive = []


def test_surfel_maps_argument_checks(lib, p):
    f = lib.mi_surfel_maps
    good = [p, 0, 2, 48, 64, p, 1.0, 0.1, 10.0, 0.1, p, p, None]
    for i in (0, 5, 10, 11):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=2, h=48, w=64, zs=1.0, lo=0.1, hi=10.0, jump=0.1, v=p, n=p)
        a.update(kw)
        return f(p, 1, a["batch"], a["h"], a["w"], p, a["zs"], a["lo"], a["hi"], a["jump"], a["v"], a["n"], None)
    assert call(batch=0) == SHAPE and call(h=2) == SHAPE and call(w=2) == SHAPE and call(w=-1) == SHAPE
    assert call(batch=4, h=32768, w=16384) == SHAPE and call(batch=65535, h=256, w=129) == SHAPE     # batch h w >= 2^31
    assert call(batch=65536, h=3, w=3) == PARAM
    assert call(lo=0.0) == PARAM and call(lo=float("nan")) == PARAM and call(hi=0.05) == PARAM and call(hi=float("inf")) == PARAM
    assert call(zs=0.0) == PARAM and call(zs=float("inf")) == PARAM and call(jump=0.0) == PARAM and call(jump=float("nan")) == PARAM
    assert call(v=p + 4) == ALIGN and call(n=p + 8) == ALIGN


def test_linearise_argument_checks(lib, p):
    f, wb = lib.mi_icp_linearise, lib.mi_icp_workspace_bytes
    need = wb(3, 120, 160)
    assert need >= 3 * (12 * 8 + 10 * 256 + 8) and need % 16 == 0         # poses, 10 slab records of 256 bytes, two words
    assert wb(0, 120, 160) == 0 and wb(3, 2, 160) == 0 and wb(3, 120, 2) == 0 and wb(65536, 3, 3) == 0 and wb(4, 32768, 16384) == 0
    good = [p, p, p, p, p, p, 3, 120, 160, 125.0, 125.0, 80.0, 60.0, 1, 0.1, ANGLE, p, p, need, None]
    for i in (0, 1, 2, 3, 4, 5, 16, 17):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=3, h=120, w=160, fx=125.0, fy=125.0, cx=80.0, cy=60.0, stride=1, dist=0.1, ang=ANGLE, ws=p, wbytes=need, v1=p, n2=p)
        a.update(kw)
        return f(a["v1"], p, p, a["n2"], p, p, a["batch"], a["h"], a["w"], a["fx"], a["fy"], a["cx"], a["cy"], a["stride"], a["dist"],
                 a["ang"], p, a["ws"], a["wbytes"], None)
    assert call(batch=0) == SHAPE and call(h=2) == SHAPE and call(w=0) == SHAPE and call(batch=70000, h=3, w=3) == PARAM
    for s in (0, 3, 5, 16, -1):
        assert call(stride=s) == PARAM, s
    for s in (1, 2, 4, 8):
        assert call(stride=s, wbytes=need - 1) == CAPACITY, s             # every other check passed
    assert call(fx=0.0) == PARAM and call(fy=float("inf")) == PARAM and call(cx=float("nan")) == PARAM and call(cy=float("inf")) == PARAM
    assert call(dist=0.0) == PARAM and call(dist=float("inf")) == PARAM and call(ang=0.0) == PARAM and call(ang=3.2) == PARAM
    assert call(ang=float("nan")) == PARAM
    assert call(ws=p + 4) == ALIGN and call(v1=p + 4) == ALIGN and call(n2=p + 8) == ALIGN


def test_refine_argument_checks(lib, p):
    f, need = lib.mi_icp_refine, lib.mi_icp_workspace_bytes(2, 48, 64)

    def arr(*v):
        a = (ctypes.c_int32 * len(v))(*v)
        p_keepalive.append(a)
        return ctypes.cast(a, ctypes.c_void_p)
    st, it = arr(4, 2, 1), arr(4, 4, 6)
    good = [p, p, p, p, p, p, 2, 48, 64, 50.0, 50.0, 32.0, 24.0, st, it, 3, 0.1, ANGLE, 64, p, p, p, p, p, p, p, p, need, None]
    for i in (0, 1, 2, 3, 4, 5, 13, 14, 19, 20, 21, 22, 23, 24, 25, 26):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=2, h=48, w=64, st=st, it=it, stages=3, dist=0.1, ang=ANGLE, minc=64, ws=p, wbytes=need, fx=50.0)
        a.update(kw)
        return f(p, p, p, p, p, p, a["batch"], a["h"], a["w"], a["fx"], 50.0, 32.0, 24.0, a["st"], a["it"], a["stages"], a["dist"],
                 a["ang"], a["minc"], p, p, p, p, p, p, p, a["ws"], a["wbytes"], None)
    assert call(wbytes=need - 1) == CAPACITY and call(ws=p + 8) == ALIGN
    assert call(batch=0) == SHAPE and call(h=1) == SHAPE and call(batch=65536) == PARAM
    assert call(stages=0) == PARAM and call(stages=5) == PARAM and call(minc=0) == PARAM
    assert call(st=arr(4, 3, 1)) == PARAM and call(st=arr(16, 2, 1)) == PARAM and call(it=arr(4, -1, 6)) == PARAM
    assert call(it=arr(30, 30, 5)) == PARAM and call(it=arr(30, 30, 4), wbytes=0) == CAPACITY           # 65 and 64 in all
    assert call(it=arr(0, 0, 0), wbytes=0) == CAPACITY                                                   # no iterations: legal
    assert call(st=arr(8, 8, 8, 8), it=arr(1, 1, 1, 1), stages=4, wbytes=0) == CAPACITY
    assert call(fx=-1.0) == PARAM and call(dist=float("nan")) == PARAM and call(ang=4.0) == PARAM


def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import DenseRgbdRefiner
    Kt = torch.from_numpy(rgbd_camera(48, 64))
    m = DenseRgbdRefiner(Kt)
    assert (m.depth_scale, m.min_depth, m.max_depth, m.schedule, m.distance_threshold, m.normal_max_jump, m.min_correspondences) == \
        (1.0, 0.1, 10.0, ((4, 4), (2, 4), (1, 6)), 0.1, 0.1, 64)
    assert abs(m.angle_threshold - np.deg2rad(30.0)) < 1e-15 and m.camera == (50.0, 50.0, 32.0, 24.0)
    assert torch.allclose(m.K_inv @ m.K, torch.eye(3), atol=1e-6) and m.K.dtype == torch.float32
    for kw in (dict(depth_scale=0.0), dict(min_depth=0.0), dict(min_depth=2.0, max_depth=1.0), dict(schedule=()),
               dict(schedule=((1, 1),) * 5), dict(schedule=((3, 1),)), dict(schedule=((1, -1),)), dict(schedule=((1, 40), (2, 25))),
               dict(schedule=(1, 2)), dict(distance_threshold=0.0), dict(angle_threshold_deg=0.0), dict(angle_threshold_deg=181.0),
               dict(normal_max_jump=0.0), dict(min_correspondences=0)):
        with pytest.raises(ValueError):
            DenseRgbdRefiner(Kt, **kw)
    with pytest.raises(ValueError, match="3x3"):
        DenseRgbdRefiner(torch.eye(4))
    assert DenseRgbdRefiner(Kt, schedule=((8, 0),)).schedule == ((8, 0),)
    for shape in ((2, 48, 64), (2, 1, 48, 64), (48, 64)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(torch.ones(shape), torch.ones(shape))
    with pytest.raises(RuntimeError, match=r"\(B, H, W\) or \(B, 1, H, W\)"):
        m(torch.ones(2, 3, 48, 64), torch.ones(2, 3, 48, 64))
    maps = (torch.zeros(1, 48, 64, 4), torch.zeros(1, 48, 64, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.surfel_maps(torch.ones(1, 48, 64), torch.eye(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icp_linearise(maps, maps, torch.eye(3)[None], torch.zeros(1, 3), (50.0, 50.0, 32.0, 24.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icp_refine(maps, maps, torch.eye(3)[None], torch.zeros(1, 3), (50.0, 50.0, 32.0, 24.0))


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import DenseRgbdRefiner
    assert DenseRgbdRefiner is real.DenseRgbdRefiner and "DenseRgbdRefiner" in real.__all__
    from pytorch_model.geometry.dense_rgbd import DenseRgbdRefiner as again
    assert again is DenseRgbdRefiner


def test_synth_depth_room_is_deterministic_and_consistent():
    a, b = synth_depth_room(3, 48, 64), synth_depth_room(3, 48, 64)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    d1, d2, R, t = a
    assert d1.shape == (48, 64) and d1.dtype == np.float32 and d2.dtype == np.float32
    assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 0.05) < 1e-12
    assert abs(IO.rotation_angle_deg(R, np.eye(3)) - 2.0) < 1e-9
    other = synth_depth_room(4, 48, 64)
    assert np.array_equal(d1, other[0]) and not np.array_equal(d2, other[1])      # the first camera is the room's frame
    R5, t5 = synth_depth_room(3, 48, 64, rotation_deg=5.0, translation=0.2)[2:]
    assert abs(IO.rotation_angle_deg(R5, np.eye(3)) - 5.0) < 1e-9 and abs(np.linalg.norm(t5) - 0.2) < 1e-12
    # every pixel sees the room: all depths inside the camera's range, the sphere nearer than the walls behind it
    for d in (d1, d2):
        assert (d > 1.0).all() and (d < 4.0).all()
    flat = synth_depth_room(3, 48, 64, sphere=False)[0]
    assert (flat >= d1).all() and 0.02 < (flat > d1).mean() < 0.2
    # the two frames are views of one scene under (R, t): at the truth nearly every pixel finds its surface again, with a
    # point-to-plane residual far below the 5 cm motion; at the identity it does not
    m1, m2, R, t, cam = IO.room(3, 48, 64)[:5]
    at_truth, at_identity = IO.linearise(m1, m2, R, t, cam), IO.linearise(m1, m2, np.eye(3), np.zeros(3), cam)
    rms = [np.sqrt(s[27] / s[28]) for s in (at_truth, at_identity)]
    assert m1[3].mean() > 0.75 and m2[3].mean() > 0.75                  # valid normals: all but borders, creases, the sphere's rim
    assert at_truth[28] > 0.75 * 48 * 64 and rms[0] < 0.005 and rms[1] > 4 * rms[0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_keeps_the_truth_to_within_its_bias(seed):
    m1, m2, R, t, cam = IO.room(seed, 48, 64)[:5]
    o = IO.refine(m1, m2, R, t, cam)
    assert o["ok"] and o["steps"] == 14 and o["min_ratio"] > 1e-3 and o["last_step"] < 1e-9
    assert IO.rotation_angle_deg_small(o["R"], R) <= 5.2624e-2 * 1.001 and np.abs(o["t"] - t).max() <= 1.6994e-3 * 1.001
    i = IO.refine(m1, m2, np.eye(3), np.zeros(3), cam)
    assert IO.rotation_angle_deg_small(o["R"], i["R"]) < 1e-9 and np.abs(o["t"] - i["t"]).max() < 1e-9
    assert np.allclose(o["information"], o["information"].T) and o["count"] > 2000


def test_oracle_degenerate_scenes():
    h, w = 48, 64
    ki = IO.k_inv32(rgbd_camera(h, w))
    cam = IO.camera_of(rgbd_camera(h, w))
    for depth in (IO.plane_depth(h, w), IO.walls_depth(h, w)):
        for dtype in (F64, F32):
            m = IO.surfel_maps(depth, ki, dtype=dtype)
            s = IO.linearise(m, m, np.eye(3), np.zeros(3), cam, dtype=dtype)
            x, ratio = IO.solve(s)
            assert s[28] > 1000 and x is None and ratio < 1e-9
            o = IO.refine(m, m, np.eye(3), np.zeros(3), cam, dtype=dtype)
            assert not o["ok"] and o["steps"] == 0 and np.array_equal(o["R"], np.eye(3)) and not o["t"].any()
    m1 = IO.room(1, h, w)[0]
    empty = IO.surfel_maps(np.zeros((h, w), F32), ki)
    o = IO.refine(m1, empty, np.eye(3), np.zeros(3), cam)
    assert not o["ok"] and o["count"] == 0 and o["rmse"] == 0.0 and o["steps"] == 0 and not o["information"].any()
    assert not empty[1].any() and not empty[3].any()


# ---- the kernels' arithmetic on the host ----------------------------------------------------------------------------------------

# tests/native/icp_host.cpp around csrc/icp_math.h, compiled as plain C++ (no HIP)
icp_host = host_program("icp_host.cpp", hip=False)


def test_native_solve_matches_the_oracle(icp_host):
    rng = np.random.default_rng(5)
    systems = []
    for seed in (0, 1, 2):
        m1, m2, R, t, cam = IO.room(seed, 48, 64)[:5]
        for stride in (1, 4):
            systems.append(IO.linearise(m1, m2, np.eye(3), np.zeros(3), cam, stride))                 # well conditioned
    ki = IO.k_inv32(rgbd_camera(48, 64))
    m = IO.surfel_maps(IO.plane_depth(48, 64), ki)
    plane = IO.linearise(m, m, np.eye(3), np.zeros(3), IO.camera_of(rgbd_camera(48, 64)))
    systems.append(plane)                                                                              # singular
    for cond in (1e3, 1e5, 1e9):                                                                       # ill conditioned
        q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
        A = q @ np.diag(np.geomspace(1.0, 1.0 / cond, 6)) @ q.T
        s = np.zeros(29)
        s[:21] = [A[i, j] for i in range(6) for j in range(i, 6)]
        s[21:27] = rng.normal(size=6)
        s[27], s[28] = 1.0, 500
        systems.append(s)
    few = systems[0].copy()
    few[28] = 63
    nan = systems[0].copy()
    nan[3] = np.nan
    systems += [few, nan]
    out = run(icp_host, "solve", [[64, *s] for s in systems])
    seen = []
    for s, o in zip(systems, out):
        x, ratio = IO.solve(s, 64)
        assert bool(o[0]) == (x is not None)
        seen.append(bool(o[0]))
        if x is None:
            assert not o[2:].any() and o[1] <= 1e-6
            continue
        assert abs(o[1] - ratio) <= 1e-9 * ratio
        A, b = IO.full_matrix(s), s[21:27]
        assert np.abs(A @ o[2:] + b).max() <= 1e-9 * np.abs(b).max()
        if ratio > 1e-3:
            assert np.abs(o[2:] - x).max() <= 1e-12 * np.abs(x).max()
    assert seen == [True] * 6 + [False] + [True, True, False] + [False, False]      # cond 1e9: a pivot below 1e-6 max diag


def test_native_exp_and_update_match_the_oracle(icp_host):
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    omegas = [axis * m for m in (0.0, 1e-9, 0.9e-8, 1.1e-8, 1e-3, 1.0)]
    for w, e in zip(omegas, run(icp_host, "exp", omegas)):
        E = e.reshape(3, 3)
        assert np.abs(E - IO.exp_so3(w)).max() <= 1e-15
        th = np.linalg.norm(w)
        if th >= 1e-8:
            assert abs(np.linalg.det(E) - 1) < 1e-14 and abs(IO.rotation_angle_deg(E, np.eye(3)) - np.degrees(th)) < 1e-6
        else:
            assert np.array_equal(E, np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]))
    R, t = synth_depth_room(0, 48, 64)[2:]
    xs = [np.array([0.01, -0.02, 0.005, 0.03, -0.01, 0.02]), np.zeros(6), np.array([1e-9, 0, 0, 1e-9, 0, 0])]
    for x, o in zip(xs, run(icp_host, "update", [[*R.ravel(), *t, *x] for x in xs])):
        Rn, tn = IO.update(R, t, x)
        assert np.abs(o[:9].reshape(3, 3) - Rn).max() <= 1e-15 and np.abs(o[9:] - tn).max() <= 1e-15


def test_native_vertex_and_normal_match_the_oracle(icp_host):
    h, w = 37, 53
    ki = IO.k_inv32(rgbd_camera(h, w))
    d = synth_depth_room(1, h, w)[0].copy()
    d[2, 3], d[2, 4], d[2, 5], d[2, 6], d[2, 7] = np.nan, np.inf, 0.0, 0.0999, 10.001
    d[4:9, 5:10] += F32(0.5)                                                          # a step: the jump gate
    v, vok, n, nok = IO.surfel_maps(d, ki, dtype=F32)
    px = [(y, x) for y in range(1, h - 1) for x in range(1, w - 1)]
    out = run(icp_host, "vertex", [[d[y, x], x, y, *ki.ravel()[:6], 1.0, 0.1, 10.0] for y, x in px])
    for (y, x), o in zip(px, out):
        assert bool(o[0]) == vok[y, x] and np.array_equal(o[1:].astype(F32), v[y, x])
    assert not vok[2, 3:8].any() and vok.mean() > 0.99
    cases = [(y, x) for y, x in px if vok[y, x] and vok[y, x - 1] and vok[y, x + 1] and vok[y - 1, x] and vok[y + 1, x]]
    out = run(icp_host, "normal", [[0.1, *v[y, x], *v[y, x - 1], *v[y, x + 1], *v[y - 1, x], *v[y + 1, x]] for y, x in cases])
    for (y, x), o in zip(cases, out):
        assert bool(o[0]) == nok[y, x], (y, x)
        assert np.array_equal(o[1:].astype(F32), n[y, x])
        if nok[y, x]:
            assert np.dot(o[1:], v[y, x]) < 0 and abs(np.linalg.norm(o[1:]) - 1) < 1e-6      # faces the camera, unit length
    assert not nok[3, 7] and not nok[4, 7] and not nok[8, 7] and not nok[9, 7] and not nok[6, 4] and not nok[6, 5]   # the step's rim
    assert nok[6, 7] and nok[11, 7] and nok[6, 12] and (9, 7) in cases and (8, 7) in cases            # its inside, the wall around
    # orientation: a wall seen from either side of its normal, a flat patch with the neighbours swapped
    c = np.array([0.1, 0.2, 2.0], F32)
    l, r_, u, dn = c + F32([-0.01, 0, 0.002]), c + F32([0.01, 0, -0.002]), c + F32([0, -0.01, 0.001]), c + F32([0, 0.01, -0.001])
    a, b = run(icp_host, "normal", [[0.1, *c, *l, *r_, *u, *dn], [0.1, *c, *r_, *l, *u, *dn]])
    assert a[0] == 1 and b[0] == 1 and np.allclose(a[1:], b[1:], atol=1e-6) and np.dot(a[1:], c) < 0
    z = run(icp_host, "normal", [[0.1, *c, *c, *c, *u, *dn], [0.001, *c, *l, *r_, *u, *dn]])          # zero cross product; jump
    assert z[0][0] == 0 and not z[0][1:].any() and z[1][0] == 0


def test_native_row_is_the_float32_oracles(icp_host):
    h, w = 37, 53
    m1, m2, R, t, cam = IO.room(2, h, w, dtype=F32)[:5]
    Rp, tp = (x.astype(F32) for x in IO.perturbed(R, t))
    J, r = IO.rows(m1, m2, Rp, tp, cam, 1, dtype=F32)
    src = [(y, x) for y in range(h) for x in range(w) if m1[3][y, x]]
    thr2, cos_thr = F32(IO.DIST) * F32(IO.DIST), F32(np.cos(F64(F32(np.deg2rad(30.0)))))
    # pass 1 finds each source pixel's target; pass 2 feeds the target's surfel
    dummy = [0.0] * 6
    first = run(icp_host, "row", [[*Rp.ravel(), *tp, *m1[0][y, x], *m1[2][y, x], *dummy, *cam, w, h, thr2, cos_thr] for y, x in src])
    recs, keep = [], []
    for (y, x), o in zip(src, first):
        if o[0] >= 1 and m2[3][int(o[2]), int(o[1])]:
            iy, ix = int(o[2]), int(o[1])
            recs.append([*Rp.ravel(), *tp, *m1[0][y, x], *m1[2][y, x], *m2[0][iy, ix], *m2[2][iy, ix], *cam, w, h, thr2, cos_thr])
            keep.append((y, x))
    out = [o for o in run(icp_host, "row", recs) if o[0] == 2]
    assert len(out) == len(r) and len(r) > 0.7 * h * w and len(first) - len(out) > 20
    got = np.array(out)
    assert np.array_equal(got[:, 3:9].astype(F32), J) and np.array_equal(got[:, 9].astype(F32), r)
