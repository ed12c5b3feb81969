"""K32 feature tracking without a GPU: the host-side argument checks of the five entries (MI_E_* before any launch, in the
header's order of precedence), the section's own header and library, FeatureTracker's constructor and its refusal of CPU
tensors, the export through the `pytorch_model` alias, synth_flow_pair, the numpy oracle on the ten scenes of flow_oracle.SCENES, on flat
regions and on hand-made replenish / check cases, and the kernels' arithmetic (csrc/flow_math.h) compiled for the host in
tests/native/flow_host.cpp, plain and under the host's address and undefined-behaviour sanitizers.

Tolerances against the float64 oracle, measured on this file's ten scenes (flow_oracle.SCENES, 40 points each) over the points whose status and total iteration count agree with the float64 oracle's -- all 400, for both:
  - position |kp2 - kp2_64|: float32 oracle max 1.392e-5 px (scene l4r7), native program the same -> POS_TOL = 2.8e-5 px;
  - residual |r - r_64|: float32 oracle max 7.110e-6 gray levels (l4r7), native program the same   -> RES_TOL = 1.5e-5.
The native program and the float32 oracle agree bit for bit, so the two deviations are one.  The float64 oracle's own largest
error against the true position A p + d, per scene in flow_oracle.SCENES' order (shift, shift_u8, rot2, rot-3, l1, l2r3, l1r2,
big, l4r5, l4r7): 0.024, 0.041, 0.216, 0.321, 0.090, 0.121, 0.092, 0.134, 0.076, 0.032 px; the ground-truth bound of a scene
is that figure plus POS_TOL.  No scene point's min_eig is within 1 % of min_eigen (the smallest is 0.026 against 1e-3)."""
import ctypes

import numpy as np
import pytest
import torch

import flow_oracle as FO
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import synth_flow_pair

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
POS_TOL, RES_TOL, CAP = FO.POS_TOL, FO.RES_TOL, FO.CAP
RECORD = np.dtype([("y", "<f4"), ("x", "<f4"), ("residual", "<f4"), ("status", "<i4"), ("code", "<i4"), ("iterations", "<i4")])


@pytest.fixture(scope="module")
def lib():
    return N.load_flow()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


p_keepalive = []


def test_the_section_has_a_header_and_a_library_of_its_own(lib):
    assert sorted(N.FLOW_SIGNATURES) == ["mi_flow_check", "mi_flow_pyramid", "mi_flow_pyramid_bytes", "mi_flow_replenish", "mi_flow_track"]
    assert not set(N.FLOW_SIGNATURES) & set(N.SIGNATURES) and len(N.SIGNATURES) == 127
    c = N.FLOW_CONSTANTS
    assert (c["MI_FLOW_MAX_LEVELS"], c["MI_FLOW_MAX_RADIUS"], c["MI_FLOW_MAX_K"], c["MI_FLOW_MAX_CELLS"]) == (8, 10, 4096, 16384)
    assert (c["MI_FLOW_OK"], c["MI_FLOW_PADDING"], c["MI_FLOW_FLAT"], c["MI_FLOW_LEFT"]) == (FO.OK, FO.PADDING, FO.FLAT, FO.LEFT)
    assert N.library_of("mi_flow_track") is lib and N.library_of("mi_sim3_refit") is N.load_sim3() and N.library_of("mi_rigid_refit") is N.load()
    assert N.load().mi_abi_version() == 3
    for name in N.FLOW_SIGNATURES:
        assert not hasattr(N.load(), name)                                   # the product library exports its own header only
    assert lib.mi_flow_pyramid_bytes.restype is ctypes.c_size_t


def test_pyramid_argument_checks(lib, p):
    f, nb = lib.mi_flow_pyramid, lib.mi_flow_pyramid_bytes
    offs, need = FO.level_offsets(3, 83, 97, 3)
    assert nb(3, 83, 97, 3) == need and need % 256 == 0 and all(o * 4 % 256 == 0 for o in offs)
    assert nb(1, 83, 97, 1) == (83 * 97 * 4 + 255) // 256 * 256
    assert nb(0, 83, 97, 3) == 0 and nb(3, 0, 97, 3) == 0 and nb(3, 83, 97, 0) == 0 and nb(3, 83, 97, 9) == 0 and nb(65536, 83, 97, 3) == 0
    assert nb(1, 83, 97, 5) > 0 and nb(1, 83, 97, 6) == 0                    # 83x97 -> 6x7 at level 4, 3x4 at level 5
    good = [p, 1, 3, 83, 97, 3, p, need, None]
    for i in (0, 6):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(gray=p, u8=1, batch=3, h=83, w=97, levels=3, pyr=p, nbytes=need)
        a.update(kw)
        return f(a["gray"], a["u8"], a["batch"], a["h"], a["w"], a["levels"], a["pyr"], a["nbytes"], None)
    assert call(batch=0) == SHAPE and call(h=0) == SHAPE and call(w=-1) == SHAPE
    assert call(levels=0) == PARAM and call(levels=9) == PARAM and call(levels=6) == PARAM and call(batch=65536) == PARAM
    assert call(h=40000) == PARAM
    assert call(batch=65535, h=32768, w=32768, levels=1) == PARAM and nb(65535, 32768, 32768, 1) == 0      # beyond MI_FLOW_MAX_PIXELS
    assert nb(4, 32768, 32768, 1) == 1 << 34 and N.FLOW_CONSTANTS["MI_FLOW_MAX_PIXELS"] == 1 << 32
    assert call(pyr=p + 4) == ALIGN and call(gray=p + 2, u8=0) == ALIGN
    assert call(nbytes=need - 1) == CAPACITY
    # precedence: NULL, shape, parameters, alignment, capacity
    assert call(gray=None, batch=0) == NULL and call(batch=0, levels=0, pyr=p + 4, nbytes=0) == SHAPE
    assert call(levels=0, pyr=p + 4, nbytes=0) == PARAM and call(pyr=p + 4, nbytes=0) == ALIGN


def test_track_argument_checks(lib, p):
    f = lib.mi_flow_track
    good = [p, p, p, p, 3, 83, 97, 3, 40, 7, 30, 0.01, 1e-3, p, p, p, p, p, None]
    for i in (0, 1, 2, 13, 14, 15, 16, 17):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(pyr1=p, guess=p, batch=3, h=83, w=97, levels=3, k=40, r=7, its=30, eps=0.01, eig=1e-3, kp=p)
        a.update(kw)
        return f(a["pyr1"], p, a["kp"], a["guess"], a["batch"], a["h"], a["w"], a["levels"], a["k"], a["r"], a["its"], a["eps"], a["eig"],
                 a.get("kp2", p), p, p, a.get("res", p), a.get("its_out", p), None)
    assert call(guess=None, batch=0) == SHAPE                                # the guess may be NULL
    assert call(batch=0) == SHAPE and call(k=0) == SHAPE and call(h=0) == SHAPE and call(w=0) == SHAPE
    for kw in (dict(batch=65536), dict(k=4097), dict(levels=0), dict(levels=9), dict(r=0), dict(r=11), dict(its=0), dict(its=65),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(eig=-1e-3), dict(eig=float("nan")),
               dict(eig=float("inf")), dict(r=10), dict(levels=4)):           # 83x97 at level 2 is 21x25: r = 10 needs 23; level 3 is 11x13
        assert call(**kw) == PARAM, kw
    assert call(r=9, pyr1=p + 4) == ALIGN and call(pyr1=p + 4) == ALIGN and call(kp=p + 2) == ALIGN and call(guess=p + 2) == ALIGN
    assert call(kp2=p + 2) == ALIGN and call(res=p + 1) == ALIGN and call(its_out=p + 2) == ALIGN            # the outputs too
    assert call(batch=65535, h=32768, w=32768, levels=1) == PARAM
    assert call(k=0, r=0, pyr1=p + 4) == SHAPE and call(r=0, pyr1=p + 4) == PARAM and call(pyr1=None, k=0) == NULL


def test_check_argument_checks(lib, p):
    f = lib.mi_flow_check
    for i in (0, 1, 2, 3, 7, 8):
        a = [p, p, p, p, 3, 40, 1.0, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i
    assert f(p, p, p, p, 0, 40, 1.0, p, p, None) == SHAPE and f(p, p, p, p, 3, 0, 1.0, p, p, None) == SHAPE
    assert f(p, p, p, p, 65536, 40, 1.0, p, p, None) == PARAM and f(p, p, p, p, 3, 4097, 1.0, p, p, None) == PARAM
    for d in (-1.0, float("nan"), float("inf")):
        assert f(p, p, p, p, 3, 40, d, p, p, None) == PARAM
    assert f(p, p, p, p, 0, 40, -1.0, p, p, None) == SHAPE and f(None, p, p, p, 0, 40, -1.0, p, p, None) == NULL
    assert f(p + 2, p, p, p, 3, 40, 1.0, p, p, None) == ALIGN and f(p, p + 1, p, p, 3, 40, 1.0, p, p, None) == ALIGN
    assert f(p, p, p, p, 3, 40, 1.0, p, p + 2, None) == ALIGN and f(p + 2, p, p, p, 3, 40, -1.0, p, p, None) == PARAM


def test_replenish_argument_checks(lib, p):
    f = lib.mi_flow_replenish
    good = [p, p, p, p, 3, 40, 64, 83, 97, 16, p, p, p, None]
    for i in (0, 1, 2, 3, 10, 11, 12):
        a = list(good)
        a[i] = None
        assert f(*a) == NULL, i

    def call(**kw):
        a = dict(batch=3, k=40, n=64, h=83, w=97, cell=16)
        a.update(kw)
        return f(p, p, p, p, a["batch"], a["k"], a["n"], a["h"], a["w"], a["cell"], p, p, p, None)
    assert call(batch=0) == SHAPE and call(k=0) == SHAPE and call(n=0) == SHAPE and call(h=0) == SHAPE and call(w=0) == SHAPE
    assert call(batch=65536) == PARAM and call(k=4097) == PARAM and call(n=65537) == PARAM and call(cell=0) == PARAM
    assert call(h=480, w=640, cell=4) == PARAM                               # 120 x 160 = 19200 cells
    assert call(h=512, w=512, cell=3) == PARAM and call(n=0, cell=0) == SHAPE
    for i in (0, 2, 3, 10, 12):                                              # the float32 / int32 arrays, inputs and outputs
        a = list(good)
        a[i] = p + 2
        assert f(*a) == ALIGN, i
        a[9] = 0
        assert f(*a) == PARAM                                                # parameters before alignment


def test_module_constructor_cpu_refusal_and_alias():
    import onnx_image_processing_amd.pytorch_model.tracking as real
    import pytorch_model
    from onnx_image_processing_amd import ops
    from pytorch_model.tracking import FeatureTracker
    from pytorch_model.tracking.feature_tracker import FeatureTracker as again
    assert FeatureTracker is real.FeatureTracker is again and "FeatureTracker" in real.__all__ and "FeatureTracker" in pytorch_model.__doc__
    m = FeatureTracker()
    assert (m.levels, m.radius, m.max_iterations, m.epsilon, m.min_eigen, m.fb_threshold, m.cell) == (3, 7, 30, 0.01, 1e-3, 0.0, 16)
    for kw in (dict(levels=0), dict(levels=9), dict(radius=0), dict(radius=11), dict(max_iterations=0), dict(max_iterations=65),
               dict(epsilon=0.0), dict(epsilon=float("inf")), dict(min_eigen=-1.0), dict(fb_threshold=-1.0), dict(cell=0)):
        with pytest.raises(ValueError):
            FeatureTracker(**kw)
    z = torch.zeros(1, 40, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.pyramid(torch.zeros(1, 83, 97))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.flow_check(z, z, torch.ones(1, 40), torch.ones(1, 40), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.replenish(z, torch.ones(1, 40), z, None, 83, 97)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.matches(torch.ones(1, 40, dtype=torch.bool))
    pyr = ops.FlowPyramid(torch.zeros(FO.level_offsets(1, 83, 97, 3)[1] // 8, dtype=torch.int64), 1, 83, 97, 3)
    assert pyr.level(2).shape == (1, 21, 25) and pyr.level(1).shape == (1, 42, 49)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.track(pyr, pyr, z)


def test_synth_flow_pair_is_exact_and_deterministic():
    a, b = synth_flow_pair(3, 83, 97, 2.0, 1.02, (6.3, -4.7)), synth_flow_pair(3, 83, 97, 2.0, 1.02, (6.3, -4.7))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    f1, f2, A, d = a
    assert f1.shape == f2.shape == (83, 97) and f1.dtype == f2.dtype == np.float32 and A.shape == (2, 3) and d.tolist() == [6.3, -4.7]
    assert 18 <= f1.min() and f1.max() <= 238 and f1.std() > 10
    assert abs(np.linalg.det(A[:, :2]) - 1.02 ** 2) < 1e-12 and np.allclose(A @ [48.0, 41.0, 1.0], [48.0, 41.0])    # about the centre
    # an integer shift is a roll: frame 2 shows the point p of frame 1 at p + d, with no interpolation
    g1, g2, _, _ = synth_flow_pair(3, 83, 97, 0.0, 1.0, (6.0, -4.0))
    assert np.array_equal(g1[10:60, 10:60], g2[6:56, 16:66])
    # a rotation by 90 degrees about the centre of a square frame maps pixel centres onto pixel centres
    r1, r2, A90, _ = synth_flow_pair(5, 65, 65, 90.0, 1.0, (0.0, 0.0))
    xy = np.rint(np.array([10.0, 20.0, 1.0]) @ A90.T).astype(int)
    assert abs(float(r2[xy[1], xy[0]]) - float(r1[20, 10])) < 1e-3
    q1, q2, _, _ = synth_flow_pair(3, 83, 97, 2.0, 1.02, (6.3, -4.7), quantise=True)
    assert q1.dtype == np.uint8 and np.abs(q1.astype(np.float64) - f1).max() <= 0.5 + 1e-4
    assert not np.array_equal(f1, synth_flow_pair(4, 83, 97, 2.0, 1.02, (6.3, -4.7))[0])
    for bad in (dict(height=0), dict(terms=0), dict(lam=(0.0, 4.0)), dict(lam=(8.0, 4.0)), dict(scale=0.0)):
        with pytest.raises(ValueError):
            synth_flow_pair(**{**dict(seed=0, height=32, width=32), **bad})


@pytest.mark.parametrize("shape", [(83, 97), (96, 80)])
def test_oracle_pyramid_is_exact_for_uint8_frames_and_is_pyrdown(shape):
    g = np.rint(synth_flow_pair(9, *shape)[0]).astype(np.uint8)
    p64, p32 = FO.pyramid(g, 4, np.float64), FO.pyramid(g, 4, np.float32)
    assert [lv.shape for lv in p64] == FO.level_shapes(*shape, 4)
    for l in range(3):                                                       # multiples of 2^-16 below 256: float32 holds them
        assert np.array_equal(p32[l].astype(np.float64), p64[l]) and np.array_equal(p64[l] * 65536, np.rint(p64[l] * 65536))
    assert np.abs(p32[3] - p64[3]).max() < 1e-4
    # the separable [1 4 6 4 1] / 16 blur with reflect-101 borders sampled at the even pixels, written differently
    k = np.array([1, 4, 6, 4, 1]) / 16.0
    pad = np.pad(g.astype(np.float64), 2, mode="reflect")
    blur = sum(k[i] * k[j] * pad[i:i + shape[0], j:j + shape[1]] for i in range(5) for j in range(5))
    assert np.abs(blur[::2, ::2] - p64[1]).max() < 1e-10
    assert np.abs(FO.pyramid(np.full(shape, 77.0), 3)[2] - 77.0).max() == 0


@pytest.mark.parametrize("name", sorted(FO.SCENES))
def test_oracle_tracks_the_scenes_and_float32_stays_inside_the_cap(name):
    s = FO.scene(name)
    o64, o32 = s["o64"], s["o32"]
    assert o64["status"].all() and (o64["code"] == FO.OK).all()              # all 40 tracked under scene seed 1
    err = np.linalg.norm(o64["kp2"][0] - s["truth"], axis=1)
    print(f"{name}: float64 oracle max error against the truth {err.max():.4f} px, mean iterations {o64['iterations'].mean():.1f}")
    assert err.max() < 0.5
    eig = np.array([e for es in o64["min_eig"][0] for e in es])
    assert eig.size == FO.POINTS * s["levels"] and (np.abs(eig / FO.MIN_EIGEN - 1) > 0.01).all()
    same = FO.comparable(o32["status"][0], o32["iterations"][0], o64)
    assert (~same).sum() <= CAP * FO.POINTS
    dev = np.linalg.norm(o32["kp2"][0].astype(np.float64) - o64["kp2"][0], axis=1)
    rdev = np.abs(o32["residual"][0].astype(np.float64) - o64["residual"][0])
    print(f"{name}: float32 oracle, {same.sum()} comparable: position {dev[same].max():.3e} px, residual {rdev[same].max():.3e}")
    assert dev[same].max() <= POS_TOL / 2 * 1.01 and rdev[same].max() <= RES_TOL / 2 * 1.01
    assert (np.linalg.norm(o32["kp2"][0] - s["truth"], axis=1) <= err.max() + POS_TOL).all()


def test_oracle_guess_flat_region_and_loss_rules():
    s = FO.scene("shift")
    p1, p2 = FO.pyramid(s["f1"][None], 3), FO.pyramid(s["f2"][None], 3)
    g = np.broadcast_to(s["guess"], (1, FO.POINTS, 2))
    with_guess = FO.track(p1, p2, s["kp"][None], g, 7, FO.MAX_ITERATIONS, FO.EPSILON, FO.MIN_EIGEN)
    assert with_guess["status"].all() and with_guess["iterations"].sum() < s["o64"]["iterations"].sum()
    assert np.abs(with_guess["kp2"] - s["o64"]["kp2"]).max() < 0.02          # both stop within epsilon of one fixed point
    # a flat patch in frame 1 around a point, texture elsewhere
    f1 = s["f1"].copy()
    f1[20:60, 30:70] = 100.0
    q1 = FO.pyramid(f1[None], 1)
    kp = np.array([[[40.0, 50.0], [70.0, 15.0], [-1.0, -1.0], [np.nan, 5.0], [5.0, np.inf], [90.0, 5.0], [0.0, 0.0], [82.0, 96.0]]], np.float32)
    o = FO.track(q1, FO.pyramid(s["f2"][None], 1), kp, None, 7, 30, 0.01, 1e-3)
    assert o["code"][0].tolist()[:6] == [FO.FLAT, FO.OK, FO.PADDING, FO.PADDING, FO.PADDING, FO.PADDING]
    assert o["status"][0].tolist()[:6] == [0, 1, 0, 0, 0, 0] and (o["kp2"][0][[0, 2, 3, 4, 5]] == -1).all()
    assert not o["residual"][0][[0, 2, 3, 4, 5]].any() and not o["iterations"][0][[0, 2, 3, 4, 5]].any()
    assert set(o["code"][0][6:].tolist()) <= {FO.OK, FO.LEFT, FO.FLAT}       # corners of the frame: tracked or lost, never out of range
    # a guess that is not finite is padding; a huge finite one runs and leaves the frame
    g = np.zeros((1, 8, 2), np.float32)
    g[0, 1] = [np.nan, 0.0]
    o2 = FO.track(q1, FO.pyramid(s["f2"][None], 1), kp, g, 7, 30, 0.01, 1e-3)
    assert o2["code"][0, 1] == FO.PADDING
    g[0, 1] = [1e30, -1e30]
    assert FO.track(q1, FO.pyramid(s["f2"][None], 1), kp, g, 7, 30, 0.01, 1e-3)["code"][0, 1] == FO.LEFT


def test_oracle_replenish_on_hand_made_cases():
    h, w, cell = 83, 97, 16
    kp = np.array([[[5.0, 5.0], [-1.0, -1.0], [40.0, 40.0], [-1.0, -1.0], [-1.0, -1.0]]], np.float32)
    st = np.array([[1, 0, 1, 0, 0]], np.uint8)
    cand = np.array([[[20.0, 20.0], [21.0, 22.0],      # two candidates in one cell: the first wins
                      [6.0, 7.0],                      # in the cell of the live keypoint 0
                      [60.0, 90.0], [70.0, 10.0], [80.0, 50.0], [-1.0, -1.0]]], np.float32)
    out, new, counts = FO.replenish(kp, st, cand, [7], h, w, cell)
    assert counts.tolist() == [[2, 4, 3]]                                     # more accepted candidates than lost slots
    assert out[0].tolist() == [[5.0, 5.0], [20.0, 20.0], [40.0, 40.0], [60.0, 90.0], [70.0, 10.0]] and new[0].tolist() == [0, 1, 0, 1, 1]
    out, new, counts = FO.replenish(kp, st, cand, [3], h, w, cell)           # more lost slots than candidates
    assert counts.tolist() == [[2, 1, 1]] and out[0].tolist() == [[5.0, 5.0], [20.0, 20.0], [40.0, 40.0], [-1.0, -1.0], [-1.0, -1.0]]
    out, new, counts = FO.replenish(kp, st, cand, [0], h, w, cell)
    assert counts.tolist() == [[2, 0, 0]] and not new.any() and (out[0, [1, 3, 4]] == -1).all()
    out, new, counts = FO.replenish(kp, np.ones((1, 5), np.uint8), cand, [7], h, w, cell)     # nothing lost: the keypoints as they are
    assert counts[0, 0] == 5 and counts[0, 2] == 0 and np.array_equal(out, kp)
    assert FO.cell_of(82.9, 96.9, h, w, 16) == 5 * 7 + 6 and FO.cell_of(np.nan, 1e30, h, w, 16) == 6 and FO.cell_of(-5.0, -np.inf, h, w, 16) == 0


def test_oracle_check_on_each_status_combination():
    a = np.array([[[10.0, 10.0]] * 6], np.float32)
    back = np.array([[[10.3, 10.4], [10.3, 10.4], [10.3, 10.4], [10.3, 10.4], [13.0, 14.0], [np.nan, 10.0]]], np.float32)
    sf, sb = np.array([[1, 1, 0, 0, 1, 1]]), np.array([[1, 0, 1, 0, 1, 1]])
    assert not FO.check(a, back, sf, sb, 0.49)[0].any()                      # |(0.3, 0.4)| = 0.5: beyond 0.49, within 0.51
    st, fb = FO.check(a, back, sf, sb, 0.51)
    assert st[0].tolist() == [1, 0, 0, 0, 0, 0] and np.isinf(fb[0, 1:4]).all() and abs(fb[0, 0] - 0.5) < 1e-6 and abs(fb[0, 4] - 5) < 1e-6
    assert np.isnan(fb[0, 5])


# ---- tests/native/flow_host.cpp: the kernels' arithmetic, compiled for the host ------------------------------------------------------
flow_host = host_program("flow_host.cpp", hip=True)


@pytest.fixture(scope="module")
def flow_host_san(tmp_path_factory):
    """the same program under the host's address and undefined-behaviour sanitizers (a stand-alone program)"""
    return build_host(tmp_path_factory.mktemp("flow_host_san"), "flow_host.cpp", hip=True, extra=SANITIZE)


def native_pyramid(exe, frame, levels):
    h, w = frame.shape
    raw = run_host(exe, ["pyr", str(h), str(w), str(levels)], np.ascontiguousarray(frame, np.float32).tobytes(), binary=True)
    flat, out, o = np.frombuffer(raw, np.float32), [], 0
    for hl, wl in FO.level_shapes(h, w, levels):
        out.append(flat[o:o + hl * wl].reshape(hl, wl))
        o += hl * wl
    assert o == flat.size
    return out


def native_track(exe, f1, f2, levels, radius, kp, guess=None, max_iterations=FO.MAX_ITERATIONS, epsilon=FO.EPSILON, min_eigen=FO.MIN_EIGEN):
    h, w = f1.shape
    kp = np.ascontiguousarray(kp, np.float32)
    data = np.ascontiguousarray(f1, np.float32).tobytes() + np.ascontiguousarray(f2, np.float32).tobytes() + kp.tobytes()
    if guess is not None:
        data += np.ascontiguousarray(guess, np.float32).tobytes()
    raw = run_host(exe, ["track", str(h), str(w), str(levels), str(radius), str(max_iterations), "%.9g" % epsilon, "%.9g" % min_eigen,
                         str(len(kp)), "1" if guess is not None else "0"], data, binary=True)
    rec = np.frombuffer(raw, RECORD)
    assert len(rec) == len(kp)
    return dict(kp2=np.stack([rec["y"], rec["x"]], axis=1), status=rec["status"].astype(np.uint8), code=rec["code"].astype(np.uint8),
                residual=np.ascontiguousarray(rec["residual"]), iterations=rec["iterations"].astype(np.int32))


@pytest.mark.parametrize("shape", [(83, 97), (96, 80), (23, 24)])
def test_native_pyramid_is_the_float32_oracle_bit_for_bit(flow_host, shape):
    f = synth_flow_pair(11, *shape)[0]
    levels = 3 if shape[0] > 30 else 2
    for frame in (f, np.rint(f)):
        got, want = native_pyramid(flow_host, frame, levels), FO.pyramid(frame.astype(np.float32), levels, np.float32)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))


@pytest.mark.parametrize("name", sorted(FO.SCENES))
def test_native_tracker_matches_the_oracle_on_the_scenes(flow_host, name):
    """the kernel's arithmetic on the host against the float64 oracle within the measured tolerances (module docstring), under
    the 5 % cap, every point within the ground-truth bound; it is the float32 oracle bit for bit"""
    s = FO.scene(name)
    o64, o32 = s["o64"], s["o32"]
    got = native_track(flow_host, s["f1"], s["f2"], s["levels"], s["radius"], s["kp"])
    same = FO.comparable(got["status"], got["iterations"], o64)
    assert (~same).sum() <= CAP * FO.POINTS and np.array_equal(got["code"], o64["code"][0])
    dev = np.linalg.norm(got["kp2"].astype(np.float64) - o64["kp2"][0], axis=1)
    rdev = np.abs(got["residual"].astype(np.float64) - o64["residual"][0])
    print(f"{name}: native program, {same.sum()} comparable: position {dev[same].max():.3e} px, residual {rdev[same].max():.3e}")
    assert dev[same].max() <= POS_TOL / 2 * 1.01 and rdev[same].max() <= RES_TOL / 2 * 1.01
    bound = np.linalg.norm(o64["kp2"][0] - s["truth"], axis=1).max() + POS_TOL
    assert (np.linalg.norm(got["kp2"] - s["truth"], axis=1) <= bound).all()
    for key in ("kp2", "residual", "iterations", "status"):
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(o32[key][0]).view(np.uint8)), key


@pytest.mark.parametrize("radius", sorted(FO.BIT_CASES))
def test_native_tracker_bits_at_radius_1_and_at_the_other_lane_counts(flow_host, radius):
    """r = 1 (9 pixels in 64 lanes, five levels down to 6 x 7) and r = 6, 8, 9: the float32 oracle bit for bit; no accuracy is
    asked at these radii"""
    f1, f2, kp, levels, o32 = FO.bit_case(radius)
    got = native_track(flow_host, f1, f2, levels, radius, kp)
    assert np.array_equal(got["code"], o32["code"][0]) and 40 <= got["status"].sum()
    for key in ("kp2", "residual", "iterations", "status"):
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(o32[key][0]).view(np.uint8)), key
    if radius == 1:
        assert (got["code"] == FO.LEFT).sum() >= 1                           # aliased top levels: some points do leave


@pytest.mark.parametrize("name", ["shift", "l4r5"])
def test_points_that_diverge_on_the_top_level_are_lost_as_left(flow_host, name):
    """scene seed 0: one point of "shift" and two of "l4r5" diverge on the 21 x 25 top level and leave it.  The float32 oracle
    and the native program give the float64 oracle's codes; the other points stay within the tolerances and the cap"""
    s = FO.scene(name, seed=0)
    o64 = s["o64"]
    assert (o64["code"] == FO.LEFT).sum() == {"shift": 1, "l4r5": 2}[name] and set(o64["code"][0].tolist()) == {FO.OK, FO.LEFT}
    got = native_track(flow_host, s["f1"], s["f2"], s["levels"], s["radius"], s["kp"])
    for res in (dict((k, v[0]) for k, v in s["o32"].items() if k != "min_eig"), got):
        assert np.array_equal(res["code"], o64["code"][0]) and np.array_equal(res["status"], o64["status"][0])
        lost = res["status"] == 0
        assert (res["kp2"][lost] == -1).all() and not res["residual"][lost].any() and not res["iterations"][lost].any()
        same = FO.comparable(res["status"], res["iterations"], o64)
        assert (o64["status"][0] == 1).sum() - same.sum() <= CAP * FO.POINTS
        assert np.linalg.norm(res["kp2"].astype(np.float64) - o64["kp2"][0], axis=1)[same].max() <= POS_TOL
        assert np.abs(res["residual"].astype(np.float64) - o64["residual"][0])[same].max() <= RES_TOL


HOSTILE, HOSTILE_GUESS = FO.HOSTILE, FO.HOSTILE_GUESS


def test_native_tracker_on_hostile_keypoints_and_guesses(flow_host):
    """NaN, infinite and 1e30 keypoints and guesses, keypoints on the four borders and padding: the stated codes, no index out
    of range (the sanitized run below repeats this), and the one ordinary point is not disturbed"""
    s = FO.scene("shift")
    p1, p2 = FO.pyramid(s["f1"][None], 3, np.float32), FO.pyramid(s["f2"][None], 3, np.float32)
    for guess in (None, HOSTILE_GUESS):
        got = native_track(flow_host, s["f1"], s["f2"], 3, 7, HOSTILE, guess)
        want = FO.track(p1, p2, HOSTILE[None], None if guess is None else guess[None], 7, FO.MAX_ITERATIONS, FO.EPSILON, FO.MIN_EIGEN,
                        np.float32)
        assert got["code"][:7].tolist() == [FO.PADDING] * 7 and np.array_equal(got["code"], want["code"][0])
        assert np.array_equal(got["kp2"].view(np.uint32), want["kp2"][0].view(np.uint32))
        assert got["status"][13] == 1 and (got["kp2"][got["status"] == 0] == -1).all()
        if guess is not None:
            assert got["code"][7:10].tolist() == [FO.PADDING] * 3 and got["code"][10:13].tolist() == [FO.LEFT] * 3
            assert np.linalg.norm(got["kp2"][13] - (HOSTILE[13] + [-4.7, 6.3])) < 0.05
        else:
            assert set(got["code"][7:13].tolist()) <= {FO.OK, FO.LEFT, FO.FLAT}


def test_native_program_is_clean_under_the_host_sanitizers(flow_host, flow_host_san):
    """every mode once more under -fsanitize=address,undefined: the same output, no report (run_host checks stderr)"""
    s = FO.scene("shift")
    odd, even = synth_flow_pair(11, 83, 97)[0], synth_flow_pair(11, 96, 80)[0]
    for frame, levels in ((odd, 3), (even, 4), (odd[:23, :24], 2), (odd, 5)):
        assert all(np.array_equal(a, b) for a, b in zip(native_pyramid(flow_host_san, frame, levels), native_pyramid(flow_host, frame, levels)))
    for name, kp, guess in (("shift", HOSTILE, HOSTILE_GUESS), ("shift", HOSTILE, None), ("shift", s["kp"][:12], None),
                            ("l1r2", FO.scene("l1r2")["kp"][:12], None), ("big", FO.scene("big")["kp"][:6], None)):
        sc = FO.scene(name)
        a = native_track(flow_host_san, sc["f1"], sc["f2"], sc["levels"], sc["radius"], kp, guess)
        b = native_track(flow_host, sc["f1"], sc["f2"], sc["levels"], sc["radius"], kp, guess)
        assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    f1, f2, kp, levels, _ = FO.bit_case(1)                                   # r = 1, five levels, points that leave among them
    for k, g in ((kp[:24], None), (HOSTILE, HOSTILE_GUESS)):
        a, b = native_track(flow_host_san, f1, f2, levels, 1, k, g), native_track(flow_host, f1, f2, levels, 1, k, g)
        assert all(np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)) for key in a)
    pts = np.array([[np.nan, 1e30], [-np.inf, np.inf], [82.9, 96.9], [-1.0, -1.0], [16.0, 15.99]], np.float32)
    for exe in (flow_host, flow_host_san):
        raw = run_host(exe, ["cells", "83", "97", "16", str(len(pts))], pts.tobytes(), binary=True)
        assert np.frombuffer(raw, np.int32).tolist() == [FO.cell_of(y, x, 83, 97, 16) for y, x in pts] == [6, 6, 41, 0, 7]
