"""K34 camera rectification without a GPU: the section's own header and library and their exports, the host-side argument checks
of the four entries (MI_E_* before any launch, in the header's order of precedence), mi_rectify_stereo_rig (a host entry) against
the numpy oracle bit for bit with its properties and refusals, the kernels' arithmetic (csrc/rectify_math.h) compiled for the
host in tests/native/rectify_host.cpp, plain and under the host's address and undefined-behaviour sanitizers, bit for bit
against the oracle (tests/rectify_oracle.py), the modules' constructors, their refusal of CPU tensors and their export through
the `pytorch_model` alias, synth_distorted_rig, and three measurements on the oracle alone.

Measured with this file (the oracle):
  - the section's atan against numpy.arctan on 200001 points of [-50, 50] and 20001 logarithmic ones of [1e-12, 1e12], both
    signs: at most 4.45e-16 absolute and 4 ulp; asserted at 1e-15 and 8 ulp.  Its tan against numpy.tan on 150001 points of
    [0, 1.5]: at most 20 ulp, 2.6e-15 relative (tan's condition number at 1.5 is 21); asserted at 40 ulp and 6e-15.
  - round trip distort(undistort(p)) of 4000 raw pixels of the (41, 90) frame with the test coefficients, through the float32
    output: pinhole 7.1e-5 pixels after 10 iterations (the fixed-point iteration converges linearly), 1.8e-6 after 20 and 40;
    fisheye (Newton) 1.7e-6 after 10, 20 and 40: what is left is the float32 output, half an ulp of a normalised coordinate
    below 1 (3e-8) times the focal length (72) on either axis, 3e-6 pixels.  Asserted at 1.5e-4 (twice the measured) and 4e-6.
  - a float32 ramp 1.5 x - 0.75 y + 40 remapped through the rotated pinhole and fisheye maps of the (37, 83) case against
    1.5 sx - 0.75 sy + 40 at the float64 source position, where the mask is 1: at most 0.0350 gray levels.  The bound is reasoned,
    not measured: the map rounds a coordinate to 1/32 pixel, at most 1/64 off on either axis, so (1.5 + 0.75) / 64 = 0.0352,
    plus 1e-4 for the float32 steps.
  - mi_rectify_stereo_rig on six rigs: |R R^T - I| at most 4.4e-16 for r1 and 6.7e-16 for r2; the components of r1 c / |c| off
    (1, 0, 0) and of r2 t / |c| off (-1, 0, 0) at most 4.4e-16.  Asserted at 2e-15, three times the measured."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import rectify_oracle as RO
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.build import LIB, RECTIFY_LIB
from onnx_image_processing_amd.synth import synth_distorted_rig

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
NAMES = ["mi_rectify_map", "mi_rectify_points", "mi_rectify_remap", "mi_rectify_stereo_rig"]
MODELS = (RO.PINHOLE, RO.FISHEYE)


@pytest.fixture(scope="module")
def lib():
    return N.load_rectify()


_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 12)
    _keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


def doubles(values):
    flat = np.asarray(values, np.float64).reshape(-1)
    return (ctypes.c_double * len(flat))(*flat.tolist())


def _exported(path):
    r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return sorted(ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip())


K = RO.camera(41, 90)
KN = RO.new_camera(41, 90, 37, 83, RO.PINHOLE)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_section_has_a_header_and_a_library_of_its_own(lib):
    assert sorted(N.RECTIFY_SIGNATURES) == NAMES == _exported(RECTIFY_LIB)
    for other in (N.SIGNATURES, N.DEBUG_SIGNATURES, N.SIM3_SIGNATURES, N.SIMGRAPH_SIGNATURES, N.FLOW_SIGNATURES, N.STEREO_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert _exported(LIB) == sorted(N.SIGNATURES) and len(N.SIGNATURES) == 127          # the product library is what it was
    assert all(N.library_of(n) is lib for n in NAMES)
    assert N.library_of("mi_stereo_census") is N.load_stereo() and N.library_of("mi_flow_track") is N.load_flow()
    assert N.library_of("mi_depth_to_points") is N.load()
    assert N.load().mi_abi_version() == 3 and not any(hasattr(N.load(), n) for n in NAMES)
    assert N.RECTIFY_CONSTANTS == dict(
        MI_RECTIFY_COEFFS=RO.COEFFS, MI_RECTIFY_SUBPIXEL_BITS=RO.SUBPIXEL_BITS, MI_RECTIFY_OUTSIDE=RO.OUTSIDE, MI_RECTIFY_MAX_DIM=RO.MAX_DIM,
        MI_RECTIFY_MAX_BATCH=RO.MAX_BATCH, MI_RECTIFY_MAX_POINTS=RO.MAX_POINTS, MI_RECTIFY_MAX_ITERATIONS=RO.MAX_ITERATIONS,
        MI_RECTIFY_MAX_THETA=RO.MAX_THETA, MI_RECTIFY_PINHOLE=RO.PINHOLE, MI_RECTIFY_FISHEYE=RO.FISHEYE, MI_RECTIFY_U8=RO.U8,
        MI_RECTIFY_U16=RO.U16, MI_RECTIFY_F32=RO.F32, MI_RECTIFY_NEAREST=RO.NEAREST, MI_RECTIFY_LINEAR=RO.LINEAR)
    assert RO.OUTSIDE == -2147483648 and RO.MAX_DIM == 16384 and RO.SUBPIXEL_BITS == 5 and RO.COEFFS == 8
    assert N.RESTYPES["mi_rectify_remap"] is ctypes.c_int
    # the cameras are host arrays of doubles; the rig's outputs are host addresses handed through
    assert N.RECTIFY_SIGNATURES["mi_rectify_map"][1:5] == [ctypes.POINTER(ctypes.c_double)] * 4
    assert N.RECTIFY_SIGNATURES["mi_rectify_stereo_rig"][6:] == [ctypes.c_void_p] * 5


BAD_CAMERAS = [("skew", lambda k: k.__setitem__((0, 1), 0.01)), ("fx = 0", lambda k: k.__setitem__((0, 0), 0.0)),
               ("fy < 0", lambda k: k.__setitem__((1, 1), -3.0)), ("NaN", lambda k: k.__setitem__((0, 2), np.nan)),
               ("inf", lambda k: k.__setitem__((1, 2), np.inf)), ("last row", lambda k: k.__setitem__((2, 2), 2.0)),
               ("k[3]", lambda k: k.__setitem__((1, 0), 1e-9)), ("k[6]", lambda k: k.__setitem__((2, 0), 1.0))]


def bad_cameras():
    for name, spoil in BAD_CAMERAS:
        k = K.copy()
        spoil(k)
        yield name, k


def test_map_argument_checks(lib, p):
    f = lib.mi_rectify_map

    def call(**kw):
        a = dict(model=RO.PINHOLE, k=K, dist=RO.DIST[RO.PINHOLE], r=None, kn=KN, sh=41, sw=90, h=37, w=83, map=p, mask=p)
        a.update(kw)
        as_d = lambda v: None if v is None else doubles(v)
        return f(a["model"], as_d(a["k"]), as_d(a["dist"]), as_d(a["r"]), as_d(a["kn"]), a["sh"], a["sw"], a["h"], a["w"], a["map"], a["mask"], None)
    assert call(k=None) == NULL and call(dist=None) == NULL and call(kn=None) == NULL and call(map=None) == NULL
    for kw in (dict(sh=0), dict(sw=0), dict(h=0), dict(w=-1)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(sh=16385), dict(sw=16385), dict(h=16385), dict(w=1 << 30), dict(model=2), dict(model=-1)):
        assert call(**kw) == PARAM, kw
    for name, k in bad_cameras():
        assert call(k=k) == PARAM and call(kn=k) == PARAM, name
    for i in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            d = RO.DIST[RO.PINHOLE].copy()
            d[i] = bad
            assert call(dist=d) == PARAM, (i, bad)
    for i in range(4, 8):                                                      # the unused fisheye slots must be 0
        d = RO.DIST[RO.FISHEYE].copy()
        d[i] = 1e-12
        assert call(model=RO.FISHEYE, dist=d) == PARAM and call(model=RO.PINHOLE, dist=d, map=p + 4) == ALIGN, i    # legal for the pinhole
    r = RO.ROTATION.copy()
    r[1, 1] = np.nan
    assert call(r=r) == PARAM
    assert call(map=p + 4) == ALIGN and call(map=p + 2) == ALIGN
    # precedence: NULL, shape, parameters, alignment; refused by the rules, the fake pointers are never read
    assert call(k=None, sh=0) == NULL and call(sh=0, model=7, map=p + 4) == SHAPE and call(model=7, map=p + 4) == PARAM
    assert call(sh=16385, map=p + 4) == PARAM


def test_remap_argument_checks(lib, p):
    f = lib.mi_rectify_remap

    def call(**kw):
        a = dict(src=p, type=RO.U8, batch=3, sh=41, sw=90, map=p, h=37, w=83, interp=RO.LINEAR, border=0.0, dst=p)
        a.update(kw)
        return f(a["src"], a["type"], a["batch"], a["sh"], a["sw"], a["map"], a["h"], a["w"], a["interp"], a["border"], a["dst"], None)
    assert call(src=None) == NULL and call(map=None) == NULL and call(dst=None) == NULL
    for kw in (dict(batch=0), dict(sh=0), dict(sw=0), dict(h=0), dict(w=0), dict(batch=-4)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(batch=65537), dict(sh=16385), dict(sw=16385), dict(h=16385), dict(w=16385), dict(type=3), dict(type=-1), dict(interp=2),
               dict(interp=-1), dict(type=RO.U16), dict(type=RO.U16, interp=RO.LINEAR),                    # depth is not blended
               dict(border=-1.0), dict(border=256.0), dict(border=0.5), dict(border=np.nan), dict(border=np.inf),
               dict(type=RO.U16, interp=RO.NEAREST, border=65536.0), dict(type=RO.U16, interp=RO.NEAREST, border=-0.25)):
        assert call(**kw) == PARAM, kw
    assert call(type=RO.U16, interp=RO.NEAREST, border=65535.0, src=p + 1) == ALIGN                        # legal but for the alignment
    assert call(type=RO.F32, border=np.nan, dst=p + 2) == ALIGN and call(type=RO.F32, border=-1e30, src=p + 1) == ALIGN
    assert call(border=255.0, map=p + 4) == ALIGN and call(type=RO.U16, interp=RO.NEAREST, dst=p + 1) == ALIGN
    assert call(src=None, batch=0) == NULL and call(batch=0, type=9, map=p + 4) == SHAPE and call(type=9, map=p + 4) == PARAM
    assert call(border=300.0, map=p + 4) == PARAM


def test_points_argument_checks(lib, p):
    f = lib.mi_rectify_points

    def call(**kw):
        a = dict(pts=p, batch=2, n=63, model=RO.PINHOLE, k=K, dist=RO.DIST[RO.PINHOLE], r=None, kn=None, it=10, res=0.5, out=p, ok=p)
        a.update(kw)
        as_d = lambda v: None if v is None else doubles(v)
        return f(a["pts"], a["batch"], a["n"], a["model"], as_d(a["k"]), as_d(a["dist"]), as_d(a["r"]), as_d(a["kn"]), a["it"], a["res"],
                 a["out"], a["ok"], None)
    assert call(pts=None) == NULL and call(k=None) == NULL and call(dist=None) == NULL and call(out=None) == NULL and call(ok=None) == NULL
    assert call(batch=0) == SHAPE and call(n=0) == SHAPE and call(n=-5) == SHAPE
    for kw in (dict(batch=1 << 13, n=(1 << 11) + 1), dict(batch=1 << 30, n=1 << 30), dict(model=2), dict(it=0), dict(it=-1), dict(it=65),
               dict(res=0.0), dict(res=-1.0), dict(res=np.nan), dict(res=np.inf)):
        assert call(**kw) == PARAM, kw
    assert call(batch=1 << 13, n=1 << 11, out=p + 2) == ALIGN                  # 2^24 points are legal
    assert call(it=1, out=p + 2) == ALIGN and call(it=64, pts=p + 1) == ALIGN  # both ends of the iteration count are legal
    for name, k in bad_cameras():
        assert call(k=k) == PARAM and call(kn=k) == PARAM, name
    d = RO.DIST[RO.PINHOLE].copy()
    d[7] = np.nan
    assert call(dist=d) == PARAM
    d = RO.DIST[RO.FISHEYE].copy()
    d[4] = 0.5
    assert call(model=RO.FISHEYE, dist=d) == PARAM
    assert call(kn=KN, r=RO.ROTATION, out=p + 2) == ALIGN
    assert call(pts=None, n=0) == NULL and call(n=0, it=0, out=p + 2) == SHAPE and call(it=0, out=p + 2) == PARAM


# ---- mi_rectify_stereo_rig: a host entry, run here ----------------------------------------------------------------------------------
def rig_inputs(i):
    """six rigs: (k1, k2, R, t, h, w)"""
    k1, k2 = RO.camera(480, 640), RO.camera(480, 640, 0.83)
    r = [np.eye(3), RO.rotation(0.01, -0.02, 0.005), RO.rotation(-0.05, 0.08, -0.03), RO.rotation(0.2, 0.1, -0.15), RO.rotation(0.0, 0.3, 0.0),
         RO.rotation(0.002, 0.001, -0.001)][i]
    c = [np.array([0.12, 0.0, 0.0]), np.array([0.1, 0.003, -0.002]), np.array([0.5, -0.05, 0.04]), np.array([0.075, 0.02, 0.03]),
         np.array([1.0, 0.0, 0.4]), np.array([64.0, 1.0, -2.0])][i]
    return k1, k2, r, -r @ c, (480, 37, 41, 1, 720, 16384)[i], (640, 83, 90, 70, 1280, 1)[i]


def rig_call(lib, k1, k2, r, t, h, w):
    out = [(ctypes.c_double * 9)() for _ in range(3)] + [ctypes.c_double(), ctypes.c_double()]
    st = lib.mi_rectify_stereo_rig(doubles(k1), doubles(k2), doubles(r), doubles(t), h, w, out[0], out[1], out[2], ctypes.byref(out[3]),
                                   ctypes.byref(out[4]))
    return st, [np.array(list(a)).reshape(3, 3) for a in out[:3]] + [out[3].value, out[4].value]


@pytest.mark.parametrize("i", range(6))
def test_stereo_rig_is_the_oracle_bit_for_bit(lib, i):
    st, got = rig_call(lib, *rig_inputs(i))
    want = RO.stereo_rig(*rig_inputs(i))
    assert st == 0 and want is not None
    for g, o in zip(got, want):
        assert np.array_equal(np.asarray(g, np.float64).view(np.uint64), np.asarray(o, np.float64).view(np.uint64))


def test_stereo_rig_properties(lib):
    """r1 and r2 are orthonormal, camera 2's centre lies on the x axis of the rectified camera 1 (r1 c = (|c|, 0, 0)) and camera
    1's centre on the negative x axis of the rectified camera 2 (r2 t = (-|c|, 0, 0)); measured over the six
    rigs: orthonormality 4.4e-16 (r1) and 6.7e-16 (r2), the off-axis components relative to |c| 4.4e-16.  Asserted at 2e-15, three
    times the measured."""
    worst = [0.0, 0.0, 0.0]
    for i in range(6):
        k1, k2, r, t, h, w = rig_inputs(i)
        st, (r1, r2, k_new, baseline, fb) = rig_call(lib, k1, k2, r, t, h, w)
        assert st == 0
        c = -r.T @ t
        worst[0] = max(worst[0], np.abs(r1 @ r1.T - np.eye(3)).max())
        worst[1] = max(worst[1], np.abs(r2 @ r2.T - np.eye(3)).max())
        a, b = r1 @ c / baseline, r2 @ t / baseline
        worst[2] = max(worst[2], np.abs(a - [1, 0, 0]).max(), np.abs(b - [-1, 0, 0]).max())
        assert np.linalg.det(r1) > 0.999 and abs(baseline - np.linalg.norm(c)) <= 1e-15 * baseline
        f = (k1[1, 1] + k2[1, 1]) / 2
        assert np.array_equal(k_new, [[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]]) and fb == f * baseline
        # a point seen by both cameras lands on one row of both rectified views
        x1 = np.array([0.3, -0.2, 4.0]) * np.linalg.norm(c)
        x2 = r @ x1 + t
        p1, p2 = r1 @ x1, r2 @ x2
        assert abs(p1[1] / p1[2] - p2[1] / p2[2]) < 1e-14 and p1[0] / p1[2] > p2[0] / p2[2] and abs(p1[2] - p2[2]) < 1e-13 * p1[2]
    print(f"stereo rig: |r1 r1^T - I| {worst[0]:.3g}, |r2 r2^T - I| {worst[1]:.3g}, off-axis {worst[2]:.3g}")
    assert max(worst) <= 2e-15


def test_stereo_rig_refusals(lib):
    k1, k2, r, t, h, w = rig_inputs(1)
    call = lambda **kw: rig_call(lib, **{**dict(k1=k1, k2=k2, r=r, t=t, h=h, w=w), **kw})[0]
    assert call() == 0
    assert call(t=np.zeros(3)) == PARAM                                         # no baseline
    assert call(t=-t) == PARAM                                                  # swapped: camera 2 is on the left
    assert call(t=-r @ np.array([0.0, 0.1, 0.0])) == PARAM and call(t=-r @ np.array([0.05, -0.1, 0.0])) == PARAM       # vertical
    assert call(r=np.eye(3), t=np.array([0.0, 0.0, -0.1])) == PARAM             # x does not point to +x
    assert call(r=RO.rotation(0.0, np.pi / 2, 0.0) @ RO.rotation(0.0, np.pi / 2, 0.0), t=np.array([0.1, 0.0, 0.0])) == PARAM   # opposite axes
    for bad in (np.nan, np.inf):
        assert call(t=np.array([bad, 0.0, 0.0])) == PARAM and call(t=np.array([-0.1, 0.0, bad])) == PARAM
        rr = r.copy()
        rr[2, 0] = bad
        assert call(r=rr) == PARAM
    assert call(t=np.array([-1e200, 0.0, 0.0])) == PARAM                        # |t| overflows
    for name, k in bad_cameras():
        assert call(k1=k) == PARAM and call(k2=k) == PARAM, name
    assert call(h=0) == SHAPE and call(w=0) == SHAPE and call(h=16385) == PARAM and call(w=16385) == PARAM
    d9, d3 = doubles(np.eye(3)), doubles(t)
    out = (ctypes.c_double * 9)()
    one = ctypes.c_double()
    f = lib.mi_rectify_stereo_rig
    assert f(None, d9, d9, d3, 4, 4, out, out, out, ctypes.byref(one), ctypes.byref(one)) == NULL
    assert f(d9, d9, d9, None, 4, 4, out, out, out, ctypes.byref(one), ctypes.byref(one)) == NULL
    assert f(d9, d9, d9, d3, 4, 4, out, None, out, ctypes.byref(one), ctypes.byref(one)) == NULL
    assert f(d9, d9, d9, d3, 0, 4, out, out, out, ctypes.byref(one), None) == NULL


# ---- the modules, the functional layer and the synthetic rig --------------------------------------------------------------------------
def test_modules_constructors_cpu_refusal_and_alias():
    import onnx_image_processing_amd.pytorch_model.calibration as real
    import pytorch_model
    from onnx_image_processing_amd import ops
    from pytorch_model.calibration import StereoRectifier, Undistorter
    from pytorch_model.calibration.rectification import Undistorter as again
    assert Undistorter is real.Undistorter is again and StereoRectifier is real.StereoRectifier
    assert real.__all__ == ["Undistorter", "StereoRectifier"] and "Undistorter" in pytorch_model.__doc__ and "StereoRectifier" in pytorch_model.__doc__
    assert (ops.RECTIFY_PINHOLE, ops.RECTIFY_FISHEYE, ops.RECTIFY_NEAREST, ops.RECTIFY_LINEAR, ops.RECTIFY_OUTSIDE) == (0, 1, 0, 1, RO.OUTSIDE)
    d = RO.DIST[RO.PINHOLE]
    for kw in (dict(model="brown"), dict(camera_matrix=np.eye(4)), dict(dist_coeffs=d[:3]), dict(dist_coeffs=d[:5], model="fisheye"),
               dict(size=(0, 90)), dict(size=(41, 16385)), dict(out_size=(41, 0)), dict(interpolation="cubic"), dict(iterations=0),
               dict(iterations=65), dict(max_residual_px=0.0), dict(new_camera_matrix=np.eye(2)), dict(rotation=np.zeros(3))):
        with pytest.raises(ValueError):
            Undistorter(**{**dict(camera_matrix=K, dist_coeffs=d, size=(41, 90), device="cpu"), **kw})
    with pytest.raises(RuntimeError, match="no CPU path"):                       # the map lives on the GPU
        Undistorter(K, d, (41, 90), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rectify_map(K, d[:5], (41, 90), K, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rectify_remap(torch.zeros(1, 41, 90), torch.zeros(37, 83, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rectify_points(torch.zeros(1, 5, 2), K, d)
    assert list(ops.rectify_coeffs(d[:5], RO.PINHOLE)) == list(d[:5]) + [0.0] * 3 and list(ops.rectify_coeffs(None, RO.FISHEYE)) == [0.0] * 8
    # the rig runs on the host: the functional layer gives the oracle's bits, and a rig that cannot be rectified is a ValueError
    k1, k2, r, t, h, w = rig_inputs(2)
    got, want = ops.rectify_stereo_rig(k1, k2, r, t, (h, w)), RO.stereo_rig(k1, k2, r, t, h, w)
    assert all(np.array_equal(np.asarray(g, np.float64), np.asarray(o, np.float64)) for g, o in zip(got, want))
    with pytest.raises(ValueError, match="cannot be rectified"):
        StereoRectifier(k1, d, k2, d, r, -t, (h, w), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        StereoRectifier(k1, d, k2, d, r, t, (h, w), device="cpu")


def test_synth_distorted_rig_is_what_it_says_and_deterministic():
    a, b = synth_distorted_rig(3, 40, 160), synth_distorted_rig(3, 40, 160)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    left, right, rig = a
    assert left.shape == right.shape == (40, 160) and left.dtype == right.dtype == np.float32 and 0 <= left.min() and left.max() <= 255
    assert left.std() > 8 and not np.array_equal(left, synth_distorted_rig(4, 40, 160)[0])
    assert rig["disparity"] == 12.0 and abs(rig["focal"] * rig["baseline"] / rig["depth"] - 12.0) < 1e-12
    r1, r2, k_new, baseline, fb = RO.stereo_rig(rig["k1"], rig["k2"], rig["R"], rig["T"], 40, 160)
    assert abs(baseline - rig["baseline"]) < 1e-15 and abs(fb / rig["depth"] - 12.0) < 1e-12 and k_new[0, 0] == rig["focal"]
    assert np.abs(rig["R"] @ rig["R"].T - np.eye(3)).max() < 1e-15 and 0.02 < np.abs(rig["R"] - np.eye(3)).max() < 0.1
    q = synth_distorted_rig(3, 40, 160, quantise=True)
    assert q[0].dtype == np.uint8 and np.abs(q[0].astype(np.float32) - left).max() <= 0.5
    fish = synth_distorted_rig(3, 40, 160, "fisheye")
    assert fish[2]["model"] == "fisheye" and (fish[2]["d1"][4:] == 0).all() and not np.array_equal(fish[0], left)
    # the views are what the rig sees: the oracle's rectification of them agrees along a row shifted by the disparity (far from
    # the border, where both taps exist), within the interpolation error of the texture
    ml, mkl = RO.rectify_map(RO.PINHOLE, rig["k1"], rig["d1"], r1, k_new, 40, 160, 40, 160)
    mr, mkr = RO.rectify_map(RO.PINHOLE, rig["k2"], rig["d2"], r2, k_new, 40, 160, 40, 160)
    l, r = RO.remap(left[None], ml, RO.LINEAR, 0)[0], RO.remap(right[None], mr, RO.LINEAR, 0)[0]
    both = (mkl[8:-8, 32:-16] == 1) & (mkr[8:-8, 20:-28] == 1)
    diff = np.abs(l[8:-8, 32:-16] - r[8:-8, 20:-28])[both]
    raw = np.abs(left[8:-8, 32:-16] - right[8:-8, 20:-28])
    print(f"rectified views, 12 pixels apart: mean |difference| {diff.mean():.2f} gray levels of {both.sum()} pixels; raw views {raw.mean():.2f}")
    assert both.mean() > 0.9 and diff.mean() < 0.25 * raw.mean()
    for bad in (dict(height=0), dict(width=0), dict(model="brown"), dict(disparity=0.0), dict(terms=0), dict(lam=(0.0, 4.0))):
        with pytest.raises(ValueError):
            synth_distorted_rig(**{**dict(seed=0, height=8, width=8), **bad})


# ---- measurements on the oracle alone ---------------------------------------------------------------------------------------------------
def trig_inputs():
    x = np.concatenate([np.linspace(-50.0, 50.0, 200001), np.logspace(-12, 12, 20001), -np.logspace(-12, 12, 20001)])
    return x, np.linspace(0.0, 1.5, 150001)


def test_oracle_atan_and_tan_against_numpy():
    x, t = trig_inputs()
    ea = np.abs(RO.atan(x) - np.arctan(x))
    et = np.abs(RO.tan(t) - np.tan(t))
    ulp_a = (ea / np.spacing(np.abs(np.arctan(x)))).max()
    ulp_t, rel_t = (et[1:] / np.spacing(np.tan(t[1:]))).max(), (et[1:] / np.tan(t[1:])).max()
    print(f"atan: {ea.max():.3g} absolute, {ulp_a:.0f} ulp; tan on [0, 1.5]: {ulp_t:.0f} ulp, {rel_t:.3g} relative")
    assert ea.max() <= 1e-15 and ulp_a <= 8 and ulp_t <= 40 and rel_t <= 6e-15
    assert RO.atan(0.0) == 0.0 and RO.tan(0.0) == 0.0 and RO.atan(np.inf) == 1.5707963267948966 and RO.atan(-np.inf) == -1.5707963267948966
    assert np.isnan(RO.atan(np.nan)) and abs(RO.atan(1.0) - np.pi / 4) <= 2.3e-16


def test_oracle_round_trip_of_points():
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, 89, 4000), rng.uniform(0, 40, 4000)], -1).astype(np.float32)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    worst = {}
    for model in MODELS:
        for it in (10, 20, 40):
            out, ok = RO.undistort_points(pts, model, K, RO.DIST[model], iterations=it, max_residual_px=5.0)
            assert ok.all()
            xd, yd, has = RO.distort(model, RO.DIST[model], out[:, 0].astype(np.float64), out[:, 1].astype(np.float64))
            worst[model, it] = float(np.hypot(fx * xd + cx - pts[:, 0], fy * yd + cy - pts[:, 1]).max())
    print("round trip in pixels (through the float32 output):", {k: f"{v:.3g}" for k, v in worst.items()})
    assert worst[RO.PINHOLE, 10] <= 1.5e-4 and all(v <= 4e-6 for key, v in worst.items() if key != (RO.PINHOLE, 10))


def test_oracle_remap_of_a_ramp_against_its_closed_form():
    a, b, c = 1.5, -0.75, 40.0
    y, x = np.mgrid[0:41, 0:90].astype(np.float64)
    ramp = (a * x + b * y + c).astype(np.float32)[None]
    worst = 0.0
    for model in MODELS:
        k, dist, r, k_new, m, mask = RO.map_case(model, True, RO.MAP_SHAPES[0])
        v, u = np.mgrid[0:37, 0:83].astype(np.float64)
        ray = np.stack([(u - k_new[0, 2]) / k_new[0, 0], (v - k_new[1, 2]) / k_new[1, 1], np.ones_like(u)], -1) @ r     # R^T d, row-wise
        xd, yd, _ = RO.distort(model, dist, ray[..., 0] / ray[..., 2], ray[..., 1] / ray[..., 2])
        sx, sy = k[0, 0] * xd + k[0, 2], k[1, 1] * yd + k[1, 2]
        got = RO.remap(ramp, m, RO.LINEAR, 0.0)[0]
        err = np.abs(got - (a * sx + b * sy + c))[mask == 1]
        assert (mask == 1).sum() > 500
        worst = max(worst, float(err.max()))
        # and the map itself is the rounded source position
        inside = m[..., 0] != RO.OUTSIDE
        assert np.abs(m[..., 0][inside] / 32.0 - sx[inside]).max() <= 1 / 64 + 1e-9 and np.abs(m[..., 1][inside] / 32.0 - sy[inside]).max() <= 1 / 64 + 1e-9
    print(f"ramp through the map against its closed form: {worst:.4f} gray levels")
    assert worst <= (abs(a) + abs(b)) / 64 + 1e-4


def test_oracle_on_hand_made_maps():
    src = np.arange(12, dtype=np.uint8).reshape(1, 3, 4) * 10
    m = np.array([[[0, 0], [32, 32], [16, 0], [0, 48], [-32, 0], [-16, 0], [96, 64], [112, 64], [RO.OUTSIDE, 0], [0, RO.OUTSIDE],
                   [3 * 32 + 16, 2 * 32 + 16], [2 ** 31 - 1, 5], [-2 ** 31 + 1, 0]]], np.int32)
    lin = RO.remap(src, m, RO.LINEAR, 200)[0, 0].tolist()
    #      p00   p11  x half  y half+   X=-1,a=0  X=-1,a=16      corner  beyond       sentinels  corner+half          far
    assert lin == [0, 50, 5, 60, 200, 100, 110, (110 + 200 + 1) // 2, 200, 200, (110 + 3 * 200 + 2) // 4, 200, 200]
    near = RO.remap(src, m, RO.NEAREST, 200)[0, 0].tolist()
    assert near == [0, 50, 10, 80, 200, 0, 110, 200, 200, 200, 200, 200, 200]      # ties go up: (q + 16) >> 5
    f = src.astype(np.float32)
    f[0, 0, 1] = np.nan
    got = RO.remap(f, m[:, :3], RO.LINEAR, np.nan)[0, 0]
    assert got[0] == 0.0 and got[1] == 50.0 and np.isnan(got[2])                # a = 0 beside a NaN is p00 exactly
    assert RO.remap(f, np.array([[[-32, 0]]], np.int32), RO.LINEAR, np.inf)[0, 0, 0] == np.inf


# ---- tests/native/rectify_host.cpp: the kernels' arithmetic, compiled for the host -----------------------------------------------------
rectify_host = host_program("rectify_host.cpp", hip=True)


@pytest.fixture(scope="module")
def rectify_host_san(tmp_path_factory):
    """the same program under the host's address and undefined-behaviour sanitizers (a stand-alone program)"""
    return build_host(tmp_path_factory.mktemp("rectify_host_san"), "rectify_host.cpp", hip=True, extra=SANITIZE)


def camera_args(k, dist, r, k_new):
    values = np.concatenate([np.asarray(k, np.float64).reshape(9), np.asarray(dist, np.float64), (np.eye(3) if r is None else np.asarray(r)).reshape(9),
                             (np.zeros(9) if k_new is None else np.asarray(k_new, np.float64).reshape(9))])
    return ["%.17g" % v for v in values]


def native_trig(exe, x):
    raw = run_host(exe, ["trig", str(len(x))], np.asarray(x, np.float64).tobytes(), binary=True)
    out = np.frombuffer(raw, np.float64)
    return out[:len(x)], out[len(x):]


def native_map(exe, model, k, dist, r, k_new, sh, sw, h, w):
    raw = run_host(exe, ["map", str(model), str(sh), str(sw), str(h), str(w)] + camera_args(k, dist, r, k_new), b"", binary=True)
    assert len(raw) == h * w * 9
    return np.frombuffer(raw[:h * w * 8], np.int32).reshape(h, w, 2), np.frombuffer(raw[h * w * 8:], np.uint8).reshape(h, w)


def native_remap(exe, src, m, interpolation, border):
    type_ = {np.dtype(np.uint8): RO.U8, np.dtype(np.uint16): RO.U16, np.dtype(np.float32): RO.F32}[src.dtype]
    b, sh, sw = src.shape
    h, w = m.shape[:2]
    raw = run_host(exe, ["remap", str(type_), str(interpolation), str(b), str(sh), str(sw), str(h), str(w), "%.17g" % border],
                   np.ascontiguousarray(m).tobytes() + np.ascontiguousarray(src).tobytes(), binary=True)
    return np.frombuffer(raw, src.dtype).reshape(b, h, w)


def native_points(exe, pts, model, k, dist, r, k_new, iterations=10, max_residual_px=0.5):
    count = pts.size // 2
    raw = run_host(exe, ["points", str(model), str(count), str(iterations), "%.17g" % max_residual_px, str(int(k_new is not None))] +
                   camera_args(k, dist, r, k_new), np.ascontiguousarray(pts, np.float32).tobytes(), binary=True)
    assert len(raw) == count * 9
    return np.frombuffer(raw[:count * 8], np.float32).reshape(pts.shape), np.frombuffer(raw[count * 8:], np.uint8).reshape(pts.shape[:-1])


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differ = got.view(np.uint8) != want.view(np.uint8)
    assert not differ.any(), f"{what}: {int(differ.sum())} bytes of {differ.size} differ from the oracle"


def hostile_map(m, seed):
    """a map with sentinels in one component only, far and negative elements and the int32 extremes sprinkled in"""
    rng = np.random.default_rng(seed)
    out = m.copy()
    flat = out.reshape(-1)
    pick = rng.random(flat.size) < 0.05
    flat[pick] = rng.choice(np.array([RO.OUTSIDE, 2 ** 31 - 1, -2 ** 31 + 1, -1, -32, -33, 1 << 20, -(1 << 20), 2 ** 31 - 17], np.int64),
                            int(pick.sum())).astype(np.int32)
    return out


def test_native_atan_and_tan_are_the_oracle_bit_for_bit(rectify_host):
    x, t = trig_inputs()
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-320, 1e300, np.tan(np.pi / 16)])
    a, _ = native_trig(rectify_host, np.concatenate([x, special]))
    same(a, RO.atan(np.concatenate([x, special])), "atan")
    _, tn = native_trig(rectify_host, t)
    same(tn, RO.tan(t), "tan")


@pytest.mark.parametrize("shape", RO.MAP_SHAPES, ids=str)
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_native_map_remap_and_points_are_the_oracle_bit_for_bit(rectify_host, model, rotated, shape):
    sh, sw, h, w = shape
    k, dist, r, k_new, m, mask = RO.map_case(model, rotated, shape)
    gm, gmask = native_map(rectify_host, model, k, dist, r, k_new, sh, sw, h, w)
    same(gm, m, "map")
    same(gmask, mask, "mask")
    for type_ in (RO.U8, RO.U16, RO.F32):
        src = RO.frames(31 + type_, 2, sh, sw, type_)
        for interpolation in (RO.NEAREST, RO.LINEAR):
            if type_ == RO.U16 and interpolation == RO.LINEAR:
                continue
            border = {RO.U8: 7, RO.U16: 40000, RO.F32: -3.25}[type_]
            same(native_remap(rectify_host, src, m, interpolation, border), RO.remap(src, m, interpolation, border), (type_, interpolation))
    for n, knew in ((63, None), (65, k_new)):
        pts = RO.points(17, 1, n, sh, sw)
        want = RO.undistort_points(pts, model, k, dist, r, knew)
        got = native_points(rectify_host, pts, model, k, dist, r, knew)
        same(got[0], want[0], "points")
        same(got[1], want[1], "ok")
        assert 0 < want[1].sum() < want[1].size                                  # failures are present, and successes


def test_native_remap_on_hostile_frames_and_maps(rectify_host):
    """NaN, infinite and 1e30 gray values, a NaN border, and maps that hold sentinels in one component, the int32 extremes and
    far elements: the oracle's bits, and every index stays inside the frame (the sanitizer run below repeats it)"""
    k, dist, r, k_new, m, mask = RO.map_case(RO.PINHOLE, True, RO.MAP_SHAPES[0])
    src = RO.hostile_frames(13, 2, 41, 90)
    assert np.isnan(src).any() and np.isinf(src).any()
    for mm in (m, hostile_map(m, 3)):
        for interpolation in (RO.NEAREST, RO.LINEAR):
            for border in (0.0, np.nan, -np.inf, 1e30):
                same(native_remap(rectify_host, src, mm, interpolation, border), RO.remap(src, mm, interpolation, border), (interpolation, border))
        u8 = RO.frames(14, 1, 41, 90, RO.U8)
        same(native_remap(rectify_host, u8, mm, RO.LINEAR, 255), RO.remap(u8, mm, RO.LINEAR, 255), "u8")
        u16 = RO.frames(15, 1, 41, 90, RO.U16)
        same(native_remap(rectify_host, u16, mm, RO.NEAREST, 65535), RO.remap(u16, mm, RO.NEAREST, 65535), "u16")
    # exact-integer map elements give the source value itself, even beside a NaN
    exact = ((m[..., 0] & 31) == 0) & ((m[..., 1] & 31) == 0) & (m[..., 0] != RO.OUTSIDE) & (mask == 1)
    assert exact.any()
    got = native_remap(rectify_host, src, m, RO.LINEAR, 0.0)
    want = src[:, m[..., 1][exact] >> 5, m[..., 0][exact] >> 5]
    assert np.array_equal(got[:, exact].view(np.uint32), want.view(np.uint32))


def test_native_points_on_hostile_points_and_at_the_ends_of_the_parameters(rectify_host):
    k, k_new = RO.camera(41, 90), RO.new_camera(41, 90, 37, 83, RO.PINHOLE)
    pts = RO.points(19, 2, 200, 41, 90)
    pts[0, 5], pts[0, 6], pts[1, 7] = (np.inf, 3.0), (-1e30, -1e30), (k[0, 2], k[1, 2])          # ... and the principal point itself
    assert np.isnan(pts).any()
    for model in MODELS:
        for kw in (dict(iterations=1), dict(iterations=64), dict(max_residual_px=1e-6), dict(max_residual_px=1e6), dict(iterations=3, max_residual_px=0.05)):
            for r, knew in ((None, None), (RO.ROTATION, k_new), (RO.rotation(0.0, 2.0, 0.0), None)):       # the last one looks backwards
                want = RO.undistort_points(pts, model, k, RO.DIST[model], r, knew, **kw)
                got = native_points(rectify_host, pts, model, k, RO.DIST[model], r, knew, **kw)
                same(got[0], want[0], (model, kw))
                same(got[1], want[1], (model, kw))
                assert np.isfinite(got[0]).all() and (got[0][got[1] == 0] == 0).all() and not got[1][0, 1] and not got[1][0, 5] and not got[1][0, 6]
        want = RO.undistort_points(pts, model, k, RO.DIST[model])
        assert want[1][1, 7] == 1 and np.abs(want[0][1, 7]).max() == 0.0 and 0.5 < want[1].mean() < 0.95


def test_native_program_is_clean_under_the_host_sanitizers(rectify_host, rectify_host_san):
    """every branch once more under -fsanitize=address,undefined: the same output, no report (run_host checks stderr)"""
    x = np.concatenate([np.linspace(-3, 3, 1001), [np.nan, np.inf, -np.inf, 1e300, 0.0]])
    for a, b in zip(native_trig(rectify_host_san, x), native_trig(rectify_host, x)):
        same(a, b, "trig")
    for model in MODELS:
        for rotated, shape in ((True, RO.MAP_SHAPES[0]), (False, RO.MAP_SHAPES[3]), (True, RO.MAP_SHAPES[1]), (True, RO.MAP_SHAPES[2])):
            sh, sw, h, w = shape
            k, dist, r, k_new, m, mask = RO.map_case(model, rotated, shape)
            gm, gmask = native_map(rectify_host_san, model, k, dist, r, k_new, sh, sw, h, w)
            same(gm, m, "map")
            same(gmask, mask, "mask")
            for src, interpolation, border in ((RO.frames(31, 2, sh, sw, RO.U8), RO.LINEAR, 255), (RO.frames(31, 2, sh, sw, RO.U8), RO.NEAREST, 0),
                                               (RO.frames(32, 2, sh, sw, RO.U16), RO.NEAREST, 65535), (RO.hostile_frames(13, 2, sh, sw), RO.LINEAR, np.nan),
                                               (RO.hostile_frames(13, 2, sh, sw), RO.NEAREST, 1e30)):
                for mm in (m, hostile_map(m, 3)):
                    same(native_remap(rectify_host_san, src, mm, interpolation, border), RO.remap(src, mm, interpolation, border), (shape, interpolation))
            pts = RO.points(19, 2, 200, sh, sw)
            pts[0, 5], pts[0, 6] = (np.inf, 3.0), (-1e30, 1e30)
            for r2, knew, it in ((r, k_new, 10), (None, None, 64), (RO.rotation(0.0, 2.0, 0.0), None, 1)):
                want = RO.undistort_points(pts, model, k, dist, r2, knew, iterations=it)
                got = native_points(rectify_host_san, pts, model, k, dist, r2, knew, iterations=it)
                same(got[0], want[0], "points")
                same(got[1], want[1], "ok")
    # a camera whose pinhole denominator turns negative inside the frame, and one whose map overflows every range test
    for dist, k in ((np.array([0.1, 0.0, 0.0, 0.0, 0.0, -9.0, 0.0, 0.0]), RO.camera(41, 90)), (np.array([1e300, 1e300, 0, 0, 1e300, 0, 0, 0.0]), RO.camera(41, 90, 1e6))):
        want = RO.rectify_map(RO.PINHOLE, k, dist, None, RO.camera(41, 90, 0.5), 41, 90, 37, 83)
        got = native_map(rectify_host_san, RO.PINHOLE, k, dist, None, RO.camera(41, 90, 0.5), 41, 90, 37, 83)
        same(got[0], want[0], "map")
        same(got[1], want[1], "mask")
        assert (want[0] == RO.OUTSIDE).any()
