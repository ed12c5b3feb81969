"""CPU-only checks of the K13 depth front end: the reference's import lines resolve, the modules keep the reference's
constructor contract and refuse CPU tensors, mi_depth_to_points / mi_depth_align refuse bad arguments on the host before
any launch, and three numpy oracles (written here, independent of the kernels) reproduce the reference fixture:

  points     bit for bit;
  normals    within tol = 18 * eps32 * max(sum |w_i p_i| over the dx taps, the same over the dy taps) + 4 * eps32 of a
             float64 evaluation of the same float32 points.  The reference's convolution adds 18 non-zero products per
             output in an order its backend chooses (each partial sum is bounded by sum |w_i p_i|, 17 additions and the
             products' own roundings: 18 eps), and the normaliser divides by a norm >= 1, so an absolute error of dx / dy
             cannot grow; 4 eps covers the square root, the division and the final rounding;
  alignment  exactly at every CLEAN target pixel, and oracle <= reference wherever the oracle is non-zero.  A target is
             clean when each of the reference's four splat images has at most one writer there and no source that
             mi_depth_align silences (out of frame, depth <= 0 or >= 10000) writes it in the reference; everywhere else
             the reference's result depends on which duplicate index its index_put_ keeps.  Clean pixels must be at
             least 60 % of every case, so that the comparison cannot quietly shrink to nothing.

The GPU tests then measure the kernels against these oracles."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import native_lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_frontend.npz")
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
SOBEL_V = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], np.float64)
SOBEL_H = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], np.float64)


def tables_oracle(scale, width, height, cx, cy, fx, fy):
    """(u_tab, v_tab, z_scale) in float32: subtract, IEEE divide, multiply -- the columns of the reference's `uv`."""
    u = ((np.arange(width, dtype=F32) - F32(cx)) / F32(fx)) * F32(scale)
    v = ((np.arange(height, dtype=F32) - F32(cy)) / F32(fy)) * F32(scale)
    return u.astype(F32), v.astype(F32), F32(1.0) * F32(scale)


def points_oracle(depth, u_tab, v_tab, z_scale):
    """depth (..., H, W) of any real dtype -> float32 points (..., H, W, 3): one float32 product per coordinate."""
    d = np.asarray(depth).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([d * u_tab[None, :], d * v_tab[:, None], d * F32(z_scale)], -1).astype(F32)


def normals_oracle(points):
    """float32 points (H, W, 3) -> (normals float64 (H, W, 3), tol (H, W)): float64 Sobel responses of X + Y + Z with
    zero padding, n = (dx, dy, -1) / |.|, and the bound of the module docstring."""
    p = np.asarray(points, F32).astype(np.float64)
    h, w = p.shape[:2]
    s = np.zeros((h + 2, w + 2))
    a = np.zeros((h + 2, w + 2))
    s[1:-1, 1:-1] = p.sum(-1)
    a[1:-1, 1:-1] = np.abs(p).sum(-1)
    dx = np.zeros((h, w))
    dy = np.zeros((h, w))
    ax = np.zeros((h, w))
    ay = np.zeros((h, w))
    for i in range(3):
        for j in range(3):
            dx += SOBEL_V[i, j] * s[i:i + h, j:j + w]
            dy += SOBEL_H[i, j] * s[i:i + h, j:j + w]
            ax += abs(SOBEL_V[i, j]) * a[i:i + h, j:j + w]
            ay += abs(SOBEL_H[i, j]) * a[i:i + h, j:j + w]
    norm = np.sqrt(dx * dx + dy * dy + 1.0)
    n = np.stack([dx / norm, dy / norm, -1.0 / norm], -1)
    return n, 18.0 * EPS32 * np.maximum(ax, ay) + 4.0 * EPS32


def _project(depth, u_tab, v_tab, z_scale, rgb, rot, trans):
    """float32, in the order of include/mi355x_match.h: (d, px, py), each (H, W)."""
    d = np.asarray(depth).astype(F32)
    r = np.asarray(rot, F32).reshape(3, 3)
    t = np.asarray(trans, F32).reshape(3)
    cx, cy, fx, fy = (F32(v) for v in rgb)
    with np.errstate(all="ignore"):
        x = d * u_tab[None, :]
        y = d * v_tab[:, None]
        z = d * F32(z_scale)
        q = [((x * r[0, j] + y * r[1, j]) + z * r[2, j]) + t[j] for j in range(3)]
        px = q[0] / q[2] * fx + cx
        py = q[1] / q[2] * fy + cy
    px = np.where(q[2] == 0, F32(0), px).astype(F32)
    py = np.where(q[2] == 0, F32(0), py).astype(F32)
    return d, px, py


def align_oracle(depth, u_tab, v_tab, z_scale, rgb, rot, trans, with_clean=False):
    """mi_depth_align's definition on one frame (H, W): per target the minimum over all sources whose 2x2 splat covers
    it, 0 if none.  with_clean: also the mask of the targets at which the reference is well defined (module docstring)."""
    d, px, py = _project(depth, u_tab, v_tab, z_scale, rgb, rot, trans)
    h, w = d.shape
    with np.errstate(invalid="ignore"):
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)          # False for NaN
        heard = (d > 0) & (d < F32(10000.0))
    live = inside & heard
    buf = np.full(h * w, np.inf, F32)
    pxl, pyl, dl = px[live], py[live], d[live]
    xs = [np.trunc(pxl - F32(0.5)).astype(np.int64), np.trunc(pxl + F32(0.5)).astype(np.int64)]
    ys = [np.trunc(pyl - F32(0.5)).astype(np.int64), np.trunc(pyl + F32(0.5)).astype(np.int64)]
    for ty in ys:
        for tx in xs:
            ok = (tx < w) & (ty < h)
            np.minimum.at(buf, ty[ok] * w + tx[ok], dl[ok])
    out = np.where(np.isinf(buf), F32(0), buf).astype(F32).reshape(h, w)
    if not with_clean:
        return out
    # the reference's writers: every source writes; out-of-frame ones go to (0, 0)
    with np.errstate(invalid="ignore"):
        out_of_frame = (px < 0) | (px >= w) | (py < 0) | (py >= h)
    rx = np.where(out_of_frame, F32(0), px).reshape(-1)
    ry = np.where(out_of_frame, F32(0), py).reshape(-1)
    silenced = (out_of_frame | ~heard).reshape(-1)
    dirty = np.zeros(h * w, bool)
    for oy in (F32(-0.5), F32(0.5)):
        for ox in (F32(-0.5), F32(0.5)):
            idx = np.trunc(ry + oy).astype(np.int64) * w + np.trunc(rx + ox).astype(np.int64)
            assert idx.min() >= 0 and idx.max() < h * w, "the reference raises IndexError on this case"
            dirty |= np.bincount(idx, minlength=h * w) > 1
            dirty[idx[silenced]] = True
    return out, ~dirty.reshape(h, w)


def golden():
    return np.load(GOLDEN)


def fixture_depth(g, name):
    """The case's input frame, float32 (H, W): synth_depth_frame by seed, in metres or in millimetre counts."""
    from onnx_image_processing_amd.synth import synth_depth_frame
    h, w = (int(x) for x in g[f"{name}__hw"])
    d = synth_depth_frame(int(g[f"{name}__seed"]), h, w, hole_share=float(g[f"{name}__hole_share"]))
    if int(g[f"{name}__millimetres"]):
        d = np.round(d.astype(np.float64) * 1000.0).astype(F32)
    return d


def camera_args(g, name):
    """(scale, width, height, cx, cy, fx, fy) of the case's depth camera, Python numbers as a caller passes them."""
    h, w = (int(x) for x in g[f"{name}__hw"])
    scale, cx, cy, fx, fy = (float(x) for x in g[f"{name}__camera"])
    return scale, w, h, cx, cy, fx, fy


def points_cases(g):
    return [str(n) for n in g["meta__points_cases"]]


def align_cases(g):
    return [str(n) for n in g["meta__align_cases"]]


def check_points(got, want, what):
    got = np.ascontiguousarray(got)
    assert got.dtype == F32 and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: points differ in their bits"


def check_normals(got, points, what):
    n, tol = normals_oracle(points)
    err = np.abs(np.asarray(got, np.float64) - n).max(-1)
    print(f"{what}: normals max err {err.max():.3e}, worst share of the bound {np.max(err / tol):.3f}")
    assert np.isfinite(err).all() and (err <= tol).all(), f"{what}: {int((err > tol).sum())} normals beyond the bound"


def check_align_against_reference(got, ref, clean, what):
    assert got.shape == ref.shape and got.dtype == F32, what
    share = clean.mean()
    print(f"{what}: clean targets {100 * share:.1f} %")
    assert share >= 0.60, f"{what}: only {100 * share:.1f} % clean targets"
    assert np.array_equal(got[clean].view(np.uint32), ref[clean].view(np.uint32)), f"{what}: differs at clean targets"
    nz = got != 0
    assert (got[nz] <= ref[nz]).all(), f"{what}: larger than the reference somewhere"


# ---- the modules' contract -----------------------------------------------------------------------------------------

def test_reference_import_lines_resolve():
    from pytorch_model.depth.depth2pointcloud import DepthToPointCloud
    from pytorch_model.depth.depth2pointcloud_with_normal import DepthToPointCloudWithNormal
    from pytorch_model.depth.depth_align import DepthAlignment
    from pytorch_model.depth import DepthToPointCloud as A, DepthToPointCloudWithNormal as B
    import onnx_image_processing_amd.pytorch_model.depth as impl
    assert DepthToPointCloud is impl.DepthToPointCloud is A
    assert DepthToPointCloudWithNormal is impl.DepthToPointCloudWithNormal is B
    assert DepthAlignment is impl.DepthAlignment


def test_constructor_contract_and_no_cpu_path():
    import inspect
    from pytorch_model.depth import DepthAlignment, DepthToPointCloud, DepthToPointCloudWithNormal
    cam = ["self", "scale", "width", "height", "cx", "cy", "fx", "fy"]
    assert list(inspect.signature(DepthToPointCloud.__init__).parameters) == cam
    assert list(inspect.signature(DepthToPointCloudWithNormal.__init__).parameters) == cam
    assert list(inspect.signature(DepthAlignment.__init__).parameters) == [
        "self", "scale", "width", "height", "depth_cx", "depth_cy", "depth_fx", "depth_fy", "rgb_cx", "rgb_cy", "rgb_fx",
        "rgb_fy", "rotation", "translation"]
    args = (0.001, 53, 37, 25.5, 18.25, 60.0, 61.5)
    mods = [DepthToPointCloud(*args), DepthToPointCloudWithNormal(*args),
            DepthAlignment(*args, 26.0, 18.0, 50.0, 50.5, torch.eye(3, dtype=torch.float64), torch.zeros(3))]
    u, v, zs = tables_oracle(*args)
    for m in mods:
        assert len(m.state_dict()) == 0 and not list(m.parameters())
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(torch.rand(37, 53, 1))
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(torch.zeros(2, 37, 53, dtype=torch.uint16))
    base = mods[0]
    assert mods[1].base_model.u_tab.dtype == torch.float32 and mods[2].rotation.dtype == torch.float32
    for m in (base, mods[1].base_model, mods[2]):
        assert np.array_equal(m.u_tab.numpy(), u) and np.array_equal(m.v_tab.numpy(), v) and np.float32(m.z_scale) == zs
    # the tables are the columns of the reference's uv buffer (loops over pixels, in-place float32 ops)
    uu = torch.zeros(37, 53, 1)
    for w in range(53):
        uu[:, w, 0] = w
    uu -= args[3]
    uu /= args[5]
    uu *= args[0]
    assert np.array_equal(uu[0, :, 0].numpy(), u)


def test_argument_errors_before_any_launch():
    """MI_E_* from the host checks (no GPU is touched: these return before the first launch)."""
    lib = native_lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    odd = ctypes.c_void_p(p.value + 2)
    pts, al = lib.mi_depth_to_points, lib.mi_depth_align
    cam = (1.0, 1.0, 1.0, 1.0)
    # NULL (the normals alone may be NULL)
    for k in (0, 5, 6, 8):
        a = [p, 0, 1, 8, 8, p, p, 1.0, p, None, None]
        a[k] = None
        assert pts(*a) == -1, k
    for k in (0, 5, 6, 12, 13, 14):
        a = [p, 0, 1, 8, 8, p, p, 1.0, *cam, p, p, p, None]
        a[k] = None
        assert al(*a) == -1, k
    # shapes: batch < 1, h < 1, w < 1, batch * h * w >= 2^31
    for b, h, w in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, -3), (2, 32768, 32768), (1 << 11, 1 << 10, 1 << 10)):
        assert pts(p, 0, b, h, w, p, p, 1.0, p, p, None) == -2, (b, h, w)
        assert al(p, 1, b, h, w, p, p, 1.0, *cam, p, p, p, None) == -2, (b, h, w)
    # depth_is_u16 outside {0, 1}
    assert pts(p, 2, 1, 8, 8, p, p, 1.0, p, p, None) == -3
    assert al(p, -1, 1, 8, 8, p, p, 1.0, *cam, p, p, p, None) == -3
    # misaligned: float32 depth on 2 bytes, outputs on 2 bytes
    assert pts(odd, 0, 1, 8, 8, p, p, 1.0, p, p, None) == -5
    assert pts(p, 1, 1, 8, 8, p, p, 1.0, odd, p, None) == -5
    assert al(odd, 0, 1, 8, 8, p, p, 1.0, *cam, p, p, p, None) == -5
    assert al(p, 0, 1, 8, 8, p, p, 1.0, *cam, p, p, odd, None) == -5
    assert lib.mi_abi_version() == 3


def test_synth_depth_frame_is_the_cloud_s_depth_image():
    from onnx_image_processing_amd.synth import synth_depth_cloud, synth_depth_frame
    f = synth_depth_frame(11, 120, 160)
    assert f.dtype == F32 and f.shape == (120, 160)
    assert np.array_equal(synth_depth_cloud(11, 120, 160)[:, 2].reshape(120, 160), f)
    holes = synth_depth_frame(11, 120, 160, hole_share=0.1)
    share = (holes == 0).mean()
    assert 0.07 < share < 0.13 and np.array_equal(holes[holes != 0], f[holes != 0])
    assert np.array_equal(holes, synth_depth_frame(11, 120, 160, hole_share=0.1))


# ---- the oracles against the reference fixture ---------------------------------------------------------------------

def test_points_oracle_reproduces_the_reference_bitwise():
    g = golden()
    names = points_cases(g)
    assert len(names) >= 4
    seen = set()
    for name in names:
        d = fixture_depth(g, name)
        args = camera_args(g, name)
        u, v, zs = tables_oracle(*args)
        check_points(points_oracle(d, u, v, zs), g[f"{name}__points"], name)
        seen.add((args[0], bool((d == 0).any())))
        assert args[3] != (args[1] - 1) / 2 and args[5] != args[6], name       # principal point off-centre, fx != fy
    assert seen == {(1.0, False), (1.0, True), (0.001, False), (0.001, True)}


def test_normals_oracle_reproduces_the_reference_within_the_derived_bound():
    g = golden()
    for name in points_cases(g):
        check_normals(g[f"{name}__normals"], g[f"{name}__points"], name)


def test_align_oracle_reproduces_the_reference_where_it_is_defined():
    g = golden()
    names = align_cases(g)
    assert len(names) >= 4
    assert int(g["meta__align_threads"]) == 1
    for name in names:
        d = fixture_depth(g, name)
        u, v, zs = tables_oracle(*camera_args(g, name))
        out, clean = align_oracle(d, u, v, zs, g[f"{name}__rgb"], g[f"{name}__rotation"], g[f"{name}__translation"],
                                  with_clean=True)
        check_align_against_reference(out, g[f"{name}__aligned"], clean, name)
        assert (out != 0).mean() > 0.5, name
