"""K21 direct RGB-D refinement on the GPU against tests/photo_oracle.py (the fp64 numpy restatement of include/mi355x_match.h).

Intensity records are compared bit for bit with the oracle run in float32, which is the header's arithmetic, and so are the
counts of every linearisation: the per-pixel arithmetic is identical, so no gate may flip (allowance 0).  Everything else is
float32 kernels against a float64 oracle, and every tolerance below is the deviation of the SAME oracle run in float32 from
its float64 run, measured on the CPU on the very scenes the test uses, times 4 for values and 2 for angles (the margins of
tests/test_gpu_icp.py).  Nothing here was taken from the kernels.
  - one photometric linearisation (test 2's 54 (shape, stride, seed, pose) cases on the textured sphere room).  On the 48
    cases other than (identity, stride 1) the two oracle runs have equal counts (0 flips, inside FLIP_CAP = 0.5 % of the
    source pixels) and their sums deviate, in the scales of icp_oracle.sums_deviation, by at most 1.736e-6 (A), 1.070e-5 (b),
    1.632e-5 (sum r^2) -> SUMS_TOL = 6.94e-6, 4.28e-5, 6.53e-5.
    At stride 8 (18 more cases; 35 samples at (37, 53): one slab, most of it past the end) the two oracle runs have equal
    counts as well (0 flips), 0.486 .. 0.887 of the sampled pixels, and with so few rows deviate by more: at most 4.099e-6
    (A), 4.873e-5 (b), 4.377e-5 (sum r^2) -> STRIDE8_SUMS_TOL = 1.64e-5, 1.95e-4, 1.75e-4.  SUMS_TOL is not widened for it.
    At the identity with stride 1 every source pixel projects onto an integer position (u = x up to rounding), where
    floorf(u) is a knife edge: the footprint is columns (x - 1, x) or (x, x + 1), and the bilinear value is the same either
    way, but for a source pixel next to the frame's border one of the two footprints holds an invalid border record.  The
    two oracle runs then disagree on 12 .. 31 of those pixels per frame (0.61 .. 0.92 % of the source pixels at (37, 53),
    0.11 .. 0.16 % at (120, 160)): above FLIP_CAP at the small size.  The flips are confined to the 2 (h - 2) + 2 (w - 2) - 4
    border-adjacent source pixels (with those masked out of frame 1 the runs have equal counts again, measured), so on
    these 6 cases that number is the cap, the sums are compared with their own measured deviation, 5.539e-2, 4.106e-2,
    1.371e-2 -> IDENTITY_TOL = 0.222, 0.164, 0.0549, and the case is compared a second time with the border-adjacent
    source pixels masked out: 2.695e-7, 4.967e-7, 5.258e-7 -> INNER_TOL = 1.08e-6, 1.99e-6, 2.10e-6.  The kernel's count
    equals the float32 oracle's on every case, these included.
  - joint refinement from identity, default schedule and weight, seeds 0 1 2, all 14 steps in both runs:
      textured plane (48, 64):   float64 oracle from the truth 4.619e-3 / 3.032e-3 / 9.901e-4 deg, 6.858e-5 / 3.863e-5 /
                  3.081e-5 m (tests/test_photo_host.py); float32 from float64 at most 3.017e-6 deg, 1.071e-7 m
      textured plane (120, 160): 5.524e-4 / 2.389e-4 / 3.816e-4 deg, 2.474e-5 / 1.517e-5 / 5.606e-6 m; 4.428e-6 deg, 1.517e-7 m
      -> PLANE_TOL = 2 / 4 times the deviation; from the truth: the oracle's own distance for the seed plus that.
      textured sphere room (48, 64): float64 oracle from the truth at most 4.429e-2 deg, 1.199e-3 m; float32 from float64
                  1.851e-6 deg, 1.153e-7 m, information 2.32e-7 (relative to its largest entry), rmse 3.80e-6, rmse_photo
                  1.96e-6 relative, both counts equal -> ROOM_TOL.
  Translations are compared by their largest component, rotations by the angle of Ra^T Rb."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import icp_oracle as IO
import photo_oracle as PO
from gpu_common import DEV, GPU, bits
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DirectRgbdRefiner
from onnx_image_processing_amd.synth import rgbd_camera

pytestmark = GPU
F32, F64 = np.float32, np.float64
ANGLE = float(np.deg2rad(IO.ANGLE_DEG))
SEEDS = (0, 1, 2)
FLIP_CAP = 0.005                         # of the source pixels
COUNT_ALLOWANCE = 0
SUMS_TOL = (6.94e-6, 4.28e-5, 6.53e-5)
STRIDE8_SUMS_TOL = (1.64e-5, 1.95e-4, 1.75e-4)             # 4 x (4.099e-6, 4.873e-5, 4.377e-5), measured at stride 8
IDENTITY_TOL = (0.222, 0.164, 0.0549)
INNER_TOL = (1.08e-6, 1.99e-6, 2.10e-6)
# float64 oracle from the truth per seed (deg, m), then the allowance from the oracle (deg, m)
PLANE_TRUTH = {(48, 64): ((4.619e-3, 6.858e-5), (3.032e-3, 3.863e-5), (9.901e-4, 3.081e-5)),
               (120, 160): ((5.524e-4, 2.474e-5), (2.389e-4, 1.517e-5), (3.816e-4, 5.606e-6))}
PLANE_TOL = {(48, 64): (2 * 3.017e-6, 4 * 1.071e-7), (120, 160): (2 * 4.428e-6, 4 * 1.517e-7)}
# (truth deg, truth m, oracle deg, oracle m, information relative, rmse relative, rmse_photo relative)
ROOM_TOL = (4.429e-2 + 2 * 1.851e-6, 1.199e-3 + 4 * 1.153e-7, 2 * 1.851e-6, 4 * 1.153e-7, 4 * 2.32e-7, 4 * 3.80e-6, 4 * 1.96e-6)
ARGS = (IO.SCHEDULE, IO.DIST, ANGLE, PO.PHOTO_WEIGHT, PO.INTENSITY_THRESHOLD, IO.MIN_CORR)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def scene(kind, seed, h, w, dtype=F64):
    return PO.scene(kind, seed, h, w, dtype)


def dev_t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t32(a):
    return dev_t(np.ascontiguousarray(a, dtype=F32))


@functools.lru_cache(maxsize=None)
def gpu_maps(kind, h, w, seeds=SEEDS):
    """the kernels' maps of both frames of the scenes `seeds`, one pair per seed: ((vertex, normal, intensity) x 2)"""
    k_inv = dev_t(IO.k_inv32(rgbd_camera(h, w)))
    out = []
    for d, g in (("depth1", "gray1"), ("depth2", "gray2")):
        depth = dev_t(np.stack([scene(kind, s, h, w)[d] for s in seeds]))
        gray = dev_t(np.stack([scene(kind, s, h, w)[g] for s in seeds]))
        out.append((*ops.surfel_maps(depth, k_inv, 1.0, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP), ops.intensity_maps(gray)))
    return tuple(out)


def solo(maps, b):
    return tuple(x[b:b + 1].contiguous() for x in maps)


def identity(n):
    return torch.eye(3, device=DEV).repeat(n, 1, 1), torch.zeros(n, 3, device=DEV)


# ---- 1. intensity maps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(37, 53), (48, 64)])
@pytest.mark.parametrize("u8", [False, True])
def test_intensity_maps_match_the_oracle_bit_for_bit(h, w, u8):
    g = np.stack([scene("room", s, h, w)["gray1" if s else "gray2"] for s in SEEDS]).copy()
    poked = [(0, 5, 7), (0, h // 2, w // 2), (1, h - 2, w - 2), (2, 1, 1), (2, 0, 9)]
    if u8:
        g = PO.as_u8(g)
    else:
        for (b, y, x), v in zip(poked, (np.nan, np.inf, -np.inf, np.nan, np.nan)):
            g[b, y, x] = v
    out = ops.intensity_maps(dev_t(g)).cpu().numpy()
    assert out.shape == (3, h, w, 4) and out.dtype == F32
    for b in range(3):
        rec, ok = PO.intensity_maps(g[b], dtype=F32)
        assert np.array_equal(bits(out[b, ..., :3]), bits(rec)) and np.array_equal(out[b, ..., 3], ok.astype(F32))
        assert np.array_equal(ok, PO.intensity_maps(g[b], dtype=F64)[1])
        assert not out[b, ..., :3][~ok].any()
        f = out[b, ..., 3]
        assert not f[0].any() and not f[-1].any() and not f[:, 0].any() and not f[:, -1].any()
    if u8:
        assert out[..., 3][:, 1:-1, 1:-1].all()
        return
    for b, y, x in poked:                                     # a poked value takes its own and its axis neighbours' records
        for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w:
                assert out[b, yy, xx, 3] == 0
    assert out[0, 5, 9, 3] == 1 and out[0, 6, 8, 3] == 1 and np.isfinite(out).all()


# ---- 2. one photometric linearisation ----------------------------------------------------------------------------------------------

def poses(h, w, variant):
    """pair b of the batch gets pose kind (b + variant) % 3 of (identity, the truth, the perturbed truth), as float32"""
    out = []
    for b, seed in enumerate(SEEDS):
        s = scene("room", seed, h, w)
        kind = (b + variant) % 3
        Rx, tx = ((np.eye(3), np.zeros(3)), (s["R"], s["t"]), IO.perturbed(s["R"], s["t"]))[kind]
        out.append((Rx.astype(F32), tx.astype(F32), kind))
    return out


def oracle_sums(seed, h, w, R, t, stride, dtype, inner=False):
    s = scene("room", seed, h, w, dtype)
    int1 = s["int1"]
    if inner:
        ok = int1[1].copy()
        ok[1, :] = ok[-2, :] = ok[:, 1] = ok[:, -2] = False
        int1 = (int1[0], ok)
    return PO.linearise(s["maps1"], int1, s["maps2"], s["int2"], R, t, s["cam"], stride, dtype=dtype)


def check_sums(got, ref, tol, what):
    dev = IO.sums_deviation(got, ref)
    print(f"{what}: count {int(ref[28])}, deviation A {dev[0]:.2e} b {dev[1]:.2e} r^2 {dev[2]:.2e} (tolerance {tol[0]:.2e} {tol[1]:.2e} "
          f"{tol[2]:.2e})")
    assert dev[0] <= tol[0] and dev[1] <= tol[1] and dev[2] <= tol[2]


@pytest.mark.parametrize("h,w", [(37, 53), (120, 160)])
@pytest.mark.parametrize("stride", [1, 2, 4, 8])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_photo_linearise_matches_the_oracle(h, w, stride, variant):
    m1, m2 = gpu_maps("room", h, w)
    ps = poses(h, w, variant)
    cam = scene("room", 0, h, w)["cam"]
    r, t = t32(np.stack([p[0] for p in ps])), t32(np.stack([p[1] for p in ps]))
    sums = ops.photo_linearise(m1[0], m1[2], m2[0], m2[2], r, t, cam, stride, IO.DIST, PO.INTENSITY_THRESHOLD).cpu().numpy()
    masked = m1[2].clone()
    masked[:, 1, :, 3] = masked[:, -2, :, 3] = masked[:, :, 1, 3] = masked[:, :, -2, 3] = 0
    inner = ops.photo_linearise(m1[0], masked, m2[0], m2[2], r, t, cam, stride, IO.DIST, PO.INTENSITY_THRESHOLD).cpu().numpy()
    nsrc = -(-h // stride) * -(-w // stride)
    for b, seed in enumerate(SEEDS):
        R, tt, kind = ps[b]
        what = f"{h}x{w} stride {stride} pair {b} pose kind {kind}"
        ref, f32 = oracle_sums(seed, h, w, R, tt, stride, F64), oracle_sums(seed, h, w, R, tt, stride, F32)
        knife = kind == 0 and stride == 1
        flips = abs(f32[28] - ref[28])
        print(f"{what}: float32 oracle count {int(f32[28])}, float64 {int(ref[28])}, kernel {int(sums[b][28])}")
        assert flips <= (2 * (h - 2) + 2 * (w - 2) - 4 if knife else FLIP_CAP * nsrc)
        assert abs(sums[b][28] - f32[28]) <= COUNT_ALLOWANCE                            # the same arithmetic: no flip is legitimate
        assert ref[28] > 0.3 * nsrc and np.isfinite(sums[b]).all()
        check_sums(sums[b], ref, IDENTITY_TOL if knife else STRIDE8_SUMS_TOL if stride == 8 else SUMS_TOL, what)
        if knife:
            ref_i, f32_i = (oracle_sums(seed, h, w, R, tt, stride, d, inner=True) for d in (F64, F32))
            assert f32_i[28] == ref_i[28] and inner[b][28] == f32_i[28] and ref_i[28] < ref[28]
            check_sums(inner[b], ref_i, INNER_TOL, what + ", border-adjacent sources masked")


# ---- 3. the textured plane: the scene the feature is for -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_refined(kind, seed, h, w, dtype=F64):
    return PO.refine_scene(scene(kind, seed, h, w, dtype), dtype=dtype)


@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
def test_textured_plane_from_identity_where_icp_is_frozen(h, w):
    m1, m2 = gpu_maps("plane", h, w)
    cam = scene("plane", 0, h, w)["cam"]
    eye, zero = identity(3)
    k18 = ops.icp_refine(m1[:2], m2[:2], eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    assert k18[6].tolist() == [False] * 3 and k18[5].tolist() == [0] * 3
    R, t, info, rmse, count, rmse_p, count_p, steps, ok = (x.cpu().numpy() for x in ops.rgbd_refine(m1, m2, eye, zero, cam, *ARGS))
    assert ok.tolist() == [True] * 3 and steps.tolist() == [14] * 3
    for b, seed in enumerate(SEEDS):
        s, ref, f32 = scene("plane", seed, h, w), oracle_refined("plane", seed, h, w), oracle_refined("plane", seed, h, w, F32)
        rot_gt, t_gt = IO.rotation_angle_deg_small(R[b], s["R"]), np.abs(t[b] - s["t"]).max()
        rot_o, t_o = IO.rotation_angle_deg_small(R[b], ref["R"]), np.abs(t[b] - ref["t"]).max()
        print(f"plane {h}x{w} seed {seed}: truth {rot_gt:.3e} deg {t_gt:.3e} m; oracle {rot_o:.3e} deg {t_o:.3e} m; counts {count[b]} / "
              f"{ref['count']}, {count_p[b]} / {ref['count_photo']}; rmse_photo {rmse_p[b]:.4e} / {ref['rmse_photo']:.4e}")
        assert ref["ok"] and ref["steps"] == 14 and f32["ok"]
        tol, truth = PLANE_TOL[(h, w)], PLANE_TRUTH[(h, w)][seed]
        assert rot_o <= tol[0] and t_o <= tol[1]
        assert rot_gt <= truth[0] * 1.001 + tol[0] and t_gt <= truth[1] * 1.001 + tol[1]
        assert abs(np.linalg.det(R[b].astype(F64)) - 1) <= 1e-5 and np.array_equal(info[b], info[b].T)
        assert int(count[b]) > 0.9 * (h - 2) * (w - 2) and int(count_p[b]) > 0.9 * (h - 2) * (w - 2)


# ---- 4. the textured sphere room -----------------------------------------------------------------------------------------------------

def test_sphere_room_module_from_identity_matches_the_joint_oracle():
    h, w = 48, 64
    m = DirectRgbdRefiner(torch.from_numpy(rgbd_camera(h, w))).to(DEV)
    frames = [dev_t(np.stack([scene("room", s, h, w)[k] for s in SEEDS])) for k in ("depth1", "gray1", "depth2", "gray2")]
    out = [x.cpu().numpy() for x in m(*frames)]
    assert out[2].shape == (3, 6, 6) and out[7].dtype == bool and len(out) == 8
    tol = ROOM_TOL
    for b, seed in enumerate(SEEDS):
        s, ref, f32 = scene("room", seed, h, w), oracle_refined("room", seed, h, w), oracle_refined("room", seed, h, w, F32)
        R, t, info, rmse, count, rmse_p, count_p, ok = (x[b] for x in out)
        rot_gt, t_gt = IO.rotation_angle_deg_small(R, s["R"]), np.abs(t - s["t"]).max()
        rot_o, t_o = IO.rotation_angle_deg_small(R, ref["R"]), np.abs(t - ref["t"]).max()
        dinfo = np.abs(info - ref["information"]).max() / np.abs(ref["information"]).max()
        print(f"room seed {seed}: truth {rot_gt:.3e} deg {t_gt:.3e} m; oracle {rot_o:.3e} deg {t_o:.3e} m; information {dinfo:.2e}; rmse "
              f"{rmse:.4e} / {ref['rmse']:.4e}, photo {rmse_p:.4e} / {ref['rmse_photo']:.4e}; counts {count} / {ref['count']}, {count_p} / "
              f"{ref['count_photo']}")
        assert f32["count"] == ref["count"] and f32["count_photo"] == ref["count_photo"]     # the float32 oracle alone stays inside
        assert ok and ref["ok"]
        assert rot_gt <= tol[0] and t_gt <= tol[1] and rot_o <= tol[2] and t_o <= tol[3]
        assert abs(np.linalg.det(R.astype(F64)) - 1) <= 1e-5
        assert np.array_equal(info, info.T) and dinfo <= tol[4]
        assert abs(int(count) - ref["count"]) <= COUNT_ALLOWANCE and abs(int(count_p) - ref["count_photo"]) <= COUNT_ALLOWANCE
        assert abs(rmse - ref["rmse"]) <= tol[5] * ref["rmse"] and abs(rmse_p - ref["rmse_photo"]) <= tol[6] * ref["rmse_photo"]
    one = m(*(x[1] for x in frames))                                                       # unbatched in, unbatched out
    assert one[0].shape == (3, 3) and one[2].shape == (6, 6) and np.array_equal(bits(one[0].cpu().numpy()), bits(out[0][1]))
    four = m(*(x.unsqueeze(1) for x in frames))                                            # (B, 1, H, W)
    assert np.array_equal(bits(four[1].cpu().numpy()), bits(out[1]))
    u8 = m(frames[0], dev_t(PO.as_u8(frames[1].cpu().numpy())), frames[2], dev_t(PO.as_u8(frames[3].cpu().numpy())))
    assert bool(u8[7].all()) and float((u8[1] - four[1]).abs().max()) < 2e-3               # uint8 gray: rounded, near the same pose


# ---- 5. photo_weight = 0 is K18 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
def test_weight_zero_returns_icp_refines_bits(h, w):
    m1, m2 = gpu_maps("room", h, w)
    cam = scene("room", 0, h, w)["cam"]
    eye, zero = identity(3)
    k18 = ops.icp_refine(m1[:2], m2[:2], eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    z = ops.rgbd_refine(m1, m2, eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, 0.0, PO.INTENSITY_THRESHOLD, IO.MIN_CORR)
    r, t, info, rmse, count, rmse_p, count_p, steps, ok = z
    assert same((r, t, info, rmse, count, steps, ok), k18) and bool(ok.all())
    assert count_p.tolist() == [0] * 3 and rmse_p.tolist() == [0.0] * 3
    joint = ops.rgbd_refine(m1, m2, eye, zero, cam, *ARGS)
    assert not torch.equal(joint[0], r) and int(joint[6].min()) > 0


# ---- 6. batches, reproducibility, graph capture --------------------------------------------------------------------------------------

def test_a_frozen_pair_beside_a_good_pair_and_reproducibility():
    h, w = 48, 64
    good = gpu_maps("plane", h, w)
    cam = scene("plane", 0, h, w)["cam"]
    const = ops.intensity_maps(torch.full((1, h, w), 100.0, device=DEV))                   # zero gradient: the plane stays free
    m1 = (good[0][0][:2].contiguous(), good[0][1][:2].contiguous(), torch.cat([const, good[0][2][1:2]]))
    m2 = (good[1][0][:2].contiguous(), good[1][1][:2].contiguous(), torch.cat([const, good[1][2][1:2]]))
    eye, zero = identity(2)
    out = ops.rgbd_refine(m1, m2, eye, zero, cam, *ARGS)
    r, t, info, rmse, count, rmse_p, count_p, steps, ok = out
    assert ok.tolist() == [False, True] and steps.tolist() == [0, 14]
    assert torch.equal(bits(r[0]), bits(eye[0])) and torch.equal(bits(t[0]), bits(zero[0]))
    assert int(count_p[0]) > 2000 and float(rmse_p[0]) == 0.0 and int(count[0]) > 2000
    assert all(bool(torch.isfinite(x.float()).all()) for x in out)
    assert same(out, ops.rgbd_refine(m1, m2, eye, zero, cam, *ARGS))                        # run to run
    one = ops.rgbd_refine(solo(m1, 1), solo(m2, 1), eye[:1], zero[:1], cam, *ARGS)          # the good pair keeps its solo bits
    assert same([x[:1] for x in one], [x[1:2] for x in out])
    full = ops.rgbd_refine(*good, *identity(3), cam, *ARGS)
    assert same([x[1:2] for x in full], [x[:1] for x in one])
    # one linearisation: run to run, and alone against inside a batch, at (120, 160) (10 slabs at stride 1)
    h, w = 120, 160
    g1, g2 = gpu_maps("room", h, w)
    cam = scene("room", 0, h, w)["cam"]
    ps = poses(h, w, 2)
    r, t = t32(np.stack([p[0] for p in ps])), t32(np.stack([p[1] for p in ps]))
    for stride in (1, 4):
        a = ops.photo_linearise(g1[0], g1[2], g2[0], g2[2], r, t, cam, stride)
        assert torch.equal(bits(a), bits(ops.photo_linearise(g1[0], g1[2], g2[0], g2[2], r, t, cam, stride)))
        for b in range(3):
            s1, s2 = solo(g1, b), solo(g2, b)
            one = ops.photo_linearise(s1[0], s1[2], s2[0], s2[2], r[b:b + 1], t[b:b + 1], cam, stride)
            assert torch.equal(bits(one[0]), bits(a[b])), (stride, b)


def test_forward_replays_from_a_captured_graph_to_the_eager_bits():
    h, w = 48, 64
    m = DirectRgbdRefiner(torch.from_numpy(rgbd_camera(h, w))).to(DEV)
    picks = (("plane", 0), ("room", 1), ("plane", 2)), (("room", 2), ("plane", 1), ("room", 0)), (("plane", 1), ("plane", 1), ("room", 1))
    sets = [tuple(dev_t(np.stack([scene(k, s, h, w)[f] for k, s in pick])) for f in ("depth1", "gray1", "depth2", "gray2"))
            for pick in picks]
    eager = [[x.clone() for x in m(*s)] for s in sets]
    static = [x.clone() for x in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m(*static)
    for i in (1, 2, 0):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert same(out, eager[i]), i
    assert bool(eager[0][7].all())


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------

def test_argument_checks_on_device_tensors():
    h, w = 48, 64
    m1, m2 = gpu_maps("room", h, w)
    cam = scene("room", 0, h, w)["cam"]
    eye, zero = identity(3)
    with pytest.raises(RuntimeError, match=r"mi_photo_linearise failed \(-3\)"):
        ops.photo_linearise(m1[0], m1[2], m2[0], m2[2], eye, zero, cam, 3)                  # bad stride
    bad = r"mi_rgbd_refine failed \(-3\)"
    with pytest.raises(RuntimeError, match=bad):
        ops.rgbd_refine(m1, m2, eye, zero, cam, ((3, 1),))
    with pytest.raises(RuntimeError, match=bad):
        ops.rgbd_refine(m1, m2, eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, -0.001)        # negative weight
    for thr in (float("nan"), float("inf"), 0.0):
        with pytest.raises(RuntimeError, match=bad):
            ops.rgbd_refine(m1, m2, eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, 0.003, thr)
        with pytest.raises(RuntimeError, match=r"mi_photo_linearise failed \(-3\)"):
            ops.photo_linearise(m1[0], m1[2], m2[0], m2[2], eye, zero, cam, 1, IO.DIST, thr)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.photo_linearise(m1[0], m1[2][:, :-1], m2[0], m2[2], eye, zero, cam)
    with pytest.raises(RuntimeError, match="float32 or uint8"):
        ops.intensity_maps(torch.zeros(1, h, w, dtype=torch.float64, device=DEV))
    # misaligned maps and a short workspace, straight at the C entries
    lib = N.load()
    buf = torch.zeros(3 * h * w * 4 + 4, device=DEV)
    off = buf[1:1 + 3 * h * w * 4]                                                          # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    need = lib.mi_rgbd_workspace_bytes(3, h, w)
    work = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
    sums = torch.empty(3, 29, dtype=torch.float64, device=DEV)
    ptr = [x.data_ptr() for x in (m1[0], m1[2], m2[0], m2[2], eye, zero)]

    def lin(maps=ptr, wbytes=need, ws=work.data_ptr()):
        return lib.mi_photo_linearise(*maps, 3, h, w, *cam, 1, 0.1, 30.0, sums.data_ptr(), ws, wbytes, None)
    assert lin(maps=[ptr[0], off.data_ptr(), *ptr[2:]]) == -5 and lin(maps=[*ptr[:3], off.data_ptr(), *ptr[4:]]) == -5
    assert lin(ws=work.data_ptr() + 8) == -5 and lin(wbytes=need - 1) == -4
    assert lib.mi_intensity_maps(ptr[0], 0, 3, h, w, off.data_ptr(), None) == -5
    st, it = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(1)
    outs = [torch.empty(3 * 36, device=DEV) for _ in range(9)]
    six = [x.data_ptr() for x in (*m1, *m2)]

    def refine(maps=six, wbytes=need):
        return lib.mi_rgbd_refine(*maps, eye.data_ptr(), zero.data_ptr(), 3, h, w, *cam, ctypes.cast(st, ctypes.c_void_p),
                                  ctypes.cast(it, ctypes.c_void_p), 1, 0.1, ANGLE, 0.003, 30.0, 64, *[x.data_ptr() for x in outs],
                                  work.data_ptr(), wbytes, None)
    assert refine(maps=[*six[:2], off.data_ptr(), *six[3:]]) == -5 and refine(wbytes=lib.mi_icp_workspace_bytes(3, h, w)) == -4
    torch.cuda.synchronize()
