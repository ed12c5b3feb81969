"""K18 dense RGB-D refinement on the GPU against tests/icp_oracle.py (the fp64 numpy restatement of include/mi355x_match.h).

Vertices are compared bit for bit with the oracle run in float32, which is the header's arithmetic.  Everything else is
float32 kernels against a float64 oracle, so every tolerance below is the deviation of the SAME oracle run in float32 from
its float64 run, measured on the CPU on the very scenes the test uses, times the margins of tests/test_gpu_rigid.py (4 for
values, 2 for angles).  Nothing here was taken from the kernels.
  - normals (test 1's poked frames, (37, 53) and (48, 64), 3 frames each): validity equal between the two oracle runs on
    every frame; components deviate by at most 1.762e-6 (float32 depth) and 2.365e-6 (uint16 millimetres) -> NORMAL_TOL =
    7.05e-6 and 9.46e-6.
  - one linearisation (test 2's 54 (shape, seed, pose, stride) cases): the float32 oracle has the float64 oracle's count
    on every case (0 gate flips -> COUNT_ALLOWANCE = 4 * 0 = 0, inside the cap of 0.5 % of the source pixels; the test
    re-asserts it for the float32 oracle).  With the scales of icp_oracle.sums_deviation (A: max |A|; b_i: sqrt(A_ii sum r^2),
    because b crosses zero at the truth; sum r^2: itself) the sums deviate by at most 1.02e-6, 4.742e-4 (a stride-4 case of
    86 rows at the truth, where b is the rounding of a cancelled sum) and 3.832e-5 -> SUMS_A_TOL = 4.08e-6, SUMS_B_TOL =
    1.90e-3, SUMS_RR_TOL = 1.53e-4.
  - the same at stride 8 (18 more cases; 35 samples at (37, 53): one slab, most of it past the end): equal counts again (0
    flips), 0.486 .. 0.877 of the sampled pixels.  With so few rows the float32 oracle's own deviation is larger than at
    strides 1 2 4: at most 1.524e-6 (A), 6.158e-4 (b), 2.634e-4 (sum r^2) -> STRIDE8_SUMS_TOL = 6.10e-6, 2.46e-3, 1.05e-3.
    The tolerances of strides 1 2 4 are not widened for it.
  - refinement from identity, default schedule, seeds 0 1 2 (all 14 steps applied in both runs, the float64 run's last step
    below 3e-16, smallest pivot ratio 7.3e-3):
      (48, 64):   float64 oracle from the truth 5.2624e-2 deg, 1.6994e-3 m (the bias of crease and sphere normals at this size);
                  float32 from float64 3.258e-6 deg, 1.007e-7 m, information 2.046e-7 (relative to its largest entry), rmse
                  3.858e-6 relative, equal counts
      (120, 160): 5.3641e-3 deg, 1.8742e-4 m; 2.121e-6 deg, 1.181e-7 m, 1.064e-7, 8.898e-6, equal counts
    -> REFINE_TOL rows: truth = oracle's distance + 2 (angle) or 4 (value) times the deviation; oracle = 2 / 4 times it.
  - refinement from the perturbed truth at (48, 64): 3.784e-6 deg, 1.223e-7 m, 1.010e-7, 2.845e-6 -> START_TOL.
  Translations are compared by their largest component, rotations by the angle of Ra^T Rb.
  - a tilted single plane against itself is degenerate in both oracle runs (pivot ratio 5.8e-13 / 0) with 2852 rows."""
import functools

import numpy as np
import pytest
import torch

import icp_oracle as IO
from gpu_common import DEV, GPU, bits
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DenseRgbdRefiner
from onnx_image_processing_amd.synth import rgbd_camera

pytestmark = GPU
F32, F64 = np.float32, np.float64
ANGLE = float(np.deg2rad(IO.ANGLE_DEG))
SEEDS = (0, 1, 2)
FLIP_CAP = 0.005                         # of the source pixels
NORMAL_TOL = {False: 7.05e-6, True: 9.46e-6}               # keyed by u16
SUMS_A_TOL, SUMS_B_TOL, SUMS_RR_TOL, COUNT_ALLOWANCE = 4.08e-6, 1.90e-3, 1.53e-4, 0
STRIDE8_SUMS_TOL = (6.10e-6, 2.46e-3, 1.05e-3)             # 4 x (1.524e-6, 6.158e-4, 2.634e-4), measured at stride 8
# (truth deg, truth m, oracle deg, oracle m, information relative, rmse relative)
REFINE_TOL = {(48, 64): (5.2631e-2, 1.6998e-3, 6.52e-6, 4.03e-7, 8.18e-7, 1.54e-5),
              (120, 160): (5.3683e-3, 1.8789e-4, 4.24e-6, 4.72e-7, 4.26e-7, 3.56e-5)}
START_TOL = (5.2633e-2, 1.6999e-3, 7.57e-6, 4.89e-7, 4.04e-7, 1.14e-5)


@functools.lru_cache(maxsize=None)
def room(seed, h, w, dtype=F64):
    return IO.room(seed, h, w, dtype=dtype)


def k_inv(h, w):
    return torch.from_numpy(IO.k_inv32(rgbd_camera(h, w))).to(DEV)


def gpu_maps(depths, h, w, scale=1.0):
    return ops.surfel_maps(torch.from_numpy(np.stack(depths)).to(DEV), k_inv(h, w), scale, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)


@functools.lru_cache(maxsize=None)
def room_maps_gpu(h, w, seeds=SEEDS):
    """the kernels' maps of both frames of the rooms `seeds`, one pair per seed"""
    return (gpu_maps([room(s, h, w)[5] for s in seeds], h, w), gpu_maps([room(s, h, w)[6] for s in seeds], h, w))


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def poses(h, w, variant):
    """pair b of the batch gets pose kind (b + variant) % 3 of (identity, the truth, the perturbed truth), as float32"""
    out = []
    for b, seed in enumerate(SEEDS):
        R, t = room(seed, h, w)[2:4]
        kind = (b + variant) % 3
        Rx, tx = ((np.eye(3), np.zeros(3)), (R, t), IO.perturbed(R, t))[kind]
        out.append((Rx.astype(F32), tx.astype(F32)))
    return out


def poked_depth(h, w, u16):
    """three room frames with holes, NaN, inf and depths outside [MIN_DEPTH, MAX_DEPTH]; (depth (3, h, w), z_scale, the
    poked pixels of frame 0)"""
    d = np.stack([room(s, h, w)[5] for s in SEEDS]).copy()
    holes = [(5, 7), (h // 2, w // 2), (h - 3, w - 4), (1, 1)]
    if u16:
        d = np.round(d * 1000.0).astype(np.uint16)
        special = [0, 99, 10001, 65535]
        scale = 0.001
    else:
        special = [0.0, np.nan, np.inf, 0.0999]
        d[1, 9, 11] = 10.001
        d[2, 3, 5] = -np.inf
        d[2, 4:9, 20:30] += F32(0.5)                          # a step: the jump gate
        scale = 1.0
    for (y, x), v in zip(holes, special):
        d[0, y, x] = v
    d[1, 12:15, 30:33] = 0                                    # a block of holes
    return d, scale, holes


# ---- 1. surfel maps ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(37, 53), (48, 64)])
@pytest.mark.parametrize("u16", [False, True])
def test_surfel_maps_match_the_oracle(h, w, u16):
    d, scale, holes = poked_depth(h, w, u16)
    vertex, normal = ops.surfel_maps(torch.from_numpy(d).to(DEV), k_inv(h, w), scale, IO.MIN_DEPTH, IO.MAX_DEPTH, IO.JUMP)
    vertex, normal = vertex.cpu().numpy(), normal.cpu().numpy()
    ki = IO.k_inv32(rgbd_camera(h, w))
    worst = 0.0
    for b in range(3):
        v32, vok32, n32, nok32 = IO.surfel_maps(d[b], ki, scale, dtype=F32)
        v64, vok64, n64, nok64 = IO.surfel_maps(d[b], ki, scale, dtype=F64)
        assert np.array_equal(bits(vertex[b, ..., :3]), bits(v32))                    # the header's float32 arithmetic
        assert np.array_equal(vertex[b, ..., 3], vok32.astype(F32)) and np.array_equal(vok32, vok64)
        assert np.array_equal(nok32, nok64)                                           # no gate flips between the oracles
        assert np.array_equal(normal[b, ..., 3], nok64.astype(F32))
        assert not normal[b, ..., :3][~nok64].any() and not vertex[b, ..., :3][~vok64].any()
        dev = np.abs(normal[b, ..., :3][nok64] - n64[nok64]).max()
        worst = max(worst, dev)
        assert np.abs(np.linalg.norm(normal[b, ..., :3][nok64], axis=-1) - 1).max() < 1e-6
        assert ((normal[b, ..., :3] * vertex[b, ..., :3]).sum(-1)[nok64] <= 0).all()  # facing the camera
        nv = normal[b, ..., 3]
        assert not nv[0].any() and not nv[-1].any() and not nv[:, 0].any() and not nv[:, -1].any()
        assert nv.mean() > 0.5
    print(f"surfel maps {h} x {w} u16={u16}: max normal deviation from the float64 oracle {worst:.3e} (tolerance {NORMAL_TOL[u16]:.1e})")
    assert worst <= NORMAL_TOL[u16]
    for y, x in holes[:3]:                                                            # a hole takes its four neighbours' normals
        assert vertex[0, y, x, 3] == 0
        for yy, xx in ((y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            assert normal[0, yy, xx, 3] == 0
    assert vertex[1, 13, 31, 3] == 0 and normal[1, 13, 29, 3] == 0 and normal[1, 11, 31, 3] == 0


# ---- 2. one linearisation --------------------------------------------------------------------------------------------------------

def check_sums(got, ref, nsrc, what, tol=(SUMS_A_TOL, SUMS_B_TOL, SUMS_RR_TOL)):
    dev = IO.sums_deviation(got, ref)
    print(f"{what}: count {int(ref[28])}, deviation A {dev[0]:.2e} b {dev[1]:.2e} r^2 {dev[2]:.2e} count {dev[3]} (tolerance "
          f"{tol[0]:.2e} {tol[1]:.2e} {tol[2]:.2e})")
    assert dev[3] <= min(COUNT_ALLOWANCE, FLIP_CAP * nsrc)
    assert dev[0] <= tol[0] and dev[1] <= tol[1] and dev[2] <= tol[2]


@pytest.mark.parametrize("h,w", [(37, 53), (120, 160)])
@pytest.mark.parametrize("stride", [1, 2, 4, 8])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_linearise_matches_the_oracle(h, w, stride, variant):
    m1, m2 = room_maps_gpu(h, w)
    ps = poses(h, w, variant)
    cam = room(0, h, w)[4]
    sums = ops.icp_linearise(m1, m2, t32(np.stack([p[0] for p in ps])), t32(np.stack([p[1] for p in ps])), cam, stride, IO.DIST,
                             ANGLE).cpu().numpy()
    nsrc = -(-h // stride) * -(-w // stride)
    for b, seed in enumerate(SEEDS):
        o1, o2 = room(seed, h, w)[:2]
        ref = IO.linearise(o1, o2, ps[b][0], ps[b][1], cam, stride)
        f1, f2 = room(seed, h, w, F32)[:2]
        flips = abs(IO.linearise(f1, f2, ps[b][0], ps[b][1], cam, stride, dtype=F32)[28] - ref[28])
        assert flips <= min(COUNT_ALLOWANCE, FLIP_CAP * nsrc)                         # the float32 oracle alone stays inside
        assert ref[28] > 0.5 * 0.8 * nsrc
        what = f"{h}x{w} stride {stride} pair {b} pose kind {(b + variant) % 3}"
        if stride == 8:
            check_sums(sums[b], ref, nsrc, what, STRIDE8_SUMS_TOL)
        else:
            check_sums(sums[b], ref, nsrc, what)
        assert np.isfinite(sums[b]).all()


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------

def solo(maps, b):
    return tuple(x[b:b + 1].contiguous() for x in maps)


def test_results_are_bitwise_reproducible_and_independent_of_the_batch():
    h, w = 120, 160
    m1, m2 = room_maps_gpu(h, w)
    ps = poses(h, w, 2)
    cam = room(0, h, w)[4]
    r, t = t32(np.stack([p[0] for p in ps])), t32(np.stack([p[1] for p in ps]))
    eye, zero = torch.eye(3, device=DEV).repeat(3, 1, 1), torch.zeros(3, 3, device=DEV)
    for stride in (1, 4):
        a = ops.icp_linearise(m1, m2, r, t, cam, stride, IO.DIST, ANGLE)
        assert torch.equal(bits(a), bits(ops.icp_linearise(m1, m2, r, t, cam, stride, IO.DIST, ANGLE)))
        for b in range(3):
            one = ops.icp_linearise(solo(m1, b), solo(m2, b), r[b:b + 1], t[b:b + 1], cam, stride, IO.DIST, ANGLE)
            assert torch.equal(bits(one[0]), bits(a[b])), (stride, b)
    full = ops.icp_refine(m1, m2, eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    again = ops.icp_refine(m1, m2, eye, zero, cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(full, again))
    for b in range(3):
        one = ops.icp_refine(solo(m1, b), solo(m2, b), eye[:1], zero[:1], cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
        assert all(torch.equal(bits(x[:1]), bits(y[b:b + 1])) for x, y in zip(one, full)), b


# ---- 4. the module from identity ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_refined(seed, h, w, start="identity", dtype=F64):
    m1, m2, R, t, cam = room(seed, h, w, dtype)[:5]
    R0, t0 = (np.eye(3), np.zeros(3)) if start == "identity" else tuple(x.astype(F32).astype(F64) for x in IO.perturbed(R, t))
    return IO.refine(m1, m2, R0, t0, cam, dtype=dtype)


def check_refined(got, ref, truth, tol, what):
    """got: (R, t, information, rmse, count, ok) numpy of one pair; tol: a row of REFINE_TOL"""
    R, t, info, rmse, count, ok = got
    rot_gt, t_gt = IO.rotation_angle_deg_small(R, truth[0]), np.abs(t - truth[1]).max()
    rot_o, t_o = IO.rotation_angle_deg_small(R, ref["R"]), np.abs(t - ref["t"]).max()
    dinfo = np.abs(info - ref["information"]).max() / np.abs(ref["information"]).max()
    print(f"{what}: truth {rot_gt:.3e} deg {t_gt:.3e} m; oracle {rot_o:.3e} deg {t_o:.3e} m; information {dinfo:.2e}; "
          f"rmse {rmse:.4e} / {ref['rmse']:.4e}; count {count} / {ref['count']}")
    assert ok and ref["ok"]
    assert rot_gt <= tol[0] and t_gt <= tol[1]
    assert rot_o <= tol[2] and t_o <= tol[3]
    assert abs(np.linalg.det(R.astype(F64)) - 1) <= 1e-5
    assert np.array_equal(info, info.T) and dinfo <= tol[4]
    assert abs(int(count) - ref["count"]) <= COUNT_ALLOWANCE and abs(rmse - ref["rmse"]) <= tol[5] * ref["rmse"]


@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
def test_refiner_from_identity_reaches_the_truth_and_the_oracle(h, w):
    K = torch.from_numpy(rgbd_camera(h, w))
    m = DenseRgbdRefiner(K).to(DEV)
    d1 = torch.from_numpy(np.stack([room(s, h, w)[5] for s in SEEDS])).to(DEV)
    d2 = torch.from_numpy(np.stack([room(s, h, w)[6] for s in SEEDS])).to(DEV)
    out = [x.cpu().numpy() for x in m(d1, d2)]
    assert out[2].shape == (3, 6, 6) and out[5].dtype == bool
    for b, seed in enumerate(SEEDS):
        ref, f32 = oracle_refined(seed, h, w), oracle_refined(seed, h, w, dtype=F32)
        assert abs(f32["count"] - ref["count"]) <= COUNT_ALLOWANCE                      # the float32 oracle alone stays inside
        check_refined([x[b] for x in out], ref, room(seed, h, w)[2:4], REFINE_TOL[(h, w)], f"{h}x{w} seed {seed}")
    steps = ops.icp_refine(*room_maps_gpu(h, w), torch.eye(3, device=DEV).repeat(3, 1, 1), torch.zeros(3, 3, device=DEV),
                           room(0, h, w)[4], IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)[5]
    assert steps.tolist() == [sum(i for _, i in IO.SCHEDULE)] * 3
    one = m(d1[1], d2[1])                                                                # unbatched in, unbatched out
    assert one[0].shape == (3, 3) and one[2].shape == (6, 6) and np.array_equal(bits(one[0].cpu().numpy()), bits(out[0][1]))
    four = m(d1.unsqueeze(1), d2.unsqueeze(1))                                          # (B, 1, H, W)
    assert np.array_equal(bits(four[1].cpu().numpy()), bits(out[1]))


# ---- 5. a given start ------------------------------------------------------------------------------------------------------------

def test_a_given_start_is_honoured():
    h, w = 48, 64
    K = torch.from_numpy(rgbd_camera(h, w))
    d1 = torch.from_numpy(np.stack([room(s, h, w)[5] for s in SEEDS])).to(DEV)
    d2 = torch.from_numpy(np.stack([room(s, h, w)[6] for s in SEEDS])).to(DEV)
    start = [tuple(x.astype(F32) for x in IO.perturbed(*room(s, h, w)[2:4])) for s in SEEDS]
    R0, t0 = t32(np.stack([s[0] for s in start])), t32(np.stack([s[1] for s in start]))
    out = [x.cpu().numpy() for x in DenseRgbdRefiner(K).to(DEV)(d1, d2, R0, t0)]
    for b, seed in enumerate(SEEDS):
        ref = oracle_refined(seed, h, w, "perturbed")
        check_refined([x[b] for x in out], ref, room(seed, h, w)[2:4], START_TOL, f"from the perturbed truth, seed {seed}")
    # no iterations: the start's own bits and the statistics of one linearisation there
    zero = DenseRgbdRefiner(K, schedule=((2, 0),)).to(DEV)(d1, d2, R0, t0)
    assert torch.equal(bits(zero[0]), bits(R0)) and torch.equal(bits(zero[1]), bits(t0))
    sums = ops.icp_linearise(*room_maps_gpu(h, w), R0, t0, room(0, h, w)[4], 2, IO.DIST, ANGLE).cpu().numpy()
    for b in range(3):
        assert np.array_equal(zero[2][b].cpu().numpy(), IO.full_matrix(sums[b]).astype(F32))
        assert int(zero[4][b]) == int(sums[b][28]) and bool(zero[5][b])
        assert float(zero[3][b]) == F32(np.sqrt(sums[b][27] / sums[b][28]))
    # the start matters: from identity the same frames pass through other poses
    ident = DenseRgbdRefiner(K, schedule=((2, 1),)).to(DEV)(d1, d2)
    given = DenseRgbdRefiner(K, schedule=((2, 1),)).to(DEV)(d1, d2, R0, t0)
    assert not torch.equal(ident[0], given[0])


# ---- 6. degenerate pairs ---------------------------------------------------------------------------------------------------------

def test_degenerate_pairs_are_frozen_beside_a_good_pair():
    h, w = 48, 64
    good1, good2 = room(1, h, w)[5:7]
    plane = IO.plane_depth(h, w)
    d1 = torch.from_numpy(np.stack([plane, good1, good1])).to(DEV)
    d2 = torch.from_numpy(np.stack([plane, np.zeros_like(good2), good2])).to(DEV)
    start = tuple(x.astype(F32) for x in IO.update(np.eye(3), np.zeros(3), np.array([0.002, 0.001, -0.002, 0.004, 0.0, -0.003])))
    R0, t0 = t32(np.stack([start[0]] * 3)), t32(np.stack([start[1]] * 3))
    cam = room(1, h, w)[4]
    m1, m2 = gpu_maps(list(d1.cpu().numpy()), h, w), gpu_maps(list(d2.cpu().numpy()), h, w)
    out = ops.icp_refine(m1, m2, R0, t0, cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    r, t, info, rmse, count, steps, ok = out
    assert ok.tolist() == [False, False, True]
    assert steps.tolist() == [0, 0, sum(i for _, i in IO.SCHEDULE)]
    for b in (0, 1):
        assert torch.equal(bits(r[b]), bits(R0[b])) and torch.equal(bits(t[b]), bits(t0[b]))
    assert int(count[1]) == 0 and float(rmse[1]) == 0 and not info[1].any() and int(count[0]) > IO.MIN_CORR
    assert all(bool(torch.isfinite(x.float()).all()) for x in out)
    one = ops.icp_refine(solo(m1, 2), solo(m2, 2), R0[:1], t0[:1], cam, IO.SCHEDULE, IO.DIST, ANGLE, IO.MIN_CORR)
    assert all(torch.equal(bits(x[:1]), bits(y[2:3])) for x, y in zip(one, out))
    # the oracle agrees on which pairs are degenerate
    ki = IO.k_inv32(rgbd_camera(h, w))
    for b, want in enumerate((False, False, True)):
        o = IO.refine(IO.surfel_maps(d1[b].cpu().numpy(), ki), IO.surfel_maps(d2[b].cpu().numpy(), ki), start[0], start[1], cam)
        assert o["ok"] is want and (want or o["steps"] == 0)


# ---- 7. graph capture --------------------------------------------------------------------------------------------------------------

def test_forward_replays_from_a_captured_graph_to_the_eager_bits():
    h, w = 48, 64
    m = DenseRgbdRefiner(torch.from_numpy(rgbd_camera(h, w))).to(DEV)
    sets = [tuple(torch.from_numpy(np.stack([room(s, h, w)[i] for s in order])).to(DEV) for i in (5, 6))
            for order in ((0, 1, 2), (2, 0, 1), (1, 1, 0))]
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
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, eager[i])), i
