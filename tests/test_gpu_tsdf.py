"""K19 TSDF fusion on the GPU against tests/tsdf_oracle.py (the numpy restatement of include/mi355x_match.h).

Integration is compared bit for bit with the oracle run in float32, which is the header's arithmetic.  The raycast and the
tracking are float32 kernels against the float64 oracle, so every tolerance below is the deviation of the SAME oracle run in
float32 from its float64 run, measured on the CPU on the very scenes the test uses, times the margins of
tests/test_gpu_rigid.py and tests/test_gpu_icp.py (4 for values, 2 for angles).  Nothing here was taken from the kernels.
  - raycast (the four views of tsdf_oracle.views fused into each volume, seen from the first and the third view): the float32
    oracle has the float64 oracle's hit and normal validity on every pixel of every case (0 flips; the test re-asserts it, and
    allows the kernel FLIP_CAP = 0.5 % of the pixels); the largest deviation of a vertex / normal component is
        (37, 53): ROOM 2.3261e-6 / 5.2596e-6, ODD 1.3516e-6 / 3.6162e-6, TINY 3.1305e-7 / no normals
        (48, 64): ROOM 4.2129e-6 / 7.9349e-6, ODD 2.1955e-6 / 2.9507e-6, TINY 3.2543e-7 / no normals
    -> RAYCAST_TOL = 4 times these.
  - tracking at (48, 64) in ROOM, the unseen second views of seeds 3 and 4, the identity as prediction (14 steps in both runs,
    equal counts 2418 and 2379): float64 oracle from the truth 5.5811e-2 deg, 1.2172e-3 m; float32 from float64 at most
    5.5397e-6 deg, 1.8737e-7 m, information 8.8324e-8 (relative to its largest entry), rmse 4.0066e-6 relative
    -> TRACK_TOL: truth = the oracle's distance + 2 (angle) or 4 (value) times the deviation; oracle = 2 / 4 times it.
  Translations are compared by their largest component, rotations by the angle of Ra^T Rb.
Runs unchanged under MI_POISON_EMPTY=1 (conftest.py): every raycast output comes from torch.empty."""
import functools

import numpy as np
import pytest
import torch

import icp_oracle as IO
import tsdf_oracle as TO
from gpu_common import DEV, GPU, bits
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU
F32, F64 = np.float32, np.float64
SHAPES = [(37, 53), (48, 64)]
SPECS = {"room": TO.ROOM, "odd": TO.ODD, "tiny": TO.TINY}
FLIP_CAP = 0.005                         # of the pixels
RAYCAST_TOL = {((37, 53), "room"): (9.31e-6, 2.11e-5), ((37, 53), "odd"): (5.41e-6, 1.45e-5), ((37, 53), "tiny"): (1.26e-6, 0.0),
               ((48, 64), "room"): (1.69e-5, 3.18e-5), ((48, 64), "odd"): (8.79e-6, 1.19e-5), ((48, 64), "tiny"): (1.31e-6, 0.0)}
# (truth deg, truth m, oracle deg, oracle m, information relative, rmse relative)
TRACK_TOL = (5.5823e-2, 1.2180e-3, 1.108e-5, 7.50e-7, 3.54e-7, 1.61e-5)
BEHIND = (np.eye(3), np.array([0.0, 0.0, -1.75]))    # a camera at world z = 1.75: the nearer part of every volume is behind it


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def poked_views(h, w, u16):
    """(depth (4, h, w), z_scale, R, t): tsdf_oracle.views with NaN, inf, 0 and out-of-range depths poked into three frames"""
    depth, R, t = TO.views(h, w)
    d = depth.copy()
    spots = [(5, 7), (h // 2, w // 2), (h - 3, w - 4), (h // 2, w // 2 + 1), (h // 2 + 1, w // 2)]
    if u16:
        d = np.round(d * 1000.0).astype(np.uint16)
        special, scale = [0, 99, 10001, 65535, 0], 0.001
    else:
        special, scale = [0.0, np.nan, np.inf, 0.0999, 10.001], 1.0
        d[3, 9, 11] = -np.inf
    for f in (0, 1, 3):
        for (y, x), v in zip(spots, special):
            d[f, y, x] = v
    d[2, 12:15, 30:33] = 0                                    # a block of holes
    return d, scale, R, t


def gpu_integrate(dims, grid, cam, depth, R, t, scale=1.0, max_weight=TO.MAX_WEIGHT, active=None, volume=None):
    """one volume: reset (unless given), then depth (F, h, w) in ONE call -> (1, nz, ny, nx, 2) on the GPU"""
    nx, ny, nz = dims
    if volume is None:
        volume = ops.tsdf_reset(torch.empty((1, nz, ny, nx, 2), dtype=torch.float32, device=DEV))
    act = None if active is None else torch.tensor([active], dtype=torch.bool, device=DEV)
    return ops.tsdf_integrate(volume, torch.from_numpy(depth)[None].to(DEV), t32(R)[None], t32(t)[None], cam, grid[0].tolist(), grid[1],
                              grid[2], max_weight, scale, TO.MIN_DEPTH, TO.MAX_DEPTH, act)


def same_volume(got, ref):
    g = got.cpu().numpy()
    return np.array_equal(bits(g[0, ..., 0]), bits(ref[0])) and np.array_equal(bits(g[0, ..., 1]), bits(ref[1]))


@functools.lru_cache(maxsize=None)
def fused_gpu(h, w, name):
    """the kernels' volume of the four clean views, (1, nz, ny, nx, 2); never written to again"""
    dims, grid = TO.grid_of(SPECS[name])
    depth, R, t = TO.views(h, w)
    return gpu_integrate(dims, grid, TO.camera(h, w)[0], depth, R, t)


def module(h, w, name="room", batch=1, volumes=None, **kw):
    spec = SPECS[name]
    m = TsdfVolume(torch.from_numpy(rgbd_camera(h, w)), spec[0], spec[2], spec[1], truncation=spec[3], batch=batch, size=(h, w), **kw).to(DEV)
    if volumes is not None:
        m.volume.copy_(torch.cat(volumes))
    return m


# ---- 1. reset ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
@pytest.mark.parametrize("batch", [1, 3])
def test_reset_writes_every_voxel(name, batch):
    nx, ny, nz = SPECS[name][0]
    vol = torch.full((batch, nz, ny, nx, 2), float("nan"), dtype=torch.float32, device=DEV)
    assert ops.tsdf_reset(vol) is vol
    assert bool((vol[..., 0] == 1).all()) and bool((vol[..., 1] == 0).all())
    m = module(37, 53, name, batch)
    m.volume.fill_(float("nan"))
    m.reset()
    assert torch.equal(bits(m.volume), bits(vol))


# ---- 2. integration ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
@pytest.mark.parametrize("u16", [False, True])
def test_integrate_is_the_float32_oracle(h, w, name, u16):
    dims, grid = TO.grid_of(SPECS[name])
    cam = TO.camera(h, w)[0]
    d, scale, R, t = poked_views(h, w, u16)
    cases = {"4 frames": dict(), "max_weight 2": dict(max_weight=2.0), "a masked frame": dict(active=[True, False, True, True])}
    for what, kw in cases.items():
        got = gpu_integrate(dims, grid, cam, d, R, t, scale, **kw)
        ref = TO.integrate(TO.reset(dims, F32), d, R, t, cam, grid, z_scale=scale, dtype=F32, **kw)
        assert same_volume(got, ref), what
        assert ref[1].max() == (2 if "max_weight" in kw else 3 if "active" in kw else 4) and (ref[1] == 0).any() == (name != "tiny")
        if what == "4 frames":
            full_gpu, full_ref = got, ref
    # on top: a frame whose pose puts part of the volume behind the camera
    got = gpu_integrate(dims, grid, cam, d[1:2], BEHIND[0][None], BEHIND[1][None], scale, volume=full_gpu)
    ref = TO.integrate(full_ref, d[1:2], BEHIND[0][None], BEHIND[1][None], cam, grid, z_scale=scale, dtype=F32)
    assert same_volume(got, ref)
    changed = ref[1] != full_ref[1]
    cz = TO.centres(dims, grid, F32)[2]
    assert changed.any() and not changed[cz <= 1.75].any() and (cz <= 1.75).any()
    # the float64 oracle has the same weights: no voxel's gate flipped
    assert np.array_equal(TO.integrate(TO.reset(dims), d, R, t, cam, grid, z_scale=scale)[1], full_ref[1])


def test_integrate_frames_and_batches_are_independent():
    h, w = 37, 53
    dims, grid = TO.grid_of(TO.ODD)
    cam = TO.camera(h, w)[0]
    d, scale, R, t = poked_views(h, w, False)
    nx, ny, nz = dims
    together = gpu_integrate(dims, grid, cam, d, R, t)
    one_by_one = None
    for f in range(4):
        one_by_one = gpu_integrate(dims, grid, cam, d[f:f + 1], R[f:f + 1], t[f:f + 1], volume=one_by_one)
    assert torch.equal(bits(together), bits(one_by_one))
    assert torch.equal(bits(together), bits(gpu_integrate(dims, grid, cam, d, R, t)))            # run to run
    # a batch of 3 volumes with their own frames, poses and masks
    orders = [(0, 1, 2, 3), (3, 1, 0, 2), (2, 2, 1, 0)]
    masks = [(1, 1, 1, 1), (1, 0, 1, 1), (0, 1, 1, 0)]
    vol = ops.tsdf_reset(torch.empty((3, nz, ny, nx, 2), dtype=torch.float32, device=DEV))
    ops.tsdf_integrate(vol, torch.from_numpy(np.stack([d[list(o)] for o in orders])).to(DEV), t32(np.stack([R[list(o)] for o in orders])),
                       t32(np.stack([t[list(o)] for o in orders])), cam, grid[0].tolist(), grid[1], grid[2], 3.0, 1.0, TO.MIN_DEPTH,
                       TO.MAX_DEPTH, torch.tensor(masks, dtype=torch.uint8, device=DEV))
    for b, (o, m) in enumerate(zip(orders, masks)):
        single = gpu_integrate(dims, grid, cam, d[list(o)], R[list(o)], t[list(o)], max_weight=3.0, active=[bool(x) for x in m])
        assert torch.equal(bits(vol[b:b + 1]), bits(single)), b
        ref = TO.integrate(TO.reset(dims, F32), d[list(o)], R[list(o)], t[list(o)], cam, grid, max_weight=3.0, active=m, dtype=F32)
        assert same_volume(vol[b:b + 1], ref), b


# ---- 3. raycast ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
def test_raycast_matches_the_float64_oracle(h, w, name):
    dims, grid = TO.grid_of(SPECS[name])
    ki = TO.camera(h, w)[1]
    _, R, t = TO.views(h, w)
    vol = fused_gpu(h, w, name)
    assert same_volume(vol, TO.fused_room(h, w, SPECS[name], F32))
    m = module(h, w, name, 2, [vol, vol])
    vertex, normal = (x.cpu().numpy() for x in m.raycast(t32(R[[0, 2]]), t32(t[[0, 2]])))
    assert vertex.shape == (2, h, w, 4) and normal.shape == (2, h, w, 4)
    tol_v, tol_n = RAYCAST_TOL[(h, w), name]
    for b, view in enumerate((0, 2)):
        v64, vok64, n64, nok64 = TO.raycast(TO.fused_room(h, w, SPECS[name]), R[view], t[view], ki, h, w, grid)
        v32, vok32, n32, nok32 = TO.raycast(TO.fused_room(h, w, SPECS[name], F32), R[view], t[view], ki, h, w, grid, dtype=F32)
        assert np.array_equal(vok32, vok64) and np.array_equal(nok32, nok64)            # the float32 oracle alone: no flips
        assert np.abs(v32 - v64).max() <= tol_v / 4 * 1.001 and np.abs(n32 - n64).max() <= tol_n / 4 * 1.001
        vok, nok = vertex[b, ..., 3] != 0, normal[b, ..., 3] != 0
        assert set(np.unique(vertex[b, ..., 3])) <= {0.0, 1.0} and set(np.unique(normal[b, ..., 3])) <= {0.0, 1.0}
        flips = int((vok != vok64).sum() + (nok != nok64).sum())
        both_v, both_n = vok & vok64, nok & nok64
        dv = float(np.abs(vertex[b, ..., :3] - v64)[both_v].max())
        dn = float(np.abs(normal[b, ..., :3] - n64)[both_n].max()) if both_n.any() else 0.0
        same = np.array_equal(bits(vertex[b, ..., :3]), bits(v32)) and np.array_equal(bits(normal[b, ..., :3]), bits(n32))
        print(f"raycast {h} x {w} {name} view {view}: hits {vok64.mean():.3f}, normals {nok64.mean():.3f}, flips {flips}, vertex {dv:.3e} "
              f"(tolerance {tol_v:.2e}), normal {dn:.3e} (tolerance {tol_n:.2e}), float32 oracle's bits: {same}")
        assert flips <= FLIP_CAP * h * w
        assert dv <= tol_v and dn <= tol_n
        assert not vertex[b, ..., :3][~vok].any() and not normal[b, ..., :3][~nok].any() and not nok[~vok].any()
        assert vok64.mean() > (0.05 if name == "tiny" else 0.75) and nok64.any() == (name != "tiny")
        if nok.any():
            assert np.abs(np.linalg.norm(normal[b, ..., :3][nok], axis=-1) - 1).max() < 1e-6
            assert ((normal[b, ..., :3] * vertex[b, ..., :3]).sum(-1)[nok] <= 0).all()         # facing the camera
    # the raycast is what icp_refine takes as maps1: the layout of surfel_maps
    live = ops.surfel_maps(torch.from_numpy(TO.views(h, w)[0][[0, 2]]).to(DEV), t32(ki), 1.0, TO.MIN_DEPTH, TO.MAX_DEPTH, IO.JUMP)
    assert live[0].shape == (2, h, w, 4) and live[0].dtype == torch.float32


@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
def test_raycast_without_hits_writes_zeros(name):
    h, w = 37, 53
    dims, grid = TO.grid_of(SPECS[name])
    ki = TO.camera(h, w)[1]
    away = (np.diag([-1.0, 1.0, -1.0]), np.zeros(3))                                  # half a turn about y: the box is behind
    inside = torch.empty_like(fused_gpu(h, w, name))
    inside[..., 0], inside[..., 1] = -0.5, 1.0                                          # every voxel observed and inside a surface
    empty = ops.tsdf_reset(torch.empty_like(inside))
    for what, vol, pose in (("away", fused_gpu(h, w, name), away), ("inside", inside, (np.eye(3), np.zeros(3))),
                            ("empty", empty, (np.eye(3), np.zeros(3)))):
        m = module(h, w, name, 1, [vol])
        vertex, normal = m.raycast(t32(pose[0])[None], t32(pose[1])[None])
        assert not bool(vertex.any()) and not bool(normal.any()), what                 # NaN (a poisoned byte left) would be True
        ref = TO.raycast(tuple(vol.cpu().numpy()[0, ..., c] for c in (0, 1)), *pose, ki, h, w, grid, dtype=F32)
        assert not ref[1].any() and not ref[3].any(), what
    # the same `inside` volume seen through a positive shell is hit: the test above is not vacuous
    shell = inside.clone()
    shell[:, :(1 if name == "tiny" else 4)] = 0.5                                       # (tsdf, weight) = (0.5, 0.5) in the nearest slices
    hit = module(h, w, name, 1, [shell]).raycast(t32(np.eye(3))[None], torch.zeros(1, 3, device=DEV))[0]
    ref = TO.raycast((shell.cpu().numpy()[0, ..., 0], shell.cpu().numpy()[0, ..., 1]), np.eye(3), np.zeros(3), ki, h, w, grid, dtype=F32)
    assert np.array_equal(hit.cpu().numpy()[0, ..., 3] != 0, ref[1]) and ref[1].any()


# ---- 4. reproducibility ----------------------------------------------------------------------------------------------------------

def three_volumes(h, w, name="room"):
    """three different models of the room: all four views, two of them, three with a capped weight"""
    dims, grid = TO.grid_of(SPECS[name])
    cam = TO.camera(h, w)[0]
    depth, R, t = TO.views(h, w)
    return [fused_gpu(h, w, name), gpu_integrate(dims, grid, cam, depth[:2], R[:2], t[:2]),
            gpu_integrate(dims, grid, cam, depth[1:], R[1:], t[1:], max_weight=2.0)]


def test_results_are_bitwise_reproducible_and_independent_of_the_batch():
    h, w = 48, 64
    vols = three_volumes(h, w)
    live = torch.from_numpy(np.stack([synth_depth_room(s, h, w)[1] for s in (3, 4, 5)])).to(DEV)
    truth = synth_depth_room(4, h, w)[2:]                                               # predictions: the identity, the truth, the identity
    Rp, tp = t32(np.stack([np.eye(3), truth[0], np.eye(3)])), t32(np.stack([np.zeros(3), truth[1], np.zeros(3)]))
    m = module(h, w, "room", 3, vols)
    ray = m.raycast(Rp, tp)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ray, m.raycast(Rp, tp)))
    trk = m.track(live, Rp, tp)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(trk, m.track(live, Rp, tp)))
    assert trk[5].all() and torch.equal(bits(m.volume), bits(torch.cat(vols)))          # tracking leaves the model alone
    fwd = m(live, Rp, tp)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(fwd, trk))
    after = m.volume.clone()
    assert not torch.equal(bits(after), bits(torch.cat(vols)))
    again = module(h, w, "room", 3, vols)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again(live, Rp, tp), fwd)) and torch.equal(bits(again.volume), bits(after))
    for b in range(3):
        one = module(h, w, "room", 1, [vols[b]])
        assert all(torch.equal(bits(x[:1]), bits(y[b:b + 1])) for x, y in zip(one.raycast(Rp[b:b + 1], tp[b:b + 1]), ray)), b
        assert all(torch.equal(bits(x[:1]), bits(y[b:b + 1])) for x, y in zip(one.track(live[b:b + 1], Rp[b:b + 1], tp[b:b + 1]), trk)), b
        assert all(torch.equal(bits(x[:1]), bits(y[b:b + 1])) for x, y in zip(one(live[b:b + 1], Rp[b:b + 1], tp[b:b + 1]), fwd)), b
        assert torch.equal(bits(one.volume[0]), bits(after[b])), b
        # forward integrated the live frame at the tracked pose
        ref = ops.tsdf_integrate(vols[b].clone(), live[b:b + 1, None], fwd[0][b:b + 1, None], fwd[1][b:b + 1, None], m.camera, m.origin,
                                 m.voxel_size, m.truncation, m.max_weight)
        assert torch.equal(bits(ref[0]), bits(after[b])), b


# ---- 5. tracking -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_tracked(seed, h, w, dtype=F64):
    _, grid = TO.grid_of(TO.ROOM)
    live = synth_depth_room(seed, h, w)[1]
    return TO.track(TO.fused_room(h, w, TO.ROOM, dtype), grid, live, np.eye(3), np.zeros(3), h, w, dtype=dtype)


def test_track_reaches_the_oracle_and_the_truth():
    h, w = 48, 64
    seeds = (3, 4)
    vol = fused_gpu(h, w, "room")
    m = module(h, w, "room", 2, [vol, vol])
    live = torch.from_numpy(np.stack([synth_depth_room(s, h, w)[1] for s in seeds])).to(DEV)
    eye, zero = torch.eye(3, device=DEV).repeat(2, 1, 1), torch.zeros(2, 3, device=DEV)
    out = [x.cpu().numpy() for x in m.track(live, eye, zero)]
    assert out[0].shape == (2, 3, 3) and out[2].shape == (2, 6, 6) and out[5].dtype == bool
    tol = TRACK_TOL
    for b, seed in enumerate(seeds):
        R, t, info, rmse, count, ok = (x[b] for x in out)
        Ro, to, o = oracle_tracked(seed, h, w)
        R32, t32_, o32 = oracle_tracked(seed, h, w, F32)
        assert o32["count"] == o["count"] and o32["ok"] and o["ok"]                       # the float32 oracle alone: no gate flips
        assert IO.rotation_angle_deg_small(R32, Ro) <= tol[2] / 2 * 1.001 and np.abs(t32_ - to).max() <= tol[3] / 4 * 1.001
        truth = synth_depth_room(seed, h, w)[2:]
        rot_gt, t_gt = IO.rotation_angle_deg_small(R, truth[0]), np.abs(t - truth[1]).max()
        rot_o, t_o = IO.rotation_angle_deg_small(R, Ro), np.abs(t - to).max()
        dinfo = np.abs(info - o["information"]).max() / np.abs(o["information"]).max()
        print(f"track seed {seed}: truth {rot_gt:.3e} deg {t_gt:.3e} m; oracle {rot_o:.3e} deg {t_o:.3e} m; information {dinfo:.2e}; "
              f"rmse {rmse:.4e} / {o['rmse']:.4e}; count {count} / {o['count']}")
        assert ok
        assert rot_gt <= tol[0] and t_gt <= tol[1]
        assert rot_o <= tol[2] and t_o <= tol[3]
        assert abs(np.linalg.det(R.astype(F64)) - 1) <= 1e-5
        assert np.array_equal(info, info.T) and dinfo <= tol[4]
        assert abs(int(count) - o["count"]) <= FLIP_CAP * h * w and abs(rmse - o["rmse"]) <= tol[5] * o["rmse"]


def test_an_empty_volume_returns_the_prediction_and_integrates_nothing():
    h, w = 48, 64
    m = module(h, w, "room", 2, [fused_gpu(h, w, "room"), ops.tsdf_reset(torch.empty_like(fused_gpu(h, w, "room")))])
    before = m.volume.clone()
    truth = [synth_depth_room(s, h, w) for s in (3, 4)]
    live = torch.from_numpy(np.stack([x[1] for x in truth])).to(DEV)
    Rp, tp = t32(np.stack([x[2] for x in truth])), t32(np.stack([x[3] for x in truth]))
    R, t, info, rmse, count, ok = m(live, Rp, tp)
    assert ok.tolist() == [True, False] and int(count[1]) == 0 and float(rmse[1]) == 0 and not bool(info[1].any())
    assert torch.equal(bits(R[1]), bits(Rp[1])) and torch.equal(bits(t[1]), bits(tp[1]))       # the prediction's bits
    assert torch.equal(bits(m.volume[1]), bits(before[1])) and not torch.equal(bits(m.volume[0]), bits(before[0]))
    assert bool((m.volume[1, ..., 0] == 1).all()) and not bool(m.volume[1, ..., 1].any())
    # the pair beside it tracked from a prediction at the truth as well as from the identity
    assert IO.rotation_angle_deg_small(R[0].cpu().numpy(), truth[0][2]) <= 2 * TRACK_TOL[0]
    ra, ta = ops.pose_compose(R, t, Rp, tp)
    for b in range(2):
        want = TO.compose(R[b].cpu().numpy(), t[b].cpu().numpy(), Rp[b].cpu().numpy(), tp[b].cpu().numpy())
        assert np.array_equal(bits(ra[b].cpu().numpy()), bits(want[0])) and np.array_equal(bits(ta[b].cpu().numpy()), bits(want[1]))


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------------

def test_forward_replays_from_a_captured_graph_to_the_eager_bits():
    h, w = 48, 64
    start = torch.cat(three_volumes(h, w))
    _, R, t = TO.views(h, w)
    sets = []
    for order, views in (((3, 4, 5), (0, 1, 0)), ((5, 3, 4), (1, 0, 0)), ((4, 4, 3), (0, 0, 2))):
        live = torch.from_numpy(np.stack([synth_depth_room(s, h, w)[1] for s in order])).to(DEV)
        sets.append((live, t32(R[list(views)]), t32(t[list(views)])))
    m = module(h, w, "room", 3)
    eager = []
    for s in sets:
        m.volume.copy_(start)
        out = [x.clone() for x in m(*s)]
        eager.append((out, m.volume.clone()))
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
        m.volume.copy_(start)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, eager[i][0])), i
        assert torch.equal(bits(m.volume), bits(eager[i][1])), i
