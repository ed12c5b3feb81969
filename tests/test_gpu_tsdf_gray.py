"""K22 TSDF intensity on the GPU against tests/tsdf_gray_oracle.py (the numpy restatement of include/mi355x_match.h).

The integration and the gather are compared bit for bit with the oracle run in float32, which is the header's arithmetic.
Direct tracking is float32 kernels against the float64 oracle, so its tolerance is the deviation of the SAME oracle run in
float32 from its float64 run, measured on the CPU on the very scenes the test uses (the textured plane of photo_oracle, frame
1 fused at the identity into ROOM, frame 2 tracked from the identity), times 2 for the angle and 4 for the translation, as in
tests/test_gpu_direct_rgbd.py.  Nothing here was taken from the kernels.
    (48, 64):   float32 from float64 at most 3.1529e-6 deg, 1.0139e-7 m (seeds 0 1 2: 4.0753e-7 / 7.8572e-9, 7.9474e-7 / 2.8515e-8,
                3.1529e-6 / 1.0139e-7); the float64 oracle from the truth 1.8643e-2 / 6.8776e-4, 1.2932e-2 / 7.4820e-4,
                1.5486e-2 / 9.1242e-4 (deg / m)
    (120, 160): float32 from float64 at most 3.7049e-6 deg, 1.2110e-7 m (1.0023e-6 / 2.0508e-8, 3.7049e-6 / 1.2110e-7, 2.8320e-6 /
                9.8842e-8); from the truth 2.4718e-2 / 8.5116e-4, 2.9137e-2 / 9.4596e-4, 2.6599e-2 / 8.8594e-4
    -> PLANE_TOL = 2 / 4 times the deviation; from the truth: the oracle's own distance for the seed plus that.
    Both runs take 14 steps and have equal counts on all six scenes; the kernels' counts are held to the float32 oracle's with
    an allowance of 0 (the same arithmetic).
Measured on an MI355X: integration, the intensity maps, the hand-placed points and the mesh's vertices are the float32 oracle's
bits; on the plane the kernels end 4.5e-7 .. 3.7e-6 deg and 6.6e-9 .. 1.2e-7 m from the float64 oracle with the float32 oracle's
counts on all six scenes.
Runs unchanged under MI_POISON_EMPTY=1 (conftest.py): every sampler output comes from torch.empty."""
import functools

import numpy as np
import pytest
import torch

import icp_oracle as IO
import photo_oracle as PO
import tsdf_gray_oracle as GO
import tsdf_oracle as TO
from gpu_common import DEV, GPU, bits
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import DirectTsdfVolume, TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera, synth_depth_room

pytestmark = GPU
F32, F64 = np.float32, np.float64
SPECS = {"room": TO.ROOM, "odd": TO.ODD, "tiny": TO.TINY}
SEEDS = (0, 1, 2)
PLANE_TOL = {(48, 64): (2 * 3.1529e-6, 4 * 1.0139e-7), (120, 160): (2 * 3.7049e-6, 4 * 1.2110e-7)}
PLANE_TRUTH = {(48, 64): ((1.8643e-2, 6.8776e-4), (1.2932e-2, 7.4820e-4), (1.5486e-2, 9.1242e-4)),
               (120, 160): ((2.4718e-2, 8.5116e-4), (2.9137e-2, 9.4596e-4), (2.6599e-2, 8.8594e-4))}
ALIGN, NULL, SHAPE = -5, -1, -2


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def same_pair(got, ref):
    """a (nz, ny, nx, 2) tensor's records against the oracle's pair of arrays, bit for bit"""
    g = got.cpu().numpy()
    return np.array_equal(bits(g[..., 0]), bits(np.asarray(ref[0], F32))) and np.array_equal(bits(g[..., 1]), bits(np.asarray(ref[1], F32)))


def empty_pair(batch, dims):
    nx, ny, nz = dims
    vol = ops.tsdf_reset(torch.empty((batch, nz, ny, nx, 2), dtype=torch.float32, device=DEV))
    return vol, ops.tsdf_gray_reset(torch.full((batch, nz, ny, nx, 2), float("nan"), dtype=torch.float32, device=DEV))


def integrate(vol, ivol, grid, cam, depth, gray, R, t, scale=1.0, max_weight=TO.MAX_WEIGHT, active=None):
    """depth, gray (B, F, h, w) numpy, R (B, F, 3, 3), t (B, F, 3), active (B, F) or None -> (vol, ivol), updated in place"""
    act = None if active is None else torch.tensor(active, dtype=torch.bool, device=DEV)
    return ops.tsdf_integrate_gray(vol, ivol, torch.from_numpy(depth).to(DEV), torch.from_numpy(gray).to(DEV), t32(R), t32(t), cam,
                                   grid[0].tolist(), grid[1], grid[2], max_weight, scale, TO.MIN_DEPTH, TO.MAX_DEPTH, act)


def module(h, w, name="room", batch=1, volumes=None, cls=DirectTsdfVolume, **kw):
    spec = SPECS[name]
    m = cls(torch.from_numpy(rgbd_camera(h, w)), spec[0], spec[2], spec[1], truncation=spec[3], batch=batch, size=(h, w), **kw).to(DEV)
    if volumes is not None:
        m.volume.copy_(torch.cat([v for v, _ in volumes]))
        if cls is DirectTsdfVolume:
            m.intensity.copy_(torch.cat([i for _, i in volumes]))
    return m


def poked_views(h, w, small):
    """(depth (4, h, w), z_scale, gray (4, h, w), R, t): the room's views with a NaN and out-of-range depths and a NaN gray poked
    in; small: the uint16 depth + uint8 gray instance (no NaN exists there: 0 and 65535 counts, out of the range)"""
    depth, R, t = TO.views(h, w)
    d, g = depth.copy(), GO.views_gray(h, w).copy()
    spots = [(5, 7), (h // 2, w // 2), (h - 3, w - 4), (h // 2, w // 2 + 1)]
    if small:
        d, g, scale = np.round(d * 1000.0).astype(np.uint16), PO.as_u8(g), 0.001
        special = [0, 99, 10001, 65535]
    else:
        special, scale = [np.nan, 0.0999, 10.001, np.inf], 1.0
        g[1, h // 2 - 2:h // 2 + 3, w // 2 - 6:w // 2 - 1] = np.nan
        g[3, 7, 9] = np.inf
    for f in (0, 1, 3):
        for (y, x), v in zip(spots, special):
            d[f, y, x] = v
    return d, scale, g, R, t


@functools.lru_cache(maxsize=None)
def fused_gpu(h, w, name):
    """the kernels' pair of volumes of the four clean views with their gray frames, each (1, nz, ny, nx, 2); never written again"""
    dims, grid = TO.grid_of(SPECS[name])
    depth, R, t = TO.views(h, w)
    vol, ivol = empty_pair(1, dims)
    return integrate(vol, ivol, grid, TO.camera(h, w)[0], depth[None], GO.views_gray(h, w)[None], R[None], t[None])


@functools.lru_cache(maxsize=None)
def plane_gpu(seed, h, w, flat=False):
    """frame 1 of the textured plane (flat: with a constant gray) fused at the identity into ROOM by the kernels"""
    dims, grid = TO.grid_of(TO.ROOM)
    s = PO.scene("plane", seed, h, w)
    gray = np.full_like(s["gray1"], 100.0) if flat else s["gray1"]
    vol, ivol = empty_pair(1, dims)
    return integrate(vol, ivol, grid, TO.camera(h, w)[0], s["depth1"][None, None], gray[None, None], np.eye(3)[None, None],
                     np.zeros((1, 1, 3)))


def plane_live(h, w, seeds=SEEDS, flat=()):
    ss = [PO.scene("plane", s, h, w) for s in seeds]
    gray = np.stack([np.full_like(s["gray2"], 100.0) if i in flat else s["gray2"] for i, s in enumerate(ss)])
    return torch.from_numpy(np.stack([s["depth2"] for s in ss])).to(DEV), torch.from_numpy(gray).to(DEV)


def identity(b):
    return torch.eye(3, device=DEV).repeat(b, 1, 1), torch.zeros(b, 3, device=DEV)


# ---- 1. integration ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
@pytest.mark.parametrize("small", [False, True], ids=["f32", "u16+u8"])
def test_integrate_is_the_float32_oracle_and_leaves_k19_its_bits(name, small):
    h, w = 48, 64
    dims, grid = TO.grid_of(SPECS[name])
    cam = TO.camera(h, w)[0]
    d, scale, g, R, t = poked_views(h, w, small)
    orders, masks = [(0, 1, 2, 3), (3, 1, 0, 2)], [(1, 1, 1, 1), (1, 0, 1, 1)]                   # batch 2, a frame off in the second
    db, gb = np.stack([d[list(o)] for o in orders]), np.stack([g[list(o)] for o in orders])
    Rb, tb = np.stack([R[list(o)] for o in orders]), np.stack([t[list(o)] for o in orders])
    vol, ivol = integrate(*empty_pair(2, dims), grid, cam, db, gb, Rb, tb, scale, 3.0, masks)
    k19 = ops.tsdf_integrate(ops.tsdf_reset(torch.empty_like(vol)), torch.from_numpy(db).to(DEV), t32(Rb), t32(tb), cam, grid[0].tolist(),
                             grid[1], grid[2], 3.0, scale, TO.MIN_DEPTH, TO.MAX_DEPTH, torch.tensor(masks, dtype=torch.bool, device=DEV))
    assert torch.equal(bits(vol), bits(k19))                                           # mi_tsdf_integrate's bits
    for b in range(2):
        ref = GO.integrate(TO.reset(dims, F32), GO.reset(dims, F32), db[b], gb[b], Rb[b], tb[b], cam, grid, max_weight=3.0, z_scale=scale,
                           active=masks[b], dtype=F32)
        assert same_pair(vol[b], ref[0]) and same_pair(ivol[b], ref[1]), b
        seen = ref[1][1] > 0
        assert seen.any() and not ref[1][0][~seen].any() and ref[1][1].max() == 3
        assert name == "tiny" or (ref[0][1] > ref[1][1]).any()                          # free space in front: tsdf alone
        # the same volume alone; and its frames one per call
        solo = integrate(*empty_pair(1, dims), grid, cam, db[b:b + 1], gb[b:b + 1], Rb[b:b + 1], tb[b:b + 1], scale, 3.0, masks[b:b + 1])
        assert torch.equal(bits(solo[0][0]), bits(vol[b])) and torch.equal(bits(solo[1][0]), bits(ivol[b])), b
        step = empty_pair(1, dims)
        for f in range(4):
            integrate(*step, grid, cam, db[b:b + 1, f:f + 1], gb[b:b + 1, f:f + 1], Rb[b:b + 1, f:f + 1], tb[b:b + 1, f:f + 1], scale, 3.0,
                      [masks[b][f:f + 1]])
        assert torch.equal(bits(step[0][0]), bits(vol[b])) and torch.equal(bits(step[1][0]), bits(ivol[b])), b
    if not small and name != "tiny":                                                  # the NaN gray was looked at: it changes the volume
        clean = GO.integrate(TO.reset(dims, F32), GO.reset(dims, F32), db[0], np.nan_to_num(gb[0], nan=50.0, posinf=50.0), Rb[0], tb[0],
                             cam, grid, max_weight=3.0, dtype=F32)
        assert not same_pair(ivol[0], clean[1])


def test_reset_and_the_module_write_every_record():
    for name, batch in (("odd", 3), ("tiny", 1)):
        nx, ny, nz = SPECS[name][0]
        ivol = torch.full((batch, nz, ny, nx, 2), float("nan"), dtype=torch.float32, device=DEV)
        assert ops.tsdf_gray_reset(ivol) is ivol and not bool(ivol.any())               # NaN would be True
        m = module(37, 53, name, batch)
        m.volume.fill_(float("nan"))
        m.intensity.fill_(float("nan"))
        m.reset()
        assert not bool(m.intensity.any()) and bool((m.volume[..., 0] == 1).all()) and not bool(m.volume[..., 1].any())


# ---- 2. the sampler ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(37, 53), (48, 64)])
@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
def test_the_models_intensity_map_is_the_float32_oracle(h, w, name):
    dims, grid = TO.grid_of(SPECS[name])
    _, R, t = TO.views(h, w)
    pair = fused_gpu(h, w, name)
    ref = GO.fused_room(h, w, SPECS[name], F32)
    assert same_pair(pair[0][0], ref[0]) and same_pair(pair[1][0], ref[1])
    m = module(h, w, name, 2, [pair, pair])
    Rb, tb = t32(R[[0, 3]]), t32(t[[0, 3]])
    vertex, normal, inten = m.raycast(Rb, tb)
    parent = TsdfVolume.raycast(m, Rb, tb)
    assert torch.equal(bits(vertex), bits(parent[0])) and torch.equal(bits(normal), bits(parent[1]))
    assert inten.shape == (2, h, w, 4)
    v, got = vertex.cpu().numpy(), inten.cpu().numpy()
    for b, view in enumerate((0, 3)):
        # the oracle's gather at the kernel's own vertex map, and the oracle's whole raycast
        I, ok = GO.sample(ref[1], v[b, ..., :3].reshape(-1, 3), v[b, ..., 3].ravel(), grid, R[view].astype(F32), t[view].astype(F32), F32)
        assert np.array_equal(got[b, ..., 3].ravel() != 0, ok) and np.array_equal(bits(got[b, ..., 0].ravel()), bits(I))
        assert not got[b, ..., 1:3].any() and set(np.unique(got[b, ..., 3])) <= {0.0, 1.0} and not got[b, ..., 0][got[b, ..., 3] == 0].any()
        maps, (rec, rok) = GO.raycast(*ref, R[view], t[view], TO.camera(h, w)[1], h, w, grid, dtype=F32)
        flips = int((rok != (got[b, ..., 3] != 0)).sum())
        print(f"intensity map {h} x {w} {name} view {view}: hits {maps[1].mean():.3f}, with intensity {ok.mean():.3f}, flips against the "
              f"oracle's own raycast {flips}, its bits: {np.array_equal(bits(got[b, ..., 0]), bits(rec[..., 0].astype(F32)))}")
        assert ok.any() and (name == "tiny" or ok.sum() > 0.9 * (v[b, ..., 3] != 0).sum())


@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
def test_hand_placed_points_are_the_float32_oracle(name):
    dims, grid = TO.grid_of(SPECS[name])
    pts, names = GO.hand_points(dims, grid)
    assert len(pts) % 64 != 0
    R, t = (x.astype(F32) for x in synth_depth_room(2, 48, 64)[2:])
    one = GO.reset(dims, F32)
    one[0][1, 0, 1], one[1][1, 0, 1] = 77.5, 3.0
    vols = [GO.synthetic(dims), one, GO.reset(dims, F32)]
    ivol = t32(np.stack([np.stack(v, axis=-1) for v in vols]))
    p3 = t32(np.stack([pts] * 3))
    for pose in (None, (R, t)):
        kw = {} if pose is None else dict(r=t32(np.stack([R] * 3)), t=t32(np.stack([t] * 3)))
        got = ops.tsdf_sample_gray(ivol, p3, grid[0].tolist(), grid[1], **kw).cpu().numpy()
        for b, v in enumerate(vols):
            I, ok = GO.sample(v, pts[:, :3], pts[:, 3], grid, *(pose or ()), dtype=F32)
            assert np.array_equal(got[b, :, 3] != 0, ok) and np.array_equal(bits(got[b, :, 0]), bits(I)), (b, pose is None)
            assert not got[b, :, 1:3].any() and set(np.unique(got[b, :, 3])) <= {0.0, 1.0}
            solo = ops.tsdf_sample_gray(ivol[b:b + 1].clone(), p3[:1], grid[0].tolist(), grid[1], **{k: x[:1] for k, x in kw.items()})
            assert torch.equal(bits(solo[0]), bits(t32(got[b])))                          # alone as in the batch
        assert not got[2].any()
    row = {n: i for i, n in enumerate(names)}
    world = ops.tsdf_sample_gray(ivol, p3, grid[0].tolist(), grid[1]).cpu().numpy()
    for n in ("far outside", "nan", "inf", "f = 0"):
        assert not world[0, row[n]].any(), n
    if name == "room":                                                                  # dyadic origin and voxel size: exact corners
        assert not world[0, row["below"]].any() and not world[0, row["above"]].any()
        assert world[0, row["g = 0"], 0] == vols[0][0][0, 0, 0] and world[0, row["g = n - 1"], 0] == vols[0][0][-1, -1, -1]
        assert world[0, row["some observed corners"], 3] == 1 and not world[0, row["no observed corner"]].any()


def test_mesh_vertices_get_their_gray_without_a_pose():
    h, w = 48, 64
    dims, grid = TO.grid_of(TO.ROOM)
    m = module(h, w, "room", 2, [fused_gpu(h, w, "room"), plane_gpu(0, h, w)])
    sized = m.extract_surface()
    v, nrm, tri, counts, inten, valid = sized
    c = counts.cpu().numpy()
    assert inten.shape == v.shape[:2] and valid.shape == v.shape[:2] and valid.dtype == torch.bool and c[:, 0].min() > 500
    parent = TsdfVolume.extract_surface(m)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(parent, sized[:4]))
    refs = [GO.fused_room(h, w, TO.ROOM, F32)[1], GO.plane_model(0, h, w, dtype=F32)[1]]
    fused = [GO.views_gray(h, w), PO.scene("plane", 0, h, w)["gray1"]]
    for b in range(2):
        n = int(c[b, 0])
        assert bool(valid[b, :n].all()) and not bool(valid[b, n:].any()) and not bool(inten[b, n:].any())       # every vertex; zeros beyond
        vb = v[b].cpu().numpy()
        I, ok = GO.sample(refs[b], vb[:, :3], vb[:, 3], grid, dtype=F32)
        assert np.array_equal(ok, valid[b].cpu().numpy()) and np.array_equal(bits(inten[b].cpu().numpy()), bits(I))
        # a convex combination of running means of the frames' gray values: inside their range, up to float32 rounding
        assert fused[b].min() - 1e-3 <= I[:n].min() and I[:n].max() <= fused[b].max() + 1e-3
        print(f"mesh gray of volume {b}: {n} vertices, median distance from the texture at the vertex "
              f"{np.median(np.abs(I[:n] - PO.texture(vb[:n, :3].astype(F64)))):.2f} gray levels")
    pv, pn, pc, pi, pok = m.extract_points(max_points=int(c[:, 0].max()) + 7)
    assert torch.equal(bits(pi[:, :v.shape[1]]), bits(inten)) and not bool(pok[:, v.shape[1]:].any()) and pi.shape[1] == v.shape[1] + 7
    empty = module(h, w, "tiny", 1)
    empty.reset()
    out = empty.extract_surface()
    assert out[4].shape == (1, 0) and out[5].shape == (1, 0)


# ---- 3. the scene the feature is for -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_tracked(seed, h, w, dtype=F64):
    vol, ivol, grid, s = GO.plane_model(seed, h, w, dtype=dtype)
    return GO.track(vol, ivol, grid, s["depth2"], s["gray2"], np.eye(3), np.zeros(3), h, w, dtype=dtype)


@pytest.mark.parametrize("h,w", [(48, 64), (120, 160)])
def test_direct_tracking_moves_on_the_textured_plane_where_k19_is_frozen(h, w):
    pairs = [plane_gpu(s, h, w) for s in SEEDS]
    depth, gray = plane_live(h, w)
    eye, zero = identity(3)
    k19 = module(h, w, "room", 3, pairs, cls=TsdfVolume).track(depth, eye, zero)
    assert k19[5].tolist() == [False] * 3 and torch.equal(bits(k19[0]), bits(eye)) and torch.equal(bits(k19[1]), bits(zero))
    m = module(h, w, "room", 3, pairs)
    before = (m.volume.clone(), m.intensity.clone())
    R, t, info, rmse, count, rmse_p, count_p, ok = (x.cpu().numpy() for x in m.track(depth, gray, eye, zero))
    assert ok.tolist() == [True] * 3 and torch.equal(bits(m.volume), bits(before[0])) and torch.equal(bits(m.intensity), bits(before[1]))
    for b, seed in enumerate(SEEDS):
        s = PO.scene("plane", seed, h, w)
        (Ro, to, o), (R32, t32_, o32) = oracle_tracked(seed, h, w), oracle_tracked(seed, h, w, F32)
        assert o["ok"] and o32["ok"] and o["steps"] == o32["steps"] == 14
        assert (o32["count"], o32["count_photo"]) == (o["count"], o["count_photo"])       # the float32 oracle alone: no gate flips
        tol, truth = PLANE_TOL[(h, w)], PLANE_TRUTH[(h, w)][b]
        assert IO.rotation_angle_deg_small(R32.astype(F64), Ro) <= tol[0] / 2 * 1.01 and np.abs(t32_ - to).max() <= tol[1] / 4 * 1.01
        rot_gt, t_gt = IO.rotation_angle_deg_small(R[b], s["R"]), np.abs(t[b] - s["t"]).max()
        rot_o, t_o = IO.rotation_angle_deg_small(R[b], Ro), np.abs(t[b] - to).max()
        print(f"plane {h}x{w} seed {seed}: truth {rot_gt:.3e} deg {t_gt:.3e} m; oracle {rot_o:.3e} deg {t_o:.3e} m (tolerance {tol[0]:.2e} "
              f"{tol[1]:.2e}); counts {count[b]} / {o32['count']}, {count_p[b]} / {o32['count_photo']}; rmse_photo {rmse_p[b]:.4e} / "
              f"{o['rmse_photo']:.4e}")
        assert rot_o <= tol[0] and t_o <= tol[1]
        assert rot_gt <= truth[0] * 1.001 + tol[0] and t_gt <= truth[1] * 1.001 + tol[1]
        assert int(count[b]) == o32["count"] and int(count_p[b]) == o32["count_photo"]
        assert abs(np.linalg.det(R[b].astype(F64)) - 1) <= 1e-5 and np.array_equal(info[b], info[b].T)


# ---- 4. photo_weight = 0 ---------------------------------------------------------------------------------------------------------------

def test_photo_weight_zero_is_the_parents_tracking():
    h, w = 48, 64
    pair = fused_gpu(h, w, "room")
    live = torch.from_numpy(TO.views(h, w, (3, 4))[0][1:]).to(DEV)                          # the unseen second views of seeds 3 and 4
    gray = torch.from_numpy(GO.views_gray(h, w, (3, 4))[1:]).to(DEV)
    eye, zero = identity(2)
    want = module(h, w, "room", 2, [pair, pair], cls=TsdfVolume).track(live, eye, zero)
    got = module(h, w, "room", 2, [pair, pair], photo_weight=0.0).track(live, gray, eye, zero)
    assert want[5].all() and len(got) == 8
    for a, b in zip(want, (*got[:5], got[7])):
        assert torch.equal(bits(a), bits(b))
    assert got[6].tolist() == [0, 0] and got[5].tolist() == [0.0, 0.0]
    moved = module(h, w, "room", 2, [pair, pair]).track(live, gray, eye, zero)             # the term, when on, is really in
    assert moved[6].min() > 1000 and not torch.equal(bits(moved[0]), bits(want[0]))


# ---- 5. a sequence -----------------------------------------------------------------------------------------------------------------------

def test_forward_tracks_and_fuses_a_sequence_of_the_plane():
    h, w = 48, 64
    m = module(h, w, "room", 1, [plane_gpu(0, h, w)])
    by_hand = [x.clone() for x in plane_gpu(0, h, w)]
    Rp, tp = identity(1)
    for seed in SEEDS:                                         # each frame predicted at the pose of the one before
        depth, gray = plane_live(h, w, (seed,))
        s = PO.scene("plane", seed, h, w)
        R, t, info, rmse, count, rmse_p, count_p, ok = m(depth, gray, Rp, tp)
        rot, tr = IO.rotation_angle_deg_small(R[0].cpu().numpy(), s["R"]), float(np.abs(t[0].cpu().numpy() - s["t"]).max())
        print(f"sequence, frame of seed {seed}: ok {bool(ok[0])}, counts {int(count[0])} + {int(count_p[0])}, {rot:.3e} deg {tr:.3e} m from "
              f"the truth")
        assert bool(ok[0]) and rot < 0.05 and tr < 2e-3         # the bounds of tests/test_tsdf_gray_host.py for a single frame
        ops.tsdf_integrate_gray(*by_hand, depth[:, None], gray[:, None], R[:, None], t[:, None], m.camera, m.origin, m.voxel_size,
                                m.truncation, m.max_weight)
        assert torch.equal(bits(m.volume), bits(by_hand[0])) and torch.equal(bits(m.intensity), bits(by_hand[1]))
        Rp, tp = R, t
    assert float(m.intensity[..., 1].max()) == 4.0


# ---- 6. reproducibility and graph capture -----------------------------------------------------------------------------------------------

def test_a_frozen_volume_beside_a_good_one_and_run_to_run():
    h, w = 48, 64
    pairs = [plane_gpu(1, h, w), plane_gpu(1, h, w, flat=True), plane_gpu(2, h, w)]
    depth, gray = plane_live(h, w, (1, 1, 2), flat=(1,))
    eye, zero = identity(3)
    m = module(h, w, "room", 3, pairs)
    out = m(depth, gray, eye, zero)
    assert out[7].tolist() == [True, False, True]
    assert torch.equal(bits(out[0][1]), bits(eye[1])) and torch.equal(bits(out[1][1]), bits(zero[1]))       # frozen: the prediction
    assert torch.equal(bits(m.volume[1]), bits(pairs[1][0][0])) and torch.equal(bits(m.intensity[1]), bits(pairs[1][1][0]))
    assert not torch.equal(bits(m.intensity[0]), bits(pairs[0][1][0]))
    again = module(h, w, "room", 3, pairs)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again(depth, gray, eye, zero), out))            # run to run
    assert torch.equal(bits(again.volume), bits(m.volume)) and torch.equal(bits(again.intensity), bits(m.intensity))
    for b in (0, 2):
        one = module(h, w, "room", 1, [pairs[b]])
        solo = one(depth[b:b + 1], gray[b:b + 1], eye[:1], zero[:1])
        assert all(torch.equal(bits(x[:1]), bits(y[b:b + 1])) for x, y in zip(solo, out)), b
        assert torch.equal(bits(one.volume[0]), bits(m.volume[b])) and torch.equal(bits(one.intensity[0]), bits(m.intensity[b])), b


def test_forward_replays_from_a_captured_graph_to_the_eager_bits():
    h, w = 48, 64
    pairs = [plane_gpu(s, h, w) for s in SEEDS]
    start = (torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs]))
    eye, zero = identity(3)
    truth = PO.scene("plane", 1, h, w)
    sets = []
    for order, flat in (((0, 1, 2), ()), ((0, 1, 2), (2,)), ((0, 1, 2), (0, 1))):
        depth, gray = plane_live(h, w, order, flat)
        Rp, tp = eye.clone(), zero.clone()
        if flat:
            Rp[1], tp[1] = t32(truth["R"]), t32(truth["t"])                               # one prediction at the truth
        sets.append((depth, gray, Rp, tp))
    m = module(h, w, "room", 3)

    def restart():
        m.volume.copy_(start[0])
        m.intensity.copy_(start[1])
    eager = []
    for s in sets:
        restart()
        out = [x.clone() for x in m(*s)]
        eager.append((out, m.volume.clone(), m.intensity.clone()))
    assert eager[0][0][7].all()
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
        restart()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, eager[i][0])), i
        assert torch.equal(bits(m.volume), bits(eager[i][1])) and torch.equal(bits(m.intensity), bits(eager[i][2])), i


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------

def test_argument_checks_on_device_tensors():
    h, w = 48, 64
    vol, ivol = (x.clone() for x in fused_gpu(h, w, "tiny"))
    dims, grid = TO.grid_of(TO.TINY)
    cam = TO.camera(h, w)[0]
    depth, gray = torch.ones(1, 2, h, w, device=DEV), torch.ones(1, 2, h, w, device=DEV)
    R, t = torch.eye(3, device=DEV).repeat(1, 2, 1, 1), torch.zeros(1, 2, 3, device=DEV)
    g = (grid[0].tolist(), grid[1], grid[2])

    def refused(match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
    refused("intensity volume must be float32", lambda: ops.tsdf_integrate_gray(vol, ivol[:, :1], depth, gray, R, t, cam, *g))
    refused("intensity volume must be float32", lambda: ops.tsdf_integrate_gray(vol, ivol.double(), depth, gray, R, t, cam, *g))
    refused("gray must be float32 or uint8", lambda: ops.tsdf_integrate_gray(vol, ivol, depth, gray.half(), R, t, cam, *g))
    refused("depth must be float32 or uint16", lambda: ops.tsdf_integrate_gray(vol, ivol, depth.double(), gray, R, t, cam, *g))
    refused("depth's shape", lambda: ops.tsdf_integrate_gray(vol, ivol, depth, gray[:, :1], R, t, cam, *g))
    refused("poses must be", lambda: ops.tsdf_integrate_gray(vol, ivol, depth, gray, R[:, :1], t, cam, *g))
    refused("active must be", lambda: ops.tsdf_integrate_gray(vol, ivol, depth, gray, R, t, cam, *g, active=torch.ones(1, 3, device=DEV).bool()))
    refused("no CPU path", lambda: ops.tsdf_integrate_gray(vol, ivol, depth, gray.cpu(), R, t, cam, *g))
    refused("no CPU path", lambda: ops.tsdf_integrate_gray(vol, ivol.cpu(), depth, gray, R, t, cam, *g))
    pts = torch.ones(1, 5, 4, device=DEV)
    refused("points must be float32", lambda: ops.tsdf_sample_gray(ivol, pts[..., :3], g[0], g[1]))
    refused("points must be float32", lambda: ops.tsdf_sample_gray(ivol, pts.double(), g[0], g[1]))
    refused("points must be float32", lambda: ops.tsdf_sample_gray(ivol, torch.ones(2, 5, 4, device=DEV), g[0], g[1]))
    refused("both r and t", lambda: ops.tsdf_sample_gray(ivol, pts, g[0], g[1], r=R[:, 0]))
    refused("pose must be", lambda: ops.tsdf_sample_gray(ivol, pts, g[0], g[1], r=R[:, 0], t=t))
    refused("voxel_size > 0", lambda: ops.tsdf_sample_gray(ivol, pts, g[0], 0.0))
    refused("no CPU path", lambda: ops.tsdf_sample_gray(ivol, pts.cpu(), g[0], g[1]))
    refused("must be float32", lambda: ops.tsdf_gray_reset(ivol[..., :1]))
    assert ops.tsdf_sample_gray(ivol, pts[:, :0], g[0], g[1]).shape == (1, 0, 4)            # no point: nothing to do
    before = (vol.clone(), ivol.clone())
    m = module(h, w, "tiny", 1, [(vol, ivol)])
    refused("depth's shape", lambda: m.integrate(depth[:, 0], gray[:, 0, :-1], R[:, 0], t[:, 0]))
    refused(r"\(1, H, W\)", lambda: m.track(depth, gray, R[:, 0], t[:, 0]))
    assert torch.equal(bits(vol), bits(before[0])) and torch.equal(bits(ivol), bits(before[1]))


def test_misaligned_buffers_are_refused_at_the_c_entries():
    lib = N.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    grid = (-1.0, -0.8, 1.2, 1.0)
    assert lib.mi_tsdf_gray_reset(p + 8, 1, 2, 2, 2, None) == ALIGN and lib.mi_tsdf_gray_reset(p, 1, 2, 2, 2, None) == 0
    common = (1, 2, 2, 2, *grid, 1.0, 64.0, p + 1024, 0, p + 2048, 0, 1, 3, 3, 50.0, 50.0, 1.0, 1.0, 1.0, 0.1, 10.0, p + 3072, p + 3200, None, None)
    assert lib.mi_tsdf_integrate_gray(p + 8, p + 512, *common) == ALIGN and lib.mi_tsdf_integrate_gray(p, p + 512 + 8, *common) == ALIGN
    assert lib.mi_tsdf_integrate_gray(p, None, *common) == NULL
    sample = lambda ivol, pts, out, r=None, t=None: lib.mi_tsdf_sample_gray(ivol, 1, 2, 2, 2, *grid, pts, 5, r, t, out, None)
    assert sample(p + 8, p + 1024, p + 2048) == ALIGN and sample(p, p + 1024 + 4, p + 2048) == ALIGN
    assert sample(p, p + 1024, p + 2048 + 8) == ALIGN and sample(p, p + 1024, p + 2048, r=p + 3072) == NULL
    assert sample(p, p + 1024, p + 2048) == 0 and lib.mi_tsdf_sample_gray(p, 1, 2, 2, 2, *grid, p + 1024, 0, None, None, p + 2048, None) == SHAPE
    torch.cuda.synchronize()
    assert not bool(buf.any())                                  # an empty volume and zero points: zeros out, nothing else touched
