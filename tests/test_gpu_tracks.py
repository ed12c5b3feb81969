"""K28 landmark tracks on the GPU against the numpy oracle (tests/tracks_oracle.py): mi_tracks_build and mi_tracks_triangulate at
the smallest shapes at which each mechanism can go wrong, and what the contract makes exact, bit for bit.

Every integer output of mi_tracks_build is defined by the inputs alone and must EQUAL the oracle's; track_keypoints equals it
bit for bit.

Tolerance of the triangulation.  The kernel runs csrc/tracks_math.h in float64 in the header's stated operation order, and so
does the oracle; tests/test_tracks_host.py measures the largest deviation of the host-compiled tracks_math.h from the oracle
over TRI_SCENES (points relative to max(|X|, 1), e2max relative to max_e2, cos_par absolute) and asserts TRI_TOL against it
with the project's margin of 4.  Measured: 0 on every quantity of every scene (the same IEEE operations in the same order), so
TRI_TOL = 0 and what remains is the floor: one float32 ulp of the value, since the outputs are rounded to float32.  point_ok
must equal the oracle's except for landmarks whose e2max or cos_par lies within that tolerance of its threshold, at most 1 %
of a scene's landmarks (measured: none on any scene).

End to end (synth_track_window at F = 6, K = 64, 0.5 px, 10 % wrong matches, poses 0.002 rad / 2 mm off): on the oracle 100 %
of the point_ok landmarks are pure and 100 % of the pure eligible tracks are point_ok on the seed used here (over seeds 1 .. 7:
100 % and 90.5 % .. 100 %); tests/test_tracks_host.py asserts the two conditions on the oracle first."""
import functools

import numpy as np
import pytest
import torch

import tracks_oracle as TO
from gpu_common import DEV, GPU, gpu, same_bits, twice
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import BundleAdjuster, LandmarkTracks
from onnx_image_processing_amd.synth import rgbd_camera, synth_ba_window, synth_track_window

pytestmark = GPU
F32, F64 = np.float32, np.float64
MARGIN = 4.0
TRI_TOL = 0.0                           # 4 x the measured deviation of the host-compiled tracks_math.h from the oracle (0)
MAX_PX, MIN_PARALLAX_DEG = 3.0, 1.0
CAMERA = rgbd_camera()
FOCAL = float((CAMERA[0, 0] + CAMERA[1, 1]) / 2)
MAX_E2, MAX_COS = float(F32((MAX_PX / FOCAL) ** 2)), float(F32(np.cos(np.radians(MIN_PARALLAX_DEG))))
E2E_SEED, E2E_LANDMARKS = 5, 64
BIG = 0x7FFFFFFF


def k_inv_gpu():
    return torch.from_numpy(np.linalg.inv(CAMERA)).float().to(DEV)


# ---- build scenes ---------------------------------------------------------------------------------------------------------------------
def _window(F, K, pairs, matches, L, min_views=2, kp_valid=None, M=None):
    """pairs [(a, b)], matches: per pair a list of (i, j); the lists are padded to M with invalid records holding garbage"""
    P = len(pairs)
    M = M or max(1, max(len(m) for m in matches))
    ij = np.empty((P, M, 2), np.int32)
    ij[..., 0], ij[..., 1] = -1, BIG
    mv = np.zeros((P, M), bool)
    for p, ms in enumerate(matches):
        for m, rec in enumerate(ms):
            ij[p, m] = rec
            mv[p, m] = True
    rng = np.random.default_rng(F * 1000 + K)
    kp = rng.uniform(0, 480, (F, K, 2)).astype(F32)
    return dict(keypoints=kp, pair_frames=np.array(pairs, np.int32).reshape(P, 2), match_ij=ij, match_valid=mv, kp_valid=kp_valid,
                min_views=min_views, L=L)


def _synth(seed, F, K, landmarks, L, span=2, min_views=2):
    kp, _, pf, ij, mv = synth_track_window(seed, F, K, landmarks, pair_span=span)[:5]
    return dict(keypoints=kp, pair_frames=pf, match_ij=ij, match_valid=mv, kp_valid=None, min_views=min_views, L=L)


def _chain16():
    """two 16-frame chains whose matches are listed last pair first: the smallest node is at the far end of the list"""
    F, K = 16, 3
    pairs = [(f, f + 1) for f in range(F - 2, -1, -1)]
    matches = [[((2 * f) % K, (2 * f + 2) % K), ((2 * f + 1) % K, (2 * f + 3) % K)] for f, _ in pairs]
    return _window(F, K, pairs, matches, 4)


def _cut():
    """20 eligible tracks of lengths 2 .. 4 into 8 slots"""
    F, K = 4, 20
    length = [2 + (7 * k) % 3 for k in range(K)]
    pairs = [(0, 1), (1, 2), (2, 3)]
    return _window(F, K, pairs, [[(k, k) for k in range(K) if length[k] >= b + 1] for _, b in pairs], 8)


def _padding():
    """valid bytes on records that are padding all the same: indices -1 and 0x7fffffff, a == b, a frame outside the window;
    a kp_valid that removes the middle of the chain 0:0 - 1:0 - 2:0; the chain 0:1 - 1:1 - 2:1 stays"""
    kv = np.ones((3, 4), bool)
    kv[1, 0] = False
    pairs = [(0, 1), (1, 2), (1, 1), (0, 3), (-1, 2)]
    matches = [[(0, 0), (1, 1), (-1, 2), (2, BIG)], [(0, 0), (1, 1), (BIG, -1), (3, 4)], [(2, 3), (0, 1)], [(2, 2), (3, 3)], [(2, 2), (3, 3)]]
    return _window(3, 4, pairs, matches, 4, kp_valid=kv)


BUILD_SCENES = {
    "1x1": lambda: _window(2, 1, [(0, 1)], [[(0, 0)]], 1),
    # 0:0 - 1:0 - 2:0 is a chain; 0:1 is matched to 1:1 AND 1:2: a conflict made directly; 1:3 - 2:3 a plain pair
    "chain-conflict": lambda: _window(3, 5, [(0, 1), (1, 2)], [[(0, 0), (1, 1), (1, 2)], [(0, 0), (3, 3)]], 3),
    # 0:0 - 1:0 - 2:0 - 0:1: two nodes of frame 0 joined through frames 1 and 2; 0:2 - 1:2 - 2:2 - 0:2 is a consistent cycle
    "conflict-via-third": lambda: _window(3, 4, [(0, 1), (1, 2), (2, 0)], [[(0, 0), (2, 2)], [(0, 0), (2, 2)], [(0, 1), (2, 2)]], 2),
    "chain16-reversed": _chain16,
    "5x37": lambda: _synth(11, 5, 37, 30, 8, span=4, min_views=3),             # 185 nodes: a multiple of neither 64 nor 256
    "cut": _cut,
    "repeats": lambda: _window(3, 6, [(0, 1), (1, 0), (0, 1), (1, 2), (2, 1)],
                               [[(0, 0), (1, 1), (0, 0)], [(0, 0), (2, 2)], [(1, 1), (3, 3), (3, 3)], [(0, 5), (1, 4)], [(5, 0), (3, 3)]], 5),
    "padding": _padding,
    "synth-6x64": lambda: _synth(5, 6, 64, 64, 32),
    "largest": lambda: _synth(7, 16, 1024, 900, 2048, span=1),                # 128 KiB of labels in LDS
}
BUILD_NAMES = list(BUILD_SCENES)


@functools.lru_cache(maxsize=None)
def build_scene(name):
    return BUILD_SCENES[name]()


@functools.lru_cache(maxsize=None)
def build_oracle(name):
    w = build_scene(name)
    return TO.build(w["keypoints"], w["pair_frames"], w["match_ij"], w["match_valid"], w["kp_valid"], w["min_views"], w["L"])


def run_build(windows, min_views, L):
    """a list of windows of one shape as a batch -> the six outputs as numpy arrays"""
    stack = lambda k: np.stack([w[k] for w in windows])
    kv = None if windows[0]["kp_valid"] is None else gpu(stack("kp_valid"))
    out = ops.tracks_build(*gpu(stack("keypoints"), stack("pair_frames"), stack("match_ij"), stack("match_valid")), kv, min_views, L)
    return tuple(o.cpu().numpy() for o in out)


def check_build(got, want, where):
    track_kp, vis, track_keypoints, track_len, kp_track, counts = got
    for k, g in (("track_kp", track_kp), ("vis", vis), ("track_len", track_len), ("kp_track", kp_track), ("counts", counts)):
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (where, k, g, want[k])
    assert np.array_equal(track_keypoints.view(np.uint32), want["track_keypoints"].view(np.uint32)), where


@pytest.mark.parametrize("name", BUILD_NAMES)
def test_build_equals_the_oracle(name):
    w, want = build_scene(name), build_oracle(name)
    got = run_build([w], w["min_views"], w["L"])
    print(f"{name}: counts {got[5][0].tolist()}")
    check_build(tuple(g[0] for g in got), want, name)


# ---- determinism and writes -------------------------------------------------------------------------------------------------------
def _ragged_batch():
    """four windows of one shape and different content; window 3 is the scene `synth-6x64`"""
    return [_synth(21, 6, 64, 40, 32), _window(6, 64, [(0, 1)] * 9, [[(0, 0)]] * 9, 32, M=64), _synth(22, 6, 64, 64, 32), build_scene("synth-6x64")]


def test_a_window_alone_and_inside_a_ragged_batch_gives_the_same_bits_twice():
    batch = _ragged_batch()
    alone = twice("tracks_build", lambda: run_build([batch[3]], 2, 32))
    inside = twice("tracks_build, batch", lambda: run_build(batch, 2, 32))
    for a, b in zip(alone, inside):
        assert np.array_equal(a[0].view(np.uint8), b[3].view(np.uint8))
    for i, w in enumerate(batch):
        check_build(tuple(g[i] for g in inside), TO.build(w["keypoints"], w["pair_frames"], w["match_ij"], w["match_valid"], None, 2, 32), i)


def test_every_output_element_is_written_over_poison(monkeypatch):
    """torch.empty replaced by a poisoned allocation: outputs and workspace start as 0xA5 bytes, the results do not change"""
    w, want = build_scene("chain-conflict"), build_oracle("chain-conflict")
    tri = tri_scene("degenerate")
    clean = run_tri(tri)
    real = torch.empty

    def poisoned(*a, **kw):
        out = real(*a, **kw)
        out.view(torch.uint8).fill_(0xA5)
        return out
    monkeypatch.setattr(torch, "empty", poisoned)
    check_build(tuple(g[0] for g in run_build([w], w["min_views"], w["L"])), want, "poisoned")
    again = run_tri(tri)
    monkeypatch.undo()
    for a, b in zip(clean, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_both_entries_capture_into_a_graph_and_replay_to_the_eager_bits():
    w = build_scene("synth-6x64")
    a = gpu(w["keypoints"][None], w["pair_frames"][None], w["match_ij"][None], w["match_valid"][None])
    tri = tri_scene("tracks")
    b = gpu(tri["R"], tri["t"], tri["obs"], tri["vis"])
    eager = ops.tracks_build(*a, None, 2, w["L"]) + ops.tracks_triangulate(*b, TRI_MIN_VIEWS, MAX_E2, MAX_COS)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):        # one stream, two kernel nodes in a line, no forked branch
            captured = ops.tracks_build(*a, None, 2, w["L"]) + ops.tracks_triangulate(*b, TRI_MIN_VIEWS, MAX_E2, MAX_COS)
    for o in captured:
        o.view(torch.uint8).fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, eager)


# ---- triangulation --------------------------------------------------------------------------------------------------------------------
def _tracks_window(seed, landmarks=64, true_poses=False):
    """the oracle's tracks of a synth_track_window scene, normalised: (R, t, obs, vis) of one window"""
    kp, _, pf, ij, mv, R0, t0, R, t, _ = synth_track_window(seed, 6, 64, landmarks)
    o = TO.build(kp, pf, ij, mv, None, 2, 40)
    return (R.astype(F32), t.astype(F32)) if true_poses else (R0, t0), TO.normalise(o["track_keypoints"], CAMERA), o["vis"]


def _ba_window(seed, F, L):
    """track form directly: synth_ba_window with misses and 5 % gross observations, the perturbed poses"""
    R0, t0, _, kp, vis = synth_ba_window(seed, F, L, visibility=0.7, outlier_fraction=0.05, pose_noise=0.002)[:5]
    return (R0, t0), TO.normalise(kp, CAMERA), vis


def _degenerate():
    """slot 0: sound, five views.  1: identical poses and observations (parallel rays).  2: sound, three views.  3: one gross
    observation.  4: one view only.  5: nobody sees it.  6: two views half a degree apart (the parallax gate)."""
    F, L = 5, 7
    R, t = synth_ba_window(1, F, 4, noise_px=0.0)[5:7]
    R, t = R.astype(F32), t.astype(F32)
    X = np.array([0.3, -0.2, 5.0])
    obs = np.zeros((F, L, 2), F32)
    vis = np.zeros((F, L), bool)
    q = np.einsum("fij,j->fi", R.astype(F64), X) + t
    proj = (q[:, :2] / q[:, 2:]).astype(F32)
    for l in (0, 2, 3):
        obs[:, l], vis[:, l] = proj, True
    vis[[1, 3], 2] = False
    R, t = np.concatenate([R, R[:1]]), np.concatenate([t, t[:1]])          # frame 5 = frame 0 again
    obs, vis = np.concatenate([obs, obs[:1]]), np.concatenate([vis, np.zeros((1, L), bool)])
    obs[[0, 5], 1], vis[[0, 5], 1] = proj[0], True
    obs[4, 3] = proj[4] + 0.02                                                # gross: 10 px
    vis[2, 4], obs[2, 4] = True, proj[2]
    c = -(R[1].astype(F64).T @ t[1])
    Xfar = c + np.array([0.0, 0.0, 1.0]) * 0.15 / np.tan(np.radians(0.5))      # 17 m ahead of a 0.15 m baseline
    for f in (0, 1):
        qf = R[f].astype(F64) @ Xfar + t[f]
        obs[f, 6], vis[f, 6] = (qf[:2] / qf[2]).astype(F32), True
    return (R, t), obs, vis


def _behind():
    """X = (0.5, 0, 2) seen by camera 0 at the origin; camera 1 stands 5 m further along z, so the point is 3 m BEHIND it, and
    its "observation" is the pixel whose line (not ray) passes through X: the lines meet at X exactly"""
    R = np.stack([np.eye(3), np.eye(3)]).astype(F32)
    t = np.array([[0, 0, 0], [0, 0, -5.0]], F32)
    obs = np.zeros((2, 1, 2), F32)
    obs[0, 0], obs[1, 0] = (0.25, 0.0), (0.5 / -3.0, 0.0)
    return (R, t), obs, np.ones((2, 1), bool)


TRI_SCENES = {
    "tracks": lambda: [_tracks_window(s) for s in (1, 2, 3)],
    "tracks-true-poses": lambda: [_tracks_window(s, true_poses=True) for s in (4, 5)],
    "ba-5x130": lambda: [_ba_window(s, 5, 130) for s in (1, 2, 3)],                  # one landmark block and two landmarks
    "ba-16x70": lambda: [_ba_window(s, 16, 70) for s in (4, 5)],
    "degenerate": lambda: [_degenerate()],
    "behind": lambda: [_behind()],
}
TRI_NAMES = list(TRI_SCENES)
TRI_MIN_VIEWS = 2


@functools.lru_cache(maxsize=None)
def tri_scene(name):
    ws = TRI_SCENES[name]()
    return dict(R=np.stack([w[0][0] for w in ws]), t=np.stack([w[0][1] for w in ws]), obs=np.stack([w[1] for w in ws]),
                vis=np.stack([w[2] for w in ws]))


@functools.lru_cache(maxsize=None)
def tri_oracle(name):
    w = tri_scene(name)
    return [TO.triangulate(w["R"][i], w["t"][i], w["obs"][i], w["vis"][i], TRI_MIN_VIEWS, MAX_E2, MAX_COS) for i in range(len(w["R"]))]


def run_tri(w):
    out = ops.tracks_triangulate(*gpu(w["R"], w["t"], w["obs"], w["vis"]), TRI_MIN_VIEWS, MAX_E2, MAX_COS)
    return tuple(o.cpu().numpy() for o in out)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, F64)).astype(F32)).astype(F64)


def tri_tolerances(want):
    """per landmark: the bound on |points - X| (L, 3), on |e2max - e2max'| and on |cos_par - cos_par'|"""
    X = want["points"]
    with np.errstate(invalid="ignore"):
        e2 = np.where(np.isfinite(want["e2max"]), want["e2max"], 0.0)
    return (TRI_TOL * np.maximum(np.abs(X).max(-1, keepdims=True), 1.0) + ulp32(X), TRI_TOL * MAX_E2 + ulp32(e2), TRI_TOL + ulp32(want["cos_par"]))


def excused(want):
    """landmarks whose e2max or cos_par lies within the tolerance of its threshold: their point_ok may differ"""
    _, te, tc = tri_tolerances(want)
    with np.errstate(invalid="ignore"):
        return (np.abs(want["e2max"] - MAX_E2) <= te) | (np.abs(want["cos_par"] - MAX_COS) <= tc)


def check_tri(got, want, where):
    points, ok, vis_out, e2max, cos_par = got
    tx, te, tc = tri_tolerances(want)
    assert (np.abs(points.astype(F64) - want["points"]) <= tx).all(), (where, np.abs(points - want["points"]).max())
    fin = np.isfinite(want["e2max"])
    assert np.array_equal(np.isinf(e2max), ~fin) and (np.abs(e2max[fin].astype(F64) - want["e2max"][fin]) <= te[fin]).all(), where
    assert (np.abs(cos_par.astype(F64) - want["cos_par"]) <= tc).all(), where
    ex = excused(want)
    assert ex.sum() <= 0.01 * len(ex), (where, int(ex.sum()))
    assert np.array_equal(ok[~ex], want["point_ok"][~ex]), (where, np.flatnonzero(ok != want["point_ok"]))
    assert np.array_equal(vis_out[:, ~ex], want["vis_out"][:, ~ex]), where


@pytest.mark.parametrize("name", TRI_NAMES)
def test_triangulation_matches_the_oracle(name):
    w, want = tri_scene(name), tri_oracle(name)
    got = twice("tracks_triangulate", lambda: run_tri(w))
    for i, o in enumerate(want):
        print(f"{name}[{i}]: {int(o['point_ok'].sum())} of {len(o['point_ok'])} ok, worst |dX| {np.abs(got[0][i] - o['points']).max():.2e}")
        check_tri(tuple(g[i] for g in got), o, (name, i))
        assert np.array_equal(got[2][i], w["vis"][i] & got[1][i][None])


def test_degenerate_landmarks_fail_and_lose_their_columns():
    got = run_tri(tri_scene("degenerate"))
    points, ok, vis_out, e2max, cos_par = (g[0] for g in got)
    assert ok.tolist() == [True, False, True, False, False, False, False], ok
    assert not vis_out[:, [1, 3, 4, 5, 6]].any() and vis_out[:5, 0].all() and vis_out[:, 2].sum() == 3
    assert not points[1].any() and np.isinf(e2max[1]) and cos_par[1] == 1.0            # parallel rays: the solve is unusable
    assert e2max[3] > MAX_E2 and np.isfinite(e2max[3])                                     # one gross observation
    assert not points[4].any() and cos_par[4] == 1.0 and not points[5].any()               # one view, no view
    assert cos_par[6] > MAX_COS and e2max[6] <= MAX_E2                                     # sound but for the parallax
    o = tri_oracle("degenerate")[0]
    assert not o["usable"][1] and o["seen"].tolist() == [5, 2, 3, 5, 1, 0, 2]
    points, ok, vis_out, e2max, _ = (g[0] for g in run_tri(tri_scene("behind")))
    o = tri_oracle("behind")[0]
    assert o["usable"][0] and not o["front"][0] and not ok[0] and not vis_out.any() and np.isinf(e2max[0]) and abs(points[0, 2] - 2.0) < 1e-5


def test_a_window_alone_and_inside_a_batch_triangulates_to_the_same_bits():
    w = tri_scene("ba-5x130")
    one = {k: v[2:3] for k, v in w.items()}
    alone, inside = run_tri(one), run_tri(w)
    assert all(np.array_equal(a[0].view(np.uint8), b[2].view(np.uint8)) for a, b in zip(alone, inside))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def purity(kp_id, eligible):
    """per eligible track: all its keypoints carry one planted landmark"""
    flat = kp_id.reshape(-1)
    return np.array([len({int(flat[n]) for n in nodes}) == 1 and flat[nodes[0]] >= 0 for _, nodes in eligible], bool)


def e2e_window():
    return synth_track_window(E2E_SEED, 6, 64, E2E_LANDMARKS)


def e2e_start(w):
    """the perturbed poses with frames 0 and 1 at the truth: two held frames pin the scale of a monocular window"""
    R0, t0 = w[5].copy(), w[6].copy()
    R0[:2], t0[:2] = w[7][:2].astype(F32), w[8][:2].astype(F32)
    return R0, t0


def pose_error(R, t, Rt, tt):
    """largest rotation (degrees) and camera-centre (metres) distance from the truth"""
    R, t = np.asarray(R, F64), np.asarray(t, F64)
    dR = np.einsum("fij,fkj->fik", R, Rt)
    ang = np.degrees(np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1) / 2, -1, 1)))
    c, ct = -np.einsum("fji,fj->fi", R, t), -np.einsum("fji,fj->fi", Rt, tt)
    return float(ang.max()), float(np.linalg.norm(c - ct, axis=1).max())


def test_matches_to_bundle_adjustment_end_to_end():
    w = e2e_window()
    kp, kp_id, pf, ij, mv = w[:5]
    R0, t0 = e2e_start(w)
    Kt = torch.from_numpy(CAMERA).float()
    tracks = LandmarkTracks(Kt, max_landmarks=64, max_reproj_px=MAX_PX, min_parallax_deg=MIN_PARALLAX_DEG).to(DEV)
    adjust = BundleAdjuster(Kt, num_fixed=2).to(DEV)
    points, tkp, vis, point_ok, track_kp, kp_track, counts = tracks(*gpu(kp, pf, ij, mv, R0, t0))
    want = TO.build(kp, pf, ij, mv, None, 2, 64)
    assert np.array_equal(track_kp.cpu().numpy(), want["track_kp"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
    pure = purity(kp_id, want["eligible"])
    ok = point_ok.cpu().numpy()[:len(pure)]
    print(f"counts {want['counts'].tolist()}, pure {int(pure.sum())}, point_ok {int(ok.sum())}, pure among ok {(ok & pure).sum() / ok.sum():.3f}, "
          f"ok among pure {(ok & pure).sum() / pure.sum():.3f}")
    assert (ok & pure).sum() >= 0.95 * ok.sum() and (ok & pure).sum() >= 0.90 * pure.sum() and ok.sum() >= 10
    assert not point_ok.cpu().numpy()[len(pure):].any()
    R_o, t_o, _, _, _, cost0, cost, _, ba_ok = adjust(*gpu(R0, t0), points, tkp, vis)
    print(f"cost {float(cost0):.2f} -> {float(cost):.2f} px^2")
    assert bool(ba_ok) and float(cost) < float(cost0)
    # the same adjuster fed the TRUE tracks of the same scene (synth_ba_window's observations, its perturbed points)
    _, _, X0, kp_l, visible = synth_ba_window(E2E_SEED, 6, E2E_LANDMARKS, 0.9, 0.5, pose_noise=0.002)[:5]
    R_t, t_t, _, _, _, _, _, _, ok_t = adjust(*gpu(R0, t0, X0, kp_l, visible))
    e0, e1, e2 = pose_error(R0, t0, w[7], w[8]), pose_error(R_o.cpu().numpy(), t_o.cpu().numpy(), w[7], w[8]), \
        pose_error(R_t.cpu().numpy(), t_t.cpu().numpy(), w[7], w[8])
    print(f"pose error, degrees / metres: start {e0[0]:.4f} / {e0[1]:.4f}, LandmarkTracks -> BundleAdjuster {e1[0]:.4f} / {e1[1]:.4f}, "
          f"BundleAdjuster on the true tracks {e2[0]:.4f} / {e2[1]:.4f}")
    assert bool(ok_t)
