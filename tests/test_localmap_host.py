"""K29 local-map tracking without a GPU: the numpy oracle's loops against its vectorised twin on random tiny windows and its
medoid against a brute force over sorted lists; the arithmetic of the kernels (csrc/localmap_math.h) compiled for the host in
tests/native/localmap_host.cpp -- by hipcc, as plain C++, and once more under the host sanitizers as that stand-alone program --
against the oracle, bit for bit; the conditions on the scenes of tests/test_gpu_localmap.py (no excused landmark, the states,
an equal-distance claim, the precision); the host-side argument checks of the entries (MI_E_* before any launch); the header of
its own, the binding and the library's export list; the Python module's constructor, its refusal of CPU tensors and the alias
import; the generator's contract.

Measured deviation of the host-compiled localmap_math.h from the oracle: 0 on every integer output and every proj of every scene
(the same IEEE float64 operations in the same order under -ffp-contract=off), asserted as equality.

Scene statistics on the committed generator (6 frames x 64 keypoints x 48 landmarks, 256 bits, pose 2 degrees / 5 cm off, seeds
1 .. 3; counts per state 0 .. 4):
  no twins, 40 px, ratio 0.8:       [1, 0, 2, 0, 45]  [0, 1, 4, 0, 43]  [6, 1, 3, 0, 38]   kept = correct: 45, 43, 38
  twins 0.25, 40 px, ratio 0.8:     [1, 0, 3, 0, 44]  [0, 1, 4, 0, 43]  [6, 1, 6, 0, 35]   kept = correct: 44, 43, 35
  twins 0.25, 150 px, ratio 1.0:    [1, 0, 3, 7, 38]  [0, 0, 5, 3, 41]  [6, 0, 4, 5, 34]   correct 34, 37, 31 (with the hand-added copy)
The crowded setting never holds a landmark in state 1: a 150 px window in a 480 x 640 image with 64 keypoints holds 22 to 27 of
them on average, and no seed from 1 to 79 gives an empty one.  What is asserted is therefore: the crowded setting shows the
states 0, 2, 3 and 4 on these seeds, state 1 occurs at 40 px with the same twins on the same seeds, and the hand-made window
`radius-out` is state 1 by construction."""
import ctypes

import numpy as np
import pytest
import torch

import localmap_oracle as LO
import test_gpu_localmap as G
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import synth_localmap_window, synth_track_window

NULL, SHAPE, PARAM = -1, -2, -3
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return N.load()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


# ---- the oracle against itself ----------------------------------------------------------------------------------------------------
def _tiny_window(rng, trial):
    L, K, nb = int(rng.integers(1, 13)), int(rng.integers(1, 13)), (256, 512)[trial % 2]
    c = dict(G.random_case(int(rng.integers(1 << 30)), L, K, nb, radius=float(rng.choice([40.0, 150.0, 600.0])), ratio=float(rng.choice([0.8, 1.0])),
                           near=0.8))
    if trial % 3 == 0:
        c["point_valid"] = None
    if trial % 4 == 0:
        c["kp_valid"] = None
    if trial % 5 == 0:                                        # a few identical keypoint descriptors: Hamming ties
        c["kp_bits"] = np.repeat(c["kp_bits"][:1], K, 0)
    return c


def test_oracle_loops_equal_the_vectorised_twin_on_tiny_windows():
    rng = np.random.default_rng(0)
    seen = np.zeros(5, np.int64)
    for trial in range(160):
        c = _tiny_window(rng, trial)
        a, b = LO.match(*G.oracle_args(c)), LO.match_vectorised(*G.oracle_args(c))
        assert LO.same(a, b), (trial, {k: (a[k], b[k]) for k in a if not np.array_equal(a[k], b[k])})
        seen += a["counts"]
    assert (seen > 20).all(), seen                            # the tiny windows reach every state
    for name in G.MATCH_NAMES:
        if name != "caps":
            c = G.match_scene(name)
            assert LO.same(LO.match(*G.oracle_args(c)), LO.match_vectorised(*G.oracle_args(c))), name


def test_oracle_medoid_against_brute_force_over_sorted_lists():
    rng = np.random.default_rng(1)
    for trial in range(120):
        F, K, L, nb = int(rng.integers(1, 17)), int(rng.integers(1, 9)), int(rng.integers(1, 9)), (256, 512)[trial % 2]
        s = G._desc_random(int(rng.integers(1 << 30)), F, K, L, nb)
        o = LO.descriptors(s["bits"], s["track_kp"], nb)
        bits = LO.words(s["bits"])
        for l in range(L):
            views = [f for f in range(F) if 0 <= s["track_kp"][f, l] < K]
            if not views:
                assert o["rep_frame"][l] == -1 and o["rep_median"][l] == nb + 1 and not o["rep_bits"][l].any()
                continue
            desc = {f: np.unpackbits(bits[f, s["track_kp"][f, l]].view(np.uint8)) for f in views}
            med = {a: sorted(int((desc[a] != desc[b]).sum()) for b in views)[(len(views) - 1) // 2] for a in views}
            want = min(views, key=lambda a: (med[a], a))
            assert (o["rep_frame"][l], o["rep_median"][l]) == (want, med[want]) and np.array_equal(o["rep_bits"][l], bits[want, s["track_kp"][want, l]])


# ---- the arithmetic on the host -----------------------------------------------------------------------------------------------------
localmap_host = host_program("localmap_host.cpp", hip=True)
localmap_plain = host_program("localmap_host.cpp", hip=False)
HOST_MATCH = [n for n in G.MATCH_NAMES if n != "caps"]


def _match_text(names):
    lines = []
    for name in names:
        c = G.match_scene(name)
        L, K, W = len(c["points"]), len(c["kp"]), c["num_bits"] // 32
        lines.append(f"{L} {K} {W} {c['height']} {c['width']} {c['min_depth']:.9g} {c['max_depth']:.9g} {c['radius']:.9g} {c['max_distance']} {c['ratio']:.9g}")
        lines.append(" ".join("%.9g" % x for x in np.concatenate([c["R"].ravel(), c["t"], c["cam"]])))
        rep, kb = LO.words(c["rep_bits"]), LO.words(c["kp_bits"])
        for l in range(L):
            lines.append(f"{1 if c['point_valid'] is None else int(c['point_valid'][l])} " + " ".join("%.9g" % x for x in c["points"][l]) + " "
                         + " ".join(str(int(x)) for x in rep[l]))
        for j in range(K):
            lines.append(f"{1 if c['kp_valid'] is None else int(c['kp_valid'][j])} {c['kp'][j, 0]:.9g} {c['kp'][j, 1]:.9g} " + " ".join(str(int(x)) for x in kb[j]))
    return "\n".join(lines) + "\n"


def _match_deviation(raw, names):
    """the number of output elements of the host program that differ from the oracle's, over `names`"""
    at = differing = 0
    for name in names:
        o = G.match_oracle(name)
        L = len(o["lm_state"])
        rows = np.array([[int(v) for v in ln] for ln in raw[at:at + L]], np.int64)
        kp_lm, counts = np.array(raw[at + L], np.int64), np.array(raw[at + L + 1], np.int64)
        at += L + 2
        want = np.column_stack([o["lm_state"], o["lm_kp"], o["lm_distance"], o["d2"], o["proj"].view(np.uint32), o["match_keypoints"].view(np.uint32)])
        differing += int((rows != want).sum() + (kp_lm != o["kp_lm"]).sum() + (counts != o["counts"]).sum())
    assert at == len(raw)
    return differing


def _desc_text(names):
    lines = []
    for name in names:
        s = G.desc_scene(name)
        F, K, W = s["bits"].shape
        lines.append(f"{F} {K} {s['track_kp'].shape[1]} {W}")
        lines += [" ".join(str(int(x)) for x in row) for row in LO.words(s["bits"]).reshape(F * K, W)]
        lines += [" ".join(str(int(x)) for x in row) for row in s["track_kp"]]
    return "\n".join(lines) + "\n"


def _desc_deviation(raw, names):
    at = differing = 0
    for name in names:
        o = G.desc_oracle(name)
        L = len(o["rep_frame"])
        rows = np.array([[int(v) for v in ln] for ln in raw[at:at + L]], np.int64)
        at += L
        differing += int((rows != np.column_stack([o["rep_frame"], o["rep_median"], o["rep_bits"]])).sum())
    assert at == len(raw)
    return differing


def test_native_arithmetic_equals_the_oracle_bit_for_bit(localmap_host, localmap_plain):
    text = _match_text(HOST_MATCH)
    raw = run_host(localmap_host, "match", text)
    assert raw == run_host(localmap_plain, "match", text)        # the plain C++ build returns the hipcc build's bits
    m = _match_deviation(raw, HOST_MATCH)
    text = _desc_text(G.DESC_NAMES)
    raw = run_host(localmap_host, "desc", text)
    assert raw == run_host(localmap_plain, "desc", text)
    d = _desc_deviation(raw, G.DESC_NAMES)
    print(f"host localmap_math.h vs the oracle: {m} differing match outputs (proj bit patterns included), {d} differing descriptor outputs")
    assert m == 0 and d == 0


def test_native_harness_under_the_host_sanitizers(tmp_path):
    """the same stand-alone program built with the host's address and undefined-behaviour sanitizers, run once per mode"""
    exe = build_host(tmp_path, "localmap_host.cpp", hip=True, extra=SANITIZE)
    names = ["17x37", "64x65", "gates", "border-out", "claims", "synth-crowded-1"]
    assert _match_deviation(run_host(exe, "match", _match_text(names)), names) == 0
    names = ["hand", "16x70x70-512", "1x5x5"]
    assert _desc_deviation(run_host(exe, "desc", _desc_text(names)), names) == 0


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def test_no_generated_scene_holds_an_excused_landmark():
    """a condition, not a measurement: 0 landmarks whose gate is decided by less than 1e-9 relative, on every generated scene of
    tests/test_gpu_localmap.py and tests/test_gpu_localmap_perf.py; the hand-made boundary cases are exactly representable"""
    for name in G.GENERATED:
        assert G.match_oracle(name)["excused"].sum() == 0, name
    for c in G._ragged_batch():
        assert LO.match(*G.oracle_args(c))["excused"].sum() == 0
    import test_gpu_localmap_perf as P
    for c in P.small_batch():
        assert LO.match_vectorised(*G.oracle_args(c))["excused"].sum() == 0
    for c in P.distinct_cases():
        assert LO.match_vectorised(*G.oracle_args(c))["excused"].sum() == 0


def test_scene_statistics_on_the_fixed_seeds():
    """the counts in this file's docstring"""
    counts = {s: np.array([G.match_oracle(f"synth-{s}-{seed}")["counts"] for seed in G.SYNTH_SEEDS]) for s in G.SETTINGS}
    print({s: c.tolist() for s, c in counts.items()})
    assert counts["easy"].tolist() == [[1, 0, 2, 0, 45], [0, 1, 4, 0, 43], [6, 1, 3, 0, 38]]
    assert counts["twins"].tolist() == [[1, 0, 3, 0, 44], [0, 1, 4, 0, 43], [6, 1, 6, 0, 35]]
    crowded = counts["crowded"].sum(0)
    assert (crowded[[0, 2, 3, 4]] > 0).all() and (counts["crowded"][:, 2:] > 0).all()      # every seed: states 2, 3 and 4
    assert crowded[1] == 0 and counts["twins"][:, 1].sum() > 0                             # state 1: at 40 px only (docstring)
    assert G.match_oracle("radius-out")["lm_state"].tolist() == [1]
    every = counts["crowded"].sum(0) + counts["twins"].sum(0)
    assert (every > 0).all()
    # a claim decided by the lower landmark index at equal distance: the hand-added copy, number 48, in every crowded scene
    for seed in G.SYNTH_SEEDS:
        c, o = G.synth_case(seed, "crowded"), G.match_oracle(f"synth-crowded-{seed}")
        assert len(c["points"]) == 49 and o["lm_state"][48] == 3
        first = G.crowded_original(seed)
        assert o["lm_state"][first] == 4 and o["kp_lm"][o["lm_kp"][first]] == first and o["lm_distance"][first] == o["lm_distance"][48]
        assert np.array_equal(c["points"][first], c["points"][48]) and np.array_equal(c["rep_bits"][first], c["rep_bits"][48])
    # precision at 40 px, ratio 0.8: the oracle's own figure on these seeds is 1.0 with and without twins
    for s in ("easy", "twins"):
        for seed in G.SYNTH_SEEDS:
            o = G.match_oracle(f"synth-{s}-{seed}")
            kept, correct = int((o["lm_state"] == 4).sum()), int(G.planted_correct(seed, s, o).sum())
            assert kept >= 35 and correct / kept >= 1.0, (s, seed, kept, correct)
    correct = [int(G.planted_correct(seed, "crowded", G.match_oracle(f"synth-crowded-{seed}")).sum()) for seed in G.SYNTH_SEEDS]
    assert correct == [34, 37, 31]


def test_hand_made_scenes_show_what_they_are_for():
    st = lambda name: G.match_oracle(name)["lm_state"].tolist()
    assert st("gates") == [4, 0, 0, 0, 0, 0, 0] and st("border-in") == [4] and st("border-out") == [0]
    assert st("radius-in") == [4] and st("radius-out") == [1] and st("tie") == [2] and st("single") == [4] and st("nearest-invalid") == [4]
    o = G.match_oracle("tie")
    assert o["lm_distance"].tolist() == [7] and o["d2"].tolist() == [7] and o["in_window"].tolist() == [3]
    assert G.match_oracle("single")["d2"].tolist() == [257] and G.match_oracle("nearest-invalid")["lm_kp"].tolist() == [1]
    o = G.match_oracle("claims")
    assert o["lm_state"].tolist() == [3, 4, 4, 3, 4] and o["kp_lm"].tolist() == [1, -1, 2, 4] and o["lm_distance"].tolist() == [10, 4, 6, 6, 3]
    alone = LO.match(*G.oracle_args({**G.match_scene("claims"), "point_valid": np.arange(5) == 0}))      # the loser, without its rival
    assert alone["lm_state"][0] == 4 and alone["lm_kp"][0] == 0
    second = LO.match(*G.oracle_args({**G.match_scene("claims"), "point_valid": np.arange(5) == 0, "kp_valid": np.arange(4) != 0}))
    assert second["lm_state"][0] == 4 and second["lm_kp"][0] == 1                                      # its second choice would qualify
    o = G.match_oracle("caps")
    assert len(o["lm_state"]) == 2048 and len(o["kp_lm"]) == 1024 and (o["counts"][[0, 2, 3, 4]] > 0).all()
    c = G.match_oracle("130x200-crowded")["counts"]
    assert c[3] > 0 and c[4] > 0
    o = G.desc_oracle("hand")
    assert o["rep_frame"].tolist() == [-1, 5, 3, 7, 4, 3] and o["rep_median"].tolist() == [257, 0, 0, 5, 2, 12]


def test_end_to_end_scene_gives_the_oracle_room():
    """the GPU end-to-end test's chain on the oracles: tracks of frames 0 .. 4, their triangulation, the medoid descriptors, the
    last frame matched under the predicted pose: enough kept matches for a pose, nearly all on the planted keypoint"""
    import tracks_oracle as TO
    w, m = G.e2e_inputs()
    o = TO.build(m["kp"], m["pf"], m["ij"], m["mv"], None, 2, 64)
    focal = float((G.CAMERA[0, 0] + G.CAMERA[1, 1]) / 2)
    tri = TO.triangulate(m["R0"], m["t0"], TO.normalise(o["track_keypoints"], G.CAMERA), o["vis"], 2, float(F32((3.0 / focal) ** 2)),
                         float(F32(np.cos(np.radians(1.0)))))
    rep = LO.descriptors(m["bits"], o["track_kp"], 256)["rep_bits"]
    got = LO.match(tri["points"].astype(F32), tri["point_ok"], rep, w[11], w[12], G.CAM4, w[0][5], None, w[10][5], 256, G.HEIGHT, G.WIDTH, 0.1, 100.0,
                   40.0, 64, 0.8)
    kept = np.flatnonzero(got["lm_state"] == 4)
    first = {s: int(np.argmax(o["track_kp"][:, s] >= 0)) for s in kept}                   # the planted landmark of a slot's first view
    ids = np.array([w[1][first[s], o["track_kp"][first[s], s]] for s in kept])
    correct = int((w[1][5][got["lm_kp"][kept]] == ids).sum())
    print(f"point_ok {int(tri['point_ok'].sum())}, counts {got['counts'].tolist()}, kept {len(kept)}, on the planted keypoint {correct}")
    assert len(kept) >= 12 and correct >= 0.9 * len(kept) and got["excused"].sum() == 0


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_descriptors_argument_checks(lib, p):
    f = lib.mi_localmap_descriptors
    for i in (0, 1, 7, 8, 9):
        a = [p, p, 3, 5, 64, 40, 256, p, p, p, None]
        a[i] = None
        assert f(*a) == NULL, i

    def call(batch=3, fr=5, k=64, l=40, nb=256):
        return f(p, p, batch, fr, k, l, nb, p, p, p, None)
    assert call(batch=0) == SHAPE and call(fr=0) == SHAPE and call(k=0) == SHAPE and call(l=0) == SHAPE and call(l=-1) == SHAPE
    assert call(batch=65536) == PARAM and call(fr=17) == PARAM and call(k=1025) == PARAM and call(l=2049) == PARAM
    assert call(nb=128) == PARAM and call(nb=0) == PARAM and call(nb=257) == PARAM and call(nb=1024) == PARAM
    assert call(fr=17, l=0) == SHAPE and call(nb=128, k=0) == SHAPE                      # shape, then parameters


def test_match_argument_checks(lib, p):
    f = lib.mi_localmap_match
    base = [p] * 9 + [3, 48, 64, 256, 480, 640, 0.1, 100.0, 40.0, 64, 0.8] + [p] * 7 + [None]
    for i in (0, 2, 3, 4, 5, 6, 8, 20, 21, 22, 23, 24, 25, 26):
        a = list(base)
        a[i] = None
        assert f(*a) == NULL, i
    a = list(base)
    a[1] = a[7] = None                                                                   # point_valid and kp_valid are optional
    a[9] = 0
    assert f(*a) == SHAPE

    def call(batch=3, l=48, k=64, nb=256, h=480, w=640, lo=0.1, hi=100.0, rad=40.0, md=64, ratio=0.8):
        return f(*[p] * 9, batch, l, k, nb, h, w, lo, hi, rad, md, ratio, *[p] * 7, None)
    assert call(batch=0) == SHAPE and call(l=0) == SHAPE and call(k=0) == SHAPE and call(k=-5) == SHAPE
    assert call(batch=65536) == PARAM and call(l=2049) == PARAM and call(k=1025) == PARAM
    assert call(nb=128) == PARAM and call(nb=384) == PARAM
    assert call(lo=0.0) == PARAM and call(lo=-1.0) == PARAM and call(lo=NAN) == PARAM and call(lo=100.0) == PARAM and call(lo=200.0) == PARAM
    assert call(hi=INF) == PARAM and call(hi=NAN) == PARAM and call(lo=INF) == PARAM
    assert call(rad=0.0) == PARAM and call(rad=-1.0) == PARAM and call(rad=INF) == PARAM and call(rad=NAN) == PARAM
    assert call(md=-1) == PARAM and call(md=257) == PARAM and call(nb=512, md=513) == PARAM
    assert call(ratio=0.0) == PARAM and call(ratio=1.0000001) == PARAM and call(ratio=NAN) == PARAM and call(ratio=-0.5) == PARAM
    assert call(h=0) == PARAM and call(w=0) == PARAM and call(w=-640) == PARAM
    assert call(k=0, ratio=NAN) == SHAPE and call(l=2049, rad=NAN) == PARAM
    assert N.load().mi_abi_version() == 3


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_module_constructor_and_cpu_refusal():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import AbsolutePoseEstimator, LocalMapTracker
    assert (ops.LOCALMAP_MAX_LANDMARKS, ops.LOCALMAP_MAX_KEYPOINTS, ops.LOCALMAP_MAX_FRAMES) == (2048, 1024, 16)
    K = torch.from_numpy(G.CAMERA).float()
    m = LocalMapTracker(K, (480, 640))
    assert (m.height, m.width, m.num_bits, m.radius_px, m.refine_radius_px, m.max_distance, m.ratio, m.min_depth, m.max_depth) == \
        (480, 640, 256, 40.0, 10.0, 64, 0.8, 0.1, 100.0)
    assert LocalMapTracker(K, (480, 640), num_bits=512).max_distance == 128 and LocalMapTracker(K, (480, 640), max_distance=0).max_distance == 0
    assert m.cam.tolist() == [float(G.CAMERA[0, 0]), float(G.CAMERA[1, 1]), float(G.CAMERA[0, 2]), float(G.CAMERA[1, 2])]
    for kw in (dict(num_bits=128), dict(radius_px=0.0), dict(radius_px=NAN), dict(refine_radius_px=INF), dict(max_distance=-1), dict(max_distance=257),
               dict(ratio=0.0), dict(ratio=1.5), dict(min_depth=0.0), dict(min_depth=200.0), dict(max_depth=INF), dict(max_depth=NAN)):
        with pytest.raises(ValueError):
            LocalMapTracker(K, (480, 640), **kw)
    for size in ((0, 640), (480,), 480, (480, -1)):
        with pytest.raises(ValueError):
            LocalMapTracker(K, size)
    with pytest.raises(ValueError):
        LocalMapTracker(torch.eye(4), (480, 640))
    c = G.synth_case(1, "easy")
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("points", "rep_bits", "R", "t", "kp", "kp_bits", "point_valid")}
    args = (t["points"], t["rep_bits"], t["R"], t["t"], t["kp"], t["kp_bits"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.match(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.match(*(x[None] for x in args), t["point_valid"][None])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(*args, AbsolutePoseEstimator(K))
    w = G.synth_window(1, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.describe(torch.from_numpy(w[10][:5].copy()), torch.from_numpy(G.planted_map(w)[3]))
    with pytest.raises(RuntimeError, match=r"bits must be \(B, F, K, 8\)"):
        m.describe(torch.zeros(5, 64, 16, dtype=torch.int32), torch.zeros(5, 48, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"points must be \(B, L, 3\) or \(L, 3\)"):
        m.match(t["points"][:, :2], *args[1:])
    with pytest.raises(RuntimeError, match="descriptors must have 8 words"):
        m.match(t["points"], torch.zeros(48, 16, dtype=torch.int32), *args[2:])
    b = [x[None] for x in args]
    cam = torch.from_numpy(G.CAM4)[None]
    ok = (b[0], None, b[1], b[2], b[3], cam, b[4], None, b[5], 480, 640, 0.1, 100.0, 40.0, 64, 0.8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.localmap_match(*ok)
    with pytest.raises(RuntimeError, match="points must be"):
        ops.localmap_match(args[0], *ok[1:])
    with pytest.raises(RuntimeError, match="expected rep_bits"):
        ops.localmap_match(*ok[:5], cam[:, :3], *ok[6:])
    with pytest.raises(RuntimeError, match="256 and 512"):
        ops.localmap_match(*ok[:2], b[1][..., :4], *ok[3:])
    with pytest.raises(RuntimeError, match="0 < ratio <= 1"):
        ops.localmap_match(*ok[:-1], 1.5)
    with pytest.raises(RuntimeError, match="0 < ratio <= 1"):
        ops.localmap_match(*ok[:-3], 0.0, 64, 0.8)
    with pytest.raises(RuntimeError, match="packed descriptors"):
        ops.localmap_descriptors(torch.zeros(1, 5, 64, 8), torch.zeros(1, 5, 48, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="expected track_kp"):
        ops.localmap_descriptors(torch.zeros(1, 5, 64, 8, dtype=torch.int32), torch.zeros(1, 4, 48, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="supported: 1 .. 16"):
        ops.localmap_descriptors(torch.zeros(1, 17, 64, 8, dtype=torch.int32), torch.zeros(1, 17, 48, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.localmap_descriptors(torch.zeros(1, 5, 64, 8, dtype=torch.int32), torch.zeros(1, 5, 48, dtype=torch.int32))


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.geometry as real
    from pytorch_model.geometry import LocalMapTracker
    assert LocalMapTracker is real.LocalMapTracker and "LocalMapTracker" in real.__all__
    from pytorch_model.geometry.local_map import LocalMapTracker as again
    assert again is LocalMapTracker


# ---- the generator --------------------------------------------------------------------------------------------------------------------
def test_generator_contract():
    g = synth_localmap_window(3, 6, 64, 48, 256)
    assert len(g) == 14 and all(np.array_equal(x, y) for x, y in zip(g[:10], synth_track_window(3, 6, 64, 48)))
    kp_id, bits, R_pred, t_pred, twin_of = g[1], g[10], g[11], g[12], g[13]
    assert bits.shape == (6, 64, 8) and bits.dtype == np.int32 and R_pred.shape == (3, 3) and R_pred.dtype == F32 and t_pred.shape == (3,) and t_pred.dtype == F32
    assert twin_of.shape == (48,) and twin_of.dtype == np.int32 and (twin_of >= 0).sum() == 12 and twin_of[0] == -1 and (twin_of < np.arange(48)).all()
    again = synth_localmap_window(3, 6, 64, 48, 256)
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(g, again))
    # the predicted pose is the stated motion away from the truth
    dR = R_pred.astype(F64) @ g[7][-1].T
    assert abs(np.degrees(np.arccos((np.trace(dR) - 1) / 2)) - 2.0) < 1e-3
    assert abs(np.linalg.norm(t_pred - dR @ g[8][-1]) - 0.05) < 1e-5
    # observations: about a tenth of the bits away from the landmark's base; twins really share a base; clutter is independent
    ub = np.unpackbits(LO.words(bits).view(np.uint8), axis=-1)
    obs = {l: ub[kp_id == l] for l in range(48)}
    for l in range(48):
        d = [(a != b).sum() for i, a in enumerate(obs[l]) for b in obs[l][i + 1:]]
        assert not d or 20 <= np.mean(d) <= 75, (l, d)                         # 2 * 0.1 * 0.9 * 256 = 46 expected between two observations
    for l in np.flatnonzero(twin_of >= 0):
        d = [(a != b).sum() for a in obs[l] for b in obs[int(twin_of[l])]]
        assert d and max(d) <= 80, (l, d)
    plain = [l for l in range(1, 48) if twin_of[l] < 0 and not (twin_of == l).any()]
    d = [(a != b).sum() for a in obs[plain[0]] for b in obs[plain[1]]]
    assert min(d) >= 90                                                        # different bases: 128 expected
    clutter = ub[kp_id < 0]
    assert 110 <= np.mean([(clutter[0] != c).sum() for c in clutter[1:]]) <= 146
    none = synth_localmap_window(3, 6, 64, 48, 256, twins=0.0)
    assert (none[13] == -1).all() and not np.array_equal(none[10], bits)
    clean = synth_localmap_window(3, 6, 64, 48, 512, flip=0.0)
    assert clean[10].shape == (6, 64, 16)
    cb = LO.words(clean[10])
    for l in range(48):
        rows = cb[clean[1] == l]
        assert (rows == rows[0]).all()
    for bad in (dict(num_bits=100), dict(flip=1.5), dict(twins=-0.1), dict(landmarks=65)):
        with pytest.raises(ValueError):
            synth_localmap_window(**{**dict(seed=1, frames=6, keypoints=64, landmarks=48, num_bits=256), **bad})
