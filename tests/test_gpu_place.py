"""K26 loop-closure retrieval on the device: `mi_place_votes` with every output and `mi_place_select` against
tests/place_oracle.py -- exact integer equality everywhere, no tolerance exists -- at the parity shapes, the planted cases
(each decided by one rule of the header), `frame_index`, the selection's corner cases, `KeyframeDatabase`, the twelve scenes end
to end (detector, NMS, top-k, SparseBAD.forward_bits, add, query, match, HomographyEstimator) and determinism with a hipGraph
replay.  The definitions up to the first test are shared with tests/test_place_host.py, which asserts the end-to-end
conditions on the oracle without a GPU."""
import functools
import os

import numpy as np
import pytest
import torch

import place_oracle as PO
from gpu_common import DEV, GPU, gpu
from onnx_image_processing_amd.synth import synth_batch, synth_place_descriptors

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32 = np.float32

# (Q, N, Kq, Kd, bits)
PARITY_SHAPES = [(1, 1, 1, 2, 256), (2, 3, 64, 64, 256), (1, 37, 96, 130, 256), (1, 5, 129, 257, 512), (3, 130, 33, 31, 512),
                 (1, 2, 1024, 1024, 512)]

# the end-to-end scenes: synth_batch(300, 12, 120, 160, (3, 5), 6), block 3, NMS radius 3, border 7, K = 64, hard bits
SCENES = dict(first_seed=300, count=12, height=120, width=160, shift=(3, 5), noise=6, block=3, nms=3, border=7, k=64, ratio=0.8)
E2E_MIN_WINNER, E2E_MAX_RUNNER_UP, E2E_MIN_SHARE, E2E_INLIER_SHARE = 40, 20, 0.85, 0.85


def flip_bits(rng, row, count):
    """`row` (W,) uint32 with exactly `count` distinct bits flipped"""
    out = row.copy()
    for b in rng.choice(32 * len(row), size=count, replace=False):
        out[b // 32] ^= np.uint32(1) << np.uint32(b % 32)
    return out


@functools.lru_cache(maxsize=None)
def parity_case(q, n, kq, kd, bits):
    """(db_bits, db_valid, q_bits, q_valid): random descriptors, a third of the query rows replaced by a database row with a
    few bits flipped (so that votes occur), ragged validity masks; in the (2, 3, 64, 64) case keyframe 0 has no valid
    descriptor, keyframe 1 exactly one, and query 1 none."""
    rng = np.random.default_rng(1000 * q + 100 * n + kq + kd + bits)
    w = bits // 32
    db = rng.integers(0, 1 << 32, size=(n, kd, w), dtype=np.uint64).astype(np.uint32)
    qb = rng.integers(0, 1 << 32, size=(q, kq, w), dtype=np.uint64).astype(np.uint32)
    for a in range(q):
        for i in rng.choice(kq, size=(kq + 2) // 3, replace=False):
            qb[a, i] = flip_bits(rng, db[rng.integers(n), rng.integers(kd)], int(rng.integers(0, bits // 4 + 8)))
    dbv, qv = rng.random((n, kd)) < 0.8, rng.random((q, kq)) < 0.8
    if (q, n, kq, kd) == (2, 3, 64, 64):
        dbv[0] = False
        dbv[1] = False
        dbv[1, 37] = True
        qv[1] = False
    return db.view(np.int32), dbv, qb.view(np.int32), qv


@functools.lru_cache(maxsize=None)
def parity_reference(shape, max_distance, ratio):
    db, dbv, qb, qv = parity_case(*shape)
    return PO.place_votes(db, dbv, qb, qv, max_distance, ratio)


@functools.lru_cache(maxsize=None)
def planted(bits):
    """one keyframe of 140 descriptors (two column tiles) and one query frame of 8 rows; see test_planted_cases"""
    rng = np.random.default_rng(bits)
    w, md = bits // 32, bits // 4
    db = rng.integers(0, 1 << 32, size=(1, 140, w), dtype=np.uint64).astype(np.uint32)
    db[0, 133] = db[0, 5]                                   # duplicates in two tiles
    db[0, 9] = 0
    db[0, 11] = 0xFFFFFFFF
    qb = np.zeros((1, 8, w), np.uint32)
    qb[0, 0] = flip_bits(rng, db[0, 5], 3)                  # nearest twice: index 5, d2 == d1
    qb[0, 1] = db[0, 7]                                     # identical
    qb[0, 2] = 0                                            # all zero
    qb[0, 3] = 0xFFFFFFFF                                   # all one
    qb[0, 4] = flip_bits(rng, db[0, 20], md)                # d1 == max_distance
    qb[0, 5] = flip_bits(rng, db[0, 21], md + 1)            # d1 == max_distance + 1
    qb[0, 6] = flip_bits(rng, db[0, 30], 10)
    qb[0, 7] = flip_bits(rng, db[0, 50], md + 20)           # nearest, but too far
    return db.view(np.int32), qb.view(np.int32)


@functools.lru_cache(maxsize=None)
def tie_case(bits, second):
    """a query against two columns at distances 20 and `second`"""
    rng = np.random.default_rng(7 + bits)
    base = rng.integers(0, 1 << 32, size=bits // 32, dtype=np.uint64).astype(np.uint32)
    picks = rng.choice(bits, size=second, replace=False)

    def flipped(sel):
        out = base.copy()
        for b in sel:
            out[b // 32] ^= np.uint32(1) << np.uint32(b % 32)
        return out
    db = np.stack([flipped(picks), flipped(picks[:20])])[None]
    return db.view(np.int32), base[None, None].view(np.int32)


def check_planted(bits, run):
    """every planted case is decided by its rule and by nothing else; run(db_bits, q_bits, max_distance, ratio) -> (votes,
    nn_index, nn_distance, nn_vote) with NULL masks"""
    db, qb = planted(bits)
    md = bits // 4

    def rows(max_distance, ratio):
        got = run(db, qb, max_distance, ratio)
        assert got[0][0, 0] == got[3][0, 0].sum()
        return got[1][0, 0], got[2][0, 0], got[3][0, 0]
    j, d, v = rows(md, 0.8)
    assert (j[0], d[0]) == (5, 3) and not v[0]                      # duplicates at 5 and 133: the lower index, d2 == d1
    assert (j[1], d[1]) == (7, 0) and v[1]                          # identical
    assert (j[2], d[2]) == (9, 0) and (j[3], d[3]) == (11, 0) and v[2] and v[3]       # all zero, all one
    assert (j[4], d[4]) == (20, md) and v[4]                        # d1 == max_distance
    assert (j[5], d[5]) == (21, md + 1) and not v[5]                # one more
    assert (j[6], d[6]) == (30, 10) and v[6] and (j[7], d[7]) == (50, md + 20) and not v[7]
    assert not rows(md, 0.99)[2][0]                                 # the duplicate pair votes at no ratio < 1 ...
    _, _, v1 = rows(md, 1.0)
    assert not v1[0] and v1[1] and v1[4] and not v1[5]              # ... nor at 1: d1 < d2 is strict
    _, _, v0 = rows(0, 0.8)
    assert list(v0) == [False, True, True, True, False, False, False, False]        # max_distance = 0: identical rows only
    _, _, va = rows(bits, 1.0)
    assert list(va) == [False] + [True] * 7                         # max_distance = num_bits: the ratio alone decides
    # a pair with (float)d1 == ratio * (float)d2 exactly does not vote; one bit further it does
    for second, vote in ((40, False), (41, True)):
        tdb, tq = tie_case(bits, second)
        got = run(tdb, tq, md, 0.5)
        assert (got[1][0, 0, 0], got[2][0, 0, 0], bool(got[3][0, 0, 0]), got[0][0, 0]) == (1, 20, vote, int(vote))


@functools.lru_cache(maxsize=None)
def oracle_scenes(num_bits):
    """(keypoints_a (12, 64, 2), bits_a (12, 64, W) int32, keypoints_b, bits_b) of the twelve scene pairs through
    oracle/numpy_oracle.py: the database frames a, and the revisits b = a moved by (3, 5) with noise"""
    from oracle import numpy_oracle as O
    s = SCENES
    a, b = synth_batch(s["first_seed"], s["count"], s["height"], s["width"], s["shift"], s["noise"])
    t = np.load(os.path.join(ROOT, "onnx_image_processing_amd", "data", "bad_tables.npz"))
    out = []
    for im in (a, b):
        sc = O.shi_tomasi_score(im, s["block"])[:, 0]
        kp, _, _ = O.select_topk_keypoints(sc, O.nms_mask(sc, s["nms"]), s["k"], 0.0, s["border"])
        _, aux = O.sparse_bad(im, kp, t[f"box_{num_bits}"], t[f"thr_{num_bits}"], True, False, 10.0, True, return_aux=True)
        out += [kp, O.pack_bits(aux["bits"]).view(np.int32)]
    return tuple(out)


def scene_figures(votes, nn_index, nn_vote, kp_q, kp_db):
    """votes (12, 12); nn_index / nn_vote (12, Kq) of query i against keyframe i -> (winners (12,), the true keyframe's
    votes, the best other keyframe's votes, the share of the true keyframe's votes that join keypoints displaced by the shift)"""
    count = votes.shape[0]
    true = np.diag(votes).copy()
    other = np.where(np.eye(count, dtype=bool), -1, votes).max(1)
    share = np.zeros(count)
    for i in range(count):
        m = nn_vote[i].astype(bool)
        d = kp_q[i][m] - kp_db[i][nn_index[i][m]]
        share[i] = (d == np.array(SCENES["shift"], F32)).all(1).mean() if m.any() else 0.0
    return votes.argmax(1), true, other, share


def assert_scene_conditions(winners, true, other, share):
    assert np.array_equal(winners, np.arange(len(winners)))
    assert true.min() >= E2E_MIN_WINNER, true
    assert other.max() <= E2E_MAX_RUNNER_UP, other
    assert share.min() >= E2E_MIN_SHARE, share


def scene_camera():
    f = float(SCENES["width"])
    return np.array([[f, 0, SCENES["width"] / 2], [0, f, SCENES["height"] / 2], [0, 0, 1]], F32)


# ---- the device ------------------------------------------------------------------------------------------------------------------
pytestmark = GPU


def host(*tensors):
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in tensors]
    return out[0] if len(out) == 1 else out


def assert_votes_equal(got, want):
    for g, w, name in zip(got, want, ("votes", "nn_index", "nn_distance", "nn_vote")):
        assert g.shape == w.shape and np.array_equal(g, w), f"{name}: {int((g != w).sum())} of {w.size} elements differ"


@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("params", ["quarter_0.8", "all_1.0"])
def test_votes_equal_the_oracle(shape, params):
    from onnx_image_processing_amd import ops
    bits = shape[4]
    md, ratio = (bits // 4, 0.8) if params == "quarter_0.8" else (bits, 1.0)
    db, dbv, qb, qv = gpu(*parity_case(*shape))
    want = parity_reference(shape, md, ratio)
    got = host(*ops.place_votes(db, dbv, qb, qv, md, ratio, want_matches=True))
    assert_votes_equal(got, want)
    assert np.array_equal(host(ops.place_votes(db, dbv, qb, qv, md, ratio)), want[0])     # the votes-only form
    if params == "quarter_0.8" and shape[2] > 1:
        assert want[0].sum() > 0                                                        # the case does vote


def test_oracle_loop_form_on_the_device_cases():
    """the vectorised oracle the large cases use is the plain double loop on the small ones"""
    for shape in PARITY_SHAPES[:2]:
        db, dbv, qb, qv = parity_case(*shape)
        for a, b in zip(PO.place_votes(db, dbv, qb, qv, shape[4] // 4, 0.8, frame=PO.frame_loop), parity_reference(shape, shape[4] // 4, 0.8)):
            assert np.array_equal(a, b)


def test_null_masks_mean_all_valid():
    from onnx_image_processing_amd import ops
    db, _, qb, _ = parity_case(1, 37, 96, 130, 256)
    want = PO.place_votes(db, None, qb, None, 64, 0.8)
    assert_votes_equal(host(*ops.place_votes(gpu(db), None, gpu(qb), None, 64, 0.8, want_matches=True)), want)


@pytest.mark.parametrize("bits", [256, 512])
def test_planted_cases(bits):
    from onnx_image_processing_amd import ops

    def run(db, qb, max_distance, ratio):
        got = host(*ops.place_votes(gpu(db), None, gpu(qb), None, max_distance, ratio, want_matches=True))
        assert_votes_equal(got, PO.place_votes(db, None, qb, None, max_distance, ratio, frame=PO.frame_loop))
        return got
    check_planted(bits, run)


def test_frame_index_gives_the_rows_of_the_full_call():
    from onnx_image_processing_amd import ops
    rng = np.random.default_rng(5)
    db = rng.integers(0, 1 << 32, size=(5, 50, 8), dtype=np.uint64).astype(np.uint32)
    qb = rng.integers(0, 1 << 32, size=(2, 40, 8), dtype=np.uint64).astype(np.uint32)
    for a in range(2):
        for i in range(0, 40, 2):
            qb[a, i] = flip_bits(rng, db[rng.integers(5), rng.integers(50)], int(rng.integers(0, 40)))
    dbv, qv = rng.random((5, 50)) < 0.8, rng.random((2, 40)) < 0.8
    index = np.array([[3, -1, 0, 3, 4, -1], [1, 1, -1, 2, 0, 4]], np.int32)
    d = gpu(db.view(np.int32), dbv, qb.view(np.int32), qv)
    full = host(*ops.place_votes(*d, 64, 0.8, want_matches=True))
    got = host(*ops.place_votes(*d, 64, 0.8, frame_index=gpu(index), want_matches=True))
    assert_votes_equal(got, PO.place_votes(db.view(np.int32), dbv, qb.view(np.int32), qv, 64, 0.8, frame_index=index))
    assert full[0].sum() > 0
    for a in range(2):
        for s, f in enumerate(index[a]):
            if f < 0:
                assert got[0][a, s] == 0 and (got[1][a, s] == -1).all() and (got[2][a, s] == 257).all() and not got[3][a, s].any()
            else:
                for g, w in zip(got, full):
                    assert np.array_equal(g[a, s], w[a, f])


SELECT_CASES = {
    # name: (Q, N, vote range, C, min_votes, exclusion per query or None)
    "ties": (3, 40, 4, 8, 1, None),
    "exclusion_empty_inside_all": (3, 40, 30, 6, 2, [(7, 7), (10, 25), (0, 40)]),
    "min_votes_above_all": (2, 40, 30, 4, 31, None),
    "more_places_than_eligible": (2, 9, 30, 64, 15, None),
    "one_candidate": (2, 300, 30, 1, 0, [(0, 5), (290, 300)]),
    "one_keyframe": (3, 1, 30, 4, 10, None),
    "largest": (2, 65536, 50, 64, 3, [(100, 60000), (65535, 65536)]),
}


@pytest.mark.parametrize("name", list(SELECT_CASES))
def test_select_equals_the_oracle(name):
    from onnx_image_processing_amd import ops
    q, n, top, c, min_votes, excl = SELECT_CASES[name]
    votes = np.random.default_rng(len(name)).integers(0, top + 1, size=(q, n)).astype(np.int32)
    lo = hi = None
    if excl is not None:
        lo, hi = np.array([e[0] for e in excl], np.int32), np.array([e[1] for e in excl], np.int32)
    want = PO.place_select(votes, c, min_votes, lo, hi)
    got = host(*ops.place_select(gpu(votes), c, min_votes, gpu(lo), gpu(hi)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if name == "min_votes_above_all":
        assert (got[0] == -1).all() and (got[1] == 0).all()
    if name == "exclusion_empty_inside_all":
        assert (got[0][2] == -1).all() and (got[0][0] >= 0).all() and not ((got[0][1] >= 10) & (got[0][1] < 25)).any()
    if name == "more_places_than_eligible":
        assert (got[0][:, -1] == -1).all() and (got[0][:, 0] >= 0).all()


def _database(**kw):
    from onnx_image_processing_amd.pytorch_model.retrieval import KeyframeDatabase
    return KeyframeDatabase(**kw).to(DEV)


def _keypoints(rng, frames, k, valid_share=0.9):
    kp = rng.integers(8, 100, size=(frames, k, 2)).astype(F32)
    kp[rng.random((frames, k)) > valid_share] = -1.0
    return kp


def test_database_add_query_and_errors():
    rng = np.random.default_rng(11)
    db_bits, q_bits, target, _ = synth_place_descriptors(21, 10, 48, 256, 0.1, 0.5)
    kp, kq = _keypoints(rng, 10, 48), _keypoints(rng, 1, 48, 1.0)
    one, two = _database(capacity=16, max_keypoints=48, min_votes=5), _database(capacity=10, max_keypoints=48, min_votes=5)
    assert host(one.add(gpu(db_bits), gpu(kp))).tolist() == list(range(10))
    assert host(two.add(gpu(db_bits[:4]), gpu(kp[:4]))).tolist() == [0, 1, 2, 3] and host(two.add(gpu(db_bits[4:]), gpu(kp[4:]))).tolist() == list(range(4, 10))
    assert one.size == two.size == 10
    qa, qk = gpu(q_bits[None]), gpu(kq)
    r1, r2 = host(*one.query(qa, qk)), host(*two.query(qa, qk))
    for a, b in zip(r1, r2):
        assert np.array_equal(a, b)                                              # two batches are one batch ...
    assert r1[2].shape == (1, 10)                                                # ... and capacity beyond size is not scored
    want = PO.place_votes(db_bits, kp[..., 0] >= 0, q_bits[None], None, 64, 0.8)[0]
    assert np.array_equal(r1[2], want)
    ci, cv = PO.place_select(want, 4, 5)
    assert np.array_equal(r1[0], ci) and np.array_equal(r1[1], cv) and r1[0][0, 0] == target
    # exclude_recent: the last keyframes leave the candidates, the votes stay
    recent = 10 - target
    ex = host(*one.query(qa, qk, exclude_recent=recent))
    ci, cv = PO.place_select(want, 4, 5, np.array([target], np.int32), np.array([10], np.int32))
    assert np.array_equal(ex[0], ci) and np.array_equal(ex[1], cv) and target not in ex[0] and np.array_equal(ex[2], want)
    with pytest.raises(RuntimeError, match="full"):
        two.add(gpu(db_bits[:1]), gpu(kp[:1]))
    one.add(gpu(db_bits[:6]), gpu(kp[:6]))
    with pytest.raises(RuntimeError, match="full"):
        one.add(gpu(db_bits[:1]), gpu(kp[:1]))
    two.reset()
    assert two.size == 0 and host(two.add(gpu(db_bits[:2]), gpu(kp[:2]))).tolist() == [0, 1]


def test_database_match_gathers_the_oracles_neighbours():
    rng = np.random.default_rng(12)
    db_bits, q_bits, target, source = synth_place_descriptors(22, 6, 40, 512, 0.1, 0.6)
    kp, kq = _keypoints(rng, 6, 40), _keypoints(rng, 1, 40)
    db = _database(capacity=8, max_keypoints=40, num_bits=512, min_votes=3, num_candidates=3)
    db.add(gpu(db_bits), gpu(kp))
    cand = np.array([[target, -1, (target + 1) % 6]], np.int32)
    k_q, k_db, valid = host(*db.match(gpu(q_bits[None]), gpu(kq), gpu(cand)))
    _, nn_i, _, nn_v = PO.place_votes(db_bits, kp[..., 0] >= 0, q_bits[None], kq[..., 0] >= 0, 128, 0.8, frame_index=cand)
    assert k_q.shape == k_db.shape == (3, 40, 2) and valid.shape == (3, 40)
    assert np.array_equal(valid, nn_v[0]) and valid[0].sum() >= 10 and not valid[1].any()
    for c in range(3):
        assert np.array_equal(k_q[c], kq[0])
        want = np.where((nn_i[0, c] >= 0)[:, None], kp[max(cand[0, c], 0)][np.maximum(nn_i[0, c], 0)], -1.0)
        assert np.array_equal(k_db[c], want)
    voted = valid[0]
    assert np.array_equal(nn_i[0, 0][voted], source[voted])                     # the planted rows find the rows they were made from


@pytest.mark.parametrize("n_frames,k", [(37, 96), (64, 130)])
@pytest.mark.parametrize("bits", [256, 512])
def test_revisited_keyframe_comes_first(n_frames, k, bits):
    db_bits, q_bits, target, _ = synth_place_descriptors(100 + n_frames + bits, n_frames, k, bits, 0.15, 0.4)
    kp = np.full((n_frames, k, 2), 10.0, F32)
    db = _database(capacity=n_frames, max_keypoints=k, num_bits=bits, min_votes=5)
    db.add(gpu(db_bits), gpu(kp))
    ci, cv, votes = host(*db.query(gpu(q_bits[None]), gpu(kp[:1])))
    assert np.array_equal(votes, PO.place_votes(db_bits, None, q_bits[None], None, bits // 4, 0.8)[0])
    assert ci[0, 0] == target and cv[0, 0] == votes[0, target] >= 10
    assert (np.delete(votes[0], target) < votes[0, target]).all()


def _device_scenes(num_bits):
    from onnx_image_processing_amd.pytorch_model.descriptor.bad import SparseBAD
    from onnx_image_processing_amd.pytorch_model.detector import ShiTomasiScore
    from onnx_image_processing_amd.pytorch_model.utils.keypoint_utils import detect_keypoints
    s = SCENES
    a, b = synth_batch(s["first_seed"], s["count"], s["height"], s["width"], s["shift"], s["noise"])
    det = ShiTomasiScore(block_size=s["block"]).to(DEV)
    bad = SparseBAD(num_pairs=num_bits, binarize=True, soft_binarize=False).to(DEV)
    out = []
    for im in gpu(a, b):
        kp, _ = detect_keypoints(det(im).squeeze(1), s["nms"], s["k"], 0.0, s["border"])
        out += [kp, bad.forward_bits(im, kp)]
    return out


@pytest.mark.parametrize("bits", [256, 512])
def test_scenes_end_to_end(bits):
    from onnx_image_processing_amd.pytorch_model.geometry import HomographyEstimator
    kp_a, bits_a, kp_b, bits_b = _device_scenes(bits)
    db = _database(capacity=16, max_keypoints=SCENES["k"], num_bits=bits, ratio=SCENES["ratio"], min_votes=E2E_MIN_WINNER, num_candidates=2)
    db.add(bits_a, kp_a)
    cand_index, cand_votes, votes = db.query(bits_b, kp_b)
    k_q, k_db, valid = db.match(bits_b, kp_b, cand_index)
    h_kp_a, h_bits_a, h_kp_b, h_bits_b, h_ci, h_cv, h_votes, h_kq, h_kdb, h_valid = host(kp_a, bits_a, kp_b, bits_b, cand_index, cand_votes,
                                                                                    votes, k_q, k_db, valid)
    # the oracle on the device's own bits
    want = PO.place_votes(h_bits_a, h_kp_a[..., 0] >= 0, h_bits_b, h_kp_b[..., 0] >= 0, bits // 4, SCENES["ratio"])
    assert np.array_equal(h_votes, want[0])
    own = np.arange(SCENES["count"])
    figures = scene_figures(h_votes, want[1][own, own], want[3][own, own], h_kp_b, h_kp_a)
    print("votes of the true keyframe", figures[1], "best other", figures[2], "displacement share", np.round(figures[3], 3))
    assert_scene_conditions(*figures)
    assert np.array_equal(h_ci[:, 0], own) and np.array_equal(h_cv[:, 0], figures[1]) and (h_ci[:, 1] == -1).all()
    first = np.arange(0, 2 * SCENES["count"], 2)                                 # match's rows of every query's first candidate
    assert np.array_equal(h_valid[first], want[3][own, own]) and not h_valid[first + 1].any()
    for i in own:
        m = h_valid[2 * i]
        assert np.array_equal(h_kdb[2 * i][m], h_kp_a[i][want[1][i, i][m]]) and np.array_equal(h_kq[2 * i], h_kp_b[i])
    # HomographyEstimator takes match's output as it is: the revisit is a shift of the frame, so the votes are its inliers
    est = HomographyEstimator(torch.from_numpy(scene_camera())).to(DEV)
    _, inlier, ok = est(k_q[0::2].contiguous(), k_db[0::2].contiguous(), valid[0::2].contiguous())
    h_inlier, h_ok = host(inlier, ok)
    print("homography inliers", h_inlier.sum(1), "of", figures[1])
    assert h_ok.all() and (h_inlier.sum(1) >= E2E_INLIER_SHARE * figures[1]).all()


def test_two_calls_and_a_graph_replay_give_equal_bytes():
    from onnx_image_processing_amd import ops
    db, dbv, qb, qv = gpu(*parity_case(1, 37, 96, 130, 256))
    lo, hi = gpu(np.array([3], np.int32), np.array([9], np.int32))

    def run():
        out = ops.place_votes(db, dbv, qb, qv, 64, 0.8, want_matches=True)
        return (*out, *ops.place_select(out[0], 5, 1, lo, hi))
    eager, again = run(), run()
    for x, y in zip(eager, again):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                                     # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for x in captured:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(x, y)
    assert int(eager[0].sum()) > 0 and int((eager[4] >= 0).sum()) > 0
