"""K26 loop-closure retrieval without a GPU: the two forms of the numpy oracle agree; the kernels' arithmetic
(csrc/place_math.h) compiled for the host in tests/native/place_host.cpp -- the best-two pair pushed and merged in every
order of a column set, the vote predicate, the selection key -- against that oracle, once more under the host sanitizers; the
argument checks of the two entries (MI_E_* before any launch); the Python layers' own checks; the generator; and the
conditions of the end-to-end GPU test of tests/test_gpu_place.py asserted on the oracle first, with the float64 homography
oracle for the inlier bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

import place_oracle as PO
import test_gpu_place as G
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.synth import synth_place_descriptors

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32 = np.float32


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.PARITY_SHAPES[:5], ids=lambda s: "x".join(map(str, s)))
def test_the_two_oracle_forms_agree(shape):
    db, dbv, qb, qv = G.parity_case(*shape)
    if shape[1] > 40:                                                   # the plain loop is slow: a few keyframes are enough
        db, dbv = db[:8], dbv[:8]
    for md, ratio in ((shape[4] // 4, 0.8), (shape[4], 1.0)):
        a = PO.place_votes(db, dbv, qb, qv, md, ratio, frame=PO.frame_loop)
        b = PO.place_votes(db, dbv, qb, qv, md, ratio, frame=PO.frame_fast)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    a = PO.place_votes(db, None, qb, None, 64, 0.8, frame=PO.frame_loop)
    for x, y in zip(a, PO.place_votes(db, None, qb, None, 64, 0.8)):
        assert np.array_equal(x, y)


def test_parity_cases_hold_the_named_frames():
    db, dbv, qb, qv = G.parity_case(2, 3, 64, 64, 256)
    assert dbv[0].sum() == 0 and dbv[1].sum() == 1 and qv[1].sum() == 0 and 0 < qv[0].sum() < 64
    for shape in G.PARITY_SHAPES:
        _, dbv, _, qv = G.parity_case(*shape)
        if dbv.shape[1] > 2:
            assert not dbv.all() and not np.array_equal(np.sort(dbv, axis=1)[:, ::-1], dbv)           # ragged, not a prefix


@pytest.mark.parametrize("bits", [256, 512])
def test_planted_cases_on_the_oracle(bits):
    G.check_planted(bits, lambda db, qb, md, ratio: PO.place_votes(db, None, qb, None, md, ratio, frame=PO.frame_loop))


def test_select_oracle_on_a_worked_example():
    votes = np.array([[5, 9, 9, 2, 7, 9]], np.int32)
    ci, cv = PO.place_select(votes, 4, 5)
    assert ci.tolist() == [[1, 2, 5, 4]] and cv.tolist() == [[9, 9, 9, 7]]
    ci, cv = PO.place_select(votes, 4, 5, np.array([2]), np.array([5]))
    assert ci.tolist() == [[1, 5, 0, -1]] and cv.tolist() == [[9, 9, 5, 0]]


# ---- the kernels' arithmetic on the host -----------------------------------------------------------------------------------------
place_host = host_program("place_host.cpp", hip=True)


def _merge_sets():
    """column sets of up to 7 columns: (num_bits, query (W,), columns [(j, descriptor (W,), valid)])"""
    rng = np.random.default_rng(3)
    sets = []
    for bits in (256, 512):
        w = bits // 32
        for n in (0, 1, 2, 3, 5, 6, 7):
            q = rng.integers(0, 1 << 32, size=w, dtype=np.uint64).astype(np.uint32)
            js = sorted(rng.choice(1024, size=n, replace=False).tolist())
            cols = [(j, G.flip_bits(rng, q, int(rng.integers(0, 12))), bool(rng.random() < 0.8)) for j in js]    # many equal distances
            sets.append((bits, q, cols))
        q = np.zeros(w, np.uint32)
        sets.append((bits, q, [(0, q.copy(), True), (1023, ~q, True), (5, q.copy(), True), (133, q.copy(), False)]))
        sets.append((bits, ~q, [(1023, q.copy(), True), (1022, q.copy(), True)]))                                # distance = num_bits twice
        sets.append((bits, q, [(3, ~q, False), (4, q.copy(), False)]))                                           # nothing valid
    return sets


def _merge_text(sets):
    out = []
    for bits, q, cols in sets:
        qu = PO.unpack(q).astype(int)
        out.append(f"{bits} {qu.sum()} {len(cols)}")
        for j, d, valid in cols:
            du = PO.unpack(d).astype(int)
            out.append(f"{j} {du.sum()} {int((qu & du).sum())} {int(valid)}")
    return "\n".join(out) + "\n"


def _merge_expected(sets):
    for bits, q, cols in sets:
        keys = sorted((int((PO.unpack(q) != PO.unpack(d)).sum()) << 16) | j for j, d, valid in cols if valid)
        d1, j1 = (keys[0] >> 16, keys[0] & 0xFFFF) if keys else (bits + 1, -1)
        d2, j2 = (keys[1] >> 16, keys[1] & 0xFFFF) if len(keys) > 1 else (bits + 1, -1)
        yield [d1, j1, d2, j2, math.factorial(len(cols)) * (len(cols) + 1), 0]


def test_native_pair_merge_in_every_order_gives_the_scan(place_host):
    sets = _merge_sets()
    out = run_host(place_host, "merge", _merge_text(sets))
    assert len(out) == len(sets) == 20
    for got, want in zip(out, _merge_expected(sets)):
        assert [int(v) for v in got] == want


def _vote_rows():
    rows = [(20, 40, 64, 0.5), (20, 41, 64, 0.5), (64, 100, 64, 0.8), (65, 100, 64, 0.8), (0, 0, 0, 1.0), (0, 1, 0, 1.0), (5, 5, 64, 1.0),
            (5, 6, 64, 1.0), (0, 257, 0, 0.8), (256, 257, 256, 1.0), (257, 257, 256, 1.0), (512, 513, 512, 1.0), (3, 4, 64, 0.75), (3, 5, 64, 0.75)]
    rng = np.random.default_rng(4)
    for _ in range(200):
        rows.append((int(rng.integers(0, 514)), int(rng.integers(0, 514)), int(rng.integers(0, 513)), float(F32(rng.uniform(0.01, 1.0)))))
    return rows


def test_native_vote_predicate(place_host):
    rows = _vote_rows()
    out = run_host(place_host, "vote", "\n".join("%d %d %d %.9g" % r for r in rows))
    want = [int(PO._vote(d1, d2, md, ratio)) for d1, d2, md, ratio in rows]
    assert [int(ln[0]) for ln in out] == want and want[:4] == [0, 1, 1, 0] and 20 < sum(want) < 200


def _key_rows():
    rng = np.random.default_rng(6)
    votes = np.concatenate([rng.integers(0, 6, size=60), [0, 1024, 2 ** 31 - 1, -1, -2 ** 31]])
    index = np.concatenate([rng.permutation(65536)[:60], [65535, 0, 7, 9, 11]])
    return votes, index


def test_native_selection_key_orders_like_the_oracle(place_host):
    votes, index = _key_rows()
    out = run_host(place_host, "key", "\n".join(f"{v} {i}" for v, i in zip(votes, index)))
    keys = [int(ln[0]) for ln in out]
    assert [(int(ln[1]), int(ln[2])) for ln in out] == list(zip(votes.tolist(), index.tolist())) and min(keys) > 0
    order = sorted(range(len(keys)), key=lambda r: -keys[r])
    assert order == np.lexsort((index, -votes.astype(np.int64))).tolist()                   # votes descending, index ascending


def test_native_harness_under_the_host_sanitizers(tmp_path):
    """the same stand-alone program built with the host's address and undefined-behaviour sanitizers, run once over every mode"""
    exe = build_host(tmp_path, "place_host.cpp", hip=True, extra=SANITIZE)
    assert len(run_host(exe, "merge", _merge_text(_merge_sets()))) == 20
    assert len(run_host(exe, "vote", "\n".join("%d %d %d %.9g" % r for r in _vote_rows()))) == 214
    votes, index = _key_rows()
    assert len(run_host(exe, "key", "\n".join(f"{v} {i}" for v, i in zip(votes, index)))) == 65


# ---- argument checks -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return N.load()


_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 12)
    _keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # an aligned fake "device" pointer: never dereferenced by a refused call


def test_votes_argument_checks(lib, p):
    f = lib.mi_place_votes

    def call(db=p, dbv=p, n=5, kd=64, qb=p, qv=p, q=2, kq=48, fi=None, slots=5, bits=256, md=64, ratio=0.8, votes=p, ni=p, nd=p, nv=p):
        return f(db, dbv, n, kd, qb, qv, q, kq, fi, slots, bits, md, ratio, votes, ni, nd, nv, None)
    assert call(db=None) == NULL and call(qb=None) == NULL and call(votes=None) == NULL
    assert call(ni=None) == NULL and call(nd=None) == NULL and call(nv=None) == NULL and call(ni=None, nd=None) == NULL
    for kw in (dict(n=0), dict(kd=0), dict(q=0), dict(kq=0), dict(kq=-3), dict(slots=0, fi=p), dict(slots=4), dict(slots=6)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(n=65537, slots=65537), dict(kd=1025), dict(kq=1025), dict(q=65536), dict(bits=128), dict(bits=0), dict(bits=384),
               dict(bits=1024), dict(md=-1), dict(md=257), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.0001), dict(ratio=float("nan")),
               dict(ratio=float("inf"))):
        assert call(**kw) == PARAM, kw
    assert call(bits=512, md=257) != PARAM
    assert call(db=p + 4) == ALIGN and call(qb=p + 2) == ALIGN and call(votes=p + 1) == ALIGN and call(fi=p + 2, slots=3) == ALIGN
    assert call(ni=p + 2) == ALIGN
    assert call(n=0, bits=100) == SHAPE and call(db=None, n=0) == NULL                     # NULL, then shape, then parameters
    assert lib.mi_abi_version() == 3


def test_select_argument_checks(lib, p):
    f = lib.mi_place_select

    def call(votes=p, q=2, n=40, lo=None, hi=None, min_votes=3, c=4, ci=p, cv=p):
        return f(votes, q, n, lo, hi, min_votes, c, ci, cv, None)
    assert call(votes=None) == NULL and call(ci=None) == NULL and call(cv=None) == NULL and call(lo=p) == NULL and call(hi=p) == NULL
    assert call(q=0) == SHAPE and call(n=0) == SHAPE and call(n=-1) == SHAPE
    assert call(n=65537) == PARAM and call(c=0) == PARAM and call(c=65) == PARAM and call(c=-1) == PARAM
    assert call(votes=p + 2) == ALIGN and call(lo=p + 1, hi=p) == ALIGN and call(ci=p + 2) == ALIGN


def test_python_layers_check_their_input():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.retrieval import KeyframeDatabase
    assert (ops.PLACE_MAX_DESCRIPTORS, ops.PLACE_MAX_KEYFRAMES, ops.PLACE_MAX_CANDIDATES) == (1024, 65536, 64)
    db = KeyframeDatabase(8, 32)
    assert (db.num_bits, db.max_distance, db.ratio, db.min_votes, db.num_candidates, db.size) == (256, 64, 0.8, 20, 4, 0)
    assert KeyframeDatabase(8, 32, num_bits=512).max_distance == 128 and KeyframeDatabase(8, 32, max_distance=0).max_distance == 0
    assert tuple(db.bits.shape) == (8, 32, 8) and tuple(db.valid.shape) == (8, 32) and tuple(db.keypoints.shape) == (8, 32, 2)
    for kw in (dict(capacity=0), dict(capacity=65537), dict(max_keypoints=0), dict(max_keypoints=1025), dict(num_bits=128),
               dict(max_distance=257), dict(max_distance=-1), dict(ratio=0.0), dict(ratio=1.5), dict(min_votes=-1), dict(num_candidates=0),
               dict(num_candidates=65)):
        with pytest.raises(ValueError):
            KeyframeDatabase(**{"capacity": 8, "max_keypoints": 32, **kw})
    bits, kp = torch.zeros(2, 32, 8, dtype=torch.int32), torch.zeros(2, 32, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        db.add(bits, kp)
    with pytest.raises(RuntimeError, match=r"bits must be \(frames, K, 8\) int32"):
        db.add(torch.zeros(2, 32, 16, dtype=torch.int32), kp)
    with pytest.raises(RuntimeError, match="keypoints must be"):
        db.query(bits, kp[:1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.place_votes(bits, None, bits, None, 64, 0.8)
    with pytest.raises(RuntimeError, match="supported: 256 and 512"):
        ops.place_votes(torch.zeros(2, 32, 4, dtype=torch.int32), None, bits, None, 64, 0.8)
    with pytest.raises(RuntimeError, match="max_distance"):
        ops.place_votes(bits, None, bits, None, 257, 0.8)
    with pytest.raises(RuntimeError, match="ratio"):
        ops.place_votes(bits, None, bits, None, 64, 0.0)
    with pytest.raises(RuntimeError, match="validity mask"):
        ops.place_votes(bits, torch.ones(2, 31, dtype=torch.bool), bits, None, 64, 0.8)
    with pytest.raises(RuntimeError, match="num_candidates"):
        ops.place_select(torch.zeros(2, 9, dtype=torch.int32), 65, 1)
    with pytest.raises(RuntimeError, match="come together"):
        ops.place_select(torch.zeros(2, 9, dtype=torch.int32), 4, 1, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.place_select(torch.zeros(2, 9, dtype=torch.int32), 4, 1)


def test_exports_resolve_through_the_alias():
    import onnx_image_processing_amd.pytorch_model.retrieval as real
    from pytorch_model.retrieval import KeyframeDatabase
    assert KeyframeDatabase is real.KeyframeDatabase and real.__all__ == ["KeyframeDatabase"]
    import pytorch_model
    assert "pytorch_model.retrieval" in pytorch_model.__doc__


# ---- the generator and the conditions of the GPU tests ---------------------------------------------------------------------------
def test_generator_is_reproducible_and_plants_a_revisit():
    a, b = synth_place_descriptors(9, 12, 40, 256, 0.1, 0.5), synth_place_descriptors(9, 12, 40, 256, 0.1, 0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    db, q, target, source = a
    assert db.shape == (12, 40, 8) and db.dtype == np.int32 and q.shape == (40, 8) and 0 <= target < 12
    assert (source >= 0).sum() == 20 and len(set(source[source >= 0])) == 20 and not np.array_equal(source, np.sort(source))
    dist = (PO.unpack(q)[:, None] != PO.unpack(db[target])[None]).sum(-1)
    kept = source >= 0
    near = dist[np.arange(40)[kept], source[kept]]
    assert 8 <= near.mean() <= 45 and near.max() < 64 and dist[~kept].min() > 80           # about flip * num_bits; the rest random
    exact = synth_place_descriptors(9, 12, 40, 512, 0.0, 1.0)
    assert np.array_equal(np.sort(exact[1].view(np.uint32), axis=0), np.sort(exact[0][exact[2]].view(np.uint32), axis=0))
    with pytest.raises(ValueError):
        synth_place_descriptors(9, 12, 40, 100, 0.1, 0.5)


@pytest.mark.parametrize("n_frames,k", [(37, 96), (64, 130)])
@pytest.mark.parametrize("bits", [256, 512])
def test_revisited_keyframe_comes_first_on_the_oracle(n_frames, k, bits):
    """the condition of test_gpu_place.test_revisited_keyframe_comes_first, same arguments"""
    db_bits, q_bits, target, _ = synth_place_descriptors(100 + n_frames + bits, n_frames, k, bits, 0.15, 0.4)
    votes = PO.place_votes(db_bits, None, q_bits[None], None, bits // 4, 0.8)[0][0]
    print(f"{n_frames} x {k} x {bits}: revisited {votes[target]}, best other {np.delete(votes, target).max()}")
    assert votes[target] >= 10 and (np.delete(votes, target) < votes[target]).all()


@pytest.mark.parametrize("bits", [256, 512])
def test_scene_conditions_hold_on_the_oracle(bits):
    """what test_gpu_place.test_scenes_end_to_end asserts on the device, on the numpy oracle's keypoints and bits; measured
    here: 256 bits 49 .. 60 votes for the true keyframe, at most 14 for another, displacement share >= 0.913; 512 bits
    51 .. 61, at most 9, >= 0.912"""
    import homography_oracle as HO
    import pose_oracle
    kp_a, bits_a, kp_b, bits_b = G.oracle_scenes(bits)
    assert (kp_a[..., 0] >= 0).all() and (kp_b[..., 0] >= 0).all()
    votes, nn_i, _, nn_v = PO.place_votes(bits_a, kp_a[..., 0] >= 0, bits_b, kp_b[..., 0] >= 0, bits // 4, G.SCENES["ratio"])
    own = np.arange(G.SCENES["count"])
    figures = G.scene_figures(votes, nn_i[own, own], nn_v[own, own], kp_b, kp_a)
    print("votes of the true keyframe", figures[1], "best other", figures[2], "displacement share", np.round(figures[3], 3))
    G.assert_scene_conditions(*figures)
    # the inlier bound of the device test, on the float64 homography oracle with HomographyEstimator's defaults
    K = G.scene_camera()
    focal = (K[0, 0] + K[1, 1]) / 2
    for i in (0, 5, 11):
        p1, p2 = pose_oracle.normalise(kp_b[i], K), pose_oracle.normalise(kp_a[i][np.maximum(nn_i[i, i], 0)], K)
        _, inlier, _, count, _ = HO.ransac(p1, p2, nn_v[i, i], 256, 3.0 / focal, 3, 0, b=i)
        print(f"scene {i}: {count} homography inliers of {figures[1][i]} votes")
        assert count >= G.E2E_INLIER_SHARE * figures[1][i]
