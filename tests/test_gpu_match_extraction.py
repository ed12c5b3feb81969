"""Match extraction (K7, csrc/mnn.hip) and the outlier filters against the numpy oracle at every dispatch of the library:
both one-pass kernels, the row + column kernel pair (m > 1024), the band kernels on the Sinkhorn duals in all their forms
(one chunk, FULL, SPLIT, the two-chunk form behind debug key 17 = 0), the select kernel's counting rank (n <= 1024) and
its strided bitonic network (n up to 4096), the column merge in the select prologue and in its own kernel (batch > 32),
max_matches above 1024 and above n.  The inputs carry what random scores never do: many distinct matches with EQUAL
scores, duplicated rows in different 32-row bands, duplicated columns, and a mutual pair of score exactly 0.0.

Everything about the matches is compared exactly; every GPU call runs twice and must repeat bit for bit (the column
merge is atomic).  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from gpu_common import DEV, gpu, mods  # noqa: F401  (mods: the module fixture)
from helpers import bad_tables, p_close
from onnx_image_processing_amd.synth import synth_batch
from oracle import numpy_oracle as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs and comparisons
def _planted_p(rng, batch, n, m):
    """P (batch, n+1, m+1) float32 >= 0: a background below 0.5, a random partial permutation of planted pairs with one of
    sixteen values in [1, 2) (distinct matches share scores), duplicated rows (one in another 32-row band) and a
    duplicated column (argmax ties: the first index must win), and an all-zero row 0 and column 0 (a mutual pair of
    score exactly 0.0)."""
    p = (rng.random((batch, n + 1, m + 1)) ** 8 * 0.5).astype(np.float32)
    k = 3 * min(n, m) // 4
    for b in range(batch):
        rows, cols = rng.permutation(n)[:k], rng.permutation(m)[:k]
        p[b, rows, cols] = (1.0 + rng.integers(0, 16, k) / 16.0).astype(np.float32)
    if n > 8 and m > 8:
        p[:, 3] = p[:, 2]
        if n > 40:
            p[:, n - 1] = p[:, 2]
        p[:, :, 4] = p[:, :, 1]
    p[:, 0, :] = 0.0
    p[:, :, 0] = 0.0
    return p


def _keypoints(rng, batch, n, m):
    return (rng.integers(0, 400, (batch, n, 2)).astype(np.float32), rng.integers(0, 400, (batch, m, 2)).astype(np.float32))


def _mutual_scores(core, threshold):
    """Scores of the mutual nearest-neighbour pairs of one core matrix with score >= threshold, found the slow way (first
    index on ties), independently of O.mnn_extract."""
    best = core.max(1)
    scores = []
    for i in range(core.shape[0]):
        j = int(np.flatnonzero(core[i] == best[i])[0])
        if int(np.flatnonzero(core[:, j] == core[:, j].max())[0]) == i and best[i] >= np.float32(threshold):
            scores.append(best[i])
    return np.asarray(scores, np.float32)


def _check_oracle_output(p, ref, n, m, max_matches, threshold, planted):
    """The preconditions of a case, on the oracle's own output: what the case is there to reach is really in it."""
    _, _, sc, valid, ij = ref
    cnt = min(max_matches, n)
    for b in range(p.shape[0]):
        mutual = _mutual_scores(p[b, :n, :m], threshold)
        if planted and n > 8 and m > 8:
            matched = np.sort(sc[b][valid[b]])
            assert matched.size >= 2 and (np.diff(matched) == 0).any(), "no two matches share a score"
        if planted and threshold == 0.0 and n > 8 and m > 8 and cnt > (mutual > 0).sum():
            # (where the positive matches alone fill the max_matches slots, the 0.0 pair falls to the cut)
            zero = (sc[b, :cnt] == 0.0) & ~valid[b, :cnt] & (ij[b, :cnt] == -1).all(-1)
            assert zero.any(), "no mutual pair of score 0.0"
        if cnt > mutual.size:
            assert (sc[b] == -1.0).any(), "no non-match slot"


def _equal_oracle(got, ref):
    names = ("mk1", "mk2", "scores", "valid", "ij")
    assert len(got) == 5
    for name, g, r in zip(names, got, ref):
        g = g.cpu().numpy()
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name == "ij":
            g = g.astype(np.int64)                 # the kernel writes int32, the oracle int64: values
        bad = np.argwhere(g != r)
        assert bad.size == 0, f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {r[tuple(bad[0])]}"


def _twice(run):
    """The GPU call twice: equal bits."""
    first = [t.clone() for t in run()]
    second = run()
    for a, c in zip(first, second):
        assert torch.equal(a, c), "the call does not repeat bit for bit"
    return first


# ------------------------------------------------------------------ A. mi_mnn_extract on a materialised P
EXTRACT_CASES = [
    (2, 1024, 1024, 100, 0.1),      # mnn_p_kernel<16>, 1024 keys
    (2, 33, 1000, 50, 0.0),         # mnn_p_kernel<16>, small n
    (2, 700, 520, 1000, 0.0),       # max_matches > n
    (1, 96, 1024, 96, 0.1),         # mnn_p_kernel<16>, n << m
    (2, 64, 1500, 64, 0.0),         # row and column kernels
    (1, 1500, 64, 2000, 0.0),       # 2048 keys, max_matches > 1024 and > n
    (1, 2048, 300, 2048, 0.0),      # 2048 keys, n a power of two
    (1, 1025, 513, 1025, 0.0),      # one past both limits
    (1, 4096, 512, 4096, 0.0),      # the largest n
    (1, 3000, 1100, 1200, 0.1),     # m > 1024 and n > 1024 together
    (2, 1, 1, 5, 0.0), (2, 2, 1, 1, 0.0),     # smallest extents
    (33, 130, 512, 50, 0.0),        # batch > 32
]


@pytest.mark.parametrize("batch,n,m,max_matches,threshold", EXTRACT_CASES)
def test_mnn_extract_vs_oracle(mods, batch, n, m, max_matches, threshold):
    from onnx_image_processing_amd import ops
    rng = np.random.default_rng(batch * 100003 + n * 31 + m)
    p = _planted_p(rng, batch, n, m)
    k1, k2 = _keypoints(rng, batch, n, m)
    ref = O.mnn_extract(p, k1, k2, max_matches, threshold)
    _check_oracle_output(p, ref, n, m, max_matches, threshold, planted=True)
    pt, t1, t2 = gpu(p), gpu(k1), gpu(k2)
    got = _twice(lambda: ops.mnn_extract(pt, t1, t2, max_matches, threshold, return_indices=True))
    _equal_oracle(got, ref)


def test_mnn_extract_argument_errors(mods):
    from onnx_image_processing_amd import ops
    rng = np.random.default_rng(3)
    k = lambda n: gpu(rng.integers(0, 400, (1, n, 2)).astype(np.float32))
    with pytest.raises(RuntimeError):
        ops.mnn_extract(torch.zeros((1, 4098, 9), device=DEV), k(4097), k(8), 10, 0.1)      # n above the key array
    p = gpu(rng.random((1, 9, 9)).astype(np.float32))
    with pytest.raises(RuntimeError):
        ops.mnn_extract(p, k(8), k(8), 0, 0.1)
    # the band kernels stop at m = 1024
    n, m = 8, 1025
    pitch = (m + 7) // 8 * 8
    u, v = torch.zeros((1, n + 1), device=DEV), torch.zeros((1, m + 1), device=DEV)
    with pytest.raises(RuntimeError):
        ops.mnn_from_duals(torch.zeros((1, n, pitch), device=DEV), m, pitch, u, v, k(n), k(m), 10, 0.1)
    state = (torch.zeros((1, n, pitch), dtype=torch.int16, device=DEV), torch.zeros((1, n, 2), device=DEV),
             torch.zeros((1, m, 2), device=DEV), pitch)
    with pytest.raises(RuntimeError):
        ops.mnn_from_duals_dots(state, m, 0.05, u, v, k(n), k(m), 10, 0.1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ B. matches from the duals, on the solver's own P
EPS, UNUSED, ITERS = 0.05, 1.0, 5
DUALS_THRESHOLD = 0.1


def _solve_z(ops, batch, n, m, seed):
    """fp32-Z form: (z, pitch, P, u, v) of a random cost in [0.5, 2.5) with a diagonal below 0.05 (real matches: ten units
    of z above everything else in their row), rows 3 and 42 copies of row 2 (a column tie inside the four rows one wave
    holds, and one across two 32-row bands) and the row padding of z poisoned."""
    rng = np.random.default_rng(seed)
    cost = (0.5 + rng.random((batch, n, m)) * 2.0).astype(np.float32)
    d = np.arange(min(n, m))
    cost[:, d, d] = (rng.random((batch, d.size)) * 0.05).astype(np.float32)
    if n > 3:
        cost[:, 3] = cost[:, 2]
    if n > 42:
        cost[:, 42] = cost[:, 2]
    pitch = (m + 3) // 4 * 4
    z = np.full((batch, n, pitch), np.nan, np.float32)
    z[:, :, :m] = -cost / np.float32(EPS)
    zt = gpu(z)
    p, u, v = ops.sinkhorn(zt, m, pitch, -UNUSED / EPS, ITERS, return_duals=True)
    return zt, pitch, p, u, v


def _solve_dots(ops, batch, n, m, seed):
    """dot-product form: (state, P, u, v) of random 256-bit descriptors, the first half of them shared between the two
    images (real matches), descriptors 3 and 42 of the first image copies of its descriptor 2."""
    rng = np.random.default_rng(seed)
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, 8), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, 8), dtype=np.uint64).astype(np.uint32)
    k = (min(n, m) + 1) // 2
    b2[:, :k] = b1[:, :k]
    if n > 3:
        b1[:, 3] = b1[:, 2]
    if n > 42:
        b1[:, 42] = b1[:, 2]
    p, u, v, state = ops.sinkhorn_bits(gpu(b1.view(np.int32)), gpu(b2.view(np.int32)), True, EPS, UNUSED, ITERS,
                                       return_state=True)
    return state, p, u, v


def _duals_vs_oracle(ops, batch, n, m, form):
    """ops.mnn_from_duals[_dots] == O.mnn_extract on the P the same solver call wrote: the band kernels evaluate P with
    the expression of the solver's last pass, so nothing may differ."""
    seed = batch * 100003 + n * 31 + m
    rng = np.random.default_rng(seed + 1)
    k1, k2 = _keypoints(rng, batch, n, m)
    t1, t2 = gpu(k1), gpu(k2)
    max_matches = n + 3
    if form == "z":
        z, pitch, p, u, v = _solve_z(ops, batch, n, m, seed)
        run = lambda: ops.mnn_from_duals(z, m, pitch, u, v, t1, t2, max_matches, DUALS_THRESHOLD, return_indices=True)
    else:
        state, p, u, v = _solve_dots(ops, batch, n, m, seed)
        run = lambda: ops.mnn_from_duals_dots(state, m, EPS, u, v, t1, t2, max_matches, DUALS_THRESHOLD, return_indices=True)
    assert bool(torch.isfinite(p).all())
    twins = [i for i in (3, 42) if i < n]          # rows whose input is row 2's
    for i in twins:
        assert torch.equal(p[:, 2], p[:, i]), "identical input rows gave different rows of P"
    pn = p.cpu().numpy()
    ref = O.mnn_extract(pn, k1, k2, max_matches, DUALS_THRESHOLD)
    _check_oracle_output(pn, ref, n, m, max_matches, DUALS_THRESHOLD, planted=False)
    assert ref[3].sum() > 0
    if twins and m > 2:                            # the tie is decided in a match: (2, 2) is one, its twins have none
        assert ((ref[4][:, :, 0] == 2) & (ref[4][:, :, 1] == 2)).any(1).all() and not np.isin(ref[4][:, :, 0], twins).any()
    return run, ref


DUALS_SHAPES = [(512, 512), (500, 512), (300, 77), (1024, 1024), (1000, 1000), (33, 1000), (2048, 300), (4096, 512), (1, 1)]


@pytest.mark.parametrize("form", ["z", "dots"])
@pytest.mark.parametrize("n,m", DUALS_SHAPES)
def test_mnn_from_duals_vs_oracle(mods, n, m, form):
    from onnx_image_processing_amd import ops
    run, ref = _duals_vs_oracle(ops, 2, n, m, form)
    _equal_oracle(_twice(run), ref)


@pytest.mark.parametrize("form", ["z", "dots"])
@pytest.mark.parametrize("n,m", [(64, 520), (130, 512)])
def test_mnn_from_duals_vs_oracle_batch_33(mods, n, m, form):
    """More than 32 pairs: the bands' column winners are merged by mnn_colmerge_kernel, not in the select prologue."""
    from onnx_image_processing_amd import ops
    run, ref = _duals_vs_oracle(ops, 33, n, m, form)
    _equal_oracle(_twice(run), ref)


@pytest.mark.parametrize("form", ["z", "dots"])
@pytest.mark.parametrize("n,m", [(700, 520), (1024, 1024)])
def test_mnn_from_duals_two_chunk_kernel_vs_oracle(mods, n, m, form):
    """512 < m <= 1024 with debug key 17 = 0: one wave holds both 512-column chunks of its rows (the form the wave-pair
    kernel replaced).  The same oracle output."""
    from onnx_image_processing_amd import _native as N, ops
    run, ref = _duals_vs_oracle(ops, 2, n, m, form)
    with N.debug_library() as lib:
        try:
            assert lib.mi_debug_set(17, 0) == 0
            got = _twice(run)
        finally:
            assert lib.mi_debug_set(17, 1) == 0
    _equal_oracle(got, ref)
    _equal_oracle(_twice(run), ref)                # and the product's wave-pair form at the same shape


# ------------------------------------------------------------------ C. the wrapper past 1024 keypoints
def test_wrapper_1100_keypoints_vs_oracle(mods):
    """max_keypoints = 1100: no dot-product Sinkhorn, no band kernels -- the generic two-pass Sinkhorn, the row and column
    kernels and the 2048-key bitonic select, end to end."""
    from onnx_image_processing_amd import ops
    k, max_matches, threshold = 1100, 1200, 0.1
    cfg = dict(block_size=3, num_pairs=512, binarize=True, soft_binarize=False, sinkhorn_iterations=20, epsilon=0.05,
               unused_score=1.0, nms_radius=1)
    a, b = synth_batch(2300, 1, 240, 320)
    box, thr = bad_tables(512)
    okw = {key: val for key, val in cfg.items() if key != "num_pairs"}
    # 240 x 320, NMS radius 1, border 7: 3716 and 3717 local maxima with positive score, of which the best 1100 are kept
    o1, o2, op = O.match_pair(a, b, box, thr, k, **okw)
    for im, okp in ((a, o1), (b, o2)):
        s = O.shi_tomasi_score(im, 3)[:, 0]
        _, ksc, ids = O.select_topk_keypoints(s, O.nms_mask(s, 1), k, 0.0, 7)
        assert (ksc > 0).all() and (ids >= 0).all() and (okp >= 0).all()
    assert not ops.mnn_duals_supported(1, k, k)
    model = mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=k, **cfg).to(DEV)
    wrap = mods["MatchExtractionWrapper"](model, max_matches=max_matches, match_threshold=threshold)
    ta, tb = gpu(a), gpu(b)
    k1, k2, p = [t.cpu().numpy() for t in model(ta, tb)]
    assert np.array_equal(k1, o1) and np.array_equal(k2, o2)
    ok, worst = p_close(p, op)
    assert ok, f"P vs oracle: worst ratio {worst:.3g}"
    ref = O.mnn_extract(p, k1, k2, max_matches, threshold)
    assert ref[3].sum() > 500 and (ref[2] == -1.0).any()
    got = _twice(lambda: wrap(ta, tb))
    assert len(got) == 4
    for name, g, r in zip(("mk1", "mk2", "scores", "valid"), got, ref):
        assert np.array_equal(g.cpu().numpy(), r), name


# ------------------------------------------------------------------ D. filters and core maxima
FILTER_SHAPES = [(2, 37, 513), (2, 130, 1024), (1, 5, 1500), (2, 1, 1), (1, 9, 2), (1, 600, 600)]


def _filter_p(batch, n, m):
    """P (batch, n+1, m+1) of random entries in [0, 1) with, where the extents allow, planted rows: 0: best == second, 512
    columns apart (one lane, two trips of the kernel's column loop); 1: best / second == 1.5 exactly, in different
    lanes; 2: the best in the last column; 3: all entries equal; 4: best 0.75 against a dustbin entry of 0.25 (a margin
    of exactly 0.5)."""
    rng = np.random.default_rng(batch * 100003 + n * 31 + m)
    p = (rng.random((batch, n + 1, m + 1)) ** 3).astype(np.float32)
    if n >= 5 and m >= 2:
        if m > 512:
            p[:, 0, 0] = p[:, 0, 512] = 2.0
        ca, cb = (5, 70) if m > 70 else (0, m - 1)
        p[:, 1, ca], p[:, 1, cb] = 3.0, 2.0
        p[:, 2, m - 1] = 4.0
        p[:, 3, :] = 0.5
        p[:, 4, :] *= np.float32(0.5)
        p[:, 4, min(3, m - 1)], p[:, 4, m] = 0.75, 0.25
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("batch,n,m", FILTER_SHAPES)
def test_match_filters_vs_oracle(mods, batch, n, m):
    from onnx_image_processing_amd import ops
    p = _filter_p(batch, n, m)
    pt = gpu(p)
    core = gpu(p[:, :n, :m])
    off = lambda x: -1.0 if x is None else x
    for rt in (1.0, 1.5, None):
        for dm in (0.5, 0.0, None):
            ref_p, ref_v = O.match_filters(p, rt, dm)
            got_p, got_v = _twice(lambda: ops.match_filters(pt.clone(), off(rt), off(dm)))
            assert np.array_equal(got_v.cpu().numpy(), ref_v), (rt, dm)
            assert np.array_equal(_bits(got_p.cpu().numpy()), _bits(ref_p)), (rt, dm)
            (mask,) = _twice(lambda: (ops.match_filter_masks(pt, True, off(rt), off(dm)),))
            assert np.array_equal(mask.cpu().numpy(), ref_v), (rt, dm)
            if rt is None and dm is not None and n == m:           # the stand-alone margin filter takes a square P
                for b in range(batch):
                    assert np.array_equal(mask[b].cpu().numpy(), O.dustbin_margin_filter(p[b], dm)), dm
        (mask,) = _twice(lambda: (ops.match_filter_masks(core, False, off(rt), -1.0),))
        for b in range(batch):
            want = np.ones(n, bool) if rt is None else O.probability_ratio_filter(p[b, :n, :m], rt)
            assert np.array_equal(mask[b].cpu().numpy(), want), rt
    assert np.array_equal(_bits(pt.cpu().numpy()), _bits(p))       # the mask-only form leaves P alone
    if n >= 5 and m > 512:                                         # what the planted rows are there for
        v = O.match_filters(p, 1.5, 0.5)[1]
        assert not v[:, 0].any() and v[:, 1].all() and v[:, 2].all() and not v[:, 3].any() and v[:, 4].all()
        assert O.match_filters(p, 1.0, None)[1][:, 0].all()


@pytest.mark.parametrize("batch,n,m", FILTER_SHAPES)
def test_core_maxima_vs_numpy(mods, batch, n, m):
    from onnx_image_processing_amd import ops
    p = _filter_p(batch, n, m)
    p[:, n, :] = 9.0                               # the dustbins hold the largest entries: they must not be looked at
    p[:, :, m] = 9.0
    pt = gpu(p)
    rows, cols = _twice(lambda: ops.core_maxima(pt))
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(p[:, :n, :m].max(2)))
    assert np.array_equal(_bits(cols.cpu().numpy()), _bits(p[:, :n, :m].max(1)))
