"""Match extraction from the Sinkhorn duals (K7, csrc/mnn.hip) writing the match record itself, and its band kernel finding
winners by value first and place second.

A. The _records entries (mi_mnn_from_duals_records, mi_mnn_from_duals_dots_records) against the separate outputs of the
   unchanged entries for the same duals, exactly, into a record pre-filled with NaN (every slot is written).
B. ops.mnn_from_duals_dots against O.mnn_extract on the P the same solver call wrote, exactly, on descriptors planted with
   every tie the winners' "first place attaining the maximum" has to break: two identical columns among one lane's eight,
   two identical columns in different lanes, a row and its copy among one wave's four, a copy of it in another 32-row
   band; with and without the caller vouching for dots < 1024 (256-bit descriptors: every dot product is below 1024);
   and with a row of u poisoned by NaN.
C. The wrapper's four outputs are views of one record, and distributed.pack_records returns it without a launch.

Every GPU call runs twice and must repeat bit for bit.  Run with `-m gpu` on an MI355X."""
import functools

import numpy as np
import pytest
import torch

from gpu_common import DEV, gpu, mods  # noqa: F401  (mods: the module fixture)
from onnx_image_processing_amd.synth import synth_batch
from oracle import numpy_oracle as O

pytestmark = pytest.mark.gpu

EPS, UNUSED, ITERS = 0.05, 1.0, 5
# (batch, n, m, max_matches, threshold)
SHAPES = [
    (2, 64, 64, 10, 0.0),
    (3, 33, 40, 50, 0.1),           # max_matches > n, ragged band
    (2, 512, 512, 100, 0.1),        # FULL
    (33, 130, 512, 50, 0.0),        # batch > 32
    (1, 96, 1024, 96, 0.1),         # SPLIT
    (1, 1024, 1024, 100, 0.1),      # SPLIT, FULL
]
ROW, TWIN = 2, 3                    # row 2 and its copy, row 3: two of the four rows one wave holds
COL, COL_IN_LANE, COL_ACROSS = 9, 10, 20     # columns 8..15 are lane 1's; column 20 is lane 2's


def _twice(run):
    """The GPU call twice: equal bits (NaN included: the bytes are compared)."""
    first = [t.clone() for t in run()]
    second = run()
    torch.cuda.synchronize()
    for a, c in zip(first, second):
        assert a.dtype == c.dtype and a.shape == c.shape
        assert torch.equal(a.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8)), "the call does not repeat bit for bit"
    return first


def _far_row(n):
    """The row of another 32-row band that also copies ROW (None: the matrix has one band)."""
    return n - 1 if n > 32 else None


@functools.lru_cache(maxsize=None)
def _case(batch, n, m):
    """Planted 256-bit descriptors, the solver's P, duals and state for them, and keypoints: computed once per shape and
    shared (nothing below writes to any of it).  The first half of the descriptors is shared between the two images (real
    matches); descriptor ROW of image 1 also sits at rows TWIN and _far_row(n), and at columns COL, COL_IN_LANE and
    COL_ACROSS of image 2 -- and nowhere else, so the match of ROW is (ROW, COL) by first-index ties alone."""
    from onnx_image_processing_amd import ops
    rng = np.random.default_rng(batch * 100003 + n * 31 + m)
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, 8), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, 8), dtype=np.uint64).astype(np.uint32)
    k = (min(n, m) + 1) // 2
    b2[:, :k] = b1[:, :k]
    b2[:, ROW] = rng.integers(0, 2 ** 32, size=(batch, 8), dtype=np.uint64).astype(np.uint32)
    b1[:, TWIN] = b1[:, ROW]
    if _far_row(n) is not None:
        b1[:, _far_row(n)] = b1[:, ROW]
    for c in (COL, COL_IN_LANE, COL_ACROSS):
        b2[:, c] = b1[:, ROW]
    k1 = rng.integers(0, 400, (batch, n, 2)).astype(np.float32)
    k2 = rng.integers(0, 400, (batch, m, 2)).astype(np.float32)
    p, u, v, state = ops.sinkhorn_bits(gpu(b1.view(np.int32)), gpu(b2.view(np.int32)), True, EPS, UNUSED, ITERS,
                                       return_state=True)
    assert state.num_bits == 256
    assert bool(torch.isfinite(p).all())
    # identical inputs give identical probabilities: the ties are real
    assert torch.equal(p[:, ROW], p[:, TWIN])
    if _far_row(n) is not None:
        assert torch.equal(p[:, ROW], p[:, _far_row(n)])
    assert torch.equal(p[:, :, COL], p[:, :, COL_IN_LANE]) and torch.equal(p[:, :, COL], p[:, :, COL_ACROSS])
    return dict(p=p.cpu().numpy(), u=u, v=v, state=state, k1=k1, k2=k2, t1=gpu(k1), t2=gpu(k2))


def _equal_oracle(got, ref):
    assert len(got) == 5
    for name, g, r in zip(("mk1", "mk2", "scores", "valid", "ij"), got, ref):
        g = g.cpu().numpy()
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name == "ij":
            g = g.astype(np.int64)
        bad = np.argwhere(g != r)
        assert bad.size == 0, f"{name}: {len(bad)} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {r[tuple(bad[0])]}"


# ------------------------------------------------------------------ A. the record against the separate outputs
def _separate_and_record(ops, N, entry, args_head, batch, max_matches, extra):
    """Both entries on the same arguments: (mk1, mk2, scores, valid, ij) of the unchanged entry and (record, valid, ij) of
    its _records form, the record pre-filled with NaN and the byte outputs with 0xEE."""
    mk1 = torch.full((batch, max_matches, 2), float("nan"), device=DEV)
    mk2 = torch.full((batch, max_matches, 2), float("nan"), device=DEV)
    sc = torch.full((batch, max_matches), float("nan"), device=DEV)
    valid = torch.full((batch, max_matches), 0xEE, dtype=torch.uint8, device=DEV)
    ij = torch.full((batch, max_matches, 2), -7, dtype=torch.int32, device=DEV)
    N.call(entry, *args_head, mk1.data_ptr(), mk2.data_ptr(), sc.data_ptr(), valid.data_ptr(), ij.data_ptr(), N.stream_ptr())
    rec = torch.full((batch, max_matches, 6), float("nan"), device=DEV)
    rvalid = torch.full((batch, max_matches), 0xEE, dtype=torch.uint8, device=DEV)
    rij = torch.full((batch, max_matches, 2), -7, dtype=torch.int32, device=DEV)
    N.call(entry + "_records", *args_head, *extra, rec.data_ptr(), rvalid.data_ptr(), rij.data_ptr(), N.stream_ptr())
    return mk1, mk2, sc, valid, ij, rec, rvalid, rij


def _check_record(out):
    mk1, mk2, sc, valid, ij, rec, rvalid, rij = out
    assert not bool(torch.isnan(rec).any()), "a slot of the record was not written"
    assert not bool(torch.isnan(sc).any())
    assert torch.equal(rec[..., 0:2], mk1) and torch.equal(rec[..., 2:4], mk2) and torch.equal(rec[..., 4], sc)
    assert torch.equal(rec[..., 5], valid.to(torch.float32))
    assert bool(((valid == 0) | (valid == 1)).all())
    assert torch.equal(rvalid, valid) and torch.equal(rij, ij)
    assert torch.equal(valid == 1, sc > 0)


@pytest.mark.parametrize("batch,n,m,max_matches,threshold", SHAPES)
def test_record_equals_separate_outputs_dots(mods, batch, n, m, max_matches, threshold):
    from onnx_image_processing_amd import _native as N, ops
    c = _case(batch, n, m)
    dots, row_info, col_info, pitch, (work, status) = c["state"]
    wbytes = int(N.load().mi_mnn_duals_workspace_bytes(batch, n, m))
    scratch = torch.empty((wbytes // 8,), dtype=torch.int64, device=DEV)
    head = (dots.data_ptr(), row_info.data_ptr(), col_info.data_ptr(), batch, n, m, pitch, EPS, c["u"].data_ptr(),
            c["v"].data_ptr(), c["t1"].data_ptr(), c["t2"].data_ptr(), max_matches, threshold, scratch.data_ptr(), wbytes,
            status)
    for flags in (0, ops.MI_SOLVER_DOTS_BELOW_1024):
        out = _twice(lambda: _separate_and_record(ops, N, "mi_mnn_from_duals_dots", head, batch, max_matches, (flags,)))
        _check_record(out)
        assert int(out[3].sum()) > 0


@pytest.mark.parametrize("batch,n,m,max_matches,threshold", SHAPES)
def test_record_equals_separate_outputs_z(mods, batch, n, m, max_matches, threshold):
    """The fp32-Z entry: Z is the log of the solver's own P core (any finite Z will do), u = v = 0."""
    from onnx_image_processing_amd import _native as N, ops
    c = _case(batch, n, m)
    pitch = (m + 3) // 4 * 4
    z = np.full((batch, n, pitch), np.nan, np.float32)
    z[:, :, :m] = np.log(np.maximum(c["p"][:, :n, :m], np.float32(1e-30)))
    zt = gpu(z)
    u = torch.zeros((batch, n + 1), device=DEV)
    v = torch.zeros((batch, m + 1), device=DEV)
    wbytes = int(N.load().mi_mnn_duals_workspace_bytes(batch, n, m))
    scratch = torch.empty((wbytes // 8,), dtype=torch.int64, device=DEV)
    head = (zt.data_ptr(), batch, n, m, pitch, u.data_ptr(), v.data_ptr(), c["t1"].data_ptr(), c["t2"].data_ptr(),
            max_matches, threshold, scratch.data_ptr(), wbytes)
    out = _twice(lambda: _separate_and_record(ops, N, "mi_mnn_from_duals", head, batch, max_matches, ()))
    _check_record(out)
    assert int(out[3].sum()) > 0


# ------------------------------------------------------------------ B. the band kernel against the oracle
def _run(ops, c, m, max_matches, threshold, vouch, u=None):
    return _twice(lambda: ops.mnn_from_duals_dots(c["state"], m, EPS, c["u"] if u is None else u, c["v"], c["t1"], c["t2"],
                                                  max_matches, threshold, return_indices=True, dots_below_1024=vouch))


@pytest.mark.parametrize("batch,n,m,max_matches,threshold", SHAPES)
def test_band_kernel_vs_oracle_with_planted_ties(mods, batch, n, m, max_matches, threshold):
    from onnx_image_processing_amd import ops
    c = _case(batch, n, m)
    ref = O.mnn_extract(c["p"], c["k1"], c["k2"], max_matches, threshold)
    # what the ties are planted for, on the oracle's own answer at full length: ROW is matched to COL (the first of its
    # three equal columns), its copies are matched to nothing
    full = O.mnn_extract(c["p"], c["k1"], c["k2"], n, threshold)
    copies = [TWIN] + ([_far_row(n)] if _far_row(n) is not None else [])
    for b in range(batch):
        rows = full[4][b][full[3][b]]
        assert [ROW, COL] in rows.tolist() and not np.isin(rows[:, 0], copies).any()
    assert ref[3].sum() > 0
    plain = _run(ops, c, m, max_matches, threshold, vouch=False)       # the uint16 converted
    _equal_oracle(plain, ref)
    vouched = _run(ops, c, m, max_matches, threshold, vouch=True)      # read as an fp16 denormal
    _equal_oracle(vouched, ref)
    for a, d in zip(plain, vouched):
        assert torch.equal(a, d)
    default = _run(ops, c, m, max_matches, threshold, vouch=None)      # a 256-bit state vouches by itself
    for a, d in zip(default, vouched):
        assert torch.equal(a, d)


@pytest.mark.parametrize("batch,n,m,max_matches,threshold", [(3, 33, 40, 50, 0.1), (2, 512, 512, 100, 0.1)])
def test_nan_row_has_no_match(mods, batch, n, m, max_matches, threshold):
    """u of one matched row is NaN: every probability of the row is NaN, none of them wins its row or a column.  That is
    the oracle's answer for a P whose row lies below every probability.  Where every match is listed (max_matches > n)
    the other rows keep their matches, slot for slot but for the poisoned row's."""
    from onnx_image_processing_amd import ops
    c = _case(batch, n, m)
    before = O.mnn_extract(c["p"], c["k1"], c["k2"], max_matches, threshold)
    u = c["u"].clone()
    p = c["p"].copy()
    rows = []
    for b in range(batch):
        # the pair's best listed match whose row has no copy (a copy would inherit the match)
        listed = [int(i) for i in before[4][b][before[3][b]][:, 0] if i != ROW]
        assert listed, "no match to lose"
        rows.append(listed[0])
        u[b, rows[b]] = float("nan")
        p[b, rows[b], :] = -1.0
    ref = O.mnn_extract(p, c["k1"], c["k2"], max_matches, threshold)
    for b in range(batch):
        assert not (ref[4][b][:, 0] == rows[b]).any()
    for vouch in (False, True):
        _equal_oracle(_run(ops, c, m, max_matches, threshold, vouch, u=u), ref)
    if max_matches > n:
        for b in range(batch):
            keep = before[3][b] & (before[4][b][:, 0] != rows[b])
            for name, x, y in zip(("mk1", "mk2", "scores", "ij"), (before[0], before[1], before[2], before[4]),
                                  (ref[0], ref[1], ref[2], ref[4])):
                assert np.array_equal(x[b][keep], y[b][ref[3][b]]), name


# ------------------------------------------------------------------ C. the wrapper hands out one record
def test_wrapper_outputs_are_one_record(mods):
    from onnx_image_processing_amd import distributed as D
    from onnx_image_processing_amd.graph import GraphedModule
    cfg = dict(block_size=3, num_pairs=256, binarize=True, soft_binarize=False, sinkhorn_iterations=10, epsilon=0.1,
               nms_radius=2)
    wrapper = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=48, **cfg),
                                             max_matches=30, match_threshold=0.1).to(DEV)
    a, b = [gpu(x) for x in synth_batch(4100, 1, 96, 128)]

    def slow(mk1, mk2, scores, valid):
        return torch.cat([mk1.clone(), mk2.clone(), scores.clone().unsqueeze(-1), valid.to(torch.float32).unsqueeze(-1)], dim=-1)

    out = wrapper(a, b)
    rec = D.pack_records(*out)
    assert rec.data_ptr() == out[0].data_ptr() and rec.shape == (1, 30, 6) and rec.is_contiguous()
    assert out[3].dtype == torch.bool and int(out[3].sum()) > 0
    assert torch.equal(rec, slow(*out))
    again = wrapper(a, b)
    assert torch.equal(D.pack_records(*again), rec) and D.pack_records(*again).data_ptr() != rec.data_ptr()
    # replayed from a captured graph the outputs are the capture's own buffers: still one record, nothing to launch
    graphed = GraphedModule(wrapper, a, b)
    for _ in range(2):
        gout = graphed(a, b)
        grec = D.pack_records(*gout)
        torch.cuda.synchronize()
        assert grec.data_ptr() == gout[0].data_ptr()
        assert torch.equal(grec, rec) and torch.equal(grec, slow(*gout))
