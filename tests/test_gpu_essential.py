"""K10 (csrc/essential.hip) against the staged fp64 oracle of tests/essential_oracle.py at every dispatch.

    shape (batch, n, m)                         what it reaches
    (1, 3, 3)                                   top_k 3 = n = m
    (2, 31, 20), (1, 32, 64), (3, 33, 65)       32-row band edges, m < 64, lane-pair edges at columns 63 / 64
    (2, 257, 301)                               nine bands (the second trip of em_sparse_kernel's band loop), odd m
    (1, 100, 512), (1, 100, 513)                em_band_kernel<., ., 8> / <., ., 16>, columns 511 / 512
    (1, 40, 1023)                               odd m, wide: the last lane pair's clamped load
    (1, 1024, 1024)                             the limit

Forms: the banded form (a workspace; em_band_kernel<SRC, K, Q> + em_sparse_kernel<SRC, K>) at top_k 1..4, the dense form
(em_estimate_kernel<SRC>) at top_k 1..8, banded=True at top_k 5 (no workspace exists: the dense form's bits), both
sources (EmSrcP; EmSrcDots at 256 and 512 bits, eps 0.05, on the P the same solve wrote), with and without validity
masks, n_iter 1, 2 and 30, and the fall-back into em_dense_front from a ninth candidate in a row and a ninth winner in
a column (the inputs with exactly eight of each stay sparse; both counts are asserted from the oracle first).

Every call: E within the case's bound of the fp64 oracle (essential_oracle.py: formed from the reference alone, the
margin chosen on the CPU), finite, the same bits on a second call, between guard rows that stay untouched.  Every banded
call runs on a workspace of exactly mi_essential_matrix_workspace_bytes bytes, NaN-filled, between NaN-filled guard
bands; afterwards the guards are intact and thr_row, cand_cnt, the candidate sets and col_part equal the oracle's
exactly (floats as bits).  MI_REPORT=1 prints the worst error / bound per form.
"""
import functools
import os

import numpy as np
import pytest
import torch

import essential_oracle as EO
from gpu_common import DEV, gpu, mods, twice  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

WORST = {}


def _note(form, ratio):
    WORST[form] = max(WORST.get(form, 0.0), float(ratio))
    if os.environ.get("MI_REPORT"):
        print(f"[essential] {form}: error / bound {ratio:.3g} (worst so far {WORST[form]:.3g})")


class _Out:
    """`rows` rows of `pitch` floats between two guard rows, every byte 0xFF (a NaN)."""

    def __init__(self, rows, pitch):
        self.full = torch.full(((rows + 2) * pitch,), -1, dtype=torch.int32, device=DEV).view(rows + 2, pitch)
        self.ptr = self.full[1].data_ptr()

    def read(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[0] == -1).all()), f"{what}: the row in front of the output was written"
        assert bool((self.full[-1] == -1).all()), f"{what}: the row behind the output was written"
        return self.full[1:-1].cpu().numpy().view(np.float32)


class _Work:
    """A workspace of exactly `nbytes` bytes (16-byte aligned) between two guard bands, every byte 0xFF."""
    GUARD = 4096

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.full = torch.full((nbytes + 2 * self.GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ptr = self.full.data_ptr() + self.GUARD
        assert self.ptr % 16 == 0

    def read(self, what):
        torch.cuda.synchronize()
        assert bool((self.full[:self.GUARD] == 0xFF).all()), f"{what}: bytes in front of the workspace were written"
        assert bool((self.full[self.GUARD + self.nbytes:] == 0xFF).all()), f"{what}: bytes behind the workspace were written"
        return self.full[self.GUARD: self.GUARD + self.nbytes].cpu().numpy()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(src, dims, pts, masks, top_k, n_iter, banded):
    """One poisoned call of mi_essential_matrix (src = ("p", P)) or mi_essential_matrix_dots (src = ("dots", dots,
    row_info, col_info, pitch, u, v)): (E (b, 3, 3), the workspace's bytes or None)."""
    from onnx_image_processing_amd import _native as N
    batch, n, m = dims
    wbytes = int(N.load().mi_essential_matrix_workspace_bytes(batch, n, m, top_k)) if banded else 0
    assert (wbytes > 0) == (banded and top_k <= 4)
    if wbytes:
        assert wbytes == EO.workspace_layout(batch, n, m, top_k)[1]
    work = _Work(wbytes) if wbytes else None
    e = _Out(batch, 9)
    tail = (batch, n, m, pts[0].data_ptr(), pts[1].data_ptr(), _ptr(masks[0]), _ptr(masks[1]), top_k, n_iter,
            EO.N_ITER_MANIFOLD, e.ptr, work.ptr if work else None, wbytes, N.stream_ptr())
    if src[0] == "p":
        N.call("mi_essential_matrix", src[1].data_ptr(), *tail)
    else:
        _, dots, ri, ci, pitch, u, v = src
        N.call("mi_essential_matrix_dots", dots.data_ptr(), ri.data_ptr(), ci.data_ptr(), pitch, 0.05, u.data_ptr(), v.data_ptr(), *tail)
    what = f"{src[0]} {dims} top_k {top_k} banded {banded}"
    return e.read(what).reshape(batch, 3, 3), (work.read(what) if work else None)


def _twice(*args):
    return twice("E and the workspace", lambda: _call(*args))


def _check_e(e, refs, form):
    assert np.isfinite(e).all()
    for b, ref in enumerate(refs):
        err = np.abs(e[b].astype(np.float64) - ref["E"]).max()
        _note(form(ref), err / ref["bound"])
        assert err <= ref["bound"], (b, err, ref["bound"], err / ref["bound"])


def _check_stages(work, refs, dims, top_k):
    """thr_row, cand_cnt, the candidate sets and col_part of a banded call against the oracle, exactly."""
    batch, n, m = dims
    offs, total = EO.workspace_layout(batch, n, m, top_k)
    nb = -(-n // EO.BAND_ROWS)
    assert work.nbytes == total
    take = lambda k, count, dtype: work[offs[k]: offs[k] + count * np.dtype(dtype).itemsize].view(dtype)  # noqa: E731
    thr_row = take(0, batch * n, np.uint32).reshape(batch, n)
    cand_cnt = take(1, batch * n, np.uint8).reshape(batch, n)
    cand_j = take(2, batch * n * 8, np.int32).reshape(batch, n, 8)
    cand_x = take(3, batch * n * 8, np.uint32).reshape(batch, n, 8)
    col_part = take(4, batch * nb * m * top_k, np.uint32).reshape(batch, nb, m, top_k)
    for b, ref in enumerate(refs):
        assert np.array_equal(thr_row[b], ref["thr_row"].view(np.uint32)), (b, "thr_row")
        assert np.array_equal(cand_cnt[b], ref["cand_cnt"]), (b, "cand_cnt", np.flatnonzero(cand_cnt[b] != ref["cand_cnt"])[:8])
        assert ((ref["cnt"] > 8) == (cand_cnt[b] == 255)).all()
        assert np.array_equal(col_part[b], ref["col_part"].view(np.uint32)), (b, "col_part")
        kept = ref["cnt"] <= 8
        slots = (np.arange(8)[None, :] < ref["cnt"][:, None]) & kept[:, None]
        ii, jj = np.nonzero(slots)[0], cand_j[b][slots]
        assert ((jj >= 0) & (jj < m)).all(), (b, "candidate column out of range")
        seen = np.zeros((n, m), np.int32)
        np.add.at(seen, (ii, jj), 1)
        assert seen.max(initial=0) <= 1, (b, "a candidate is listed twice")
        got = np.zeros((n, m), np.uint32)
        got[ii, jj] = cand_x[b][slots]
        want = np.where(ref["cand"] & kept[:, None], ref["core"], np.float32(0.0)).astype(np.float32).view(np.uint32)
        assert np.array_equal(got, want), (b, "candidate sets", np.argwhere(got != want)[:8])


def _band_form(dims):
    return "banded Q=16" if dims[2] > 512 else "banded Q=8"


# ------------------------------------------------------------------ the P source
def _p_inputs(batch, n, m, top_k, variant, masked):
    c = EO.p_case(batch, n, m, top_k, variant)
    masks = (gpu(c["valid1"].view(np.uint8)), gpu(c["valid2"].view(np.uint8))) if masked else (None, None)
    return ("p", gpu(c["p"])), (gpu(c["pts1"]), gpu(c["pts2"])), masks


def _p_keys():
    return [k for k in EO.p_cases() if k[5] == "base" and k[6] == EO.N_ITER]


@pytest.mark.parametrize("key", _p_keys(), ids=lambda k: f"{k[0]}x{k[1]}x{k[2]}-k{k[3]}-{'masked' if k[4] else 'plain'}")
def test_p_source_against_the_oracle(mods, key):
    batch, n, m, top_k, masked, variant, n_iter = key
    dims = (batch, n, m)
    refs = EO.reference(*key)
    src, pts, masks = _p_inputs(batch, n, m, top_k, variant, masked)
    e_dense, _ = _twice(src, dims, pts, masks, top_k, n_iter, False)
    _check_e(e_dense, refs, lambda ref: "dense P")
    if top_k <= 4:
        assert not any(ref["dense"] for ref in refs)                       # these inputs stay on the sparse path
        e_band, work = _twice(src, dims, pts, masks, top_k, n_iter, True)
        _check_e(e_band, refs, lambda ref: _band_form(dims))
        _check_stages(work, refs, dims, top_k)
    if top_k == 5:                                                         # no banded form: the dense form's bits
        from onnx_image_processing_amd import ops
        mk = [None if x is None else x.view(torch.bool) for x in masks]
        e5 = ops.essential_matrix(src[1], pts[0], pts[1], mk[0], mk[1], 5, n_iter, EO.N_ITER_MANIFOLD, banded=True).cpu().numpy()
        assert np.array_equal(e5.view(np.uint32), e_dense.view(np.uint32))
        e5b, none = _call(src, dims, pts, masks, 5, n_iter, True)
        assert none is None and np.array_equal(e5b.view(np.uint32), e_dense.view(np.uint32))


@pytest.mark.parametrize("n_iter", (1, 2))
@pytest.mark.parametrize("shape", EO.ITER_SHAPES, ids=str)
def test_iteration_counts_one_and_two(mods, shape, n_iter):
    key = shape + (3, False, "base", n_iter)
    refs = EO.reference(*key)
    src, pts, masks = _p_inputs(*shape, 3, "base", False)
    for banded in (False, True):
        e, _ = _twice(src, shape, pts, masks, 3, n_iter, banded)
        _check_e(e, refs, lambda ref: f"n_iter {n_iter}")


@pytest.mark.parametrize("top_k", (1, 3, 4))
@pytest.mark.parametrize("variant", ("row9", "col9"))
@pytest.mark.parametrize("shape", EO.VARIANT_SHAPES, ids=str)
def test_ninth_candidate_and_ninth_winner_fall_back_to_the_dense_front(mods, shape, variant, top_k):
    """Exactly 8 candidates in a row / 8 winners in a column stay sparse (the base inputs above); 9 send the pair through
    em_dense_front inside em_sparse_kernel.  The counts are asserted from the oracle before the GPU is asked."""
    batch, n, m = shape
    for ref, meta, base in zip(EO.reference(*shape, top_k, False, variant), EO.p_case(*shape, top_k, variant)["meta"],
                               EO.reference(*shape, top_k, False, "base")):
        assert base["cnt"][meta["row8"]] == 8 and base["col_cnt"][meta["col8"]] == 8 and not base["dense"]
        assert ref["cnt"][meta["row8"]] == (9 if variant == "row9" else 8) and ref["col_cnt"][meta["col8"]] == (9 if variant == "col9" else 8)
        assert ref["dense"] and (ref["cand_cnt"][meta["row8"]] == 255) == (variant == "row9")
    refs = EO.reference(*shape, top_k, False, variant)
    src, pts, masks = _p_inputs(batch, n, m, top_k, variant, False)
    e, work = _twice(src, shape, pts, masks, top_k, EO.N_ITER, True)
    _check_e(e, refs, lambda ref: "fall-back")
    _check_stages(work, refs, shape, top_k)
    e_dense, _ = _call(src, shape, pts, masks, top_k, EO.N_ITER, False)
    _check_e(e_dense, refs, lambda ref: "dense P")


# ------------------------------------------------------------------ the dots source
@functools.lru_cache(maxsize=None)
def _dots_solution(batch, n, m, bits):
    """sinkhorn_bits on dots_case: the P it wrote (numpy), and on the device the dots at the solver's pitch and at a
    pitch 8 columns wider with 0xFFFF in columns m..pitch, row / column info and the duals."""
    from onnx_image_processing_amd import ops
    c = EO.dots_case(batch, n, m, bits)
    t1, t2 = gpu(c["b1"].view(np.int32)), gpu(c["b2"].view(np.int32))
    p, u, v, state = ops.sinkhorn_bits(t1, t2, True, 0.05, 1.0, 20, want_p=True, return_state=True)
    dots, ri, ci, pitch = state[:4]
    wide = torch.full((batch, n, pitch + 8), -1, dtype=torch.int16, device=DEV)
    wide[:, :, :m] = dots[:, :, :m]
    torch.cuda.synchronize()
    p_np = p.cpu().numpy()
    assert np.isfinite(p_np).all()
    return dict(case=c, p=p_np, tight=("dots", dots, ri, ci, pitch, u, v), wide=("dots", wide, ri, ci, pitch + 8, u, v),
                pts=(gpu(c["pts1"]), gpu(c["pts2"])), masks=(gpu(c["valid1"].view(np.uint8)), gpu(c["valid2"].view(np.uint8))),
                keep=state)


_DOTS_KEYS = [(c, masked, k) for c in EO.DOTS_CASES for masked in (False, True) for k in EO.DOTS_TOP_K if k <= min(c[0][1:])]


@pytest.mark.parametrize("bits_case,masked,top_k", _DOTS_KEYS,
                         ids=lambda v: v if not isinstance(v, tuple) else f"{v[0][0]}x{v[0][1]}x{v[0][2]}-{v[1]}bits")
def test_dots_source_against_the_oracle(mods, bits_case, masked, top_k):
    """mi_essential_matrix_dots against the oracle run on the P the same mi_sinkhorn_dots call wrote (that write is held
    by tests/test_gpu_sinkhorn.py), and the call on a wider, 0xFFFF-padded pitch against the tight one, bit for bit."""
    dims, bits = bits_case
    batch, n, m = dims
    s = _dots_solution(batch, n, m, bits)
    c = s["case"]
    masks = s["masks"] if masked else (None, None)
    refs = [EO.reference_pair(s["p"][b], c["valid1"][b] if masked else None, c["valid2"][b] if masked else None,
                              c["pts1"][b], c["pts2"][b], top_k) for b in range(batch)]
    for b, ref in enumerate(refs):                                     # the condition, on the P this GPU wrote
        shift = EO.one_weight_shift(ref["weights"], c["pts1"][b], c["pts2"][b])
        assert shift >= EO.CONDITION * ref["bound"], (top_k, b, shift / ref["bound"])
    e_dense, _ = _twice(s["tight"], dims, s["pts"], masks, top_k, EO.N_ITER, False)
    _check_e(e_dense, refs, lambda ref: "dense dots")
    e_wide, _ = _call(s["wide"], dims, s["pts"], masks, top_k, EO.N_ITER, False)
    assert np.array_equal(e_wide.view(np.uint32), e_dense.view(np.uint32)), (top_k, "dense form, wide pitch")
    if top_k <= 4:
        e_band, work = _twice(s["tight"], dims, s["pts"], masks, top_k, EO.N_ITER, True)
        _check_e(e_band, refs, lambda ref: "fall-back" if ref["dense"] else _band_form(dims))
        _check_stages(work, refs, dims, top_k)
        e_wide, work_wide = _call(s["wide"], dims, s["pts"], masks, top_k, EO.N_ITER, True)
        assert np.array_equal(e_wide.view(np.uint32), e_band.view(np.uint32)), (top_k, "banded form, wide pitch")
        _check_stages(work_wide, refs, dims, top_k)
    elif top_k == 5:
        e5, none = _call(s["tight"], dims, s["pts"], masks, 5, EO.N_ITER, True)
        assert none is None and np.array_equal(e5.view(np.uint32), e_dense.view(np.uint32))


# ------------------------------------------------------------------ mi_normalise_keypoints
@pytest.mark.parametrize("count", (1, 255, 256, 257))
def test_normalise_keypoints_against_fp64(mods, count):
    """(y, x) pixels -> K^-1 [x, y, 1]: within 3 roundings of |x k0| + |y k1| + |k2| (two products, two sums, or two
    fused steps and one), per coordinate; the output sits between guard rows."""
    from onnx_image_processing_amd import _native as N
    rng = np.random.default_rng(count)
    kp = (rng.random((count, 2)) * [480.0, 640.0]).astype(np.float32)
    k_inv = np.linalg.inv(np.array([[500.0, 0.3, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]])).astype(np.float32)
    out = _Out(count, 2)
    kp_dev, k_dev = gpu(kp), gpu(k_inv)
    N.call("mi_normalise_keypoints", kp_dev.data_ptr(), count, k_dev.data_ptr(), out.ptr, N.stream_ptr())
    got = out.read("mi_normalise_keypoints").astype(np.float64)
    y, x, k = kp[:, 0].astype(np.float64), kp[:, 1].astype(np.float64), k_inv.astype(np.float64)
    for r in range(2):
        want = x * k[r, 0] + y * k[r, 1] + k[r, 2]
        scale = np.abs(x * k[r, 0]) + np.abs(y * k[r, 1]) + np.abs(k[r, 2])
        assert (np.abs(got[:, r] - want) <= 3 * EO.U * scale).all(), (r, (np.abs(got[:, r] - want) / scale).max() / EO.U)
