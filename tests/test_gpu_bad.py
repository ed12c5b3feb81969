"""The BAD descriptors (K4 csrc/bad.hip, K4o csrc/bad_oriented.hip) against fp64 at every dispatch of their entry
points.

The reference, the bounds, the firm / fragile rule and the inputs are tests/bad_oracle.py's (test_bad_host.py checks
that file against the project's other oracle and the inputs against the fragile caps).  Bits must be the reference's on
firm pairs and a candidate's on fragile ones; floats lie within the a-priori bounds; nothing is fitted to a measurement.

Every call goes through _native.call with outputs that carry a guard row of sentinels at each end, and a status array
with guards of its own; every call runs twice and must repeat bit for bit.  For every table the fast and the general
path must give the same bytes.  MI_REPORT=1 prints the worst error / bound.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import bad_oracle as B
from gpu_common import DEV, mods, twice  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

BITS_FILL, STATUS_FILL = 0x5A5A5A5A, 0xEE
FORM = {B.RAW: "raw", B.SOFT: "soft", B.HARD: "hard"}
ids = dict(ids=lambda c: c["name"])


def _report(what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[bad] {what}: worst error / bound {ratio:.3g}")


# ------------------------------------------------------------------ guarded buffers
class _Out:
    """`rows` rows of `pitch` 4-byte elements between two guard rows, all holding the sentinel (NaN / BITS_FILL); the
    payload's base is `misalign` bytes past a 16-byte boundary."""

    def __init__(self, rows, pitch, dtype, misalign=0):
        self.fill = float("nan") if dtype == torch.float32 else BITS_FILL
        self.flat = torch.full(((rows + 2) * pitch + 8,), self.fill, dtype=dtype, device=DEV)
        start = ((misalign - (self.flat.data_ptr() + 4 * pitch)) % 16) // 4
        self.full = self.flat[start:start + (rows + 2) * pitch].view(rows + 2, pitch)
        self.ptr = self.full[1].data_ptr()
        assert self.ptr % 16 == misalign

    def _kept(self, t):
        return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == BITS_FILL).all())

    def read(self, what):
        torch.cuda.synchronize()
        assert self._kept(self.full[0]) and self._kept(self.full[-1]), f"{what}: a guard row of the output was written"
        body = self.full[1:-1].cpu().numpy()
        return body if body.dtype == np.float32 else body.view(np.uint32)


class _Status:
    def __init__(self, total):
        self.total = total
        self.full = torch.full((total + 128,), STATUS_FILL, dtype=torch.uint8, device=DEV)
        self.ptr = self.full.data_ptr() + 64

    def read(self, what):
        torch.cuda.synchronize()
        s = self.full.cpu().numpy()
        assert (s[:64] == STATUS_FILL).all() and (s[64 + self.total:] == STATUS_FILL).all(), f"{what}: status guard written"
        return s[64:64 + self.total]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the cases' arrays are read-only


_plans = {}


def _plan(N, table):
    """The fast path's device plan of a table, 16-byte aligned, built once."""
    if table not in _plans:
        box, thr = B.table(table)
        geom, thr_d = _dev(B.pack_geom(box).view(np.int32)), _dev(thr)
        buf = torch.zeros(int(N.load().mi_bad_plan_bytes(len(thr))) + 16, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        N.call("mi_bad_plan_build", geom.data_ptr(), thr_d.data_ptr(), len(thr), buf.data_ptr(), N.stream_ptr())
        torch.cuda.synchronize()
        _plans[table] = buf
    return _plans[table]


# ------------------------------------------------------------------ the calls
def _plain(N, case, mode, normalize, want_desc, want_bits, plan=False, u8=False, pair=False):
    """mi_sparse_bad / _u8 / _pair on a case: desc (b, k, P) float32 or None, bits (b, k, P) bool or None, status (b k,)
    uint8 or None (with a plan only)."""
    x = B.inputs(case)
    b, h, w, k, pairs = case["b"], case["h"], case["w"], case["k"], len(x["thr"])
    img = x["image"].astype(np.uint8) if u8 else x["image"]
    if u8:
        assert np.array_equal(img.astype(np.float32), x["image"]), "the u8 entry needs a uint8-valued case"
    parts = [_dev(img[:b // 2]), _dev(img[b // 2:])] if pair else [_dev(img)]
    kp, geom, thr = _dev(x["kp"]), _dev(x["geom"].view(np.int32)), _dev(x["thr"])
    plan_ptr = _plan(N, case["table"]).data_ptr() if plan else None
    what = f"{case['name']} mode {mode} norm {int(normalize)} plan {int(plan)} u8 {int(u8)} pair {int(pair)}"

    def run():
        desc = _Out(b * k, pairs, torch.float32) if want_desc else None
        bits = _Out(b * k, pairs // 32, torch.int32) if want_bits else None
        status = _Status(b * k) if plan else None
        tail = (geom.data_ptr(), thr.data_ptr(), pairs, mode, float(B.TEMPERATURE), int(normalize),
                desc.ptr if desc else None, bits.ptr if bits else None, plan_ptr, status.ptr if status else None, N.stream_ptr())
        if pair:
            assert b % 2 == 0
            N.call("mi_sparse_bad_pair", parts[0].data_ptr(), parts[1].data_ptr(), int(u8), b // 2, h, w, kp.data_ptr(), k, *tail)
        else:
            N.call("mi_sparse_bad_u8" if u8 else "mi_sparse_bad", parts[0].data_ptr(), b, h, w, kp.data_ptr(), k, *tail)
        return (desc.read(what) if desc else None, bits.read(what) if bits else None, status.read(what) if status else None)
    desc, bits, status = twice(what, run)
    if desc is not None:
        desc = desc.reshape(b, k, pairs)
    if bits is not None:
        bits = B.unpack_bits(bits, pairs).reshape(b, k, pairs)
    return desc, bits, status


def _oriented(N, case, mode, normalize, want_desc, want_bits, status=True, misalign=0, pair=False):
    """mi_sparse_bad_oriented / _pair on a case: desc, bits as _plain."""
    x = B.inputs(case)
    b, h, w, k, pairs = case["b"], case["h"], case["w"], case["k"], len(x["thr"])
    parts = [_dev(x["image"][:b // 2]), _dev(x["image"][b // 2:])] if pair else [_dev(x["image"])]
    kp, geom, thr = _dev(x["kp"]), _dev(x["geom"].view(np.int32)), _dev(x["thr"])
    amap = _dev(x["amap"]) if x["amap"] is not None else None
    akp = None if amap is not None else _dev(x["theta"])
    max_reach = 0.0 if case["wide_window"] and not case["table"].startswith("wide") else B.reach(x["box"])
    assert (max_reach == 0.0 or max_reach > 22.5) == case["wide_window"]
    what = (f"{case['name']} mode {mode} norm {int(normalize)} status {int(status)} bits base +{misalign} pair {int(pair)}")

    def run():
        desc = _Out(b * k, pairs, torch.float32) if want_desc else None
        bits = _Out(b * k, pairs // 32, torch.int32, misalign) if want_bits else None
        st = _Status(b * k) if status else None
        tail = (geom.data_ptr(), thr.data_ptr(), pairs, mode, float(B.TEMPERATURE), int(normalize), int(case["bilinear"]),
                float(max_reach), desc.ptr if desc else None, bits.ptr if bits else None, st.ptr if st else None, N.stream_ptr())
        if pair:
            N.call("mi_sparse_bad_oriented_pair", parts[0].data_ptr(), parts[1].data_ptr(), b // 2, h, w, kp.data_ptr(), k,
                   akp.data_ptr(), *tail)
        else:
            N.call("mi_sparse_bad_oriented", parts[0].data_ptr(), b, h, w, kp.data_ptr(), k,
                   amap.data_ptr() if amap is not None else None, akp.data_ptr() if akp is not None else None, *tail)
        out = (desc.read(what) if desc else None, bits.read(what) if bits else None)
        if st:
            assert np.isin(st.read(what), (0, 1)).all(), f"{what}: a status byte is neither 0 nor 1"
        return out
    desc, bits = twice(what, run)
    if desc is not None:
        desc = desc.reshape(b, k, pairs)
    if bits is not None:
        bits = B.unpack_bits(bits, pairs).reshape(b, k, pairs)
    return desc, bits


# ------------------------------------------------------------------ the comparison
def _check_float(case, what, mode, desc, plain=None):
    """An un-normalised descriptor against the candidates; a normalised one (plain: the same call's un-normalised
    output) against the fp64 normalisation of `plain`, and with nearest sampling, on keypoints without fragile pairs,
    against the reference's own normalised form as well."""
    ref = B.expected(case)
    assert np.isfinite(desc).all(), f"{what}: not finite"
    assert (desc[~ref["valid"]] == 0).all(), f"{what}: an invalid keypoint's descriptor is not zero"
    if plain is None:
        ratio = B.float_ratio(ref, desc, FORM[mode])
    else:
        ratio = B.normalised_ratio(desc, plain, mode == B.HARD)
        rows = ref["firm"].all(-1) & ~ref["fragile"].any(-1)
        if not case["bilinear"]:                      # (bilinear: every value moves with the sine; the chain above holds it)
            value, bound = B.forms(ref)[FORM[mode] + "_n"]
            ratio = max(ratio, B.worst_ratio(desc[rows], value[rows], bound[rows]))
    _report(what, ratio)
    assert ratio <= 1.0, f"{what}: error {ratio:.3g} times the bound"


def _same(what, a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            same = np.array_equal(x.view(np.uint8), y.view(np.uint8))
            assert same, f"{what}: the two paths give different bytes"


def _all_float_forms(case, label, call):
    """call(mode, normalize, want_desc, want_bits) -> (desc, bits, ...): raw, soft and hard, plain and normalised, and in
    the hard mode desc only, bits only and both together.  Returns every output, keyed, for path-against-path checks."""
    ref, outs = B.expected(case), {}
    for mode in (B.RAW, B.SOFT, B.HARD):
        plain = call(mode, False, True, False)[0]
        _check_float(case, f"{label} {FORM[mode]}", mode, plain)
        normed = call(mode, True, True, False)[0]
        _check_float(case, f"{label} {FORM[mode]} normalised", mode, normed, plain)
        outs[mode, 0], outs[mode, 1] = plain, normed
    bits = call(B.HARD, True, False, True)[1]
    B.check_bits(ref, bits, f"{label} bits")
    both_desc, both_bits = call(B.HARD, False, True, True)[:2]
    B.check_bits(ref, both_bits, f"{label} desc + bits")
    assert np.array_equal(both_desc != 0, both_bits) and np.isin(both_desc, (0.0, 1.0)).all(), f"{label}: desc and bits disagree"
    if not ref["fragile"].any():
        assert np.array_equal(bits, ref["bits"]) and np.array_equal(both_bits, ref["bits"])
    outs["bits"], outs["both"] = bits, (both_desc, both_bits)
    return outs


# ------------------------------------------------------------------ K4: mi_sparse_bad, _u8, _pair
def _expected_status(case, u8):
    """With a plan, on an image whose windows are all uint8-valued: 1 = the fast kernel's (an invalid keypoint, or a
    pixel of the image), 0 = flagged for the general kernel -- among them every valid keypoint with x < 0."""
    kp = B.inputs(case)["kp"].reshape(-1, 2)
    y, x = kp[:, 0], kp[:, 1]
    onpixel = (y == np.floor(y)) & (x == np.floor(x)) & (x >= 0) & (y <= case["h"] - 1) & (x <= case["w"] - 1)
    return np.where(~(y >= 0) | onpixel, 1, 0).astype(np.uint8)


@pytest.mark.parametrize("case", B.PLAIN_CASES, **ids)
def test_general_kernel_vs_fp64(mods, case):
    """No plan: sparse_bad_kernel with one wave per keypoint, every mode and output combination, every table size (the
    rolled group loop from 576 pairs on)."""
    from onnx_image_processing_amd import _native as N
    _all_float_forms(case, case["name"] + " general", lambda *a: _plain(N, case, *a))
    if case["image"] in ("u8", "const"):
        outs = _all_float_forms(case, case["name"] + " general u8", lambda *a: _plain(N, case, *a, u8=True))
        _same(case["name"] + " u8 against float pixels", (outs["bits"], outs[B.RAW, 0]),
              (_plain(N, case, B.HARD, True, False, True)[1], _plain(N, case, B.RAW, False, True, False)[0]))


@pytest.mark.parametrize("case", B.PLAIN_CASES, **ids)
def test_fast_kernel_and_chunked_general_kernel_vs_fp64(mods, case):
    """With a plan: bad_fast_kernel<8>, <4> or <0> (float and uint8 pixels) and the chunked general kernel behind it.
    Same bytes as without a plan; which kernel took a keypoint is read from the status array.  Below 32 pixels (31x64,
    8x8) the fast path must not run at all: the status array keeps its sentinel."""
    from onnx_image_processing_amd import _native as N
    ref = B.expected(case)
    fast_runs = case["h"] >= 32 and case["w"] >= 32
    for u8 in ((False, True) if case["image"] in ("u8", "const") else (False,)):
        label = f"{case['name']} plan{' u8' if u8 else ''}"
        for normalize, want_desc, want_bits in ((True, False, True), (False, True, False), (True, True, False), (False, True, True)):
            desc, bits, status = _plain(N, case, B.HARD, normalize, want_desc, want_bits, plan=True, u8=u8)
            _same(label, (desc, bits), _plain(N, case, B.HARD, normalize, want_desc, want_bits, u8=u8)[:2])
            if bits is not None:
                B.check_bits(ref, bits, label)
                assert np.array_equal(bits, ref["bits"]) or ref["fragile"].any()
            if desc is not None and not normalize:
                _check_float(case, label + " hard", B.HARD, desc)
            if not fast_runs:
                assert (status == STATUS_FILL).all(), f"{label}: the fast path ran on a {case['h']}x{case['w']} image"
            else:
                assert np.isin(status, (0, 1)).all()
                if case["image"] in ("u8", "const"):
                    assert np.array_equal(status, _expected_status(case, u8)), f"{label}: the wrong keypoints were flagged"
        if fast_runs and case["kps"] == "chunks":
            assert (status[:16] == 1).all() and (status[16:32] == 0).all()     # a chunk with nothing, one with all flagged
    if fast_runs and case["image"] == "mixed" and case["k"] > 1:
        assert (status == 0).any() and (status == 1).any()
    # modes that have no fast kernel go to the one-wave-per-keypoint form even with a plan and a status array
    desc, _, status = _plain(N, case, B.RAW, False, True, False, plan=True)
    assert (status == STATUS_FILL).all()
    _check_float(case, case["name"] + " plan raw", B.RAW, desc)


@pytest.mark.parametrize("name,u8", [("learned512-mixed-64x80", False), ("learned512-u8-64x80-chunks", True),
                                     ("syn320-u8-64x80-chunks", True), ("syn128-u8-31x64", False)])
def test_pair_entry_vs_fp64(mods, name, u8):
    """mi_sparse_bad_pair: two base pointers, keypoints and outputs of both batches behind one launch."""
    from onnx_image_processing_amd import _native as N
    case = B.CASE[name]
    outs = _all_float_forms(case, name + " pair", lambda *a: _plain(N, case, *a, u8=u8, pair=True))
    for normalize, want_desc, want_bits in ((True, False, True), (True, True, False)):
        desc, bits, _ = _plain(N, case, B.HARD, normalize, want_desc, want_bits, plan=True, u8=u8, pair=True)
        _same(name + " pair, plan", (desc, bits), (outs[B.HARD, 1] if want_desc else None, outs["bits"] if want_bits else None))


# ------------------------------------------------------------------ K4o: mi_sparse_bad_oriented, _pair
@pytest.mark.parametrize("case", B.ORIENTED_CASES, **ids)
def test_oriented_fp64_kernel_vs_fp64(mods, case):
    """status = NULL: bad_oriented_kernel<double, DESC, 48 | 60> for every keypoint, nearest and bilinear."""
    from onnx_image_processing_amd import _native as N
    if os.environ.get("MI_REPORT"):
        print(f"[bad] {case['name']}: {100 * B.fragile_share(B.expected(case)):.3f} % fragile pairs")
    _all_float_forms(case, case["name"] + " no status", lambda *a: _oriented(N, case, *a, status=False))


@pytest.mark.parametrize("case", B.ORIENTED_CASES, **ids)
def test_oriented_two_pass_kernels_vs_fp64(mods, case):
    """With a status array.  256 / 512 pairs, nearest: bad_oriented_bits_kernel<48 | 60, 4 | 8, DESC> and the fp64 rest
    kernel; any other table, bilinear sampling, desc and bits together, or a bits base off 16 bytes:
    bad_oriented_kernel<int, ., .> (BO_PICK(int)) and the rest kernel.  Each against fp64, and byte for byte against the
    generic kernel that debug key 13 selects."""
    from onnx_image_processing_amd import _native as N
    ref = B.expected(case)
    outs = _all_float_forms(case, case["name"], lambda *a: _oriented(N, case, *a))
    shifted = _oriented(N, case, B.HARD, True, False, True, misalign=4)[1]
    B.check_bits(ref, shifted, case["name"] + " bits base + 4")
    assert np.array_equal(shifted, outs["bits"])
    with N.debug_library() as lib:
        assert lib.mi_debug_set(13, 1) == 0
        for (mode, normalize), fast in [(key, v) for key, v in outs.items() if isinstance(key, tuple)]:
            _same(f"{case['name']} {FORM[mode]} norm {normalize} against the generic kernel",
                  (fast,), (_oriented(N, case, mode, bool(normalize), True, False)[0],))
        _same(case["name"] + " bits against the generic kernel", (outs["bits"],), (_oriented(N, case, B.HARD, True, False, True)[1],))


@pytest.mark.parametrize("name", ["learned512-mixed-48", "learned256-mixed-60", "syn128-mixed-48", "learned512-mixed-bilinear"])
def test_oriented_pair_entry_vs_fp64(mods, name):
    from onnx_image_processing_amd import _native as N
    case = B.CASE[name]
    outs = _all_float_forms(case, name + " pair", lambda *a: _oriented(N, case, *a, pair=True))
    _same(name + " pair against one base pointer", (outs["bits"], outs[B.RAW, 0]),
          (_oriented(N, case, B.HARD, True, False, True)[1], _oriented(N, case, B.RAW, False, True, False)[0]))
    no_status = _oriented(N, case, B.HARD, True, False, True, status=False, pair=True)[1]
    B.check_bits(B.expected(case), no_status, name + " pair, no status")
