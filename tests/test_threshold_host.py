"""CPU-only checks of the K14 thresholds: the reference's import lines resolve, the modules keep the reference's
constructor contract and refuse CPU tensors, the C entries refuse bad arguments on the host before any launch, and three
numpy oracles (written here, independent of the kernels) reproduce the fixture made by running the reference
(tests/golden/make_golden_threshold.py):

  histogram   np.bincount of v - min_val over the counted values (float32 truncated toward zero; out-of-range values,
              NaN and floats beyond int32 dropped);
  Otsu        int64 cumulative sums, then the float32 score in the order include/mi355x_match.h states, first maximum:
              the reference's thresh EXACTLY on every Otsu case (no allowance);
  multi-Otsu  every combination in itertools.combinations order, class sums from int64 prefix sums, the fp64 score in the
              header's fixed order, first maximum: the reference's thresholds on every case that does not carry the
              fixture's `differs` flag.  The reference sums float32 products in an order its backend chooses, so a near-tie
              may fall the other way; such a case stays in the fixture with the flag, the test asserts that the fp64 score
              at the oracle's choice is >= the fp64 score at the reference's choice, and at most 1 case in 20 may carry it.

The GPU tests then hold the kernels to these oracles exactly."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from helpers import native_lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "threshold.npz")
F32 = np.float32


def hist_oracle(frame, min_val, bins):
    """int64 (bins,): counts of v - min_val over one frame of any accepted dtype"""
    v = np.asarray(frame).reshape(-1)
    if v.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            v = v[np.abs(v) < 2147483648.0]                      # drops NaN and the infinities as well
        v = np.trunc(v)
    d = v.astype(np.int64) - int(min_val)
    d = d[(d >= 0) & (d < bins)]
    return np.bincount(d, minlength=bins).astype(np.int64)


def otsu_oracle(hist, min_val):
    """thresh (python int) of one int64 histogram whose bin i holds the value min_val + i; also the float32 scores"""
    hist = np.asarray(hist, np.int64)
    vals = np.arange(hist.size, dtype=np.int64) + int(min_val)
    num_bk = np.cumsum(hist)
    fc_bk = np.cumsum(hist * vals)
    num_wh = num_bk[-1] - num_bk
    fc_wh = fc_bk[-1] - fc_bk
    with np.errstate(all="ignore"):
        mean_bk = fc_bk.astype(F32) / num_bk.astype(F32)
        mean_wh = fc_wh.astype(F32) / num_wh.astype(F32)
        d = mean_bk - mean_wh
        var = (num_bk * num_wh).astype(F32) * (d * d)
    assert var.dtype == F32
    var = np.where(np.isnan(var), F32(0), var)
    return int(min_val) + int(np.argmax(var)), var


_COMBOS = {}


def combinations_lex(m, k):
    """(C(m, k), k) int32: the k-subsets of {1 .. m} in lexicographic order, built without a Python loop over subsets:
    the subsets that start with a are a followed by the (k-1)-subsets whose first element exceeds a, and those are a
    suffix of the lexicographically ordered (k-1)-subsets."""
    if (m, k) in _COMBOS:
        return _COMBOS[(m, k)]
    if k == 1:
        out = np.arange(1, m + 1, dtype=np.int32)[:, None]
    else:
        tails = combinations_lex(m, k - 1)
        starts = np.searchsorted(tails[:, 0], np.arange(1, m + 1), side="right")     # first tail with element 0 > a
        parts = [np.concatenate([np.full((len(tails) - s, 1), a, np.int32), tails[s:]], axis=1)
                 for a, s in zip(range(1, m + 1), starts) if s < len(tails)]
        out = np.concatenate(parts, axis=0)
    assert out.shape == (math.comb(m, k), k)
    _COMBOS[(m, k)] = out
    return out


def multi_otsu_scores(hist, min_val, combos):
    """fp64 scores (len(combos),) of threshold tuples `combos` (rows 1 <= th_1 < ... <= bins - 1), in the header's order"""
    hist = np.asarray(hist, np.int64)
    bins = hist.size
    vals = np.arange(bins, dtype=np.int64) + int(min_val)
    pn = np.concatenate([[0], np.cumsum(hist)]).astype(np.int64)
    ps = np.concatenate([[0], np.cumsum(hist * vals)]).astype(np.int64)
    combos = np.asarray(combos, np.int64).reshape(-1, np.asarray(combos).shape[-1])
    n_class = combos.shape[1] + 1
    bounds = np.concatenate([np.zeros((len(combos), 1), np.int64), combos, np.full((len(combos), 1), bins, np.int64)], axis=1)
    n = [pn[bounds[:, i + 1]] - pn[bounds[:, i]] for i in range(n_class)]
    s = [ps[bounds[:, i + 1]] - ps[bounds[:, i]] for i in range(n_class)]
    with np.errstate(all="ignore"):
        m = [s[i].astype(np.float64) / n[i].astype(np.float64) for i in range(n_class)]
        v = np.zeros(len(combos), np.float64)
        for i, j in itertools.combinations(range(n_class), 2):
            d = m[i] - m[j]
            v = v + (n[i].astype(np.float64) * n[j].astype(np.float64)) * (d * d)
    empty = np.zeros(len(combos), bool)
    for i in range(n_class):
        empty |= n[i] == 0
    return np.where(empty, 0.0, v)


def multi_otsu_oracle(hist, min_val, n_class):
    """the n_class - 1 thresholds (list of python ints, inclusive upper bounds) of one int64 histogram"""
    bins = np.asarray(hist).size
    combos = combinations_lex(bins - 1, n_class - 1)
    best = int(np.argmax(multi_otsu_scores(hist, min_val, combos)))          # the first maximum
    return [int(min_val) + int(t) - 1 for t in combos[best]]


def apply_oracle(frame, thresholds):
    """uint8 labels: the number of thresholds t with v > t, compared in the frame's own type"""
    f = np.asarray(frame)
    f = f if f.dtype.kind == "f" else f.astype(np.int64)
    out = np.zeros(f.shape, np.uint8)
    for t in thresholds:
        with np.errstate(invalid="ignore"):
            out += (f > (F32(t) if f.dtype.kind == "f" else int(t))).astype(np.uint8)
    return out


def binary_oracle(frame, thresh, low, high, dtype):
    f = np.asarray(frame)
    f = f if f.dtype.kind == "f" else f.astype(np.int64)
    with np.errstate(invalid="ignore"):
        below = f <= (F32(thresh) if f.dtype.kind == "f" else int(thresh))
    return np.where(below, low, high).astype(dtype)


def golden():
    return np.load(GOLDEN)


def otsu_cases(g):
    return [str(n) for n in g["meta__otsu_cases"]]


def multi_cases(g):
    return [str(n) for n in g["meta__multi_cases"]]


# ---- the modules' contract -----------------------------------------------------------------------------------------

def test_reference_import_lines_resolve():
    from pytorch_model.threshold.otsu import OtsuThreshold
    from pytorch_model.threshold.multi_otsu import MultiOtsuThreshold
    from pytorch_model.threshold import OtsuThreshold as A, MultiOtsuThreshold as B
    import onnx_image_processing_amd.pytorch_model.threshold as impl
    assert OtsuThreshold is impl.OtsuThreshold is A
    assert MultiOtsuThreshold is impl.MultiOtsuThreshold is B


def test_constructor_contract_and_no_cpu_path():
    import inspect
    from pytorch_model.threshold import MultiOtsuThreshold, OtsuThreshold
    sig = inspect.signature(OtsuThreshold.__init__).parameters
    assert list(sig) == ["self", "min_val", "max_val", "dtype", "device"]
    assert sig["dtype"].default is torch.int32 and sig["device"].default == "cpu"
    sig = inspect.signature(MultiOtsuThreshold.__init__).parameters
    assert list(sig) == ["self", "min_val", "max_val", "device", "n_class", "calc_hist"]
    assert sig["n_class"].default == 3 and sig["calc_hist"].default is False and sig["device"].default == "cpu"
    assert list(inspect.signature(OtsuThreshold.forward).parameters) == ["self", "img_HxW"]
    assert list(inspect.signature(MultiOtsuThreshold.forward).parameters) == ["self", "input"]
    o = OtsuThreshold(0, 255)
    assert (o.min_val, o.max_val, o.BINS, o.dtype) == (0, 255, 256, torch.int32)            # max_val inclusive
    assert OtsuThreshold(10, 4095, dtype=torch.float32).BINS == 4086
    m = MultiOtsuThreshold(0, 255)
    assert (m.min_val, m.max_val, m.BINS, m.n_class, m.calc_hist) == (0, 255, 255, 3, False)   # max_val exclusive
    assert m.COMBINATIONS == math.comb(254, 2) == 32131 and m.DTYPE is torch.float32
    assert MultiOtsuThreshold(0, 255, n_class=4).COMBINATIONS == 2_699_004                  # no mask is built
    assert MultiOtsuThreshold(0, 65536, n_class=3).COMBINATIONS == math.comb(65535, 2) <= 2 ** 31 - 1
    for mod in (o, m):
        assert len(mod.state_dict()) == 0 and not list(mod.parameters()) and not list(mod.buffers())
    with pytest.raises(RuntimeError, match="no CPU path"):
        o(torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(255, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        MultiOtsuThreshold(0, 255, calc_hist=True)(torch.zeros(8, 8))


def test_value_errors():
    from pytorch_model.threshold import MultiOtsuThreshold, OtsuThreshold
    from onnx_image_processing_amd import ops
    for dtype in (torch.float64, torch.int64, torch.uint16, torch.bool):
        with pytest.raises(ValueError, match="dtype"):
            OtsuThreshold(0, 255, dtype=dtype)
    for lo, hi in ((0, -1), (5, 3), (0, 65536)):
        with pytest.raises(ValueError, match="bins"):
            OtsuThreshold(lo, hi)
    OtsuThreshold(0, 65535)
    OtsuThreshold(7, 7)
    for n in (1, 0, 6, -2):
        with pytest.raises(ValueError, match="n_class"):
            MultiOtsuThreshold(0, 255, n_class=n)
    with pytest.raises(ValueError, match="bins"):
        MultiOtsuThreshold(0, 3, n_class=4)                                                 # n_class > BINS
    MultiOtsuThreshold(0, 4, n_class=4)
    with pytest.raises(ValueError, match="bins"):
        MultiOtsuThreshold(0, 65537, n_class=2)
    with pytest.raises(ValueError, match="combinations"):
        MultiOtsuThreshold(0, 2400, n_class=4)                                              # C(2399, 3) = 2.3e9
    MultiOtsuThreshold(0, 2300, n_class=4)                                                  # C(2299, 3) = 2.02e9
    with pytest.raises(ValueError, match="combinations"):
        MultiOtsuThreshold(0, 600, n_class=5)
    assert ops.multi_otsu_combinations(33, 5) == math.comb(32, 4)


def test_argument_errors_before_any_launch():
    """MI_E_* from the host checks (no GPU is touched: these return before the first launch)."""
    lib = native_lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    odd1, odd2, odd4 = (ctypes.c_void_p(p.value + k) for k in (1, 2, 4))
    hist, otsu, multi, apply_ = lib.mi_histogram, lib.mi_otsu_threshold, lib.mi_multi_otsu_threshold, lib.mi_threshold_apply
    ws_bytes = lib.mi_multi_otsu_workspace_bytes
    NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
    # NULL
    for k in (0, 6):
        a = [p, 0, 1, 64, 0, 256, p, None]
        a[k] = None
        assert hist(*a) == NULL, k
    for k in (0, 4):
        a = [p, 1, 256, 0, p, None]
        a[k] = None
        assert otsu(*a) == NULL, k
    for k in (0, 5, 6):
        a = [p, 1, 64, 0, 3, p, p, 1 << 20, None]
        a[k] = None
        assert multi(*a) == NULL, k
    for k in (0, 4, 10):
        a = [p, 0, 1, 64, p, 1, 0, 0, 0, 0, p, None]
        a[k] = None
        assert apply_(*a) == NULL, k
    # shapes
    for batch, pixels, bins in ((0, 64, 256), (-1, 64, 256), (1, 0, 256), (1, -5, 256), (1, 64, 0), (1, 64, 65537),
                                (1 << 30, 1 << 40, 256)):
        assert hist(p, 0, batch, pixels, 0, bins, p, None) == SHAPE, (batch, pixels, bins)
    for batch, bins in ((0, 256), (1, 0), (1, 65537)):
        assert otsu(p, batch, bins, 0, p, None) == SHAPE, (batch, bins)
    assert apply_(p, 0, 0, 64, p, 1, 0, 0, 0, 0, p, None) == SHAPE
    assert apply_(p, 0, 1, 0, p, 1, 0, 0, 0, 0, p, None) == SHAPE
    # parameters: dtype codes, class counts, label / binary combinations, thresholds beyond int32
    assert hist(p, 4, 1, 64, 0, 256, p, None) == PARAM and hist(p, -1, 1, 64, 0, 256, p, None) == PARAM
    for n_class in (1, 0, 6):
        assert multi(p, 1, 64, 0, n_class, p, p, 1 << 20, None) == PARAM, n_class
    assert apply_(p, 0, 1, 64, p, 0, 0, 0, 0, 0, p, None) == PARAM                          # no threshold
    assert apply_(p, 0, 1, 64, p, 5, 0, 0, 0, 0, p, None) == PARAM                          # more than 4
    assert apply_(p, 0, 1, 64, p, 1, 2, 0, 0, 0, p, None) == PARAM                          # labels are uint8
    assert apply_(p, 0, 1, 64, p, 2, 2, 1, 0, 255, p, None) == PARAM                        # two-valued: one threshold
    assert apply_(p, 0, 1, 64, p, 1, 1, 1, 0, 255, p, None) == PARAM                        # bin_img is never uint16
    assert apply_(p, 0, 1, 64, p, 1, 0, 2, 0, 255, p, None) == PARAM
    assert otsu(p, 1, 256, 2 ** 31 - 200, p, None) == PARAM
    # multi-Otsu limits: n_class > bins, bins beyond the cap, more than 2^31 - 1 candidates; the size query says 0
    for bins, n_class in ((3, 4), (1, 2), (65537, 2), (2400, 4), (600, 5), (65536, 4)):
        assert multi(p, 1, bins, 0, n_class, p, p, 1 << 30, None) == SHAPE, (bins, n_class)
        assert ws_bytes(1, bins, n_class) == 0, (bins, n_class)
    assert ws_bytes(0, 64, 3) == 0 and ws_bytes(1, 64, 6) == 0
    # short workspaces
    for batch, bins, n_class in ((1, 64, 3), (16, 255, 4), (3, 33, 5), (2, 65536, 3)):
        need = ws_bytes(batch, bins, n_class)
        assert need >= batch * 16 * (bins + 1) + 16 * batch, (batch, bins, n_class)
        assert multi(p, batch, bins, 0, n_class, p, p, need - 1, None) == CAPACITY
        assert multi(p, batch, bins, 0, n_class, p, p, 0, None) == CAPACITY
    # alignment: element size of the frames and of the outputs, 8 bytes for histograms and workspace, 4 for thresholds
    assert hist(odd1, 1, 1, 64, 0, 256, p, None) == ALIGN and hist(odd2, 3, 1, 64, 0, 256, p, None) == ALIGN
    assert hist(p, 0, 1, 64, 0, 256, odd4, None) == ALIGN
    assert otsu(odd4, 1, 256, 0, p, None) == ALIGN and otsu(p, 1, 256, 0, odd2, None) == ALIGN
    assert multi(odd4, 1, 64, 0, 3, p, p, 1 << 20, None) == ALIGN
    assert multi(p, 1, 64, 0, 3, odd2, p, 1 << 20, None) == ALIGN
    assert multi(p, 1, 64, 0, 3, p, odd4, 1 << 20, None) == ALIGN
    assert apply_(odd2, 2, 1, 64, p, 1, 0, 0, 0, 0, p, None) == ALIGN
    assert apply_(p, 0, 1, 64, odd2, 1, 0, 0, 0, 0, p, None) == ALIGN
    assert apply_(p, 0, 1, 64, p, 1, 2, 1, 0, 255, odd2, None) == ALIGN
    assert lib.mi_abi_version() == 3


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from onnx_image_processing_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.histogram(torch.zeros(4, 4, dtype=torch.uint8), 0, 256)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.otsu(torch.zeros(4, 4), 0, 255)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.otsu_threshold(torch.zeros(256, dtype=torch.int64), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.multi_otsu_threshold(torch.zeros(64, dtype=torch.int64), 0, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.threshold_apply(torch.zeros(4, 4), torch.zeros((), dtype=torch.int32))
    with pytest.raises(ValueError, match="dtype"):
        ops.otsu(torch.zeros(4, 4), 0, 255, dtype=torch.float64)


def test_synth_threshold_frames():
    from onnx_image_processing_amd.synth import THRESHOLD_FAMILIES, synth_threshold_frame
    assert THRESHOLD_FAMILIES == ("uniform", "bimodal", "sawtooth", "constant", "trimodal", "spikes")
    for family in THRESHOLD_FAMILIES:
        a = synth_threshold_frame(5, 48, 64, family)
        assert a.dtype == np.uint8 and a.shape == (48, 64)
        assert np.array_equal(a, synth_threshold_frame(5, 48, 64, family))
        small = synth_threshold_frame(5, 48, 64, family, levels=32)
        assert small.max() < 32
        wide = synth_threshold_frame(5, 48, 64, family, levels=4096)
        assert wide.dtype == np.uint16 and wide.max() < 4096
    assert len(np.unique(synth_threshold_frame(5, 48, 64, "constant"))) == 1
    assert len(np.unique(synth_threshold_frame(5, 48, 64, "spikes"))) == 3
    assert len(np.unique(synth_threshold_frame(5, 48, 64, "uniform"))) > 200
    tri = np.bincount(synth_threshold_frame(5, 480, 640, "trimodal").reshape(-1), minlength=256)
    assert tri[80:100].sum() < tri[120:136].sum() / 4 and tri[160:180].sum() < tri[120:136].sum() / 4   # valleys
    with pytest.raises(ValueError):
        synth_threshold_frame(5, 8, 8, "other")


# ---- the oracles --------------------------------------------------------------------------------------------------------

def test_combination_order_is_itertools_order():
    for m, k in ((7, 1), (7, 2), (7, 3), (7, 4), (12, 3), (4, 4), (9, 2)):
        want = np.array(list(itertools.combinations(range(1, m + 1), k)), np.int32)
        assert np.array_equal(combinations_lex(m, k), want), (m, k)


def test_multi_otsu_oracle_against_a_plain_loop():
    """the vectorised oracle against the definition written as a loop over combinations, on histograms with gaps"""
    rng = np.random.default_rng(7)
    for bins, n_class in ((8, 2), (8, 3), (8, 4), (8, 5), (12, 3)):
        for trial in range(4):
            hist = rng.integers(0, 50, bins).astype(np.int64)
            hist[rng.integers(0, bins, 3)] = 0
            pn = np.concatenate([[0], np.cumsum(hist)])
            ps = np.concatenate([[0], np.cumsum(hist * (np.arange(bins) + 3))])
            best, best_v = None, -1.0
            for th in itertools.combinations(range(1, bins), n_class - 1):
                b = (0,) + th + (bins,)
                n = [int(pn[b[i + 1]] - pn[b[i]]) for i in range(n_class)]
                s = [int(ps[b[i + 1]] - ps[b[i]]) for i in range(n_class)]
                v = 0.0
                if all(n):
                    m = [float(s[i]) / float(n[i]) for i in range(n_class)]
                    for i, j in itertools.combinations(range(n_class), 2):
                        d = m[i] - m[j]
                        v = v + (float(n[i]) * float(n[j])) * (d * d)
                if v > best_v:
                    best, best_v = th, v
            assert multi_otsu_oracle(hist, 3, n_class) == [3 + t - 1 for t in best], (bins, n_class, trial)


def test_histogram_oracle_drops_what_is_not_counted():
    f = np.array([0.0, 0.9, -0.9, 1.5, 255.99, 256.0, -1.0, np.nan, np.inf, -np.inf, 3e9, 2.0], F32)
    assert hist_oracle(f, 0, 256).sum() == 6 and hist_oracle(f, 0, 256)[0] == 3 and hist_oracle(f, 0, 256)[255] == 1
    assert np.array_equal(hist_oracle(np.array([5, 6, 9, 10], np.uint16), 6, 4), [1, 0, 0, 1])
    assert np.array_equal(hist_oracle(np.array([-3, -2, 0, 7], np.int32), -3, 4), [1, 1, 0, 1])


# ---- the oracles against the reference fixture ---------------------------------------------------------------------------

def test_otsu_oracle_reproduces_the_reference_exactly():
    g = golden()
    names = otsu_cases(g)
    assert len(names) >= 13
    families, wide = set(), 0
    for name in names:
        frame, max_val = g[f"{name}__frame"], int(g[f"{name}__max_val"])
        assert frame.shape[0] <= 48 and frame.shape[1] <= 64
        thresh, _ = otsu_oracle(hist_oracle(frame, 0, max_val + 1), 0)
        assert thresh == int(g[f"{name}__thresh"]), name
        assert np.array_equal(binary_oracle(frame, thresh, 0, max_val, np.int32), g[f"{name}__bin_img"]), name
        families.add(str(g[f"{name}__family"]))
        wide += max_val == 4095
    assert len(families) == 6 and wide >= 1


def test_multi_otsu_oracle_reproduces_the_reference():
    g = golden()
    names = multi_cases(g)
    assert len(names) >= 40
    seen, flagged = set(), 0
    for name in names:
        hist, n_class = g[f"{name}__hist"], int(g[f"{name}__n_class"])
        ref = [int(t) for t in g[f"{name}__thresholds"]]
        if f"{name}__frame" in g:
            assert np.array_equal(hist_oracle(g[f"{name}__frame"], 0, hist.size), hist), name
        got = multi_otsu_oracle(hist, 0, n_class)
        seen.add((n_class, hist.size))
        if int(g[f"{name}__differs"]):
            flagged += 1
            v = multi_otsu_scores(hist, 0, np.array([[t + 1 for t in got], [t + 1 for t in ref]]))
            print(f"{name}: reference {ref}, fp64 definition {got}, fp64 scores {v[1]!r} <= {v[0]!r}")
            assert v[0] >= v[1], name
        else:
            assert got == ref, name
    assert seen == {(2, 64), (3, 64), (3, 255), (4, 32)}
    assert flagged * 20 <= len(names), f"{flagged} of {len(names)} cases differ from the fp64 definition"
    assert int(g["meta__full_frame_pixels"]) == 480 * 640
