"""CPU half of the BAD descriptor net (K4, K4o): no GPU.

1. tests/bad_oracle.py against oracle/numpy_oracle.py -- two independent statements of SparseBAD.forward (direct box
   sums against a summed-area table) -- on every case that test_gpu_bad.py runs, and against the reference's recorded
   outputs in tests/golden at the allowances those fixtures already have.
2. The condition the GPU cases' INPUTS have to meet: at most 0.5 % fragile pairs (25 % with the special angles).
3. A float32 model of two proofs that csrc/bad_oriented.hip makes in comments only: the threshold test
   (d - fl(t a)) <= fma(t, a, -fl(t a)) decides d <= t a exactly, and clamp(rint(x)) places a centre where
   rint(clamp(x)) does."""
import os

import numpy as np
import pytest

import bad_oracle as B
from helpers import bad_tables, load_golden
from onnx_image_processing_amd.synth import synth_batch
from oracle import numpy_oracle as O

F32 = np.float32
ALL_CASES = B.PLAIN_CASES + B.ORIENTED_CASES


def _report(what, value):
    if os.environ.get("MI_REPORT"):
        print(f"[bad host] {what}: {value}")


# ------------------------------------------------------------------ 1. the two oracles
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_bad_oracle_agrees_with_the_numpy_oracle(case):
    x, ref = B.inputs(case), B.expected(case)
    img4 = x["image"][:, None]
    kw = dict(binarize=False, normalize_descriptors=False, return_aux=True)
    if case["angles"]:
        mode = "bilinear" if case["bilinear"] else "nearest"
        _, aux = O.sparse_bad_oriented(img4, x["kp"], x["theta"], x["box"], x["thr"], sampling_mode=mode, **kw)
    else:
        _, aux = O.sparse_bad(img4, x["kp"], x["box"], x["thr"], **kw)
    assert np.array_equal(aux["valid"], ref["valid"])
    # the numpy oracle takes its bit from mean1 - mean2 - t in fp64, which at an exact tie s1 - s2 == t * area is rounding
    # noise of either sign (two divisions by an odd area); bad_oracle and the kernels compare the exact integers.  Inside
    # the fp64 rounding band of that expression, 2^-52 (2 M + |t|), its bit is therefore replaced by ours.
    band = 2.0 ** -52 * (2 * float(np.abs(x["image"]).max()) + np.abs(x["thr"].astype(np.float64)))
    noise = (np.abs(aux["centered"]) <= band) & (ref["cands"][ref["nominal"]] == 0) & ~case["bilinear"]
    aux["bits"] = np.where(noise, ref["bits"], aux["bits"])
    B.check_bits(ref, aux["bits"], case["name"])
    firm_equal = (aux["bits"] == ref["bits"]) | ref["fragile"]
    assert firm_equal.all(), f"{case['name']}: {int((~firm_equal).sum())} firm bits differ between the oracles"
    ratio = B.float_ratio(ref, aux["centered"] * ref["valid"][:, :, None], "raw")
    _report(f"{case['name']} raw, numpy oracle against the candidates", f"{ratio:.3g}")
    assert ratio <= 1.0, f"{case['name']}: the oracles' responses differ by {ratio:.3g} bounds"
    if case["bilinear"]:
        return                                           # every bilinear value moves with the sine: candidates only
    # the float forms, on the keypoints whose pairs are all firm (the two files may round sin / cos differently)
    rows = ref["firm"].all(-1) & ~ref["fragile"].any(-1)
    want = B.forms(ref, temperature=B.TEMPERATURE)
    okw = dict(temperature=B.TEMPERATURE)
    if case["angles"]:
        okw["sampling_mode"] = "bilinear" if case["bilinear"] else "nearest"
    for form, kws in (("raw_n", dict(binarize=False)), ("soft", dict(binarize=True, normalize_descriptors=False)),
                      ("soft_n", dict(binarize=True)), ("hard_n", dict(binarize=True, soft_binarize=False))):
        if case["angles"]:
            got = O.sparse_bad_oriented(img4, x["kp"], x["theta"], x["box"], x["thr"], **kws, **okw)
        else:
            got = O.sparse_bad(img4, x["kp"], x["box"], x["thr"], **kws, **okw)
        value, bound = want[form]
        use = rows & ~noise.any(-1) if form == "hard_n" else rows      # its noise bits enter the numpy oracle's norm
        ratio = B.worst_ratio(got[use], value[use], bound[use])
        assert ratio <= 1.0, f"{case['name']} {form}: {ratio:.3g} bounds"


def test_bad_oracle_vs_recorded_bilinear_outputs():
    """tests/golden/bad_bilinear.npz at test_oracle_golden.py's allowances: no hard bit differs, raw within 1e-3, the
    normalised sigmoid within 1e-4 (the reference's fp32 box means are off by up to 2e-4 each)."""
    g = load_golden("bad_bilinear")
    a, _ = synth_batch(int(g["seed"]), 2, 96, 128)
    zero = np.zeros((2, 40), F32)
    for name, pairs in (("raw", 256), ("soft", 256), ("hard", 512)):
        box, thr = bad_tables(pairs)
        for tag, kp, th in (("int", g["kp"], zero), ("frac", g["kf"], zero), ("ori", g["kf"], B.sample_map(g["ang"][:, 0], g["kf"]))):
            ref = B.reference(a[:, 0], kp, box, thr, th, bilinear=True, window=60)
            want, recorded = B.forms(ref, temperature=10.0), g[f"{name}_{tag}"]
            if name == "hard":
                assert np.array_equal(ref["bits"], recorded != 0), f"bilinear hard {tag}"
            else:
                value = want["raw"][0] if name == "raw" else want["soft_n"][0]
                np.testing.assert_allclose(value, recorded, rtol=0, atol=1e-3 if name == "raw" else 1e-4)


def test_bad_oracle_vs_recorded_oriented_pipeline_outputs():
    """tests/golden/angle_pipeline.npz: the reference's descriptors of image 1 at its own keypoints and its own angle
    map.  Hard: every recorded bit is a candidate's and no firm bit differs (the fixture's allowance is 0 bits); raw,
    normalised: 3e-5 on the keypoints without fragile pairs."""
    g = load_golden("angle_pipeline")
    a, _ = synth_batch(int(g["seed"]), 1, int(g["h"]), int(g["w"]))
    for name, pairs in (("hard", 512), ("soft", 256)):
        box, thr = bad_tables(pairs)
        kp, recorded = g[name + "_k1"], g[name + "_desc1"]
        ref = B.reference(a[:, 0], kp, box, thr, B.sample_map(g["angle_map"][:, 0], kp), window=48)
        if name == "hard":
            B.check_bits(ref, recorded != 0, "angle pipeline, hard")
            assert (((recorded != 0) == ref["bits"]) | ref["fragile"]).all()
        else:
            rows = ~ref["fragile"].any(-1)
            assert rows.sum() > rows.size // 2
            np.testing.assert_allclose(B.forms(ref)["raw_n"][0][rows], recorded[rows], rtol=0, atol=3e-5)


# ------------------------------------------------------------------ 2. the inputs' fragile shares
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_fragile_share_of_the_case_inputs(case):
    ref = B.expected(case)
    share = B.fragile_share(ref)
    _report(f"{case['name']} fragile share", f"{100 * share:.3f} %")
    assert ref["valid"].sum() >= ref["valid"].size // 2
    if case["angles"] == "special":
        assert 0.0 < share <= B.FRAGILE_CAP_SPECIAL           # the case exists for its exact ties
    else:
        assert share <= B.FRAGILE_CAP
    if not case["angles"] and case["image"] in ("u8", "const"):
        assert share == 0.0                                   # no sine, exact sums: nothing to be fragile about


def test_case_inputs_hold_what_they_are_for():
    for case in ALL_CASES:
        x = B.inputs(case)
        kp, h, w = x["kp"].reshape(-1, 2), case["h"], case["w"]
        assert len(x["thr"]) % 64 == 0 and np.isfinite(x["thr"]).all()
        box = x["box"]
        x0, r = box[:, :4], box[:, 4:5]
        if not case["table"].startswith("wide"):
            assert (x0 - r >= 0).all() and (x0 + r <= 31).all(), case["name"]     # the fast plan's geometry check passes
            assert B.reach(box) <= 22.5
            if case["table"].startswith("syn"):
                assert (np.abs(x0 - 16) + r <= 15).all()
        else:
            assert B.reach(box) > 22.5 and np.abs(x0 - 16).max() <= 15 and case["wide_window"]
        if case["kps"] in ("frac", "int") and case["k"] > 1:
            assert (kp[:, 0] < 0).any() and ((kp[:, 0] >= 0) & (kp[:, 1] < 0)).any()
            assert (kp[:, 0] > h - 1).any() and (kp != np.floor(kp)).any()
        if case["image"] == "mixed":
            img = x["image"]
            assert (img == 256).any() and (img == -1).any() and np.signbit(img[img == 0]).any()
            assert (img != np.rint(img)).any()
    for name in ("tie256-u8-64x80", "tie256o-u8-48"):      # the tie tables meet their own case's box differences exactly
        x, ref = B.inputs(B.CASE[name]), B.expected(B.CASE[name])
        area = (2 * x["box"][:, 4] + 1) ** 2
        t = x["thr"].astype(np.float64)
        assert (t == np.rint(t)).all()                     # area is odd: d0 / area is a float only for integer t
        gap = (ref["cands"][ref["nominal"]] * area)[ref["valid"]]        # s1 - s2 - t * area, exact
        gap = gap[ref["firm"][ref["valid"]]]
        ties = (gap == 0) & np.broadcast_to(t != 0, ref["firm"].shape)[ref["valid"]][ref["firm"][ref["valid"]]]
        _report(f"{name} exact ties with a non-zero product", int(ties.sum()))
        assert ties.sum() >= 300, (name, int(ties.sum()))
        near = np.abs(gap) <= np.broadcast_to(area, ref["firm"].shape)[ref["valid"]][ref["firm"][ref["valid"]]]
        assert (near & (gap > 0)).sum() >= 100 and (near & (gap < 0)).sum() >= 100        # both outcomes next to the ties
    t = B.table("const512")[1]
    assert set(np.signbit(t[t == 0]).tolist()) == {True, False} and (np.floor(t.astype(np.float64) * 9) == -1).any()
    sizes = sorted({len(B.table(c["table"])[1]) for c in B.PLAIN_CASES})
    assert sizes == [64, 128, 256, 320, 512, 576, 1024]


# ------------------------------------------------------------------ 3. the in-kernel proofs, in float32
def _threshold_model(t32: np.ndarray, radius: int) -> tuple:
    """bad_oriented_bits_kernel's bit for every integer d in [-255 a, 255 a] against the exact d <= t a, for each
    threshold of t32: (cases, disagreements)."""
    a = (2 * radius + 1) ** 2
    d = np.arange(-255 * a, 255 * a + 1, dtype=np.int64)
    d32 = d.astype(F32)
    assert np.array_equal(d32.astype(np.int64), d)
    cases = wrong = 0
    for t in np.unique(t32):
        p = t * F32(a)                                        # fl(t a)
        assert p.dtype == F32 and np.isfinite(p)
        exact = float(t) * a                                  # 24 bits x 8 bits: exact in fp64
        e = exact - float(p)                                  # the product's residual: what fma(t, a, -p) returns
        assert float(F32(e)) == e, (t, a)
        got = (d32 - p) <= F32(e)                             # one rounded fp32 subtraction, one comparison
        wrong += int((got != (d <= exact)).sum())
        cases += d.size
    return cases, wrong


def test_fp32_threshold_test_decides_exactly():
    cases = wrong = 0
    for pairs in (256, 512):
        box, thr = bad_tables(pairs)
        for r in np.unique(box[:, 4]):
            c, w = _threshold_model(thr[box[:, 4] == r].astype(F32), int(r))
            cases, wrong = cases + c, wrong + w
    learned = cases
    rng = np.random.default_rng(5)
    for r in range(0, 8):
        a = (2 * r + 1) ** 2
        d0 = np.concatenate([rng.integers(-255 * a, 255 * a + 1, 48), [0, 1, -1, 255 * a, -255 * a, a, -a]])
        t = (d0.astype(np.float64) / a).astype(F32)           # fl(d0 / a) and the floats either side
        t = np.concatenate([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))])
        big = np.array([s * m for s in (1, -1) for m in (1e3, 65536.0, 1e6, 2.0 ** 24, 1e10, 1e20, 1e30)], F32)
        small = np.array([0.0, -0.0, 1e-9, -1e-9, 1e-38, -1e-38], F32)
        c, w = _threshold_model(np.concatenate([t, big, small]), r)
        cases, wrong = cases + c, wrong + w
    _report("threshold model", f"{cases} cases ({learned} from the learned tables), {wrong} disagreements")
    assert cases >= 64_000_000 and wrong == 0


def _place_fast(p, size):
    """bad_oriented_bits_kernel: clamp(rint(((p s - 1) + 1) * (0.5 (size - 1))), 0, size - 1), rint by a saturating
    float-to-int conversion that sends NaN to 0."""
    scale, half = F32(2.0 / ((size - 1) + 1e-8)), F32(0.5) * F32(size - 1)
    x = ((p * scale - F32(1)) + F32(1)) * half
    assert x.dtype == F32
    with np.errstate(invalid="ignore"):
        i = np.where(np.isnan(x), 0.0, np.clip(np.rint(x.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    return np.clip(i, 0, size - 1)


def _place_generic(p, size):
    """nearest_centre_o: rint(fmin(fmax(((p s - 1 + 1) / 2) * (size - 1), 0), size - 1)); fmax(NaN, 0) = 0."""
    scale = F32(2.0 / ((size - 1) + 1e-8))
    x = (((p * scale - F32(1)) + F32(1)) / F32(2)) * F32(size - 1)
    assert x.dtype == F32
    return np.rint(np.fmin(np.fmax(x, F32(0)), F32(size - 1))).astype(np.int64)


@pytest.mark.parametrize("size", [2, 33, 640])
def test_centre_placement_clamp_of_rint_equals_rint_of_clamp(size):
    halves = np.arange(-40, size + 40, dtype=np.float64) + 0.5
    sweep = [np.arange(-40 * 16, (size + 40) * 16, dtype=np.float64) / 16]
    for v in (halves, np.arange(-3, size + 3, dtype=np.float64)):     # every x.5 and every integer, +-3 floats around
        v = v.astype(F32)
        lo = hi = v
        sweep.append(v)
        for _ in range(3):
            lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
            sweep += [lo, hi]
    sweep.append(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 0.0, -0.0]))
    p = np.concatenate(sweep).astype(F32)
    fast, generic = _place_fast(p, size), _place_generic(p, size)
    assert np.array_equal(fast, generic), p[fast != generic][:8]
    assert fast[np.isnan(p)].tolist() == [0]
    assert set(np.unique(fast)) == set(range(size))                     # the sweep reaches every pixel and both clamps
    assert (fast[p > size + 1] == size - 1).all() and (fast[p < -1] == 0).all()
