"""K10 without a GPU: the staged fp64 oracle of tests/essential_oracle.py against oracle/numpy_oracle.py and the golden
fixture, the figures its margin was chosen from, the one-weight condition of every case the GPU file runs, planted errors
in a numpy restatement of the head, and the workspace layout against the library's size query (a host call).

Planted errors (head_f32, one changed line each) and where they land, on the cases of PLANT_CASES:
    row_gt, col_k_plus_1, valid_after, hartley_2, no_shift    outside the bound on at least one case (most on every case)
    one_iteration_less                                        outside on every case at n_iter = 30, 2 and 1: thirty steps
                                                              of the shifted iteration have not converged to within a
                                                              bound, so the count itself is held
    ge_001                                                    inside the bound: an entry of exactly fp32(0.01) carries a
                                                              weight of 0.01 among weights of 0.3 to 0.9 and a column
                                                              threshold usually removes it.  E cannot see it; the
                                                              candidate sets of the banded form can, and the GPU file
                                                              compares those exactly
"""
import ctypes
import functools

import numpy as np
import pytest

import essential_oracle as EO
from helpers import load_golden
from oracle import numpy_oracle as O

F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _reports(key):
    batch, n, m, top_k, masked, variant, n_iter = key
    c = EO.p_case(batch, n, m, top_k, variant)
    return [EO.case_report(ref, c["pts1"][b], c["pts2"][b], n_iter) for b, ref in enumerate(EO.reference(*key))]


def _keys(shape):
    return [k for k in EO.p_cases() if k[:3] == shape]


@pytest.mark.parametrize("shape", EO.SHAPES, ids=str)
def test_staged_oracle_equals_numpy_oracle(shape):
    """Weights identical to O.essential_weights, E (through the Hartley parameters and the 81 sums) equal to
    O.essential_from_weights in fp64, the planted counts are what the inputs claim, and a pair is flagged for the dense
    front exactly where a row or a column holds more than 8."""
    for key in _keys(shape):
        batch, n, m, top_k, masked, variant, n_iter = key
        c = EO.p_case(batch, n, m, top_k, variant)
        assert np.isnan(c["p"][:, n, :]).all() and np.isnan(c["p"][:, :, m]).all()
        for b, ref in enumerate(EO.reference(*key)):
            v1, v2 = (c["valid1"][b], c["valid2"][b]) if masked else (None, None)
            want = O.essential_weights(c["p"][b], v1, v2, top_k)
            assert np.array_equal(ref["weights"].view(np.uint32), want.view(np.uint32)), key
            e64 = O.essential_from_weights(want, c["pts1"][b], c["pts2"][b], n_iter, EO.N_ITER_MANIFOLD, dtype=F64)
            assert np.abs(ref["E"] - e64).max() <= 1e-9, key
            assert ref["dense"] == bool((ref["cnt"] > 8).any() or ((want != 0).sum(0) > 8).any())
            meta = c["meta"][b]
            if meta["special"]:
                r8, c8 = meta["row8"], meta["col8"]
                assert ref["cnt"][r8] == (9 if variant == "row9" else 8) and ref["cand_cnt"][r8] == (255 if variant == "row9" else 8)
                assert ref["col_cnt"][c8] == (9 if variant == "col9" else 8)
                assert not ref["weights"][meta["zero_row"]].any() and not ref["weights"][:, meta["zero_col"]].any()
                assert ref["dense"] == (variant != "base" or top_k > 4), key
                if 2 * top_k <= m - 2:
                    tie = ref["core"][meta["tie_row"]]
                    assert (tie == ref["thr_row"][meta["tie_row"]]).sum() == top_k + 1 and ref["cnt"][meta["tie_row"]] == 2 * top_k
                near = ref["core"][meta["thr_row"]]
                assert (near == EO.THR).sum() == 1 and ref["cnt"][meta["thr_row"]] == 1      # 0.01 and its lower neighbour stay out
                if masked:
                    assert not ref["weights"][meta["masked_row"]].any()
                    assert meta["masked_col"] is None or not ref["weights"][:, meta["masked_col"]].any()


def test_staged_oracle_on_the_golden_fixture():
    g = load_golden("essential_matrix")
    for i in range(3):
        p = g[f"grid{i}_P"]
        n, m = p.shape[0] - 1, p.shape[1] - 1
        st = EO.stages(p, None, None, 3)
        assert np.array_equal(st["weights"], O.essential_weights(p, None, None, 3))
        idx = np.arange(32 * 32, dtype=F32)
        ph = np.stack([idx % 32, idx // 32, np.ones(32 * 32, F32)], axis=-1).astype(F32)
        pn = (ph @ np.linalg.inv(np.asarray(g["grid_K"], F32)).astype(F32).T)[:, :2].astype(F32)
        e64, bound = EO.e_bound(st["weights"], pn[:n], pn[:m])
        assert np.abs(O.essential_matrix_grid(p, g["grid_K"]).astype(F64) - e64).max() <= bound
        assert np.abs(g[f"grid{i}_E"].astype(F64) - e64).max() <= 1e-4 * max(1.0, np.abs(e64).max())
    p, k1, k2 = g["st_P"][0], g["st_k1"][0], g["st_k2"][0]
    v1, v2 = k1[:, 0] >= 0, k2[:, 0] >= 0
    st = EO.stages(p, v1, v2, 3)
    assert np.array_equal(st["weights"], O.essential_weights(p, v1, v2, 3))
    kinv = np.linalg.inv(np.asarray(g["cam_K"], F32)).astype(F32)
    norm = lambda kp: (np.stack([kp[:, 1], kp[:, 0], np.ones(len(kp), F32)], axis=-1) @ kinv.T)[:, :2].astype(F32)  # noqa: E731
    e64, bound = EO.e_bound(st["weights"], norm(k1), norm(k2))
    assert np.abs(O.essential_matrix_keypoints(p, k1, k2, v1, v2, g["cam_K"]).astype(F64) - e64).max() <= bound


@pytest.mark.parametrize("shape", EO.SHAPES, ids=str)
def test_fp32_evaluations_lie_inside_the_bound_and_one_weight_is_four_bounds(shape):
    for key in _keys(shape):
        for ref, (err, floor, raw, shift) in zip(EO.reference(*key), _reports(key)):
            assert err <= ref["bound"], (key, err / ref["bound"])
            assert shift >= EO.CONDITION * ref["bound"], (key, shift / ref["bound"])


def test_margin_is_the_smallest_power_of_two():
    """Over every case: the fp32 evaluations need more than half of MARGIN (and no more than MARGIN, above)."""
    worst = max((err - floor) / raw for key in EO.p_cases() for err, floor, raw, _ in _reports(key))
    assert EO.MARGIN / 2 < worst <= EO.MARGIN, worst


@pytest.mark.parametrize("bits_case", EO.DOTS_CASES, ids=str)
def test_dots_inputs_meet_the_condition_on_a_cpu_solve(bits_case):
    """The dots inputs through the numpy Sinkhorn (the GPU file uses the P the solver wrote and asserts the same there)."""
    (batch, n, m), bits = bits_case
    c = EO.dots_case(batch, n, m, bits)
    p = EO.sinkhorn_p(c, 0)
    for top_k in (k for k in EO.DOTS_TOP_K if k <= min(n, m)):
        for v1, v2 in ((None, None), (c["valid1"][0], c["valid2"][0])):
            ref = EO.reference_pair(p, v1, v2, c["pts1"][0], c["pts2"][0], top_k)
            assert np.array_equal(ref["weights"], O.essential_weights(p, v1, v2, top_k))
            err, floor, raw, shift = EO.case_report(ref, c["pts1"][0], c["pts2"][0])
            assert err <= ref["bound"] and shift >= EO.CONDITION * ref["bound"], (top_k, err / ref["bound"], shift / ref["bound"])


# ------------------------------------------------------------------ planted errors
PLANT_CASES = [((2, 31, 20), 3), ((3, 33, 65), 2), ((3, 33, 65), 3), ((2, 257, 301), 3), ((1, 100, 513), 4)]
CAUGHT_AT_30 = ("row_gt", "col_k_plus_1", "valid_after", "hartley_2", "no_shift")


def _plant_errors(plant, n_iter):
    """error / bound of head_f32(plant) on every pair of PLANT_CASES, masks on."""
    out = []
    for (batch, n, m), top_k in PLANT_CASES:
        c = EO.p_case(batch, n, m, top_k)
        for b, ref in enumerate(EO.reference(batch, n, m, top_k, True, "base", n_iter)):
            e = EO.head_f32(c["p"][b], c["valid1"][b], c["valid2"][b], c["pts1"][b], c["pts2"][b], top_k, n_iter, plant=plant)
            out.append(np.abs(e.astype(F64) - ref["E"]).max() / ref["bound"])
    return np.array(out)


def test_the_restatement_itself_is_inside_every_bound():
    for n_iter in (1, 2, 30):
        assert _plant_errors(None, n_iter).max() <= 1.0


@pytest.mark.parametrize("plant", EO.PLANTS)
def test_planted_errors_leave_the_bound(plant):
    r30 = _plant_errors(plant, 30)
    if plant in CAUGHT_AT_30:
        assert r30.max() > 1.0, r30
    elif plant == "one_iteration_less":
        assert min(r30.min(), _plant_errors(plant, 2).min(), _plant_errors(plant, 1).min()) > 1.0
    else:
        assert plant == "ge_001" and r30.max() <= 1.0            # E cannot see it (module docstring); the stages can:
        (batch, n, m), top_k = PLANT_CASES[0]
        c = EO.p_case(batch, n, m, top_k)
        row = c["meta"][0]["thr_row"]
        assert (c["p"][0][row, :m] >= EO.THR).sum() == 2 and EO.stages(c["p"][0], None, None, top_k)["cnt"][row] == 1


# ------------------------------------------------------------------ the workspace layout (a host call)
@pytest.fixture(scope="module")
def lib():
    from onnx_image_processing_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.mi_essential_matrix_workspace_bytes.restype = ctypes.c_size_t
    lib.mi_essential_matrix_workspace_bytes.argtypes = [ctypes.c_int] * 4
    return lib


def test_workspace_layout_equals_the_size_query(lib):
    shapes = list(EO.SHAPES) + [(65535, 1, 1), (7, 1024, 1), (5, 1, 1024), (128, 512, 512)]
    for batch, n, m in shapes:
        for top_k in (1, 2, 3, 4):
            offs, total = EO.workspace_layout(batch, n, m, top_k)
            assert lib.mi_essential_matrix_workspace_bytes(batch, n, m, top_k) == total
            assert all(o % 256 == 0 for o in offs) and total % 256 == 0
        for top_k in (0, 5, 8):
            assert lib.mi_essential_matrix_workspace_bytes(batch, n, m, top_k) == 0
    assert lib.mi_essential_matrix_workspace_bytes(1, 1025, 8, 3) == 0 and lib.mi_essential_matrix_workspace_bytes(1, 8, 1025, 3) == 0
    assert lib.mi_essential_matrix_workspace_bytes(65536, 8, 8, 3) == 0
