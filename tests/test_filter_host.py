"""K35 disparity post-filters without a GPU: the section's own header and library and their exports, the host-side argument checks
of the four entries (MI_E_* before any launch, in the header's order of precedence), DisparityFilter's and StereoMatcher's
keywords, the refusal of CPU tensors and the export through the `pytorch_model` alias, synth_textureless_pair, the oracle on
hand-made frames, the kernels' union-find, implied-union rules and median network (csrc/filter_math.h) compiled for the host in
tests/native/filter_host.cpp and run phase by phase as the kernels run them, plain and under the host's address and
undefined-behaviour sanitizers, bit for bit against the oracle (tests/filter_oracle.py), and the property the speckle filter is
for, on the oracle.

Measured with this file (stereo_oracle + filter_oracle; synth_textureless_pair(seed, 40, 160), D = 64, 8 paths, default penalties
and tests, speckle filter max_size 30, max_diff 1.0; seeds 0 / 1 / 2):
  - wrong accepted pixels in the textureless patch: 160 -> 66, 123 -> 69, 135 -> 62 (59 %, 44 %, 54 % fewer);
  - correct pixels lost outside the patch: 2, 2, 0."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest
import torch

import filter_oracle as FO
import stereo_oracle as SO
from helpers import SANITIZE, build_host, host_program, run_host
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd.build import FILTER_LIB, LIB
from onnx_image_processing_amd.synth import synth_stereo_pair, synth_textureless_pair

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
NAMES = ["mi_filter_components", "mi_filter_median", "mi_filter_speckle", "mi_filter_workspace_bytes"]
U8, F32 = 0, 1
NAN, INF = float("nan"), float("inf")
# (37, 83): one tile row of two ragged columns over two more rows; (1, 70), (70, 1): lines across a border; the tile is 16 rows of
# 64 columns, so (20, 72) is 2 x 2 tiles and (70, 150) 5 x 3, both with a ragged last row and column of tiles
SHAPES = [(37, 83), (1, 70), (70, 1), (20, 72), (70, 150)]
SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def lib():
    return N.load_filter()


_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 12)
    _keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


def _exported(path):
    r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return sorted(ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip())


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_section_has_a_header_and_a_library_of_its_own(lib):
    assert sorted(N.FILTER_SIGNATURES) == NAMES == _exported(FILTER_LIB)
    for other in (N.SIGNATURES, N.DEBUG_SIGNATURES, N.SIM3_SIGNATURES, N.SIMGRAPH_SIGNATURES, N.FLOW_SIGNATURES, N.STEREO_SIGNATURES,
                  N.RECTIFY_SIGNATURES):
        assert not set(NAMES) & set(other)
    assert _exported(LIB) == sorted(N.SIGNATURES) and len(N.SIGNATURES) == 127          # the product library is what it was
    assert all(N.library_of(n) is lib for n in NAMES)
    assert N.library_of("mi_stereo_select") is N.load_stereo() and N.library_of("mi_depth_to_points") is N.load()
    assert N.load().mi_abi_version() == 3 and not any(hasattr(N.load(), n) for n in NAMES)
    assert N.FILTER_CONSTANTS == dict(MI_FILTER_MAX_PIXELS=1 << 26, MI_FILTER_NO_LABEL=FO.NO_LABEL, MI_FILTER_TILE_W=FO.TILE_W,
                                      MI_FILTER_TILE_H=FO.TILE_H, MI_FILTER_U8=U8, MI_FILTER_F32=F32, MI_FILTER_SPECKLE=FO.SPECKLE)
    assert FO.SPECKLE not in (SO.OK, SO.NOT_UNIQUE, SO.LR)
    assert N.RESTYPES["mi_filter_workspace_bytes"] is ctypes.c_size_t and N.RESTYPES["mi_filter_speckle"] is ctypes.c_int


def test_workspace_bytes(lib):
    f = lib.mi_filter_workspace_bytes
    assert f(1, 1, 1) == 16 and f(2, 21, 90) == 2 * 21 * 90 * 8 and f(3, 37, 83) == (3 * 37 * 83 * 8 + 15) // 16 * 16
    assert f(16, 480, 640) == 16 * 480 * 640 * 8
    assert f(0, 21, 90) == 0 and f(2, 0, 90) == 0 and f(2, 21, -1) == 0 and f(1 << 10, 1 << 8, 1 << 8) == 0 and f(1 << 30, 1 << 30, 1 << 30) == 0


def test_components_argument_checks(lib, p):
    f = lib.mi_filter_components
    big = 1 << 30

    def call(**kw):
        a = dict(values=p, type=F32, batch=2, h=21, w=90, min_valid=0.0, max_diff=1.0, labels=p, sizes=p, work=p, wbytes=big)
        a.update(kw)
        return f(a["values"], a["type"], a["batch"], a["h"], a["w"], a["min_valid"], a["max_diff"], a["labels"], a["sizes"], a["work"],
                 a["wbytes"], None)
    assert call(values=None) == NULL and call(labels=None) == NULL and call(work=None) == NULL
    assert call(batch=0) == SHAPE and call(h=0) == SHAPE and call(w=-2) == SHAPE
    for kw in (dict(type=2), dict(type=-1), dict(max_diff=-0.5), dict(max_diff=INF), dict(max_diff=NAN), dict(min_valid=NAN),
               dict(batch=1 << 10, h=1 << 8, w=1 << 8), dict(batch=1 << 30, h=1 << 30, w=1 << 30),
               dict(type=U8, min_valid=-1.0), dict(type=U8, min_valid=0.5), dict(type=U8, min_valid=257.0), dict(type=U8, max_diff=0.5),
               dict(type=U8, max_diff=256.0), dict(type=U8, min_valid=-INF)):
        assert call(**kw) == PARAM, kw
    assert call(values=p + 2) == ALIGN and call(labels=p + 2) == ALIGN and call(sizes=p + 1) == ALIGN and call(work=p + 8) == ALIGN
    assert call(wbytes=2 * 21 * 90 * 8 - 1) == CAPACITY and call(wbytes=0) == CAPACITY
    # precedence: NULL, shape, parameters, alignment, capacity
    assert call(values=None, batch=0) == NULL and call(batch=0, type=7, labels=p + 2, wbytes=0) == SHAPE
    assert call(type=7, labels=p + 2, wbytes=0) == PARAM and call(labels=p + 2, wbytes=0) == ALIGN
    assert call(min_valid=-INF, wbytes=0) == CAPACITY and call(type=U8, values=p + 1, min_valid=256.0, max_diff=255.0, wbytes=0) == CAPACITY
    assert call(sizes=None, wbytes=0) == CAPACITY                              # sizes may be NULL, a uint8 map needs no alignment


def test_speckle_argument_checks(lib, p):
    f = lib.mi_filter_speckle
    big = 1 << 30

    def call(**kw):
        a = dict(x=p, batch=2, h=21, w=90, min_valid=0.0, max_diff=1.0, max_size=30, invalid=-1.0, out=p + 64, removed=p, work=p, wbytes=big)
        a.update(kw)
        return f(a["x"], a["batch"], a["h"], a["w"], a["min_valid"], a["max_diff"], a["max_size"], a["invalid"], a["out"], a["removed"],
                 a["work"], a["wbytes"], None)
    assert call(x=None) == NULL and call(out=None) == NULL and call(work=None) == NULL
    assert call(batch=0) == SHAPE and call(h=-1) == SHAPE and call(w=0) == SHAPE
    for kw in (dict(max_diff=-1.0), dict(max_diff=INF), dict(max_diff=NAN), dict(min_valid=NAN), dict(max_size=-1), dict(invalid=0.0),
               dict(invalid=5.0), dict(invalid=INF), dict(min_valid=-INF, invalid=-INF), dict(min_valid=-INF, invalid=-1.0),
               dict(batch=1 << 10, h=1 << 8, w=1 << 8)):
        assert call(**kw) == PARAM, kw
    assert call(x=p + 2) == ALIGN and call(out=p + 1) == ALIGN and call(work=p + 4) == ALIGN
    assert call(wbytes=2 * 21 * 90 * 8 - 8) == CAPACITY
    assert call(x=None, batch=0) == NULL and call(batch=0, max_size=-1, out=p + 1, wbytes=0) == SHAPE
    assert call(max_size=-1, out=p + 1, wbytes=0) == PARAM and call(out=p + 1, wbytes=0) == ALIGN
    # legal and refused for capacity alone: a NaN invalid_value, everything valid, no removed map, max_size 0, in place
    assert call(invalid=NAN, wbytes=0) == CAPACITY and call(min_valid=-INF, invalid=NAN, wbytes=0) == CAPACITY
    assert call(removed=None, max_size=0, out=p, wbytes=0) == CAPACITY and call(removed=p + 1, wbytes=0) == CAPACITY


def test_median_argument_checks(lib, p):
    f = lib.mi_filter_median
    q = p + 1024
    assert f(None, 2, 21, 90, 3, 0.0, -1.0, q, None) == NULL and f(p, 2, 21, 90, 3, 0.0, -1.0, None, None) == NULL
    assert f(p, 0, 21, 90, 3, 0.0, -1.0, q, None) == SHAPE and f(p, 2, 0, 90, 3, 0.0, -1.0, q, None) == SHAPE and f(p, 2, 21, 0, 3, 0.0, -1.0, q, None) == SHAPE
    for k, mv, inv in ((0, 0.0, -1.0), (1, 0.0, -1.0), (4, 0.0, -1.0), (7, 0.0, -1.0), (3, NAN, -1.0), (3, 0.0, 0.0), (5, 0.0, 2.0), (5, -INF, -1.0)):
        assert f(p, 2, 21, 90, k, mv, inv, q, None) == PARAM, (k, mv, inv)
    assert f(p, 2, 21, 90, 3, 0.0, -1.0, p, None) == PARAM                     # not in place
    assert f(p, 1 << 10, 1 << 8, 1 << 8, 3, 0.0, -1.0, q, None) == PARAM
    assert f(p + 2, 2, 21, 90, 3, 0.0, -1.0, q, None) == ALIGN and f(p, 2, 21, 90, 5, 0.0, NAN, q + 1, None) == ALIGN
    assert f(None, 0, 21, 90, 4, 0.0, -1.0, q + 1, None) == NULL and f(p, 0, 21, 90, 4, 0.0, -1.0, q + 1, None) == SHAPE
    assert f(p, 2, 21, 90, 4, 0.0, -1.0, q + 1, None) == PARAM


def test_module_keywords_cpu_refusal_and_alias():
    import onnx_image_processing_amd.pytorch_model.stereo as real
    import pytorch_model
    from onnx_image_processing_amd import ops
    from pytorch_model.stereo import DisparityFilter, StereoMatcher
    from pytorch_model.stereo.disparity_filter import DisparityFilter as again
    assert DisparityFilter is real.DisparityFilter is again and "DisparityFilter" in real.__all__ and "DisparityFilter" in pytorch_model.__doc__
    assert ops.FILTER_SPECKLE == FO.SPECKLE and ops.FILTER_NO_LABEL == FO.NO_LABEL
    f = DisparityFilter()
    assert (f.speckle_size, f.speckle_range, f.median, f.active) == (0, 1.0, 0, False)
    assert DisparityFilter(30, 2.0, 5).active and DisparityFilter(median=3).active and DisparityFilter(speckle_size=1).active
    for cls in (DisparityFilter, StereoMatcher):
        for kw in (dict(speckle_size=-1), dict(speckle_size=1.5), dict(speckle_range=-1.0), dict(speckle_range=INF), dict(speckle_range=NAN),
                   dict(median=1), dict(median=4), dict(median=7)):
            with pytest.raises(ValueError):
                cls(**kw)
    m = StereoMatcher()
    assert not m.filter.active and (m.max_disparity, m.p1, m.p2, m.paths, m.uniqueness, m.lr_max_diff) == (128, 10, 120, 8, 10, 1)
    m = StereoMatcher(max_disparity=64, speckle_size=30, speckle_range=2.0, median=3)
    assert (m.filter.speckle_size, m.filter.speckle_range, m.filter.median) == (30, 2.0, 3)
    z = torch.zeros(1, 21, 90)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DisparityFilter(30)(z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DisparityFilter(median=3)(z)
    with pytest.raises(RuntimeError, match="differ in shape"):
        DisparityFilter(30)(z, torch.zeros(1, 21, 91, dtype=torch.uint8))
    for call in (lambda: ops.filter_components(z, 0.0, 1.0), lambda: ops.filter_speckle(z, 30, 1.0), lambda: ops.filter_median(z),
                 lambda: ops.filter_components(torch.zeros(1, 1, 8, 8, dtype=torch.uint8), 0, 0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    d, c = DisparityFilter()(z, None)                                          # inactive: nothing is called
    assert d is z and c is None


def test_synth_textureless_pair_is_what_it_says_and_deterministic():
    a, b = synth_textureless_pair(1, 40, 160), synth_textureless_pair(1, 40, 160)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    left, right, disp, visible, patch = a
    base = synth_stereo_pair(1, 40, 160)
    assert left.dtype == right.dtype == np.float32 and patch.dtype == bool and patch.sum() == 8 * 80 and patch[0:8, 70:150].all()
    assert np.array_equal(disp, base[2]) and np.array_equal(visible, base[3])
    assert np.array_equal(left[~patch], base[0][~patch]) and np.abs(left[patch] - 128).max() <= 1
    right_patch = np.zeros_like(patch)
    right_patch[0:8, 66:146] = True
    assert np.array_equal(right[~right_patch], base[1][~right_patch]) and np.abs(right[right_patch] - 128).max() <= 1
    assert not np.array_equal(left[patch], right[right_patch]) and (disp[patch] == 4.0).all()
    rng = np.random.default_rng(1001)
    assert np.array_equal(left[0:8, 70:150], (128 + rng.uniform(-1, 1, (8, 80))).astype(np.float32))
    assert np.array_equal(right[0:8, 66:146], (128 + rng.uniform(-1, 1, (8, 80))).astype(np.float32))
    for bad in ((0, 7, 160), (0, 40, 149)):
        with pytest.raises(ValueError):
            synth_textureless_pair(*bad)


# ---- the oracle on hand-made frames ---------------------------------------------------------------------------------------------------
def test_oracle_components_on_hand_made_frames():
    x = np.array([[1, 1, -1, 5, 5],
                  [-1, 1, -1, 5, 9],
                  [2, 2, 2, -1, 9],
                  [np.nan, 7, np.inf, np.inf, 9]], np.float32)
    labels, sizes = FO.components(x, 0.0, 1.0)
    assert labels.tolist() == [[0, 0, -1, 3, 3], [-1, 0, -1, 3, 9], [0, 0, 0, -1, 9], [-1, 16, 17, 18, 9]]
    assert sizes.tolist() == [[6, 6, 0, 3, 3], [0, 6, 0, 3, 3], [6, 6, 6, 0, 3], [0, 1, 1, 1, 3]]      # inf - inf does not join
    labels, sizes = FO.components(x, 0.0, 0.0)
    assert labels[2].tolist() == [10, 10, 10, -1, 9] and labels[1, 1] == 0 and sizes[2, 0] == 3
    u = np.array([[0, 0, 1], [2, 0, 1], [2, 2, 1]], np.uint8)
    assert FO.components(u, 0, 0)[0].tolist() == [[0, 0, 2], [3, 0, 2], [3, 3, 2]]
    assert FO.components(u, 1, 1)[0].tolist() == [[-1, -1, 2], [2, -1, 2], [2, 2, 2]] and FO.components(u, 1, 1)[1][2, 2] == 6      # 2 - 1 joins at (2, 1) - (2, 2)
    assert FO.components(u, 1, 0)[1].tolist() == [[0, 0, 3], [3, 0, 3], [3, 3, 3]]
    z = np.array([[-0.0, 0.0, 1e30, -1e30]], np.float32)
    assert FO.components(z, -np.inf, 1.0)[0].tolist() == [[0, 0, 2, 3]] and FO.components(z, 0.0, 1.0)[0].tolist() == [[0, 0, 2, -1]]


def test_oracle_speckle_and_median_on_hand_made_frames():
    x = np.array([[1, 1, -1, 5, 5],
                  [-1, 1, -1, 5, 9],
                  [2, 2, 2, -1, 9],
                  [np.nan, 7, 30, 40, 9]], np.float32)
    out, removed = FO.speckle(x, 3, 1.0)
    assert out.tolist() == [[1, 1, -1, -1, -1], [-1, 1, -1, -1, -1], [2, 2, 2, -1, -1], [-1, -1, -1, -1, -1]]
    assert removed.tolist() == [[0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1], [0, 1, 1, 1, 1]]      # the NaN was never valid
    out, removed = FO.speckle(x, 0, 1.0)
    assert np.array_equal(out[:3], x[:3]) and out[3].tolist() == [-1, 7, 30, 40, 9] and not removed.any()
    assert (FO.speckle(x, 20, 1.0)[0] == -1).all() and FO.speckle(x, 20, 1.0)[1].sum() == 15
    m = FO.median(x, 3)
    assert m[0, 0] == 1 and m[0, 2] == -1 and m[3, 0] == -1                    # replicated taps count; invalid centres stay invalid
    assert m[1, 3] == 5                                                        # valid taps 5 5 5 9 2 9 -> rank 2 of [2 5 5 5 9 9]
    assert m[2, 1] == 2                                                        # 1 2 2 2 7 30 -> rank 2
    z = np.array([[-0.0, 0.0]], np.float32)
    assert FO.median(z, 3, -1.0, -2.0).view(np.uint32).tolist() == [[0x80000000, 0]]      # six -0 before three +0, rank 4; then three and six
    assert FO.median(np.array([[0.0, -0.0]], np.float32), 5, -1.0, -2.0).view(np.uint32).tolist() == [[0, 0x80000000]]
    k = FO.key(np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all() and np.array_equal(FO.unkey(k).view(np.uint32), np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32).view(np.uint32))


def test_oracle_frames_are_what_their_names_say():
    for h, w in ((20, 72), (70, 150)):
        _, _, _, labels, sizes = FO.case("constant", h, w)
        assert (labels == 0).all() and (sizes == h * w).all()
        _, _, _, labels, sizes = FO.case("alternating", h, w)
        assert np.array_equal(labels.ravel(), np.arange(h * w)) and (sizes == 1).all()
        for name in ("spiral", "comb"):
            values, _, _, labels, sizes = FO.case(name, h, w)
            on = values > 0
            assert 0.4 < on.mean() < 0.7 and (labels[on] == 0).all() and (sizes[on] == on.sum()).all() and (labels[~on] == -1).all()
        _, _, _, labels, _ = FO.case("ramp025", h, w)
        assert np.array_equal(labels, np.repeat(np.arange(h)[:, None] * w, w, 1))        # 0.25 joins along a row, 0.5 down a column does not
        assert (FO.case("ramp05", h, w)[3] == 0).all()
        assert len(np.unique(FO.case("percolation0", h, w)[3])) > 20
        values = FO.case("hostile", h, w)[0]
        assert np.isnan(values).any() and np.isposinf(values).any() and np.isneginf(values).any() and (values == 1e30).any() and np.signbit(values[values == 0]).any()


# ---- the property ---------------------------------------------------------------------------------------------------------------------
def wrong_pixels(disparity, truth, visible):
    """accepted, and either not visible or off by more than 1"""
    return (disparity >= 0) & (~visible | (np.abs(disparity - truth) > 1))


@pytest.mark.parametrize("seed", SEEDS)
def test_speckle_filter_on_a_textureless_patch(seed):
    left, right, truth, visible, patch = synth_textureless_pair(seed, 40, 160)
    o = SO.run(left, right, 64, 8)
    before = o["disparity"]
    after, code = FO.disparity_filter(before, o["code"], 30, 1.0)
    w0, w1 = wrong_pixels(before, truth, visible), wrong_pixels(after, truth, visible)
    lost = ((before >= 0) & ~w0 & ~((after >= 0) & ~w1) & ~patch)
    print(f"seed {seed}: wrong pixels in the patch {int(w0[patch].sum())} -> {int(w1[patch].sum())}, correct pixels lost outside it {int(lost.sum())}")
    assert 3 * w1[patch].sum() <= 2 * w0[patch].sum()                          # at least a third fewer
    assert lost.sum() <= 8
    assert np.array_equal(code == FO.SPECKLE, (before >= 0) & (after < 0)) and np.array_equal(code[after >= 0], o["code"][after >= 0])


# ---- tests/native/filter_host.cpp: the kernels' phases, compiled for the host -----------------------------------------------------------
filter_host = host_program("filter_host.cpp", hip=True)


@pytest.fixture(scope="module")
def filter_host_san(tmp_path_factory):
    """the same program under the host's address and undefined-behaviour sanitizers (a stand-alone program)"""
    return build_host(tmp_path_factory.mktemp("filter_host_san"), "filter_host.cpp", hip=True, extra=SANITIZE)


def hexf(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]


def native_components(exe, values, min_valid, max_diff):
    h, w = values.shape
    raw = run_host(exe, ["components", str(int(values.dtype != np.uint8)), str(h), str(w), hexf(min_valid), hexf(max_diff)],
                   np.ascontiguousarray(values).tobytes(), binary=True)
    assert len(raw) == 8 * h * w
    return np.frombuffer(raw[:4 * h * w], np.int32).reshape(h, w), np.frombuffer(raw[4 * h * w:], np.int32).reshape(h, w)


def native_speckle(exe, x, max_size, max_diff, min_valid, invalid_value):
    h, w = x.shape
    raw = run_host(exe, ["speckle", str(h), str(w), hexf(min_valid), hexf(max_diff), str(max_size), hexf(invalid_value)],
                   np.ascontiguousarray(x, np.float32).tobytes(), binary=True)
    assert len(raw) == 5 * h * w
    return np.frombuffer(raw[:4 * h * w], np.float32).reshape(h, w), np.frombuffer(raw[4 * h * w:], np.uint8).reshape(h, w)


def native_median(exe, x, k, min_valid, invalid_value):
    h, w = x.shape
    raw = run_host(exe, ["median", str(h), str(w), str(k), hexf(min_valid), hexf(invalid_value)], np.ascontiguousarray(x, np.float32).tobytes(), binary=True)
    return np.frombuffer(raw, np.float32).reshape(h, w)


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    differ = got.view(np.uint8) != want.view(np.uint8)
    assert not differ.any(), f"{what}: {int(differ.sum())} bytes of {differ.size} differ from the oracle"


def check_frame(exe, name, h, w):
    values, min_valid, max_diff, labels, sizes = FO.case(name, h, w)
    got = native_components(exe, values, min_valid, max_diff)
    same(got[0], labels, (name, h, w, "labels"))
    same(got[1], sizes, (name, h, w, "sizes"))
    if values.dtype == np.uint8:
        return
    invalid = FO.invalid_for(min_valid)
    for max_size in (0, 1, 30, h * w):
        out, removed = native_speckle(exe, values, max_size, max_diff, min_valid, invalid)
        want = FO.speckle(values, max_size, max_diff, min_valid, invalid, sizes)
        same(out, want[0], (name, h, w, max_size, "speckle"))
        same(removed, want[1], (name, h, w, max_size, "removed"))
    for k in (3, 5):
        same(native_median(exe, values, k, min_valid, invalid), FO.median(values, k, min_valid, invalid), (name, h, w, k, "median"))


@pytest.mark.parametrize("h,w", SHAPES)
def test_native_program_is_the_oracle_bit_for_bit(filter_host, h, w):
    for name in FO.PATTERNS:
        check_frame(filter_host, name, h, w)


def test_native_program_on_stereo_disparities(filter_host):
    for seed in (11, 21):
        d = FO.stereo_disparity(40, 160, seed)
        assert (d < 0).any() and (d >= 0).any()
        labels, sizes = FO.components(d, 0.0, 1.0)
        got = native_components(filter_host, d, 0.0, 1.0)
        same(got[0], labels, (seed, "labels"))
        same(got[1], sizes, (seed, "sizes"))
        for max_size in (1, 30):
            out, removed = native_speckle(filter_host, d, max_size, 1.0, 0.0, -1.0)
            want = FO.speckle(d, max_size, 1.0, 0.0, -1.0, sizes)
            same(out, want[0], (seed, max_size))
            same(removed, want[1], (seed, max_size))
        same(native_median(filter_host, d, 3, 0.0, -1.0), FO.median(d, 3), (seed, "median 3"))
        same(native_median(filter_host, d, 5, 0.0, -1.0), FO.median(d, 5), (seed, "median 5"))


def test_native_program_is_clean_under_the_host_sanitizers(filter_host, filter_host_san):
    """every phase once more under -fsanitize=address,undefined: the same output, no report (run_host checks stderr)"""
    for (h, w), names in (((37, 83), FO.PATTERNS), ((70, 150), ("spiral", "comb", "percolation0", "hostile", "classes")),
                          ((1, 70), ("constant", "hostile_all")), ((70, 1), ("constant", "alternating")), ((20, 72), ("comb", "steps05"))):
        for name in names:
            values, min_valid, max_diff, labels, sizes = FO.case(name, h, w)
            a, b = native_components(filter_host_san, values, min_valid, max_diff), native_components(filter_host, values, min_valid, max_diff)
            same(a[0], b[0], (name, h, w))
            same(a[1], b[1], (name, h, w))
            if values.dtype == np.uint8:
                continue
            invalid = FO.invalid_for(min_valid)
            a, b = native_speckle(filter_host_san, values, 30, max_diff, min_valid, invalid), native_speckle(filter_host, values, 30, max_diff, min_valid, invalid)
            same(a[0], b[0], (name, h, w))
            same(a[1], b[1], (name, h, w))
            for k in (3, 5):
                same(native_median(filter_host_san, values, k, min_valid, invalid), native_median(filter_host, values, k, min_valid, invalid), (name, h, w, k))
