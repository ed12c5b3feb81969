"""K35 disparity post-filters on the GPU against tests/filter_oracle.py, bit for bit and without a tolerance: labels and sizes as
int32, the speckle filter's output and the median as float32 bit patterns, the removed map as bytes.  Every output and the workspace
hold 0xA5 bytes on entry; every case runs twice; a batch of three different frames equals the three runs alone.

Shapes: (37, 83), (1, 70), (70, 1), and -- the tile of the labelling kernel being 16 rows of 64 columns -- (20, 72), 2 x 2 tiles, and
(70, 150), 5 x 3 tiles, so that a frame spans at least two tiles in each direction with a ragged last row and column of tiles.
Frames (filter_oracle.PATTERNS): a constant plane, alternating 0 / 10, a one-pixel spiral and a serpentine comb over the whole
frame, random validity at density 0.6 (seeds 0 to 2), ramps and steps of multiples of 0.25 at max_diff 0.25 and 0.5, a hostile
frame (NaN, both infinities, -0.0, 1e30 in a tenth of the pixels; once with every non-NaN pixel valid and a NaN invalid_value),
stereo_oracle disparities, a uint8 map of three classes.  max_size 0, 1, 30, h * w; sizes NULL; removed NULL; in place; median 3
and 5; a hipGraph replay; StereoMatcher(speckle_size=30) against the oracle composition and into ops.depth_to_points; the
textureless-patch property through the kernels."""
import numpy as np
import pytest
import torch

import filter_oracle as FO
import stereo_oracle as SO
from gpu_common import DEV, GPU, gpu, same_bits, twice
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.stereo import DisparityFilter, StereoMatcher
from onnx_image_processing_amd.synth import synth_textureless_pair

pytestmark = GPU

SHAPES = [(37, 83), (1, 70), (70, 1), (20, 72), (70, 150)]
TYPES = {torch.uint8: 0, torch.float32: 1}


def garbage(shape, dtype):
    """a buffer that holds 0xA5 bytes on entry"""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t


def workspace(b, h, w):
    wbytes = int(N.load_filter().mi_filter_workspace_bytes(b, h, w))
    assert wbytes >= b * h * w * 8
    return garbage((wbytes,), torch.uint8), wbytes


def run_components(values, min_valid, max_diff, want_sizes=True):
    """(B, h, w) numpy frames through mi_filter_components -> (labels, sizes or None) as numpy"""
    v = gpu(np.asarray(values))
    b, h, w = v.shape
    labels = garbage((b, h, w), torch.int32)
    sizes = garbage((b, h, w), torch.int32) if want_sizes else None
    work, wbytes = workspace(b, h, w)
    N.call("mi_filter_components", v.data_ptr(), TYPES[v.dtype], b, h, w, float(min_valid), float(max_diff), labels.data_ptr(),
           None if sizes is None else sizes.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    torch.cuda.synchronize()
    return labels.cpu().numpy(), None if sizes is None else sizes.cpu().numpy()


def run_speckle(x, max_size, max_diff, min_valid, invalid_value, want_removed=True, in_place=False):
    v = gpu(np.asarray(x, np.float32))
    b, h, w = v.shape
    out = v if in_place else garbage((b, h, w), torch.float32)
    removed = garbage((b, h, w), torch.uint8) if want_removed else None
    work, wbytes = workspace(b, h, w)
    N.call("mi_filter_speckle", v.data_ptr(), b, h, w, float(min_valid), float(max_diff), int(max_size), float(invalid_value), out.data_ptr(),
           None if removed is None else removed.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if removed is None else removed.cpu().numpy()


def run_median(x, k, min_valid, invalid_value):
    v = gpu(np.asarray(x, np.float32))
    b, h, w = v.shape
    out = garbage((b, h, w), torch.float32)
    N.call("mi_filter_median", v.data_ptr(), b, h, w, k, float(min_valid), float(invalid_value), out.data_ptr(), N.stream_ptr())
    torch.cuda.synchronize()
    return (out.cpu().numpy(),)


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differ = got.view(np.uint8) != want.view(np.uint8)
    assert not differ.any(), f"{what}: {int(differ.sum())} bytes of {differ.size} differ from the oracle"


@pytest.mark.parametrize("h,w", SHAPES)
def test_components_are_the_oracle_bit_for_bit(h, w):
    for name in FO.PATTERNS:
        values, min_valid, max_diff, labels, sizes = FO.case(name, h, w)
        got = twice((name, h, w), lambda: run_components(values[None], min_valid, max_diff))
        same(got[0][0], labels, (name, h, w, "labels"))
        same(got[1][0], sizes, (name, h, w, "sizes"))
    for name in ("percolation0", "classes"):                                   # sizes NULL: the labels alone
        values, min_valid, max_diff, labels, _ = FO.case(name, h, w)
        got = run_components(values[None], min_valid, max_diff, want_sizes=False)
        assert got[1] is None
        same(got[0][0], labels, (name, h, w, "labels without sizes"))


@pytest.mark.parametrize("h,w", SHAPES)
def test_speckle_is_the_oracle_bit_for_bit(h, w):
    for name in FO.FLOAT_PATTERNS:
        values, min_valid, max_diff, _, sizes = FO.case(name, h, w)
        invalid = FO.invalid_for(min_valid)
        for max_size in (0, 1, 30, h * w):
            want = FO.speckle(values, max_size, max_diff, min_valid, invalid, sizes)
            got = twice((name, h, w, max_size), lambda: run_speckle(values[None], max_size, max_diff, min_valid, invalid))
            same(got[0][0], want[0], (name, h, w, max_size, "out"))
            same(got[1][0], want[1], (name, h, w, max_size, "removed"))
        want = FO.speckle(values, 30, max_diff, min_valid, invalid, sizes)
        got = run_speckle(values[None], 30, max_diff, min_valid, invalid, want_removed=False)
        assert got[1] is None
        same(got[0][0], want[0], (name, h, w, "removed NULL"))
        got = run_speckle(values[None], 30, max_diff, min_valid, invalid, in_place=True)
        same(got[0][0], want[0], (name, h, w, "in place"))
        same(got[1][0], want[1], (name, h, w, "in place, removed"))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("h,w", SHAPES)
def test_median_is_the_oracle_bit_for_bit(h, w, k):
    for name in FO.FLOAT_PATTERNS:
        values, min_valid, _, _, _ = FO.case(name, h, w)
        invalid = FO.invalid_for(min_valid)
        got = twice((name, h, w, k), lambda: run_median(values[None], k, min_valid, invalid))
        same(got[0][0], FO.median(values, k, min_valid, invalid), (name, h, w, k))


@pytest.mark.parametrize("names", [("constant", "spiral", "percolation0"), ("alternating", "comb", "percolation2")], ids="-".join)
@pytest.mark.parametrize("h,w", SHAPES)
def test_a_batch_of_three_frames_equals_the_three_runs_alone(h, w, names):
    cases = [FO.case(name, h, w) for name in names]
    frames = np.stack([c[0] for c in cases])
    labels, sizes = run_components(frames, 0.0, 1.0)
    out, removed = run_speckle(frames, 30, 1.0, 0.0, -1.0)
    med = run_median(frames, 5, 0.0, -1.0)[0]
    for b, (values, _, _, want_labels, want_sizes) in enumerate(cases):
        same(labels[b], want_labels, (names[b], h, w))
        same(sizes[b], want_sizes, (names[b], h, w))
        alone = run_components(values[None], 0.0, 1.0)
        same(labels[b], alone[0][0], (names[b], "alone"))
        same(sizes[b], alone[1][0], (names[b], "alone"))
        alone = run_speckle(values[None], 30, 1.0, 0.0, -1.0)
        same(out[b], alone[0][0], (names[b], "speckle alone"))
        same(removed[b], alone[1][0], (names[b], "removed alone"))
        same(out[b], FO.speckle(values, 30, 1.0, 0.0, -1.0, want_sizes)[0], (names[b], "speckle"))
        same(med[b], run_median(values[None], 5, 0.0, -1.0)[0][0], (names[b], "median alone"))
    u8 = np.stack([FO.classes(h, w), np.rot90(FO.classes(w, h)).copy(), FO.classes(h, w)[::-1].copy()])
    labels, sizes = run_components(u8, 1, 0)
    for b in range(3):
        want = FO.components(u8[b], 1, 0)
        same(labels[b], want[0], ("classes", b))
        same(sizes[b], want[1], ("classes", b))


def test_stereo_disparities():
    frames = np.stack([FO.stereo_disparity(40, 160, seed) for seed in (11, 21, 22)])
    labels, sizes = twice("stereo", lambda: run_components(frames, 0.0, 1.0))
    for b in range(3):
        want = FO.components(frames[b], 0.0, 1.0)
        same(labels[b], want[0], b)
        same(sizes[b], want[1], b)
        for max_size in (1, 30):
            got = run_speckle(frames[b][None], max_size, 1.0, 0.0, -1.0)
            want_out = FO.speckle(frames[b], max_size, 1.0, 0.0, -1.0, want[1])
            same(got[0][0], want_out[0], (b, max_size))
            same(got[1][0], want_out[1], (b, max_size))
        for k in (3, 5):
            same(run_median(frames[b][None], k, 0.0, -1.0)[0][0], FO.median(frames[b], k), (b, k))


def test_ops_give_the_same_bits_as_the_entries():
    frames = np.stack([FO.case(name, 37, 83)[0] for name in ("percolation0", "steps025", "hostile")])
    x = gpu(frames)
    labels, sizes = ops.filter_components(x.unsqueeze(1), 0.0, 0.5)
    want = run_components(frames, 0.0, 0.5)
    assert labels.shape == sizes.shape == (3, 1, 37, 83) and labels.dtype == sizes.dtype == torch.int32
    same(labels[:, 0].cpu().numpy(), want[0], "labels")
    same(sizes[:, 0].cpu().numpy(), want[1], "sizes")
    only, none = ops.filter_components(x, 0.0, 0.5, want_sizes=False)
    assert none is None and torch.equal(only, labels[:, 0])
    u8 = gpu(np.stack([FO.classes(37, 83)] * 2))
    assert torch.equal(ops.filter_components(u8, 1, 0)[1].cpu(), torch.from_numpy(np.stack([FO.components(FO.classes(37, 83), 1, 0)[1]] * 2)))
    out, removed = ops.filter_speckle(x, 30, 0.5, want_removed=True)
    want = run_speckle(frames, 30, 0.5, 0.0, -1.0)
    same(out.cpu().numpy(), want[0], "speckle")
    same(removed.cpu().numpy(), want[1], "removed")
    assert same_bits([ops.filter_speckle(x.unsqueeze(1), 30, 0.5)[:, 0]], [out])
    depth = ops.filter_speckle(x, 30, 0.5, min_valid=0.25, invalid_value=0.0)          # a depth frame: min_depth, 0 for "no depth"
    same(depth.cpu().numpy(), np.stack([FO.speckle(f, 30, 0.5, 0.25, 0.0)[0] for f in frames]), "depth frame")
    for k in (3, 5):
        same(ops.filter_median(x, k).cpu().numpy(), run_median(frames, k, 0.0, -1.0)[0], k)
    assert ops.filter_median(x.unsqueeze(1)).shape == (3, 1, 37, 83)
    with pytest.raises(RuntimeError):
        ops.filter_median(x, 4)                                                # MI_E_PARAM, no fall-back
    with pytest.raises(RuntimeError):
        ops.filter_speckle(x, 30, 1.0, invalid_value=1.0)


def test_speckle_and_median_replay_from_one_graph():
    sets = [gpu(FO.stereo_disparity(40, 160, seed)[None]) for seed in (11, 21, 22)]
    f = DisparityFilter(speckle_size=30, speckle_range=1.0, median=3)
    code0 = torch.zeros((1, 40, 160), dtype=torch.uint8, device=DEV)

    def run(x):
        return f(x, code0)
    eager = [[t.clone() for t in run(s)] for s in sets]
    static = sets[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(static)
    for i in (1, 2, 0):
        static.copy_(sets[i])
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[i]), i
    want = FO.disparity_filter(sets[0][0].cpu().numpy(), code0[0].cpu().numpy(), 30, 1.0, 3)
    same(out[0][0].cpu().numpy(), want[0], "graph, disparity")
    same(out[1][0].cpu().numpy(), want[1], "graph, code")


def wrong_pixels(disparity, truth, visible):
    return (disparity >= 0) & (~visible | (np.abs(disparity - truth) > 1))


def test_stereo_matcher_with_the_speckle_filter_and_the_property():
    """StereoMatcher(speckle_size=30) is the oracle composition bit for bit; its depth through ops.depth_to_points equals the
    unfiltered chain wherever nothing was removed; and on the textureless patch the kernels give the oracle's figures: at least
    a third fewer wrong pixels in the patch, at most 8 correct pixels lost outside it (see tests/test_filter_host.py)"""
    scenes = [synth_textureless_pair(seed, 40, 160) for seed in (0, 1, 2)]
    left, right = gpu(np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]))
    plain, filtered = StereoMatcher(max_disparity=64), StereoMatcher(max_disparity=64, speckle_size=30, speckle_range=1.0)
    d0, c0 = plain(left, right)
    d1, c1 = filtered(left, right)
    assert d1.shape == c1.shape == (3, 40, 160) and c1.dtype == torch.uint8
    fx, baseline = 100.0, 0.17
    u_tab = ((torch.arange(160, dtype=torch.float32) - 79.5) / fx).to(DEV)
    v_tab = ((torch.arange(40, dtype=torch.float32) - 19.5) / fx).to(DEV)
    p0 = ops.depth_to_points(plain.depth(d0, fx, baseline), u_tab, v_tab, 1.0).cpu().numpy()
    p1 = ops.depth_to_points(filtered.depth(d1, fx, baseline), u_tab, v_tab, 1.0).cpu().numpy()
    d0, c0, d1, c1 = (t.cpu().numpy() for t in (d0, c0, d1, c1))
    for b, (l, r, truth, visible, patch) in enumerate(scenes):
        o = SO.run(l, r, 64, 8)
        same(d0[b], o["disparity"], (b, "unfiltered"))
        want_d, want_c = FO.disparity_filter(o["disparity"], o["code"], 30, 1.0)
        same(d1[b], want_d, (b, "disparity"))
        same(c1[b], want_c, (b, "code"))
        removed = c1[b] == ops.FILTER_SPECKLE
        assert removed.any() and np.array_equal(removed, (d0[b] >= 0) & (d1[b] < 0))
        assert np.array_equal(p1[b][~removed].view(np.uint32), p0[b][~removed].view(np.uint32)) and not p1[b][removed].any()
        w0, w1 = wrong_pixels(d0[b], truth, visible), wrong_pixels(d1[b], truth, visible)
        lost = (d0[b] >= 0) & ~w0 & ~((d1[b] >= 0) & ~w1) & ~patch
        print(f"seed {b}: wrong pixels in the patch {int(w0[patch].sum())} -> {int(w1[patch].sum())}, correct pixels lost outside it {int(lost.sum())}")
        assert 3 * w1[patch].sum() <= 2 * w0[patch].sum() and lost.sum() <= 8
    both = StereoMatcher(max_disparity=64, speckle_size=30, median=3)(left[:1], right[:1])
    o = SO.run(scenes[0][0], scenes[0][1], 64, 8)
    want_d, want_c = FO.disparity_filter(o["disparity"], o["code"], 30, 1.0, 3)
    same(both[0][0].cpu().numpy(), want_d, "median, then speckle")
    same(both[1][0].cpu().numpy(), want_c, "median, then speckle: code")
