"""K14 thresholds on the MI355X against the numpy oracles of test_threshold_host.py (which reproduce the reference
fixture): histograms equal np.bincount exactly on both accumulation paths and at their boundary, Otsu equals the float32
oracle exactly (also at 65536 bins, which the reference cannot run), multi-Otsu equals the fp64 oracle exactly (also at
2.7 million candidates and on histograms whose gaps make exact ties), apply and bin_img in every dtype, the modules on
the fixture, determinism, dirty output and workspace buffers, and the fused Otsu captured into one graph.  Also meant to
run under MI_POISON_EMPTY=1 (conftest.py)."""
import numpy as np
import pytest
import torch

from test_threshold_host import (F32, apply_oracle, binary_oracle, golden, hist_oracle, multi_cases, multi_otsu_oracle,
                                 otsu_cases, otsu_oracle)
from gpu_common import DEV, GPU, gpu
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import THRESHOLD_FAMILIES, synth_threshold_frame

pytestmark = GPU
NP_DTYPES = {"uint8": np.uint8, "uint16": np.uint16, "int32": np.int32, "float32": np.float32}


def _values(seed, h, w, lo, hi):
    """int64 (h, w), uniform over [lo, hi)"""
    return np.random.default_rng(seed).integers(lo, hi, (h, w))


def _frame(seed, h, w, dtype, min_val, bins):
    """a frame of `dtype` whose values cover [min_val, min_val + bins) and overshoot it on both sides where the type
    allows, with both ends of the range present; float32 frames also carry fractions, NaN and infinities"""
    info = np.iinfo(np.int32 if dtype == "float32" else NP_DTYPES[dtype])
    lo, hi = max(min_val - 9, info.min), min(min_val + bins + 9, info.max + 1)
    v = _values(seed, h, w, lo, hi)
    flat = v.reshape(-1)
    if flat.size >= 2:
        flat[0], flat[-1] = min_val, min_val + bins - 1
    if dtype != "float32":
        return v.astype(NP_DTYPES[dtype])
    f = v.astype(F32) + np.where(v >= 0, F32(0.75), F32(-0.75)) * (np.abs(v) < 1 << 20)   # truncates back to v
    f = f.reshape(-1)
    if f.size >= 8:
        f[3], f[4], f[5], f[6] = np.nan, np.inf, -np.inf, 3e9
    return f.reshape(h, w)


def _check_hist(frames, min_val, bins, what):
    got = ops.histogram(gpu(frames), min_val, bins)
    assert got.dtype == torch.int64
    got = got.cpu().numpy()
    if frames.ndim < 3:
        assert got.shape == (bins,)
        assert np.array_equal(got, hist_oracle(frames, min_val, bins)), what
        return
    assert got.shape == (frames.shape[0], bins)
    for b in range(frames.shape[0]):
        assert np.array_equal(got[b], hist_oracle(frames[b], min_val, bins)), f"{what} frame {b}"


@pytest.mark.parametrize("h,w", [(1, 1), (1, 77), (37, 53), (9, 128), (480, 640)])
@pytest.mark.parametrize("dtype", list(NP_DTYPES))
def test_histogram_equals_bincount(h, w, dtype):
    frame = _frame(h * w, h, w, dtype, 0, 256)
    _check_hist(frame, 0, 256, f"{dtype} {h}x{w}")
    if h * w >= 1000 and dtype != "uint8":
        assert hist_oracle(frame, 0, 256).sum() < h * w                  # something was out of range and was dropped


@pytest.mark.parametrize("bins", [1, 2, 255, 256, 4096, 4097, 65536])
def test_histogram_bin_counts_on_both_paths_and_min_val(bins):
    """LDS sub-histograms up to 4096 bins (8 copies up to 1024 bins, then 4 and 2), global atomics above"""
    for dtype, min_val in (("uint16", 0), ("uint16", 7), ("int32", -5), ("float32", -3), ("int32", 100000)):
        if dtype == "uint16" and min_val + bins > 65536 + 7:
            continue
        frames = np.stack([_frame(bins + k, 37, 53, dtype, min_val, bins) for k in range(2)])
        _check_hist(frames, min_val, bins, f"{dtype} bins {bins} min_val {min_val}")
    frame = (_values(bins, 24, 40, 0, 300)).astype(np.uint8)               # wraps: still a uint8 frame
    _check_hist(frame, 3, min(bins, 256), f"uint8 bins {bins}")


@pytest.mark.parametrize("dtype", list(NP_DTYPES))
def test_histogram_of_a_constant_frame(dtype):
    """every pixel in one bin: the highest contention, on the LDS path and on the global path"""
    frame = np.full((480, 640), 77, NP_DTYPES[dtype])
    for bins in (256, 65536 if dtype != "uint8" else 200):
        got = ops.histogram(gpu(frame), 0, bins).cpu().numpy()
        assert got[77] == 480 * 640 and got.sum() == 480 * 640, (dtype, bins)
    assert int(ops.histogram(gpu(frame), 78, 100).sum()) == 0            # nothing in range: all zeros, not stale memory


def test_histogram_batch_equals_each_frame_alone():
    """5 frames of differing content whose starts are not 16-byte aligned (37 * 53 bytes each), and 3 full frames"""
    frames = np.stack([synth_threshold_frame(20 + k, 37, 53, THRESHOLD_FAMILIES[k]) for k in range(5)])
    batch = ops.histogram(gpu(frames), 0, 256)
    for b in range(5):
        alone = ops.histogram(gpu(frames[b]), 0, 256)
        assert torch.equal(alone, batch[b]) and np.array_equal(alone.cpu().numpy(), hist_oracle(frames[b], 0, 256)), b
    full = np.stack([synth_threshold_frame(30 + k, 480, 640, f) for k, f in enumerate(("trimodal", "uniform", "spikes"))])
    _check_hist(full, 0, 256, "480x640 batch")
    _check_hist(full.astype(np.uint16) * 257, 0, 65536, "480x640 uint16 batch, global path")
    # a sliced (non-contiguous) batch and an unaligned view
    sliced = ops.histogram(gpu(full)[:, 1:, 3:], 0, 256).cpu().numpy()
    assert np.array_equal(sliced, np.stack([hist_oracle(f[1:, 3:], 0, 256) for f in full]))
    flat = gpu(full.reshape(-1))
    assert np.array_equal(ops.histogram(flat[5:5 + 4001], 0, 256).cpu().numpy(), hist_oracle(full.reshape(-1)[5:4006], 0, 256))


def _otsu_gpu(hist, min_val):
    return ops.otsu_threshold(gpu(np.asarray(hist, np.int64)), min_val).cpu().numpy()


def test_otsu_equals_the_fixture_and_the_oracle():
    g = golden()
    for name in otsu_cases(g):
        frame, max_val = g[f"{name}__frame"], int(g[f"{name}__max_val"])
        hist = ops.histogram(gpu(frame), 0, max_val + 1)
        got = ops.otsu_threshold(hist, 0)
        assert got.dtype == torch.int32 and got.shape == ()
        assert int(got) == int(g[f"{name}__thresh"]) == otsu_oracle(hist.cpu().numpy(), 0)[0], name


def test_otsu_on_degenerate_and_gapped_histograms():
    rng = np.random.default_rng(3)
    hists = []
    one = np.zeros(256, np.int64)
    one[91] = 3072
    hists.append(one)                                                      # one occupied bin: every score NaN -> 0 -> bin 0
    two = np.zeros(256, np.int64)
    two[[40, 200]] = (1000, 2072)
    hists.append(two)                                                      # two occupied bins: a plateau of equal scores
    gaps = rng.integers(0, 4000, 256)
    gaps[rng.random(256) < 0.6] = 0
    hists.append(gaps)
    first = np.zeros(256, np.int64)
    first[[0, 255]] = (5, 9)
    hists.append(first)
    hists.append(np.zeros(256, np.int64))                                  # an empty histogram
    hists.append(rng.integers(0, 1 << 22, 256))                            # 5e8 pixels: the int64 product matters
    hists = np.stack(hists).astype(np.int64)
    for min_val in (0, 17, -40):
        want = [otsu_oracle(h, min_val)[0] for h in hists]
        assert _otsu_gpu(hists, min_val).tolist() == want, min_val
        for b in (1, 2):
            assert int(_otsu_gpu(hists[b], min_val)) == want[b]
    assert want[0] == -40 and want[1] == 0 and want[4] == -40
    for bins in (1, 2, 3, 255, 257, 1024, 1025, 5000):
        h = rng.integers(0, 1000, (2, bins))
        h[:, bins // 3: bins // 2] = 0
        assert _otsu_gpu(h, 5).tolist() == [otsu_oracle(x, 5)[0] for x in h], bins


def test_otsu_at_65536_bins():
    """uint16 depth counts over their whole range: 4.3e9 mask elements in the reference, one scan here"""
    frames = [synth_threshold_frame(41, 480, 640, "trimodal", levels=65536),
              synth_threshold_frame(42, 120, 160, "bimodal", levels=65536), np.full((120, 160), 65535, np.uint16)]
    want, hists = [], []
    for f in frames:
        hists.append(hist_oracle(f, 0, 65536))
        want.append(otsu_oracle(hists[-1], 0)[0])
    got_hist = ops.histogram(gpu(frames[0]), 0, 65536)
    assert np.array_equal(got_hist.cpu().numpy(), hists[0])
    assert _otsu_gpu(np.stack(hists), 0).tolist() == want
    assert 10000 < want[0] < 55000 and want[2] == 0
    thresh, bin_img = ops.otsu(gpu(frames[0]), 0, 65535, torch.int32)
    assert int(thresh) == want[0]
    assert np.array_equal(bin_img.cpu().numpy(), binary_oracle(frames[0], want[0], 0, 65535, np.int32))


def _gapped_hist(rng, bins, keep):
    h = rng.integers(1, 5000, bins)
    h[rng.random(bins) > keep] = 0
    return h.astype(np.int64)


@pytest.mark.parametrize("n_class,bins", [(n, b) for n in (2, 3, 4, 5) for b in (8, 33)] + [(3, 64), (3, 255), (5, 48)])
def test_multi_otsu_equals_the_fp64_oracle(n_class, bins):
    rng = np.random.default_rng(100 * n_class + bins)
    hists = [_gapped_hist(rng, bins, 1.0), _gapped_hist(rng, bins, 0.5), _gapped_hist(rng, bins, 0.15)]
    spikes = np.zeros(bins, np.int64)
    spikes[rng.choice(bins, n_class, replace=False)] = rng.integers(1, 100, n_class)        # exactly n_class occupied bins
    few = np.zeros(bins, np.int64)
    few[rng.choice(bins, n_class - 1, replace=False)] = 7                                   # every candidate scores 0
    frame = synth_threshold_frame(bins, 48, 64, "trimodal", levels=bins)
    hists += [spikes, few, hist_oracle(frame, 0, bins), rng.integers(0, 1 << 24, bins)]
    hists = np.stack(hists).astype(np.int64)
    for min_val in (0, 11):
        want = [multi_otsu_oracle(h, min_val, n_class) for h in hists]
        got = ops.multi_otsu_threshold(gpu(hists), min_val, n_class)
        assert got.dtype == torch.int32 and got.shape == (len(hists), n_class - 1)
        assert got.cpu().numpy().tolist() == want, (n_class, bins, min_val)
        alone = ops.multi_otsu_threshold(gpu(hists[1]), min_val, n_class)
        assert alone.shape == (n_class - 1,) and alone.cpu().numpy().tolist() == want[1]
    assert want[4] == [11 + k for k in range(n_class - 1)]                                  # all ties: the first combination


def test_multi_otsu_four_classes_at_255_bins():
    """2.7 million candidates per histogram, which the reference cannot build"""
    rng = np.random.default_rng(9)
    frame = synth_threshold_frame(51, 480, 640, "trimodal", levels=255)
    hists = np.stack([hist_oracle(frame, 0, 255), _gapped_hist(rng, 255, 0.3)])
    want = [multi_otsu_oracle(h, 0, 4) for h in hists]
    got = ops.multi_otsu_threshold(gpu(hists), 0, 4)
    assert got.cpu().numpy().tolist() == want


def test_multi_otsu_large_ranges_without_lds_prefix():
    """2 classes over 4096 and 65536 bins (prefix sums read from the workspace), 3 classes over 2048 (the last in LDS is 2047)"""
    rng = np.random.default_rng(10)
    for n_class, bins in ((2, 4096), (2, 65536), (3, 2047), (3, 2048)):
        h = _gapped_hist(rng, bins, 0.4)
        assert ops.multi_otsu_threshold(gpu(h), 0, n_class).cpu().numpy().tolist() == multi_otsu_oracle(h, 0, n_class), (n_class, bins)


def test_multi_otsu_on_the_fixture():
    g = golden()
    for name in multi_cases(g):
        hist, n_class = g[f"{name}__hist"], int(g[f"{name}__n_class"])
        got = ops.multi_otsu_threshold(gpu(hist), 0, n_class).cpu().numpy().tolist()
        assert got == multi_otsu_oracle(hist, 0, n_class), name
        if not int(g[f"{name}__differs"]):
            assert got == [int(t) for t in g[f"{name}__thresholds"]], name
        if f"{name}__frame" in g:
            assert np.array_equal(ops.histogram(gpu(g[f"{name}__frame"]), 0, hist.size).cpu().numpy(), hist), name


def test_apply_and_bin_img_equal_the_fixture_in_every_dtype():
    g = golden()
    outs = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32}
    for name in otsu_cases(g):
        frame, max_val = g[f"{name}__frame"], int(g[f"{name}__max_val"])
        want = g[f"{name}__bin_img"]
        for in_dtype in ("uint8", "uint16", "int32", "float32"):
            if in_dtype == "uint8" and max_val > 255:
                continue
            x = gpu(frame.astype(NP_DTYPES[in_dtype]))
            for dtype, npdt in outs.items():
                if dtype == torch.uint8 and max_val > 255:
                    continue
                thresh, bin_img = ops.otsu(x, 0, max_val, dtype)
                assert int(thresh) == int(g[f"{name}__thresh"]) and bin_img.dtype == dtype and bin_img.shape == frame.shape
                assert np.array_equal(bin_img.cpu().numpy(), want.astype(npdt)), (name, in_dtype, dtype)


def test_labels_equal_the_oracle():
    rng = np.random.default_rng(12)
    for dtype in NP_DTYPES:
        for h, w in ((1, 1), (37, 53), (9, 128)):
            frames = np.stack([_frame(7 * k + h, h, w, dtype, 0, 256) for k in range(3)])
            for n_thresh in (1, 2, 3, 4):
                th = np.sort(rng.integers(-3, 260, (3, n_thresh))).astype(np.int32)
                got = ops.threshold_apply(gpu(frames), gpu(th))
                assert got.dtype == torch.uint8 and got.shape == frames.shape
                for b in range(3):
                    assert np.array_equal(got[b].cpu().numpy(), apply_oracle(frames[b], th[b])), (dtype, h, w, n_thresh, b)
                one = ops.threshold_apply(gpu(frames[1]), gpu(th[1]))
                assert torch.equal(one, got[1])
            th1 = rng.integers(0, 256, 3).astype(np.int32)
            for out_dtype, npdt in ((torch.uint8, np.uint8), (torch.int32, np.int32), (torch.float32, np.float32)):
                got = ops.threshold_apply(gpu(frames), gpu(th1), binary=(3, 250, out_dtype)).cpu().numpy()
                for b in range(3):
                    assert np.array_equal(got[b], binary_oracle(frames[b], th1[b], 3, 250, npdt)), (dtype, h, w, out_dtype, b)
    nan = ops.threshold_apply(torch.full((4, 4), float("nan"), device=DEV), gpu(np.int32([5])), binary=(0, 255, torch.int32))
    assert bool((nan == 255).all())                                                         # torch.where(img <= thresh, ...)
    with pytest.raises(RuntimeError, match="uint8, uint16, int32 or float32"):
        ops.threshold_apply(torch.zeros(4, 4, device=DEV, dtype=torch.float64), gpu(np.int32([5])))
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.threshold_apply(torch.zeros(2, 4, 4, device=DEV), gpu(np.int32([5, 6, 7])))


def test_modules_reproduce_the_reference_fixture():
    from pytorch_model.threshold.multi_otsu import MultiOtsuThreshold
    from pytorch_model.threshold.otsu import OtsuThreshold
    g = golden()
    by_size = {}
    for name in otsu_cases(g):
        frame, max_val = g[f"{name}__frame"], int(g[f"{name}__max_val"])
        for dtype in (torch.int32, torch.float32) + ((torch.uint8,) if max_val <= 255 else ()):
            model = OtsuThreshold(0, max_val, dtype=dtype, device=DEV)
            thresh, bin_img = model(gpu(frame))
            assert thresh.dtype == torch.int64 and thresh.shape == () and int(thresh) == int(g[f"{name}__thresh"]), name
            assert bin_img.dtype == dtype and torch.equal(bin_img.to(torch.int32).cpu(), torch.from_numpy(g[f"{name}__bin_img"]))
            t2, b2 = model(gpu(frame.astype(np.float32)))                  # the reference's hosts also hand in float32
            assert int(t2) == int(thresh) and torch.equal(b2, bin_img)
        if max_val == 255:
            by_size.setdefault(frame.shape, []).append(name)
    for shape, names in by_size.items():                                    # a leading batch dimension
        frames = np.stack([g[f"{n}__frame"] for n in names])
        thresh, bin_img = OtsuThreshold(0, 255, device=DEV)(gpu(frames))
        assert thresh.shape == (len(names),) and thresh.cpu().tolist() == [int(g[f"{n}__thresh"]) for n in names]
        assert np.array_equal(bin_img.cpu().numpy(), np.stack([g[f"{n}__bin_img"] for n in names]))
    groups = {}
    for name in multi_cases(g):
        if int(g[f"{name}__differs"]):
            continue
        hist, n_class = g[f"{name}__hist"], int(g[f"{name}__n_class"])
        ref = [int(t) for t in g[f"{name}__thresholds"]]
        from_hist = MultiOtsuThreshold(0, hist.size, device=DEV, n_class=n_class)(gpu(hist))
        assert isinstance(from_hist, list) and len(from_hist) == n_class - 1
        assert all(t.dtype == torch.int64 and t.shape == () for t in from_hist) and [int(t) for t in from_hist] == ref, name
        as_float = MultiOtsuThreshold(0, hist.size, device=DEV, n_class=n_class)(gpu(hist.astype(np.float32)))
        assert [int(t) for t in as_float] == ref                             # float32 counts, as the reference takes them
        if f"{name}__frame" in g:
            frame = g[f"{name}__frame"]
            from_img = MultiOtsuThreshold(0, hist.size, device=DEV, n_class=n_class, calc_hist=True)(gpu(frame))
            assert [int(t) for t in from_img] == ref, name
            groups.setdefault((n_class, hist.size, frame.shape), []).append(name)
    for (n_class, bins, _), names in groups.items():
        frames = np.stack([g[f"{n}__frame"] for n in names])
        out = MultiOtsuThreshold(0, bins, device=DEV, n_class=n_class, calc_hist=True)(gpu(frames))
        assert len(out) == n_class - 1 and all(t.shape == (len(names),) for t in out)
        assert torch.stack(out, 1).cpu().tolist() == [[int(t) for t in g[f"{n}__thresholds"]] for n in names]


def test_two_runs_are_bit_identical_and_dirty_buffers_do_not_show():
    """The C entries take outputs and workspaces of any content."""
    frames = np.stack([synth_threshold_frame(80 + k, 37, 53, THRESHOLD_FAMILIES[k % 6], levels=200) for k in range(4)])
    x = gpu(frames)
    batch, pixels, s = 4, 37 * 53, N.stream_ptr
    runs = []
    for junk in (None, 0x00, 0xFF, 0x5A, 0x7F):
        def buf(nbytes):
            t = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            if junk is not None:
                t.fill_(junk)
            return t
        out = {}
        for bins in (200, 5000):
            hist = buf(batch * bins * 8)
            N.call("mi_histogram", x.data_ptr(), N.MI_PIX_U8, batch, pixels, 0, bins, hist.data_ptr(), s())
            out[f"hist{bins}"] = hist.view(torch.int64).reshape(batch, bins)
        hist = out["hist200"]
        thresh = buf(batch * 4)
        N.call("mi_otsu_threshold", hist.data_ptr(), batch, 200, 0, thresh.data_ptr(), s())
        out["thresh"] = thresh.view(torch.int32)
        for n_class in (3, 4):
            need = N.load().mi_multi_otsu_workspace_bytes(batch, 200, n_class)
            ws, th = buf(need), buf(batch * (n_class - 1) * 4)
            N.call("mi_multi_otsu_threshold", hist.data_ptr(), batch, 200, 0, n_class, th.data_ptr(), ws.data_ptr(), need, s())
            out[f"multi{n_class}"] = th.view(torch.int32).reshape(batch, n_class - 1)
        labels, img = buf(batch * pixels), buf(batch * pixels * 4)
        N.call("mi_threshold_apply", x.data_ptr(), N.MI_PIX_U8, batch, pixels, out["multi4"].data_ptr(), 3, N.MI_PIX_U8, 0, 0, 0,
               labels.data_ptr(), s())
        N.call("mi_threshold_apply", x.data_ptr(), N.MI_PIX_U8, batch, pixels, out["thresh"].data_ptr(), 1, N.MI_PIX_F32, 1, 0, 199,
               img.data_ptr(), s())
        out["labels"], out["img"] = labels, img.view(torch.int32)
        runs.append({k: v.cpu() for k, v in out.items()})
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), k
    first = runs[0]
    for b in range(batch):
        h = hist_oracle(frames[b], 0, 200)
        assert np.array_equal(first["hist200"][b].numpy(), h) and np.array_equal(first["hist5000"][b].numpy()[:200], h)
        assert int(first["thresh"][b]) == otsu_oracle(h, 0)[0]
        assert first["multi3"][b].tolist() == multi_otsu_oracle(h, 0, 3) and first["multi4"][b].tolist() == multi_otsu_oracle(h, 0, 4)
        assert np.array_equal(first["labels"].reshape(batch, 37, 53)[b].numpy(), apply_oracle(frames[b], first["multi4"][b].tolist()))


def test_fused_otsu_captured_in_one_graph():
    """ops.otsu on 4 frames as one straight-line graph (nothing is read back between histogram, search and apply):
    replayed on new frame content it equals the eager result on that content."""
    h, w, batch = 120, 160, 4
    first = gpu(np.stack([synth_threshold_frame(90 + k, h, w, THRESHOLD_FAMILIES[k]) for k in range(batch)]))
    second = gpu(np.stack([synth_threshold_frame(95 + k, h, w, THRESHOLD_FAMILIES[5 - k]) for k in range(batch)]))
    static = first.clone()

    def run(x):
        thresh, img = ops.otsu(x, 0, 255, torch.uint8)
        multi = ops.multi_otsu_threshold(ops.histogram(x, 0, 255), 0, 3)
        return thresh, img, multi, ops.threshold_apply(x, multi)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, run(first)):
        assert torch.equal(got, want)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(second)
    for got, want in zip(outs, eager):
        assert torch.equal(got, want)
    sec = second.cpu().numpy()
    for b in range(batch):
        hist = hist_oracle(sec[b], 0, 256)
        assert int(eager[0][b]) == otsu_oracle(hist, 0)[0]
        assert np.array_equal(eager[1][b].cpu().numpy(), binary_oracle(sec[b], int(eager[0][b]), 0, 255, np.uint8))
        assert eager[2][b].tolist() == multi_otsu_oracle(hist_oracle(sec[b], 0, 255), 0, 3)
