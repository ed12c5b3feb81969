"""K14 rates: the fused Otsu (histogram + search + bin_img) and the 3-class multi-Otsu over 255 bins (histogram + search)
on 16 uint8 frames of 480x640 in one call each beat a torch-on-GPU formulation of the same operation written here from
stock ops and run frame by frame, as the reference's modules work.  Two formulations are timed per operation -- the
reference's masked form (BINS x BINS masks; the (n_class, COMBINATIONS, BINS) mask) and a bincount + cumsum form that
scores every candidate from prefix sums as the kernels do -- and the faster one is the yardstick; the test prints which.
Reported without a condition (no stock formulation exists): Otsu over the 16-bit range and 4-class multi-Otsu at 255 bins."""
import itertools

import numpy as np
import torch

from test_threshold_host import combinations_lex
from gpu_common import DEV, GPU_PERF, time_ms
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_threshold_frame

pytestmark = GPU_PERF
H, W, FRAMES = 480, 640, 16
MULTI_BINS, MULTI_CLASSES = 255, 3


def torch_histogram(img, bins):
    """the reference's calc_histogram: scatter_add of ones"""
    idx = img.reshape(-1).to(torch.int64)
    return torch.zeros(bins, device=img.device, dtype=torch.int64).scatter_add(0, idx, torch.ones_like(idx))


def torch_otsu_masked(img, c):
    """the reference's OtsuThreshold.forward, masks built once"""
    hist = torch_histogram(img, 256)
    hist_class = hist * c["vals256"]
    num_bk = torch.sum(hist * c["mask_bk"], dim=1)
    mean_bk = torch.sum(hist_class * c["mask_bk"], dim=1) / num_bk
    num_wh = torch.sum(hist * c["mask_wh"], dim=1)
    mean_wh = torch.sum(hist_class * c["mask_wh"], dim=1) / num_wh
    var = num_bk * num_wh * ((mean_bk - mean_wh) ** 2)
    thresh = torch.argmax(torch.where(torch.isnan(var), c["zero32"], var))
    return thresh, torch.where(img <= thresh, c["lo"], c["hi"])


def torch_otsu_cumsum(img, c):
    """the same float32 scores from bincount + cumsum"""
    hist = torch.bincount(img.reshape(-1).to(torch.int64), minlength=256)
    num_bk = torch.cumsum(hist, 0)
    fc_bk = torch.cumsum(hist * c["vals256"], 0)
    num_wh = num_bk[-1] - num_bk
    fc_wh = fc_bk[-1] - fc_bk
    var = num_bk * num_wh * ((fc_bk / num_bk - fc_wh / num_wh) ** 2)
    thresh = torch.argmax(torch.where(torch.isnan(var), c["zero32"], var))
    return thresh, torch.where(img <= thresh, c["lo"], c["hi"])


def torch_multi_masked(img, c):
    """the reference's MultiOtsuThreshold.forward with calc_hist=True, mask built once"""
    hist = torch_histogram(img, MULTI_BINS).to(torch.float32)
    fc_sum = torch.sum(hist * c["cls_val"] * c["mask"], dim=2)
    num = torch.sum(hist * c["mask"], dim=2)
    mean = fc_sum / num
    var = torch.zeros(c["mask"].shape[1], dtype=torch.float32, device=img.device)
    for i, j in itertools.combinations(range(MULTI_CLASSES), 2):
        var += num[i, :] * num[j, :] * ((mean[i, :] - mean[j, :]) ** 2)
    best = torch.argmax(torch.where(torch.isnan(var), c["zero32"], var))
    return c["combos"][best] - 1


def torch_multi_cumsum(img, c):
    """every candidate from two prefix sums, fp64, in the kernels' order"""
    hist = torch.bincount(img.reshape(-1).to(torch.int64), minlength=MULTI_BINS + 1)[:MULTI_BINS]
    zero = torch.zeros(1, dtype=torch.int64, device=img.device)
    pn = torch.cat([zero, torch.cumsum(hist, 0)])
    ps = torch.cat([zero, torch.cumsum(hist * c["vals255"], 0)])
    n = (pn[c["hi_idx"]] - pn[c["lo_idx"]])                        # (COMBINATIONS, n_class)
    s = (ps[c["hi_idx"]] - ps[c["lo_idx"]])
    nf = n.to(torch.float64)
    m = s.to(torch.float64) / nf
    var = torch.zeros(n.shape[0], dtype=torch.float64, device=img.device)
    for i, j in itertools.combinations(range(MULTI_CLASSES), 2):
        d = m[:, i] - m[:, j]
        var = var + (nf[:, i] * nf[:, j]) * (d * d)
    var = torch.where((n == 0).any(1), c["zero64"], var)
    return c["combos"][torch.argmax(var)] - 1


def workload(frames=FRAMES, seed=700):
    """frames (frames, H, W) uint8 with values below 255 on the GPU, and the constants of the torch formulations"""
    host = np.stack([synth_threshold_frame(seed + i, H, W, "trimodal", levels=MULTI_BINS) for i in range(frames)])
    combos = combinations_lex(MULTI_BINS - 1, MULTI_CLASSES - 1).astype(np.int64)
    bounds = np.concatenate([np.zeros((len(combos), 1), np.int64), combos, np.full((len(combos), 1), MULTI_BINS, np.int64)], 1)
    mask_idx = (np.arange(MULTI_BINS)[None, :] >= combos[:, :1]).astype(np.int8) + (np.arange(MULTI_BINS)[None, :] >= combos[:, 1:])
    mask_idx = torch.from_numpy(mask_idx).to(DEV)
    mask_bk = torch.tril(torch.ones([256, 256], dtype=torch.int32, device=DEV))
    return dict(frames=torch.from_numpy(host).to(DEV), host=host,
                vals256=torch.arange(256, dtype=torch.int64, device=DEV), vals255=torch.arange(255, dtype=torch.int64, device=DEV),
                cls_val=torch.arange(255, dtype=torch.float32, device=DEV), mask_bk=mask_bk, mask_wh=1 - mask_bk,
                zero32=torch.tensor(0, dtype=torch.float32, device=DEV), zero64=torch.tensor(0, dtype=torch.float64, device=DEV),
                lo=torch.tensor(0, dtype=torch.int32, device=DEV), hi=torch.tensor(255, dtype=torch.int32, device=DEV),
                mask=torch.stack([(mask_idx == i).to(torch.float32) for i in range(MULTI_CLASSES)]),
                combos=torch.from_numpy(combos).to(DEV), lo_idx=torch.from_numpy(bounds[:, :-1].copy()).to(DEV),
                hi_idx=torch.from_numpy(bounds[:, 1:].copy()).to(DEV))


def operations(t):
    """name -> (hip callable, {torch formulation name: callable}) on the workload's frames"""
    x = t["frames"]
    per_frame = [x[i] for i in range(x.shape[0])]
    return {
        "otsu": (lambda: ops.otsu(x, 0, 255, torch.int32),
                 {"BINS x BINS masks": lambda: [torch_otsu_masked(f, t) for f in per_frame],
                  "bincount + cumsum": lambda: [torch_otsu_cumsum(f, t) for f in per_frame]}),
        "multi-otsu 3 x 255": (lambda: ops.multi_otsu_threshold(ops.histogram(x, 0, MULTI_BINS), 0, MULTI_CLASSES),
                               {"combination mask": lambda: [torch_multi_masked(f, t) for f in per_frame],
                                "bincount + cumsum": lambda: [torch_multi_cumsum(f, t) for f in per_frame]}),
    }


def unmeasured_operations(t):
    """name -> hip callable: what no stock formulation can run"""
    x16 = torch.from_numpy(t["host"].astype(np.uint16) * 257).to(DEV)          # the same content over the 16-bit range
    hist = ops.histogram(t["frames"], 0, MULTI_BINS)
    return {"otsu over 65536 bins (uint16 frames)": lambda: ops.otsu(x16, 0, 65535, torch.int32),
            "multi-otsu 4 x 255 (2.7 M candidates, search only)": lambda: ops.multi_otsu_threshold(hist, 0, 4)}


def test_torch_formulations_compute_the_same_thing():
    """the yardsticks are formulations of the same operations: the float32 Otsu forms and the fp64 prefix-sum multi-Otsu
    form return the kernels' thresholds; the reference's float32 mask sums may settle a near-tie one bin away"""
    t = workload(2)
    x = t["frames"]
    thresh, img = ops.otsu(x, 0, 255, torch.int32)
    multi = ops.multi_otsu_threshold(ops.histogram(x, 0, MULTI_BINS), 0, MULTI_CLASSES)
    for b in range(2):
        for fn in (torch_otsu_masked, torch_otsu_cumsum):
            tt, ti = fn(x[b], t)
            assert int(tt) == int(thresh[b]) and torch.equal(ti, img[b]), fn.__name__
        assert torch_multi_cumsum(x[b], t).tolist() == multi[b].tolist()
        assert (torch_multi_masked(x[b], t) - multi[b]).abs().max() <= 1


def test_hip_thresholds_beat_torch_on_gpu_for_sixteen_frames():
    t = workload()
    failed = []
    for name, (hip_fn, torch_fns) in operations(t).items():
        hip = time_ms(hip_fn)
        refs = {k: time_ms(fn) for k, fn in torch_fns.items()}
        best = min(refs, key=refs.get)
        print(f"{name}: 16 frames HIP {hip:.3f} ms; torch-on-GPU " + ", ".join(f"{k} {v:.3f} ms" for k, v in refs.items())
              + f"; yardstick: {best} ({refs[best] / hip:.1f}x)")
        if not hip < refs[best]:
            failed.append(name)
    for name, hip_fn in unmeasured_operations(t).items():
        print(f"{name}: 16 frames HIP {time_ms(hip_fn):.3f} ms (no torch formulation can run it)")
    assert not failed, failed
