#!/usr/bin/env python3
"""Generate tests/golden/threshold.npz by RUNNING THE REFERENCE threshold modules on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_threshold.py

Frames come from onnx_image_processing_amd/synth.py (synth_threshold_frame: six content families) and are stored verbatim
next to the reference's outputs, so the fixture does not depend on the generator staying as it is.

Otsu cases <name> (OtsuThreshold(0, max_val), max_val = 255, and one 12-bit case with max_val = 4095):
    <name>__frame (H, W) uint8 / uint16, <name>__family, <name>__max_val, <name>__thresh (int64),
    <name>__bin_img (H, W) int32.  The reference is run with dtype int32 and, for the 8-bit cases, uint8 and float32 as
    well, on the integer frame and on the same frame as float32: all must agree, or the generator stops.
Multi-Otsu cases <name> (MultiOtsuThreshold(0, BINS, n_class=n, calc_hist=True) for (n, BINS) in (2, 64), (3, 64),
(3, 255), (4, 32); frames with BINS levels):
    <name>__frame, <name>__family, <name>__n_class, <name>__hist (BINS,) int64 -- the reference's calc_histogram --,
    <name>__thresholds (n - 1,) int64, <name>__differs (1 when the fp64 definition of tests/test_threshold_host.py picks
    another tuple than the reference's float32 sums: the case stays, flagged).
One more (3, 255) case runs the reference on the histogram of a 480x640 frame (calc_hist=False, float32 counts as the
reference takes them); only its histogram is stored.  Recorded: torch version, thread count."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference/pytorch_model/threshold")

import torch  # noqa: E402

from multi_otsu import MultiOtsuThreshold  # noqa: E402
from otsu import OtsuThreshold  # noqa: E402

sys.path.insert(1, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from onnx_image_processing_amd.synth import THRESHOLD_FAMILIES, synth_threshold_frame  # noqa: E402
from test_threshold_host import multi_otsu_oracle  # noqa: E402

OUT = os.path.join(HERE, "threshold.npz")
# (seed, h, w) per family for the 8-bit Otsu cases: the full small size and an odd one
OTSU_SIZES = ((61, 48, 64), (62, 37, 53))
MULTI = ((2, 64), (3, 64), (3, 255), (4, 32))
MULTI_SIZES = ((71, 48, 64), (72, 29, 41))


def main():
    store = {"meta__torch_version": np.array(torch.__version__), "meta__threads": np.int64(torch.get_num_threads())}
    otsu_names, multi_names = [], []

    models = {dt: OtsuThreshold(0, 255, dtype=dt) for dt in (torch.int32, torch.uint8, torch.float32)}
    for family in THRESHOLD_FAMILIES:
        for seed, h, w in OTSU_SIZES:
            frame = synth_threshold_frame(seed, h, w, family)
            name = f"otsu_{family}_{h}x{w}"
            thresh, bin_img = models[torch.int32](torch.from_numpy(frame))
            for dt, model in models.items():
                for x in (torch.from_numpy(frame), torch.from_numpy(frame.astype(np.float32))):
                    t2, b2 = model(x)
                    assert int(t2) == int(thresh) and b2.dtype == dt and torch.equal(b2.to(torch.int32), bin_img), (name, dt)
            store.update({f"{name}__frame": frame, f"{name}__family": np.array(family), f"{name}__max_val": np.int64(255),
                          f"{name}__thresh": np.int64(int(thresh)), f"{name}__bin_img": bin_img.numpy()})
            otsu_names.append(name)
            print(f"{name:36s} thresh {int(thresh)}")
    frame = synth_threshold_frame(63, 24, 32, "trimodal", levels=4096)
    name = "otsu_trimodal_12bit_24x32"
    x = torch.from_numpy(frame.astype(np.int32))
    thresh, bin_img = OtsuThreshold(0, 4095)(x)
    assert bin_img.dtype == torch.int32
    store.update({f"{name}__frame": frame, f"{name}__family": np.array("trimodal"), f"{name}__max_val": np.int64(4095),
                  f"{name}__thresh": np.int64(int(thresh)), f"{name}__bin_img": bin_img.numpy()})
    otsu_names.append(name)
    print(f"{name:36s} thresh {int(thresh)}")

    flagged = 0
    for n_class, bins in MULTI:
        model = MultiOtsuThreshold(0, bins, n_class=n_class, calc_hist=True)
        for family in THRESHOLD_FAMILIES:
            for seed, h, w in MULTI_SIZES:
                frame = synth_threshold_frame(seed, h, w, family, levels=bins)
                name = f"multi_{n_class}x{bins}_{family}_{h}x{w}"
                hist = model.calc_histogram(torch.from_numpy(frame))
                th = np.array([int(t) for t in model(torch.from_numpy(frame))], np.int64)
                hist = hist.numpy().astype(np.int64)
                differs = int(multi_otsu_oracle(hist, 0, n_class) != [int(t) for t in th])
                flagged += differs
                store.update({f"{name}__frame": frame, f"{name}__family": np.array(family), f"{name}__n_class": np.int64(n_class),
                              f"{name}__hist": hist, f"{name}__thresholds": th, f"{name}__differs": np.int64(differs)})
                multi_names.append(name)
                print(f"{name:36s} thresholds {th.tolist()}{'  DIFFERS from the fp64 definition' if differs else ''}")
    full = synth_threshold_frame(73, 480, 640, "trimodal", levels=255)
    hist = np.bincount(full.reshape(-1), minlength=255).astype(np.int64)
    name = "multi_3x255_trimodal_480x640_hist"
    th = np.array([int(t) for t in MultiOtsuThreshold(0, 255, n_class=3)(torch.from_numpy(hist.astype(np.float32)))], np.int64)
    differs = int(multi_otsu_oracle(hist, 0, 3) != [int(t) for t in th])
    flagged += differs
    store.update({f"{name}__family": np.array("trimodal"), f"{name}__n_class": np.int64(3), f"{name}__hist": hist,
                  f"{name}__thresholds": th, f"{name}__differs": np.int64(differs)})
    multi_names.append(name)
    print(f"{name:36s} thresholds {th.tolist()}{'  DIFFERS' if differs else ''}")

    store["meta__full_frame_pixels"] = np.int64(full.size)
    store["meta__otsu_cases"] = np.array(otsu_names)
    store["meta__multi_cases"] = np.array(multi_names)
    np.savez_compressed(OUT, **store)
    print(f"{len(otsu_names)} Otsu cases, {len(multi_names)} multi-Otsu cases, {flagged} flagged")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
