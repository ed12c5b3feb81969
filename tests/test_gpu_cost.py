"""The cost stage (K5, csrc/cost.hip) against fp64 at every dispatch of its three entry points: the 64-tile float kernel
(L2 and L1), the 128-tile L2 kernel, and the bits kernel in its FP4, int8 and any-length forms, on both staging paths, up
to the longest descriptor the entry points accept.  Z is held to the a-priori fp32 bounds of cost_oracle.py (nothing
here is fitted to a measurement), the dot products and the Hamming pairs exactly, the per-descriptor (scale, squared
norm) pairs to 2 u / 5 u.

Every output is allocated one row longer at both ends and filled with a sentinel: the guard rows, and for Z the columns
m..pitch, must come back untouched.  Every call runs twice and must repeat bit for bit.  MI_REPORT=1 prints the worst
error / bound of each case.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

import cost_oracle as C
from gpu_common import DEV, gpu, mods, twice, up  # noqa: F401  (mods: the module fixture)

pytestmark = pytest.mark.gpu

EPSILONS = (1.0, 0.05)
MI_E_NULL, MI_E_SHAPE, MI_E_PARAM, MI_E_ALIGN = -1, -2, -3, -5


def _report(group, what, ratio):
    if os.environ.get("MI_REPORT"):
        print(f"[cost {group}] {what}: worst error / bound {ratio:.3g}")


# ------------------------------------------------------------------ guarded outputs
class _Out:
    """`rows` rows of `pitch` elements between two guard rows, all filled with the sentinel (NaN for float32, 0x7fff for
    the 16-bit dots)."""

    def __init__(self, rows, pitch, dtype):
        self.rows, self.pitch = rows, pitch
        fill = float("nan") if dtype == torch.float32 else 0x7FFF
        self.full = torch.full((rows + 2, pitch), fill, dtype=dtype, device=DEV)
        self.ptr = self.full[1].data_ptr()

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == 0x7FFF).all())

    def read(self, what, cols=None):
        """The payload as numpy, after checking the guard rows (and, with `cols`, that columns cols..pitch kept the
        sentinel)."""
        torch.cuda.synchronize()
        assert self.untouched(self.full[0]), f"{what}: the row in front of the output was written"
        assert self.untouched(self.full[-1]), f"{what}: the row behind the output was written"
        body = self.full[1:-1]
        if cols is not None and cols < self.pitch:
            assert self.untouched(body[:, cols:]), f"{what}: columns {cols}..{self.pitch} of the row padding were written"
        return body.cpu().numpy()


def _input(a, offset_elems=0):
    """A GPU copy of `a` (float32 or uint32) whose base sits `offset_elems` elements past an allocation's start:
    (keep-alive tensor, device pointer)."""
    flat = torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1))
    buf = torch.zeros(flat.numel() + offset_elems, dtype=torch.int32, device=DEV)
    buf[offset_elems:].copy_(flat)
    ptr = buf.data_ptr() + 4 * offset_elems
    assert buf.data_ptr() % 16 == 0 and ptr % 16 == (4 * offset_elems) % 16
    return buf, ptr


# ------------------------------------------------------------------ A - C. mi_cost_logscores_f32
def _batch_for(n, m):
    return 2 if min(n, m) >= 4 else 3          # tiny shapes carry one planted descriptor per batch member


def _f32_vs_fp64(N, group, n, m, d, distance, kind, offset=0):
    batch = _batch_for(n, m)
    a, b = C.float_inputs(kind, batch, n, m, d, distance)
    (keep_a, pa), (keep_b, pb) = _input(a, offset), _input(b)
    pitch = up(m + 1, 4)
    z1, bound1 = C.float_reference(a, b, distance, 1.0)
    for epsilon in EPSILONS:
        what = f"{C.DIST_NAME[distance]} {kind} {(n, m, d)} eps {epsilon}" + (" offset base" if offset else "")

        def run():
            out = _Out(batch * n, pitch, torch.float32)
            N.call("mi_cost_logscores_f32", pa, pb, batch, n, m, d, distance, float(epsilon), out.ptr, pitch, N.stream_ptr())
            return (out.read(what, cols=m),)
        (z,) = twice(what, run)
        z = z.reshape(batch, n, pitch)[:, :, :m]
        e = C.eps32(epsilon)
        ratio = C.worst_ratio(z, z1 / e, bound1 / e)
        _report(group, what, ratio)
        assert ratio <= 1.0, f"{what}: error {ratio:.3g} times the fp32 bound"
        assert (z <= 0).all(), f"{what}: a positive log-score (the clamp)"


KINDS = ["unit", "sigmoid"]
# n < 64, m < 64 (or an unaligned base, below): the 64-tile kernel
L2_TILE64 = [(1, 1, 1), (64, 63, 32), (65, 63, 33), (37, 130, 7), (63, 200, 40)]
# d % 4 == 0, n, m >= 64, aligned bases: the 128-tile kernel; (64, 200, 32) sits across the dispatch line from the
# (63, 200, 32) that the 64-tile test adds to its list
L2_TILE128 = [(64, 64, 4), (128, 128, 32), (129, 127, 36), (200, 257, 100), (64, 300, 512), (64, 200, 32)]
L1_SHAPES = [(1, 1, 1), (65, 63, 33), (64, 64, 32), (130, 67, 256), (37, 130, 7)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,d", L2_TILE64 + [(63, 200, 32)])
def test_l2_64_tile_kernel_vs_fp64(mods, n, m, d, kind):
    from onnx_image_processing_amd import _native as N
    _f32_vs_fp64(N, "A", n, m, d, 0, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_l2_unaligned_base_stays_on_the_64_tile_kernel_vs_fp64(mods, kind):
    """desc1 one float into its buffer: the base is 4-byte aligned only, so although n, m >= 64 and d % 4 == 0 the
    128-tile kernel's 16-byte loads must not run."""
    from onnx_image_processing_amd import _native as N
    _f32_vs_fp64(N, "A", 130, 67, 256, 0, kind, offset=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,d", L2_TILE128)
def test_l2_128_tile_kernel_vs_fp64(mods, n, m, d, kind):
    from onnx_image_processing_amd import _native as N
    _f32_vs_fp64(N, "B", n, m, d, 0, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,d", L1_SHAPES)
def test_l1_kernel_vs_fp64(mods, n, m, d, kind):
    from onnx_image_processing_amd import _native as N
    _f32_vs_fp64(N, "C", n, m, d, 1, kind)


# ------------------------------------------------------------------ D. mi_cost_logscores_bits and mi_cost_dots_bits
def _bits_vs_fp64(N, num_bits, n, m, offset=0, tag=""):
    words = num_bits // 32
    batch = _batch_for(n, m) if min(n, m) >= 8 else 3
    b1, b2 = C.bit_inputs(batch, n, m, words)
    (keep_a, pa), (keep_b, pb) = _input(b1, offset), _input(b2)
    want = C.bit_dots(b1, b2)
    assert want.max() <= num_bits and (want[0, 0, 0] == num_bits)          # all-ones against all-ones: the largest dot
    zp, dp = up(m + 1, 4), up(m, 8)
    for normalized in (True, False):
        what = f"{num_bits} bits {(n, m)} normalized {int(normalized)}{tag}"

        def run_dots():
            dots = _Out(batch * n, dp, torch.int16)
            ri, ci = _Out(batch * n, 2, torch.float32), _Out(batch * m, 2, torch.float32)
            N.call("mi_cost_dots_bits", pa, pb, batch, n, m, num_bits, int(normalized), dots.ptr, dp, ri.ptr, ci.ptr,
                   N.stream_ptr())
            return dots.read(what + " dots"), ri.read(what + " row_info"), ci.read(what + " col_info")
        dots, ri, ci = twice(what + " dots", run_dots)
        got = dots.view(np.uint16).reshape(batch, n, dp)[:, :, :m].astype(np.int64)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} dot products differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        for name, info, bits in (("row_info", ri, b1), ("col_info", ci, b2)):
            inv_err, nrm_err = C.info_errors(info.reshape(batch, -1, 2), bits, normalized)
            _report("D", f"{what} {name} scale error / 2u", inv_err / 2.0)
            _report("D", f"{what} {name} norm error / 5u", nrm_err / 5.0)
            assert inv_err <= 2.0, f"{what}: {name} scale off by {inv_err:.3g} u"
            assert nrm_err <= 5.0, f"{what}: {name} squared norm off by {nrm_err:.3g} u"

        z1, bound1 = C.bit_reference(b1, b2, normalized, 1.0)
        for epsilon in EPSILONS:
            def run_z():
                out = _Out(batch * n, zp, torch.float32)
                N.call("mi_cost_logscores_bits", pa, pb, batch, n, m, num_bits, int(normalized), float(epsilon), out.ptr, zp,
                       N.stream_ptr())
                return (out.read(what + " z", cols=m),)
            (z,) = twice(what + " z", run_z)
            z = z.reshape(batch, n, zp)[:, :, :m]
            e = C.eps32(epsilon)
            ratio = C.worst_ratio(z, z1 / e, bound1 / e)
            _report("D", f"{what} eps {epsilon}", ratio)
            assert ratio <= 1.0, f"{what} eps {epsilon}: error {ratio:.3g} times the fp32 bound"
            assert (z <= 0).all()


BIT_SHAPES = [(1, 1), (127, 129), (130, 67), (300, 513)]
# 32, 96, 160: words % 4 != 0 (scalar staging); 128; 256, 512: the FP4 forms; 992; 1024: 32 words, the last on the
# vector staging path; 1056: 33 words
BIT_LENGTHS = [32, 96, 160, 128, 256, 512, 992, 1024, 1056]
# 1952: 61 words, the last length whose tiles fit 64 KiB of LDS; 4096: the longest accepted, 134 144 bytes of LDS
BIT_LENGTHS_LONG = [1952, 2048, 4096]


@pytest.mark.parametrize("n,m", BIT_SHAPES)
@pytest.mark.parametrize("num_bits", BIT_LENGTHS)
def test_bits_kernel_vs_fp64(mods, num_bits, n, m):
    from onnx_image_processing_amd import _native as N
    _bits_vs_fp64(N, num_bits, n, m)


@pytest.mark.parametrize("num_bits", BIT_LENGTHS_LONG)
def test_bits_kernel_long_descriptors_vs_fp64(mods, num_bits):
    from onnx_image_processing_amd import _native as N
    _bits_vs_fp64(N, num_bits, 130, 67)


@pytest.mark.parametrize("n,m", BIT_SHAPES)
@pytest.mark.parametrize("num_bits", [256, 512])
def test_bits_kernel_int8_fixed_length_forms_vs_fp64(mods, num_bits, n, m):
    """Debug key 14 = 1: the WORDS = 8 / 16 instances on the int8 MFMA, which the product replaced by the FP4 forms."""
    from onnx_image_processing_amd import _native as N
    with N.debug_library() as lib:
        assert lib.mi_debug_set(14, 1) == 0
        _bits_vs_fp64(N, num_bits, n, m, tag=" int8")


def test_bits_kernel_unaligned_base_vs_fp64(mods):
    """bits1 one word into its buffer: scalar staging on a WORDS = 16 instance."""
    from onnx_image_processing_amd import _native as N
    _bits_vs_fp64(N, 512, 130, 67, offset=1, tag=" offset base")


# ------------------------------------------------------------------ E. argument checks
def _refused(lib, name, base, cases, outputs):
    """Every (change, code) of `cases` applied to the valid argument dict `base` returns `code`; no output is touched."""
    fn = getattr(lib, name)
    assert fn(*base.values()) == 0, f"{name}: the unchanged arguments are refused"
    torch.cuda.synchronize()
    for out in outputs:
        out.full.fill_(float("nan") if out.full.dtype == torch.float32 else 0x7FFF)
    for change, code in cases:
        args = {**base, **change}
        rc = fn(*args.values())
        assert rc == code, f"{name} with {change}: returned {rc}, expected {code}"
    torch.cuda.synchronize()
    for out in outputs:
        assert out.untouched(out.full), f"{name}: a refused call wrote to an output"


def test_argument_checks(mods):
    from onnx_image_processing_amd import _native as N
    lib = N.load()
    batch, n, m, d, words = 2, 9, 10, 8, 2
    a, b = C.float_inputs("unit", batch, n, m, d, 0)
    b1, b2 = C.bit_inputs(batch, n, m, words)
    (k1, pa), (k2, pb), (k3, qa), (k4, qb) = _input(a), _input(b), _input(b1), _input(b2)
    z = _Out(batch * n, 12, torch.float32)
    stream = N.stream_ptr()
    shared = [({"batch": 0}, MI_E_SHAPE), ({"batch": 65536}, MI_E_SHAPE), ({"n": 0}, MI_E_SHAPE), ({"m": -1}, MI_E_SHAPE),
              ({"a": None}, MI_E_NULL), ({"b": None}, MI_E_NULL)]
    z_cases = shared + [({"z": None}, MI_E_NULL), ({"pitch": 8}, MI_E_ALIGN), ({"pitch": 14}, MI_E_ALIGN),
                        ({"z": z.ptr + 4}, MI_E_ALIGN), ({"z": z.ptr + 8}, MI_E_ALIGN), ({"epsilon": 0.0}, MI_E_PARAM),
                        ({"epsilon": -0.05}, MI_E_PARAM), ({"epsilon": float("nan")}, MI_E_PARAM)]
    f32 = dict(a=pa, b=pb, batch=batch, n=n, m=m, d=d, distance=0, epsilon=0.05, z=z.ptr, pitch=12, stream=stream)
    _refused(lib, "mi_cost_logscores_f32", f32,
             z_cases + [({"d": 0}, MI_E_SHAPE), ({"d": -4}, MI_E_SHAPE), ({"distance": 2}, MI_E_PARAM),
                        ({"distance": -1}, MI_E_PARAM)], [z])
    bad_bits = [({"num_bits": 0}, MI_E_PARAM), ({"num_bits": 48}, MI_E_PARAM), ({"num_bits": 4128}, MI_E_PARAM),
                ({"num_bits": -32}, MI_E_PARAM)]
    bits = dict(a=qa, b=qb, batch=batch, n=n, m=m, num_bits=32 * words, normalized=1, epsilon=0.05, z=z.ptr, pitch=12,
                stream=stream)
    _refused(lib, "mi_cost_logscores_bits", bits, z_cases + bad_bits, [z])
    dots, ri, ci = _Out(batch * n, 16, torch.int16), _Out(batch * n, 2, torch.float32), _Out(batch * m, 2, torch.float32)
    dd = dict(a=qa, b=qb, batch=batch, n=n, m=m, num_bits=32 * words, normalized=1, dots=dots.ptr, pitch=16, row_info=ri.ptr,
              col_info=ci.ptr, stream=stream)
    _refused(lib, "mi_cost_dots_bits", dd,
             shared + bad_bits + [({"dots": None}, MI_E_NULL), ({"row_info": None}, MI_E_NULL), ({"col_info": None}, MI_E_NULL),
                                  ({"pitch": 8}, MI_E_ALIGN), ({"pitch": 12}, MI_E_ALIGN), ({"dots": dots.ptr + 8}, MI_E_ALIGN),
                                  ({"row_info": ri.ptr + 4}, MI_E_ALIGN), ({"col_info": ci.ptr + 4}, MI_E_ALIGN)],
             [dots, ri, ci])
