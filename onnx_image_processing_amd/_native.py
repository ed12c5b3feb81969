"""ctypes binding of lib/libmi355x_match.so (the C ABI in include/mi355x_match.h).

PyTorch is plumbing only: it owns device memory and the HIP stream; every compute call
goes through the C ABI with raw device pointers.  There is no CPU or eager fallback: if the
library is missing or a tensor is not on the GPU the call raises.

The binding is DERIVED from the two headers at import (read_header): argument and return types of every MI_API
declaration, the fields of mi_match_params, and every MI_* enum member and numeric macro as a module attribute.
Declaring an entry point or a limit in the header is all a new kernel needs here.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_uint32, c_void_p

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_PKG), "include")
# MI355X_MATCH_LIB: development hook (A/B timing of two builds on one box); the default is the in-tree build
LIB_PATH = os.environ.get("MI355X_MATCH_LIB") or os.path.join(_PKG, "lib", "libmi355x_match.so")


class MatchParams(ctypes.Structure):
    """mi_match_params (include/mi355x_match.h): the hyper-parameters of the whole path for mi_match_pairs.  Its
    _fields_ are read from the header's typedef below."""


# The closed type map of the headers.  Anything else is an error at import, not a guess.
_SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "uint32_t": c_uint32,
            "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "mi_stream_t": c_void_p}
# Pointer parameters: `[const] int *` and `const double *` are the header's HOST-array convention (device integers are
# declared int32_t / uint32_t there, and a `double *` the library writes is device memory: the fp64 sums of the
# linearisations); every other pointer is an address handed through as c_void_p.
_POINTER_ARGS = {"int": POINTER(c_int), "const int": POINTER(c_int), "const double": POINTER(c_double),
                 "const mi_match_params": POINTER(MatchParams)}
_NUMBER = re.compile(r"[-+]?(?:(\d+)|(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?f?)$")


def _ctype(text: str, where: str, returns: bool = False):
    """The ctypes type of a C type as the headers spell it (`const float *`, `long long`, ...)."""
    spelled = " ".join(text.replace("*", " ").split())
    base = spelled.removeprefix("const ")
    if "*" in text:
        if returns:
            return c_char_p if base == "char" else c_void_p
        return _POINTER_ARGS.get(spelled, c_void_p)
    if base not in _SCALARS:
        raise TypeError(f"{where}: the type '{text.strip()}' is outside the binding's type map")
    return _SCALARS[base]


def _typed_names(decls: list, where: str) -> list:
    """['const float *image', 'int n', ...] -> [('image', c_void_p), ('n', c_int), ...]"""
    out = []
    for d in decls:
        m = re.fullmatch(r"(.*?)(\w+)", d.strip(), flags=re.S)
        if m is None:
            raise TypeError(f"{where}: cannot read '{d.strip()}'")
        out.append((m.group(2), _ctype(m.group(1), where)))
    return out


def read_header(text: str):
    """C header text -> (signatures: name -> argtypes, restypes: name -> return type, struct fields of mi_match_params or
    None, constants: MI_* name -> number).  Plain regular expressions over the comment-stripped text; every MI_API token
    must end up as one parsed declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MI_\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M):
        m = _NUMBER.match(value)
        if m:                                                 # MI_API's value is no number: not a constant
            constants[name] = int(value) if m.group(1) else float(value.rstrip("f"))
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for member in filter(None, (s.strip() for s in body.split(","))):
            m = re.fullmatch(r"(MI_\w+)\s*=\s*(-?\d+)", member)
            if m is None:
                raise TypeError(f"enum member '{member}': expected MI_NAME = integer")
            constants[m.group(1)] = int(m.group(2))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)       # the MI_API tokens left are the declarations'
    fields = None
    m = re.search(r"typedef\s+struct\s+mi_match_params\s*\{([^}]*)\}", text)
    if m:
        fields = _typed_names([f for f in m.group(1).split(";") if f.strip()], "mi_match_params")
    signatures, restypes = {}, {}
    for ret, name, params in re.findall(r"\bMI_API\s+([\w\s*]*?)(\w+)\s*\(([^;()]*)\)\s*;", text):
        restypes[name] = _ctype(ret, name, returns=True)
        args = [] if params.strip() == "void" else params.split(",")
        signatures[name] = [t for _, t in _typed_names(args, name)]
    tokens = len(re.findall(r"\bMI_API\b", text))
    if tokens != len(signatures):
        raise TypeError(f"{tokens} MI_API declarations, {len(signatures)} of them read: a declaration does not fit the reader")
    return signatures, restypes, fields, constants


def _read(name: str):
    with open(os.path.join(_INCLUDE, name)) as f:
        return read_header(f.read())


# name -> argtypes / name -> return type, as tests and tools read them
SIGNATURES, RESTYPES, MatchParams._fields_, _constants = _read("mi355x_match.h")
globals().update(_constants)            # MI_OK, MI_BAD_HARD, MI_SOLVER_NO_FORK, MI_POSE_MAX_N, MI_DOTS_MIN_EPSILON, ...
# include/mi355x_match_debug.h: test / tooling hooks -- exported only by lib/libmi355x_match_debug.so (debug_library()),
# not part of the product ABI; nothing in this package calls them
DEBUG_SIGNATURES, _debug_restypes, _, _ = _read("mi355x_match_debug.h")
RESTYPES.update(_debug_restypes)
# include/mi355x_match_sim3.h: the similarity-alignment section of the ABI (K30), a header and a library of its own
# (lib/libmi355x_match_sim3.so, load_sim3()): the product library exports include/mi355x_match.h and nothing else.  call()
# finds the library of a name by itself.  Its limits are SIM3_CONSTANTS["MI_SIM3_MAX_N"], ...: a dictionary.
SIM3_SIGNATURES, _sim3_restypes, _, SIM3_CONSTANTS = _read("mi355x_match_sim3.h")
RESTYPES.update(_sim3_restypes)
# include/mi355x_match_simgraph.h: the similarity pose-graph section (K31), laid out as K30's: lib/libmi355x_match_simgraph.so,
# load_simgraph(), SIMGRAPH_CONSTANTS["MI_SIMGRAPH_MAX_NODES"], ...
SIMGRAPH_SIGNATURES, _simgraph_restypes, _, SIMGRAPH_CONSTANTS = _read("mi355x_match_simgraph.h")
RESTYPES.update(_simgraph_restypes)
# include/mi355x_match_flow.h: the feature-tracking section (K32), laid out as K30's: lib/libmi355x_match_flow.so, load_flow(),
# FLOW_CONSTANTS["MI_FLOW_MAX_RADIUS"], ...
FLOW_SIGNATURES, _flow_restypes, _, FLOW_CONSTANTS = _read("mi355x_match_flow.h")
RESTYPES.update(_flow_restypes)
# include/mi355x_match_stereo.h: the stereo-depth section (K33), laid out as K30's: lib/libmi355x_match_stereo.so, load_stereo(),
# STEREO_CONSTANTS["MI_STEREO_MAX_DISPARITIES"], ...
STEREO_SIGNATURES, _stereo_restypes, _, STEREO_CONSTANTS = _read("mi355x_match_stereo.h")
RESTYPES.update(_stereo_restypes)
# include/mi355x_match_rectify.h: the camera-rectification section (K34), laid out as K30's: lib/libmi355x_match_rectify.so,
# load_rectify(), RECTIFY_CONSTANTS["MI_RECTIFY_OUTSIDE"], ...
RECTIFY_SIGNATURES, _rectify_restypes, _, RECTIFY_CONSTANTS = _read("mi355x_match_rectify.h")
RESTYPES.update(_rectify_restypes)
# include/mi355x_match_filter.h: the disparity post-filter section (K35), laid out as K30's: lib/libmi355x_match_filter.so,
# load_filter(), FILTER_CONSTANTS["MI_FILTER_SPECKLE"], ...
FILTER_SIGNATURES, _filter_restypes, _, FILTER_CONSTANTS = _read("mi355x_match_filter.h")
RESTYPES.update(_filter_restypes)

DEBUG_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_debug.so")
SIM3_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_sim3.so")
SIMGRAPH_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_simgraph.so")
FLOW_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_flow.so")
STEREO_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_stereo.so")
RECTIFY_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_rectify.so")
FILTER_LIB_PATH = os.path.join(_PKG, "lib", "libmi355x_match_filter.so")

_lib = None            # the library every call() goes through: the product, unless inside debug_library()
_product = None
_debug = None


def _open(path: str, signatures: dict) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP library is not built. Run "
            "`python -m onnx_image_processing_amd.build` (there is no CPU fallback)."
        )
    lib = ctypes.CDLL(path)
    for name, argtypes in signatures.items():
        fn = getattr(lib, name)            # AttributeError if the ABI and the binding diverge
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    return lib


def load() -> ctypes.CDLL:
    """The library in use (the product library unless a debug_library() block is active), loaded once; raises loudly
    when it has not been built."""
    global _lib, _product
    if _lib is None:
        if _product is None:
            _product = _open(LIB_PATH, SIGNATURES)
        _lib = _product
    return _lib


_sim3 = None


def load_sim3() -> ctypes.CDLL:
    """lib/libmi355x_match_sim3.so, the entries of include/mi355x_match_sim3.h, loaded once."""
    global _sim3
    if _sim3 is None:
        _sim3 = _open(SIM3_LIB_PATH, SIM3_SIGNATURES)
    return _sim3


_simgraph = None


def load_simgraph() -> ctypes.CDLL:
    """lib/libmi355x_match_simgraph.so, the entries of include/mi355x_match_simgraph.h, loaded once."""
    global _simgraph
    if _simgraph is None:
        _simgraph = _open(SIMGRAPH_LIB_PATH, SIMGRAPH_SIGNATURES)
    return _simgraph


_flow = None


def load_flow() -> ctypes.CDLL:
    """lib/libmi355x_match_flow.so, the entries of include/mi355x_match_flow.h, loaded once."""
    global _flow
    if _flow is None:
        _flow = _open(FLOW_LIB_PATH, FLOW_SIGNATURES)
    return _flow


_stereo = None


def load_stereo() -> ctypes.CDLL:
    """lib/libmi355x_match_stereo.so, the entries of include/mi355x_match_stereo.h, loaded once."""
    global _stereo
    if _stereo is None:
        _stereo = _open(STEREO_LIB_PATH, STEREO_SIGNATURES)
    return _stereo


_rectify = None


def load_rectify() -> ctypes.CDLL:
    """lib/libmi355x_match_rectify.so, the entries of include/mi355x_match_rectify.h, loaded once."""
    global _rectify
    if _rectify is None:
        _rectify = _open(RECTIFY_LIB_PATH, RECTIFY_SIGNATURES)
    return _rectify


_filter = None


def load_filter() -> ctypes.CDLL:
    """lib/libmi355x_match_filter.so, the entries of include/mi355x_match_filter.h, loaded once."""
    global _filter
    if _filter is None:
        _filter = _open(FILTER_LIB_PATH, FILTER_SIGNATURES)
    return _filter


def library_of(name: str) -> ctypes.CDLL:
    """The library that exports the entry `name`."""
    if name in FILTER_SIGNATURES:
        return load_filter()
    if name in RECTIFY_SIGNATURES:
        return load_rectify()
    if name in STEREO_SIGNATURES:
        return load_stereo()
    if name in FLOW_SIGNATURES:
        return load_flow()
    if name in SIM3_SIGNATURES:
        return load_sim3()
    return load_simgraph() if name in SIMGRAPH_SIGNATURES else load()


class debug_library:
    """with debug_library() as lib: ... -- tests / tools only.  Inside the block every call of this package goes through
    lib/libmi355x_match_debug.so (same sources, -DMI_DEBUG_HOOKS), whose mi_debug_* hooks select between equivalent
    kernel implementations; on exit the hooks are back at their defaults and the product library is in use again."""

    def __enter__(self) -> ctypes.CDLL:
        global _lib, _debug
        load()
        if _debug is None:
            _debug = _open(DEBUG_LIB_PATH, {**SIGNATURES, **DEBUG_SIGNATURES})
        self._outer = _lib
        _lib = _debug
        return _debug

    def __exit__(self, *exc) -> None:
        global _lib
        _debug.mi_debug_set(0, 0)                  # key 0: every selector back to the product's value, probes off
        _lib = self._outer


def use_debug_library() -> ctypes.CDLL:
    """tools/ only: switch this process to the debug library for good (debug_library() without the exit)."""
    return debug_library().__enter__()


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().mi_error_string(code)
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def dev(t: torch.Tensor, dtype: torch.dtype, what: str) -> int:
    """Device pointer of a contiguous GPU tensor of the expected dtype."""
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} must live on the GPU (got device {t.device}); this package has no CPU path"
        )
    if t.dtype != dtype:
        raise RuntimeError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    return t.data_ptr()


def opt(t: torch.Tensor | None, dtype: torch.dtype, what: str) -> int | None:
    """dev() of an optional tensor: None (a NULL pointer) for None."""
    return None if t is None else dev(t, dtype, what)


_timers: dict | None = None


_timed_names = None


def enable_timing(on: bool, only=None) -> None:
    """Bracket C-ABI calls with HIP events on the launch stream (bench.py's per-kernel clock): every call, or
    only the entry points named in `only`.  Off by default: no events, no overhead."""
    global _timers, _timed_names
    _timers = {} if on else None
    _timed_names = set(only) if (on and only) else None


def timings_ms() -> dict:
    """name -> list of elapsed milliseconds, one per call (synchronises)."""
    torch.cuda.synchronize()
    return {k: [s.elapsed_time(e) for s, e in v] for k, v in (_timers or {}).items()}


def call(name: str, *args) -> None:
    fn = getattr(library_of(name), name)
    if _timers is None or (_timed_names is not None and name not in _timed_names):
        check(fn(*args), name)
        return
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()                     # torch's current stream == the stream passed to the ABI
    rc = fn(*args)
    end.record()
    check(rc, name)
    _timers.setdefault(name, []).append((start, end))
