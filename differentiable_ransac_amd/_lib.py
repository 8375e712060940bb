"""ctypes binding of libdransac.so (C ABI declared in include/dransac.h).

The library is the product: there is no Python/CPU fallback.  `lib()` raises if the shared
object is missing or cannot be loaded; every wrapper raises `DransacError` on a non-zero status.
torch is imported first so that the HIP runtime torch ships (same SONAME, libamdhip64.so.7) is the
one the library binds to -- one runtime per process, shared streams and allocations.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_uint64, c_void_p
from typing import Optional

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DRANSAC_LIB") or os.path.join(_HERE, "libdransac.so")   # DRANSAC_LIB: A/B runs against another build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dransac.h")

_lib: Optional[ctypes.CDLL] = None


class DransacError(RuntimeError):
    pass


class c_pointer(c_void_p):
    """The argtype of every `T *` parameter: NULL (None), what ptr() / stream() return (a c_void_p), or a ctypes array or pointer
    (a host buffer).  Unlike c_void_p it refuses a Python int: an argument list shifted by one slot raises, it does not launch."""

    @staticmethod
    def from_param(v):      # runs once per pointer of every launch: the identity test first (what ptr() returns), no bound method
        if v.__class__ is c_void_p or v is None or isinstance(v, (c_void_p, ctypes.Array, ctypes._Pointer)):
            return v
        raise TypeError(f"a pointer slot takes None, a c_void_p (ptr(), stream()) or a ctypes array / pointer, not {type(v).__name__}")


_SCALARS = {"int": c_int, "int64_t": ctypes.c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double}
_UNTYPED = ("dr_version", "dr_last_error")      # int (void) and const char *(void): typed by hand in lib()


def parse_header(src: str) -> dict:
    """{entry: [argtype, ...]} of every `int dr_*(...)` declaration of a header text; a parameter type outside
    pointers / int / int64_t / uint64_t / float / double is an error, never a guess"""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for name, params in re.findall(r"\bint\s+(dr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        if name in _UNTYPED:
            continue
        out[name] = argtypes = []
        for prm in params.split(","):
            ctype = " ".join(re.match(r"(.*?)\w*$", " ".join(prm.split())).group(1).split())   # the parameter less its name
            if ctype.endswith("*"):
                argtypes.append(c_pointer)
            elif ctype in _SCALARS:
                argtypes.append(_SCALARS[ctype])
            else:
                raise DransacError(f"{name}: parameter `{' '.join(prm.split())}` has a type the binding does not know")
    return out


@functools.lru_cache(maxsize=None)
def entries() -> dict:
    """parse_header of include/dransac.h: the binding of the library is derived from its header"""
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise DransacError(f"{HEADER_PATH} cannot be read ({e.strerror}): the C entries are bound from this header") from None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DransacError(
                f"{LIB_PATH} not found: build it with `python -m differentiable_ransac_amd.build` "
                "(there is deliberately no CPU fallback)")
        handle = ctypes.CDLL(LIB_PATH)
        handle.dr_last_error.restype = c_char_p
        handle.dr_version.restype = c_int
        for name, argtypes in entries().items():
            fn = getattr(handle, name, None)        # (DRANSAC_LIB may name an older build: call() refuses what it lacks)
            if fn is not None:
                fn.restype, fn.argtypes = c_int, argtypes
        _lib = handle
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().dr_last_error().decode("utf-8", "replace")
        raise DransacError(f"{what} failed with status {status}: {msg}")


# Devices of the tensors whose pointers were taken since the last call(): every wrapper builds its argument list with
# ptr(...) ... stream() and hands it to call(), so call() can check that one launch never mixes GPUs and can make that
# GPU current for the launch (HIP launches on the CURRENT device, whatever device the pointers belong to).
_ctx = threading.local()


def _reset() -> None:
    _ctx.devs = set()
    _ctx.keep = []


def _devices() -> set:
    d = getattr(_ctx, "devs", None)
    if d is None:
        d = _ctx.devs = set()
    return d


def ptr(t: Optional[torch.Tensor]) -> c_void_p:
    """Device pointer of a contiguous CUDA tensor (None -> NULL).  The tensor is kept alive until the call() it is an
    argument of has enqueued its launch: `ptr(x.contiguous())` / `ptr(x.to(dtype))` create temporaries that would
    otherwise be freed as soon as ptr() returns, and the caching allocator would hand their block to the next temporary of
    the same argument list."""
    if t is None:
        return c_void_p(0)
    if not t.is_cuda or not t.is_contiguous():
        # the argument list this pointer belongs to will never reach call(): drop what its earlier ptr() calls recorded, or
        # the next call on this thread would see stale devices ("tensors of one call live on different GPUs") and pin tensors
        _reset()
        raise DransacError("libdransac operates on GPU tensors only (got a CPU tensor)" if not t.is_cuda
                           else "tensor must be contiguous")
    _devices().add(t.device.index)
    keep = getattr(_ctx, "keep", None)
    if keep is None:
        keep = _ctx.keep = []
    keep.append(t)
    return c_void_p(t.data_ptr())


def aligned(t: Optional[torch.Tensor], align: Optional[int] = None) -> Optional[torch.Tensor]:
    """`t` itself when its first byte sits on a multiple of `align` (default: four elements, the widest vector a kernel reads
    a row with), a fresh copy otherwise: a contiguous view may start anywhere inside a larger allocation
    (`packed[s:e]`, `flat[1:1 + n].view(...)`), and the kernels that read an input as float4 / float2 have no scalar form.
    Only for tensors a launch READS: a copy of a buffer that a launch writes would take the result with it."""
    if t is None:
        return None
    if not t.is_contiguous() or t.data_ptr() % (align or 4 * t.element_size()) == 0:      # (ptr() refuses a strided tensor)
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _launch_device() -> Optional[int]:
    devs = _devices()
    if len(devs) > 1:
        _reset()
        raise DransacError(f"tensors of one call live on different GPUs: {sorted(devs)}")
    return next(iter(devs)) if devs else None


def stream() -> c_void_p:
    """The current torch stream OF THE DEVICE THE CALL'S TENSORS LIVE ON (not of the current device)."""
    dev = _launch_device()
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def suffix(dtype: torch.dtype) -> str:
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    raise DransacError(f"unsupported dtype {dtype}: f32 and f64 only (SURVEY Q15)")


def scalar(dtype: torch.dtype, v: float):
    return c_float(v) if dtype == torch.float32 else c_double(v)


def call(name: str, *args) -> None:
    """One C entry with the argument list the header declares: Python ints / floats / bools by value (or ready-made ctypes values),
    ptr() / stream() / None in the pointer slots.  A list that does not fit raises before the C function is entered."""
    fn = getattr(lib(), name, None)
    argtypes = None if fn is None else fn.argtypes
    if argtypes is None or len(args) != len(argtypes):      # (ctypes itself lets a cdecl call pass surplus arguments)
        _reset()
        if name not in entries():
            raise DransacError(f"{name} is not an entry that {HEADER_PATH} declares")
        if argtypes is None:
            raise DransacError(f"{name} is declared in {HEADER_PATH}, but {LIB_PATH} does not export it")
        raise DransacError(f"{name} takes {len(argtypes)} arguments, {len(args)} given (the first one that does not fit is "
                           f"argument {min(len(args), len(argtypes)) + 1})")
    dev = _launch_device()
    _ctx.devs = set()
    try:
        if dev is not None and dev != torch.cuda.current_device():
            with torch.cuda.device(dev):       # tensors on another GPU than the current one: launch there
                status = fn(*args)
        else:
            status = fn(*args)
    except (TypeError, ctypes.ArgumentError) as e:      # "argument 3: TypeError: ..." (positions count from 1)
        raise DransacError(f"{name}: {e}") from None
    finally:
        _ctx.keep = []                         # the launch is enqueued on the tensors' stream: stream order protects them now
    check(status, name)


__all__ = ["lib", "check", "ptr", "aligned", "stream", "suffix", "scalar", "call", "entries", "parse_header", "c_pointer", "DransacError",
           "LIB_PATH", "HEADER_PATH", "c_int", "c_uint64", "c_float", "c_double", "c_void_p"]
