"""The C ABI of ``libgdrnpp_hip.so``: signature table, structs and constants read from ``include/gdrnpp_hip.h`` at import, loader,
pointer checks, and the one path every status-returning entry point is launched through (``launch``).  The only module that touches
ctypes function objects."""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_void_p

import torch

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # the library sits beside the package, where csrc/Makefile puts it
LIB_PATH = os.environ.get("GDRNPP_HIP_LIB", os.path.join(_PKG_DIR, "libgdrnpp_hip.so"))

_lib = None


# every scalar type include/gdrnpp_hip.h uses.  const char* is c_char_p; any other pointer is c_void_p, which takes what the callers
# pass: byref(struct), data_ptr() integers (of device tables too, where a typed POINTER could not be the rule) and None
C_TYPES = {"void": None, "int": c_int, "long": c_long, "long long": c_longlong, "float": c_float, "double": c_double, "size_t": c_size_t}


def _ctype(spelling: str, decl: str, strings: bool = True):
    """The ctypes type of one type as the header spells it (``strings``: const char* is a string, as in a prototype, or a plain
    pointer, as in a struct).  ``decl`` is quoted when the type is not one of ``C_TYPES``."""
    t = " ".join(spelling.replace("*", " * ").split())
    if strings and t == "const char *":
        return c_char_p
    if re.fullmatch(r"[\w ]+( \*)+", t):
        return c_void_p
    if t.removeprefix("const ") not in C_TYPES:
        raise ValueError(f"gdrnpp_hip.h: unknown type {t!r} in {' '.join(decl.split())!r}: abi.C_TYPES has no ctypes type for it")
    return C_TYPES[t.removeprefix("const ")]


def parse_header(src: str):
    """``include/gdrnpp_hip.h``, given as its path or its text -> (signatures ``name -> (restype, [argtypes])``, structs ``name ->
    ctypes.Structure`` with the header's members in the header's order, defines ``name -> int``).  Regular expressions over the text
    without its comments, and strict: a type outside ``C_TYPES``, a declaration that does not split into type, name and parameters, a
    struct member that cannot be placed (bit-field, nested struct) or a define that is no integer raises ValueError quoting it —
    skipping it, or guessing a pointer, would launch a kernel on a shifted argument list."""
    if "\n" not in src:
        if not os.path.exists(src):
            raise RuntimeError(f"gdrnpp_bop2022_amd: C header {src} is missing — the ctypes binding is derived from it "
                               f"(GDRNPP_HIP_HEADER names one kept elsewhere).  There is no second copy of the ABI.")
        with open(src) as f:
            src = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        if not re.fullmatch(r"-?\d+|\(-?\d+\)", value):
            raise ValueError(f"gdrnpp_hip.h: #define {name} {value}: not a decimal integer")
        defines[name] = int(value.strip("()"))
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M), flags=re.S)
    structs, typedef = {}, r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;"
    for name, body in re.findall(typedef, text):
        fields = []
        for member in filter(None, map(str.strip, body.split(";"))):
            m = re.fullmatch(r"(.+?[\s*])((?:\w+(?:\[\d+\])?\s*,\s*)*\w+(?:\[\d+\])?)", member, re.S)
            ctype = _ctype(m.group(1), member, strings=False) if m else None
            if ctype is None:
                raise ValueError(f"gdrnpp_hip.h: struct {name}: cannot place member {' '.join(member.split())!r}")
            for field in m.group(2).split(","):
                field, _, n = field.strip().rstrip("]").partition("[")
                fields.append((field, ctype * int(n) if n else ctype))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    signatures = {}
    for decl in filter(None, map(str.strip, re.sub(typedef, "", text).split(";"))):
        m = re.fullmatch(r"(.+?[\s*])(\w+)\s*\((.*)\)", decl, re.S)
        params = m.group(3).split(",") if m and m.group(3).strip() not in ("", "void") else []
        types = [re.fullmatch(r"\s*(.+?[\s*])\w+\s*", p, re.S) for p in params]
        if not m or not all(types):
            raise ValueError(f"gdrnpp_hip.h: cannot split {' '.join(decl.split())!r} into return type, name and named parameters")
        args = [_ctype(t.group(1), decl) for t in types]
        if None in args:
            raise ValueError(f"gdrnpp_hip.h: void parameter in {' '.join(decl.split())!r}")
        signatures[m.group(2)] = (_ctype(m.group(1), decl), args)
    return signatures, structs, defines


HEADER_PATH = os.environ.get("GDRNPP_HIP_HEADER", os.path.join(os.path.dirname(_PKG_DIR), "include", "gdrnpp_hip.h"))
SIGNATURES, STRUCTS, DEFINES = parse_header(HEADER_PATH)        # once, at import
gdrnpp_meshes, gdrnpp_roi_table = STRUCTS["gdrnpp_meshes"], STRUCTS["gdrnpp_roi_table"]


def load(path: str | None = None) -> ctypes.CDLL:
    """Load the shared library and bind every declared symbol (no compute, no GPU needed)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"gdrnpp_bop2022_amd: HIP extension {p} is missing — run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C gdrnpp_bop2022_amd/csrc`).  There is no CPU fallback."
        )
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gdrnpp_last_error()
        raise RuntimeError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the handle without building a torch.cuda.Stream object


def current_stream() -> int:
    """hipStream_t of the current device's current stream.  Called once per launch (~150 per step): the raw accessor takes
    ~0.3 us against ~8 us for torch.cuda.current_stream().cuda_stream — 1-2 ms per step of host time, which is what bounds the
    small batches once two steps are in flight."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class LaunchTimer:
    """Optional per-launch timing of the split-GEMM entry points (kinds "linear", "conv3x3", ...) and of the memory-bound
    network kernels (kinds "hbm:<kernel>", flops 0) with HIP events recorded on the stream the kernel is launched on
    (bench.py's roofline leg).  records: (kind, fp32-equivalent flops, start event, end event, algorithmic bytes =
    operands read once + result written once)."""

    def __init__(self):
        self.records = []

    def launch(self, kind, flops, fn, nbytes=0.0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        self.records.append((kind, flops, e0, e1, nbytes))
        return rc


_LAUNCH_TIMER = None


def set_launch_timer(timer):
    global _LAUNCH_TIMER
    _LAUNCH_TIMER = timer


def launch(name: str, *args, timed=None) -> None:
    """Call the status-returning entry point ``name`` with ``args`` + the current stream; a non-zero status raises RuntimeError
    with the library's last error, named after ``name``.  ``timed`` = (kind, flops, nbytes): what an installed LaunchTimer records
    for this launch (without a timer the call is direct, no closure is built)."""
    fn = getattr(_lib if _lib is not None else load(), name)
    stream = current_stream()
    if timed is None or _LAUNCH_TIMER is None:
        rc = fn(*args, stream)
    else:
        rc = _LAUNCH_TIMER.launch(timed[0], timed[1], lambda: fn(*args, stream), timed[2])
    if rc != 0:
        check(rc, name)


def copy_d2d(dst_ptr: int, src: torch.Tensor) -> None:
    """Copy a contiguous device tensor into a raw device pointer on the current stream (``gdrnpp_copy_d2d``)."""
    if not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("copy_d2d: src must be a contiguous CUDA(HIP) tensor")
    launch("gdrnpp_copy_d2d", c_void_p(int(dst_ptr)), src.data_ptr(), src.numel() * src.element_size())


def spin(micros: int) -> None:
    """One wave busy-waiting ``micros`` microseconds of the device's wall clock on the current stream (``gdrnpp_debug_spin``): the
    probe kernel of engine.streams_overlap_ratio — occupies a hardware queue, computes nothing."""
    launch("gdrnpp_debug_spin", int(micros))


def set_option(name: str, value: int) -> None:
    """Process-wide tuning switch of the library (``gdrnpp_set_option``; the one entry point without a stream)."""
    check(load().gdrnpp_set_option(name.encode(), int(value)), "gdrnpp_set_option")


def get_option(name: str) -> int:
    """Current value of a process-wide tuning switch (``gdrnpp_get_option``)."""
    value = c_int(0)
    check(load().gdrnpp_get_option(name.encode(), ctypes.byref(value)), "gdrnpp_get_option")
    return value.value


def dev_ptr(t: torch.Tensor, dtype: torch.dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t.data_ptr()


def f32_ptr(t: torch.Tensor, name: str) -> int:
    """``dev_ptr(t, torch.float32, name)`` with the checks in one test: one Python call per argument, as ``dev_ptr`` itself."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        dev_ptr(t, torch.float32, name)    # raises, saying which
    return t.data_ptr()


def opt_f32_ptr(t: torch.Tensor | None, name: str):
    """``f32_ptr`` of an optional argument: None = NULL."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        dev_ptr(t, torch.float32, name)
    return t.data_ptr()


def nhwc_ptr(t: torch.Tensor, name: str) -> int:
    """A network-side NHWC layer's tensor: logically NCHW with channels_last strides."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{name} must be a 4-D float32 CUDA(HIP) tensor")
    if not t.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError(f"{name} must be channels_last contiguous")
    return t.data_ptr()


def channels_last_f32(x_cl, what: str):
    if not x_cl.is_contiguous(memory_format=torch.channels_last) or x_cl.dtype != torch.float32 or not x_cl.is_cuda:
        raise ValueError("%s expects a float32 channels_last device tensor" % what)
    return x_cl.shape
