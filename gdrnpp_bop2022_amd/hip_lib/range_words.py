"""Range words and launch count of the three-product (fp16x2) kernels (include/gdrnpp_hip.h: GDRNPP_SPLIT2_NONFINITE |
GDRNPP_SPLIT2_SMALL_ROWS).  Every (device, stream) owns one i32[X3_SLOTS] device buffer; a launch ORs its word into the entry of
its LAYER (slot numbers are handed out by x3_policy.slot, slot 0 = launches that name no layer), so that the reader knows which
layer left the range."""
from __future__ import annotations

import torch

from .abi import DEFINES, current_stream

X3_SLOTS = 1024
X3_NONFINITE, X3_SMALL_ROWS = DEFINES["GDRNPP_SPLIT2_NONFINITE"], DEFINES["GDRNPP_SPLIT2_SMALL_ROWS"]
_X3_FLAGS = {}   # (device index, stream handle) -> i32[X3_SLOTS]
_X3_FLAG_OVERRIDE = None
_X3_LAUNCHES = 0   # launches of the three-product kernels by this process (engine.inference_step: is there a flag to check?)


def x3_flags():
    """The range words of the current device + stream (or of the enclosing x3_flag_scope)."""
    if _X3_FLAG_OVERRIDE is not None:
        return _X3_FLAG_OVERRIDE
    key = (torch.cuda.current_device(), current_stream())
    f = _X3_FLAGS.get(key)
    if f is None:
        f = _X3_FLAGS[key] = torch.zeros((X3_SLOTS,), dtype=torch.int32, device=f"cuda:{key[0]}")
    return f


def x3_flag_ptr(slot: int) -> int:
    f = x3_flags()
    return f.data_ptr() + 4 * (slot if 0 <= slot < f.numel() else 0)


class x3_flag_scope:
    """``with x3_flag_scope(words):`` — three-product launches inside record into ``words`` (i32[X3_SLOTS] device tensor) instead of
    the current stream's: a captured hipGraph must write to words its owner can read after every replay (engine.GraphedInference)."""

    def __init__(self, flag):
        if flag.dtype != torch.int32 or not flag.is_cuda or flag.numel() < 1:
            raise ValueError("x3_flag_scope needs an int32 device tensor")
        self.flag = flag

    def __enter__(self):
        global _X3_FLAG_OVERRIDE
        self.prev, _X3_FLAG_OVERRIDE = _X3_FLAG_OVERRIDE, self.flag
        return self.flag

    def __exit__(self, *exc):
        global _X3_FLAG_OVERRIDE
        _X3_FLAG_OVERRIDE = self.prev
        return False


def range_words_of(host_words) -> dict:
    """{slot: word} of the non-zero entries of a host copy of a range-word buffer."""
    nz = torch.nonzero(host_words).reshape(-1).tolist()
    return {int(i): int(host_words[i]) for i in nz}


def split2_range_words(reset: bool = True) -> dict:
    """{slot: word} of the layers whose three-product launches on the current stream left the fp16x2 range since the last reset
    (empty dict: all inside).  Synchronises the current stream (one X3_SLOTS * 4 byte read-back)."""
    f = x3_flags()
    words = range_words_of(f.cpu())
    if words and reset:
        f.zero_()
    return words


def split2_nonfinite(reset: bool = True) -> bool:
    """True when a three-product kernel launched on the current stream raised ANY bit of its range word since the last reset:
    a stored value / an A element was inf or NaN (activation beyond the fp16 range), or an A row sat below the range (rms < 2^-4).
    The caller repeats the work with the six-product kernels.  Synchronises the current stream."""
    return bool(split2_range_words(reset))


def x3_launch_count() -> int:
    return _X3_LAUNCHES


def count_x3():
    global _X3_LAUNCHES
    _X3_LAUNCHES += 1
