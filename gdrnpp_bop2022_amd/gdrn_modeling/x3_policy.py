"""Host-side policy of the split GEMMs: does a launch run the three-product fp16x2 kernels or the six-product bf16x3 ones?
The process setting and the per-thread override, the range-word slot of every layer, the demotions, the launch order and the
weight pick.  This module is the only one that assigns that state; the tile rule and the range-word buffers are hip_lib's."""
from __future__ import annotations

import threading

import torch

from .. import hip_lib
from .weight_cache import cached, weight_tag

# Partial products per fp32 product in the split GEMMs.
#   3 (default): fp16x2 operand split, 22 significant operand bits, csrc/gemm_split2_pipe.hip — where the three-product kernels
#      exist and pay: ConvNeXt MLPs, 3x3/1/1 convolutions and the transposed-convolution GEMM from 256 tiles of 256 x 128 on
#      (batches of ~64 ROIs and more); every other layer and every smaller launch runs the six-product kernels.  Against fp64 the
#      result is as close as the six-product form and closer than hipBLASLt's fp32 GEMM on the same operands (the fp32
#      accumulation chain dominates all three; tools/split2_error_probe.py, profiles/r03y_split2_accuracy.txt), and the
#      network outputs sit at the same 6e-6 from the reference's recorded forward as with six products or the vendor fp32
#      kernels — for half the matrix-pipe work.  The form has a RANGE: every launch checks both sides of it on the device and
#      reports in the range word of its layer (hip_lib.split2_range_words) — an activation beyond 65504, or an A row whose rms is
#      below 2^-4 (low halves in the fp16 subnormals).  engine.run_with_range_check then repeats the step with 6 and keeps the
#      flagged layers on 6 (demote), so the outputs are fp32-level on EVERY batch, not on the ones somebody looked at.
#   6: bf16x3 operand split, exact to 2^-26, everywhere.
_GEMM_PRODUCTS = 3
_TLS = threading.local()     # .forced: products forced for the calling host thread (the six-product repeat of a flagged step)


def set_gemm_products(n: int) -> None:
    global _GEMM_PRODUCTS
    if n not in (3, 6):
        raise ValueError(f"gemm products must be 6 (bf16x3) or 3 (fp16x2), got {n!r}")
    _GEMM_PRODUCTS = int(n)


def gemm_products() -> int:
    forced = getattr(_TLS, "forced", None)
    return _GEMM_PRODUCTS if forced is None else forced


class forced_gemm_products:
    """``with forced_gemm_products(6):`` — the calling host thread runs every split GEMM with that many products, other threads
    (streams) keep the process setting."""

    def __init__(self, n: int):
        if n not in (3, 6):
            raise ValueError(f"gemm products must be 6 or 3, got {n!r}")
        self.n = n

    def __enter__(self):
        self.prev = getattr(_TLS, "forced", None)
        _TLS.forced = self.n
        return self

    def __exit__(self, *exc):
        _TLS.forced = self.prev
        return False


# ---- which layers run the three-product kernels ----------------------------------------------------------------------------
# A layer = (the module's cache dict, a key).  It gets a range-word slot at its first three-product launch (slots follow launch
# order within a model) and loses the three-product form for good — until the weights change — when a launch of it reported
# rows below the range, or when it was the first layer of a step to overflow.
_X3_NEXT_SLOT = 1            # slot 0: launches that name no layer
_X3_DEMOTED = {}             # slot -> range word that demoted it
_X3_EPOCH = 0                # bumped by reset: slots handed out before it are forgotten
_X3_LAUNCH_SEQ = {}          # slot -> sequence number of its latest three-product launch (process-wide monotonic counter)
_X3_LAUNCH_COUNTER = 0


def note_launch(*slots: int) -> None:
    """Slots are handed out lazily (first eligible launch, any model, any batch size), so slot order is NOT launch order in
    general; the order a step launched its layers in is what decides which of several overflowing layers was the first."""
    global _X3_LAUNCH_COUNTER
    for s_ in slots:
        _X3_LAUNCH_COUNTER += 1
        _X3_LAUNCH_SEQ[s_] = _X3_LAUNCH_COUNTER


def launch_order(slots) -> list:
    """``slots`` sorted by the position of their latest three-product launch (slots never launched sort last, by number)."""
    big = _X3_LAUNCH_COUNTER + 1
    return sorted(slots, key=lambda s_: (_X3_LAUNCH_SEQ.get(s_, big), s_))


def slot(cache: dict, key: str) -> int:
    global _X3_NEXT_SLOT
    st = cache.get("x3_slot_" + key)
    if st is None or st[0] != _X3_EPOCH:
        st = cache["x3_slot_" + key] = (_X3_EPOCH, min(_X3_NEXT_SLOT, hip_lib.X3_SLOTS - 1))   # beyond the buffer: layers share the last slot
        _X3_NEXT_SLOT += 1
    return st[1]


def demote(words: dict) -> None:
    """Keep the layers of ``words`` ({slot: range word}) on the six-product kernels from now on."""
    for slot, word in words.items():
        if slot > 0:
            _X3_DEMOTED[int(slot)] = _X3_DEMOTED.get(int(slot), 0) | int(word)


def demoted() -> dict:
    return dict(_X3_DEMOTED)


def is_demoted(slot: int) -> bool:
    return slot in _X3_DEMOTED


def reset() -> None:
    """Forget the demotions and the slot numbering (new weights: new activation scales)."""
    global _X3_EPOCH, _X3_NEXT_SLOT
    _X3_EPOCH += 1
    _X3_NEXT_SLOT = 1
    _X3_DEMOTED.clear()
    _X3_LAUNCH_SEQ.clear()


def eligible(m: int, n: int, k_linear: int = 0) -> bool:
    """Three-product kernel for an [m, n] result?  ``k_linear`` = K of a linear-form launch: its A operand is addressed with
    32-bit lane offsets (m * K * 4 bytes < 4 GiB, ~480 ROIs at stage 0); beyond that the six-product kernels take over."""
    return gemm_products() == 3 and hip_lib.split2_tiles_ok(m, n) and m * k_linear * 4 < (1 << 32)


def weight_for(cache: dict, key: str, weight: torch.Tensor, pack3, m: int, n: int, k_linear: int = 0, slot_key: str | None = None):
    """-> (packed three-product weight or None, range-word slot).  None = this launch runs the six-product kernel: the shape is
    outside the three-product kernels, the layer was demoted, or its weight has rows below the range (checked once per weight
    by the pack kernel).  ``slot_key``: the layer whose slot (and demotion) this launch shares when ``key`` names a second packed
    form of the same layer's weight."""
    if not eligible(m, n, k_linear):
        return None, 0
    s_ = slot(cache, slot_key or key)
    if s_ in _X3_DEMOTED:
        return None, s_
    def build():
        packed = pack3(weight.detach())
        return packed, hip_lib.packed_rows_in_range(packed)

    hit = cached(cache, key + "_pk_x3", weight_tag(weight), build, weight)
    if hit[2]:
        note_launch(s_)
    return (hit[1] if hit[2] else None), s_


def six_product_weight(cache: dict, key: str, weight: torch.Tensor, pack6) -> torch.Tensor:
    """Packed six-product split image of ``weight``, rebuilt when the weight changes."""
    return cached(cache, key, weight_tag(weight), lambda: (pack6(weight.detach()),), weight)[1]


def split_weight(cache: dict, key3: str, key6: str, weight: torch.Tensor, pack3, pack6, m: int, n: int, k_linear: int = 0,
                 allow3: bool = True, slot_key: str | None = None):
    """-> (packed weight, range-word slot): the three-product image ``weight_for`` grants (``allow3`` False: none asked for),
    else the six-product one."""
    w_pk, s_ = weight_for(cache, key3, weight, pack3, m, n, k_linear, slot_key) if allow3 else (None, 0)
    if w_pk is None:
        w_pk = six_product_weight(cache, key6, weight, pack6)
    return w_pk, s_
