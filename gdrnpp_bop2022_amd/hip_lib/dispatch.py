"""Kernel-choice state: the thresholds between the six- and three-product GEMM kernels, the per-thread "shared chip" rule and the
split-K switch of the convolutions.  Whoever changes a threshold assigns it HERE (``dispatch.SPLIT2_MIN_TILES = 1``): the
``hip_lib`` namespace forwards reads and holds no copy."""
from __future__ import annotations

import os
import threading

SPLIT2_MIN_TILES = int(os.environ.get("GDRNPP_SPLIT2_MIN_TILES", "256"))   # tests lower it to run the three-product kernels on the 4-ROI reference fixtures; the env var is for A/B runs


# With a second step in flight on another stream (engine.StepStreams) a launch need not fill the chip by itself: from
# SPLIT2_SHARED_MIN_TILES tiles on, if it has at least SPLIT2_SHARED_MIN_ROWS rows (fewer: the 128 x 128-tile six-product kernels stay ahead).
SPLIT2_SHARED_MIN_TILES = int(os.environ.get("GDRNPP_SPLIT2_SHARED_MIN_TILES", "0"))      # 0 = off
SPLIT2_SHARED_MIN_ROWS = int(os.environ.get("GDRNPP_SPLIT2_SHARED_MIN_ROWS", "4096"))


_SHARED_TLS = threading.local()     # .min_tiles: the shared-chip rule of the calling HOST THREAD (engine.StepStreams.next sets it for
                                    # the launches of one step); unset = the process default above.  Two host threads driving
                                    # their own dealers never see each other's setting.


def shared_min_tiles() -> int:
    """The shared-chip tile rule in force for the calling host thread (0 = off)."""
    v = getattr(_SHARED_TLS, "min_tiles", None)
    return SPLIT2_SHARED_MIN_TILES if v is None else v


def shared_min_rows() -> int:
    """Fewest rows of a launch that takes the three-product form under the shared-chip rule, for the calling host thread."""
    v = getattr(_SHARED_TLS, "min_rows", None)
    return SPLIT2_SHARED_MIN_ROWS if v is None else v


class shared_min_tiles_scope:
    """``with shared_min_tiles_scope(n, rows):`` — launches of the calling host thread inside choose their GEMM kernels for a chip
    shared with other steps (three-product 256-row form from ``n`` tiles on, for launches of at least ``rows`` rows); ``None`` =
    leave whatever is in force."""

    def __init__(self, n, rows=None):
        self.n = None if n is None else int(n)
        self.rows = None if rows is None else int(rows)

    def __enter__(self):
        self.prev = getattr(_SHARED_TLS, "min_tiles", None), getattr(_SHARED_TLS, "min_rows", None)
        if self.n is not None:
            _SHARED_TLS.min_tiles = self.n
        if self.rows is not None:
            _SHARED_TLS.min_rows = self.rows
        return self

    def __exit__(self, *exc):
        _SHARED_TLS.min_tiles, _SHARED_TLS.min_rows = self.prev
        return False


def split2_tiles_ok(m: int, n: int) -> bool:
    """The three-product kernels exist as 256-row tiles only: used from 256 tiles of 256 x 128 on (every CU gets a workgroup)."""
    if n % 128:
        return False
    tiles = ((m + 255) // 256) * (n // 128)
    return tiles >= SPLIT2_MIN_TILES or (0 < shared_min_tiles() <= tiles and m >= shared_min_rows())


def split_gemm_tiles(m: int, n: int) -> int:
    """Output tiles (128x128) of an [m, n] result — the dispatch quantity between the plain and the split-K launch."""
    return ((m + 127) // 128) * (n // 128)


_CONV_SPLITK = True


def set_conv_splitk(flag: bool) -> None:
    """A/B switch: convolutions with too few output tiles for the chip run split-K (default) or as one launch."""
    global _CONV_SPLITK
    _CONV_SPLITK = bool(flag)
