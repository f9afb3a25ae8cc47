"""The range-check policy of the three-product GEMM kernels.  This module OWNS the process-wide state of that policy — the
counters ``_X3_OVERFLOW_STEPS`` and ``_RANGE_RERUNS`` — and the two functions that change it (``_note_range_words``,
``_six_product_rerun``); its consumers are ``StepHandle.result`` here and ``GraphedInference._resolve`` (streams.py)."""
from __future__ import annotations

import torch

from .. import hip_lib
from . import x3_policy


_X3_OVERFLOW_STEPS = 0          # steps of this process whose three-product kernels overflowed the fp16 range
X3_OVERFLOW_STEPS_TO_GIVE_UP = 3
_RANGE_RERUNS = 0               # steps repeated with six products (either side of the range); bench.py reports it


def range_reruns() -> int:
    return _RANGE_RERUNS


def _note_range_words(words: dict) -> None:
    """What a step's non-zero range words ({slot: word}, hip_lib.split2_range_words) change for the steps to come:
      * every layer with rows below the range stays on the six-product kernels (x3_policy.demote);
      * of the layers reporting non-finite values the FIRST in launch order does (the others saw its inf / NaN pass through);
      * a model whose activations overflow step after step is not paid for twice for ever: after X3_OVERFLOW_STEPS_TO_GIVE_UP
        such steps the process stays on six products (with a warning)."""
    global _X3_OVERFLOW_STEPS
    x3_policy.demote({s_: w for s_, w in words.items() if w & hip_lib.X3_SMALL_ROWS})
    over = x3_policy.launch_order(s_ for s_, w in words.items() if w & hip_lib.X3_NONFINITE)   # slot order is not launch order
    if over:
        _X3_OVERFLOW_STEPS += 1
        first = [s_ for s_ in over if s_ > 0][:1]
        x3_policy.demote({s_: hip_lib.X3_NONFINITE for s_ in first})
        if _X3_OVERFLOW_STEPS >= X3_OVERFLOW_STEPS_TO_GIVE_UP and x3_policy.gemm_products() == 3:
            import warnings
            x3_policy.set_gemm_products(6)
            warnings.warn(f"{_X3_OVERFLOW_STEPS} steps overflowed the fp16 range of the three-product GEMM kernels: staying on the "
                          "six-product kernels (x3_policy.set_gemm_products(3) switches back)")


def _six_product_rerun(run, words: dict):
    """Repeat a step with the six-product kernels after its three-product launches reported ``words``; the calling host thread
    only (x3_policy.forced_gemm_products), other threads / streams keep their setting."""
    global _RANGE_RERUNS
    _RANGE_RERUNS += 1
    _note_range_words(words)
    with x3_policy.forced_gemm_products(6):
        return run()


class StepHandle:
    """A launched step whose range words have not been looked at yet.  ``result()`` waits for the step (one event), reads the
    words from pinned host memory and — if a three-product launch left the range — repeats the step with six products.  Between
    launch and ``result()`` the host is free: launch the next step first and the check costs no device idle time."""

    def __init__(self, run, out, host_words=None, event=None, stream=None, done=None):
        self._run, self._out, self._host, self._event = run, out, host_words, event
        self.stream = stream                    # the stream the step was launched on (a repeat goes to the same one)
        self._done = done                       # event behind the step on that stream, for a step WITHOUT range words (nothing to wait for on the host)
        self.reran = False                      # result() repeated the step with six products

    def result(self):
        """The step's output.  A handle belongs to the stream it was launched on (StepStreams deals consecutive steps to
        different ones): a repeat is issued there, and the output is marked as used by the CALLER's current stream, which may
        be another one (its memory is then not handed to a later step of the launch stream while the caller still reads it)."""
        if self._event is not None:
            self._event.synchronize()
            words = hip_lib.range_words_of(self._host)
            self._event = self._host = None
            if words:
                if self.stream is not None and self.stream != torch.cuda.current_stream():
                    with torch.cuda.stream(self.stream):
                        self._out = _six_product_rerun(self._run, words)
                        done = torch.cuda.Event()
                        done.record()
                    torch.cuda.current_stream().wait_event(done)
                else:
                    self._out = _six_product_rerun(self._run, words)
                self.reran = True
        self._run = None
        if self.stream is not None and self.stream != torch.cuda.current_stream():
            if self._done is not None:          # no host wait happened above: the caller's stream waits for the step on the device
                torch.cuda.current_stream().wait_event(self._done)
            if isinstance(self._out, torch.Tensor) and self._out.is_cuda:
                self._out.record_stream(torch.cuda.current_stream())
        self._done = None
        return self._out


def _on_device(out) -> bool:
    """Does ``out`` (a tensor, or a dict / sequence of them) live on a GPU?"""
    if isinstance(out, torch.Tensor):
        return out.is_cuda
    if isinstance(out, dict):
        return any(_on_device(v) for v in out.values())
    if isinstance(out, (list, tuple)):
        return any(_on_device(v) for v in out)
    return False


def launch_with_range_check(run) -> StepHandle:
    """``run()`` (a forward, or a whole step) under the contract of the three-product GEMM kernels, without waiting: if any of
    them was launched, the stream's range words are copied to pinned host memory behind the work (and cleared on the stream, so
    the next step starts from zero) and an event marks the copy; ``StepHandle.result()`` does the rest.  Under hipGraph capture
    the check is the graph owner's (GraphedInference.replay)."""
    n_x3 = hip_lib.x3_launch_count()
    out = run()
    if hip_lib.x3_launch_count() == n_x3 and not (torch.cuda.is_available() and _on_device(out)):
        return StepHandle(None, out)             # a CPU run (gdrn_inference_on_dataset supports one): no stream, no event, no range words
    if torch.cuda.is_current_stream_capturing():
        return StepHandle(None, out)
    st = torch.cuda.current_stream()
    if hip_lib.x3_launch_count() == n_x3:       # six-product kernels only (small batches, --gemm-products 6): no words, no host wait in result()
        done = torch.cuda.Event()
        done.record()
        return StepHandle(None, out, stream=st, done=done)
    words = hip_lib.x3_flags()              # this stream's words: steps in flight on other streams have their own
    host = torch.empty(words.shape, dtype=words.dtype, pin_memory=True)
    host.copy_(words, non_blocking=True)
    words.zero_()
    ev = torch.cuda.Event()
    ev.record()
    return StepHandle(run, out, host, ev, stream=st)


def run_with_range_check(run):
    """The synchronous form: ``run()``, then its range check (one stream sync when three-product kernels were launched)."""
    return launch_with_range_check(run).result()
