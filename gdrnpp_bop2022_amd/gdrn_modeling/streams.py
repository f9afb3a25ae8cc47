"""The step entry points, the stream dealer (``StepStreams`` and the host-thread state ``_DEALER_TLS`` it writes and
``inference_step_async`` reads) and the hipGraph forms of the step."""
from __future__ import annotations

import threading
from typing import TYPE_CHECKING

import torch

from .. import hip_lib
from . import hip_layers, x3_policy
from .range_check import StepHandle, _six_product_rerun, launch_with_range_check, run_with_range_check

if TYPE_CHECKING:      # annotations only (they are never evaluated): no import at run time
    from .post import GdrnHipPost


def _step_closure(model, post: "GdrnHipPost", batch: dict, roi_ids):
    def run():
        out_dict = model(
            batch["roi_img"], roi_classes=batch["roi_cls"], roi_cams=batch["roi_cam"], roi_whs=batch["roi_wh"],
            roi_centers=batch["roi_center"], resize_ratios=batch["resize_ratio"],
            roi_coord_2d=batch.get("roi_coord_2d"), roi_coord_2d_rel=batch.get("roi_coord_2d_rel"),
            roi_extents=batch.get("roi_extent"))
        return post.process(batch, out_dict, roi_ids)
    return run


@torch.no_grad()
def inference_step_async(model, post: GdrnHipPost, batch: dict, roi_ids: torch.Tensor | None = None) -> StepHandle:
    """Launch one pass of the hot path over one batch of ROIs and return without waiting for the device: ``.result()`` gives
    the f32[b,16] records (after the range check of the three-product kernels).  ``batch`` must stay untouched until then."""
    if roi_ids is None:
        roi_ids = batch.get("roi_id")
    if batch["roi_img"].shape[0] == 0:            # empty shard (shard_range may give trailing ranks nothing): the caller
        return StepHandle(None, torch.zeros((0, 16), dtype=torch.float32, device=batch["roi_img"].device))   # still reaches gather_records
    run = torch.no_grad()(_step_closure(model, post, batch, roi_ids))
    dealer = getattr(_DEALER_TLS, "dealer", None)         # set by StepStreams.next() around the launches of one step
    if dealer is None or not dealer.sharing():
        return launch_with_range_check(run)
    n_foreign = getattr(_DEALER_TLS, "foreign_at_entry", hip_layers.fallback_launches())   # counted from the dealer context's entry: the
    handle = launch_with_range_check(run)                                                   # ROI preparation in front of the step is part of it
    if hip_layers.fallback_launches() != n_foreign:
        # the step launched kernels that are not this library's (a layer fell back to a PyTorch operator on its shape) while another
        # step may be running MFMAs on the other stream: foreign packed-fp32 code is exactly what MI355X gets wrong there
        # (profiles/r05p_two_stream_hazard.md).  The dealer stops sharing the chip — loudly — and this step is repeated alone.
        dealer.stop_sharing(f"{hip_layers.fallback_launches() - n_foreign} launch(es) outside this library, last: {hip_layers.last_fallback()}")
        torch.cuda.synchronize(dealer.device)
        handle = launch_with_range_check(run)
    return handle


def inference_step(model, post: GdrnHipPost, batch: dict, roi_ids: torch.Tensor | None = None) -> torch.Tensor:
    """One pass of the hot path over one batch of ROIs (the unit ``bench.py`` times).  ``roi_ids`` (or ``batch["roi_id"]``,
    set by ``batch_data_test_gpu(sort_by_class=True)``) = the global index each record carries."""
    return inference_step_async(model, post, batch, roi_ids).result()


def default_compute_streams(model, cfg=None) -> int:
    """How many compute streams consecutive steps of ``model`` may safely share the chip on: 2 when every arithmetic kernel of a
    step is this library's — code that is built and link-checked to hold no packed-fp32 instruction of the form MI355X gets wrong
    beside another stream's MFMAs (csrc/Makefile) — else 1.  Decided in two layers:
      * statically, here: ConvNeXt backbone, HIP network layers on, split GEMMs, and (``cfg`` = the model's own by default) a
        post-processing branch that is one launch of this library — plain network pose or depth refine; the ``TEST.USE_PNP``
        branches (torch elementwise ops around the PnP kernels, GdrnHipPost.process_*) and ``COORD_2D_TYPE="rel"`` (torch
        arithmetic in batch_data_test_gpu) run PyTorch operators and get 1, like the ResNet backbone (MIOpen convolutions);
      * dynamically, in ``inference_step_async``: every layer that falls back to a PyTorch operator ON ITS SHAPE (another input
        size, another norm) is counted (hip_layers.fallback_launches); a step that moved the counter inside a sharing dealer
        makes the dealer stop sharing and is repeated alone."""
    from .backbones import ConvNeXtFeatures

    cfg = getattr(model, "cfg", None) if cfg is None else cfg
    ours = (hip_layers.is_enabled() and hip_layers.mlp_gemm() == "split" and isinstance(getattr(model, "backbone", None), ConvNeXtFeatures)
            and not torch.is_autocast_enabled())
    if ours and cfg is not None:
        ours = not bool(cfg.TEST.USE_PNP) and cfg.MODEL.POSE_NET.PNP_NET.COORD_2D_TYPE != "rel"
    return 2 if ours else 1


def default_graph_streams(model, cfg=None) -> int:
    """Compute streams for the hipGraph form of the step (``GraphedStepStreams``): 4 where steps may share the chip at all
    (``default_compute_streams`` == 2) — a graph replay costs the host ~0.1 ms instead of ~3 ms of launches, so the host can keep
    FOUR steps in flight, which is what HIP offers hardware queues for (a fifth stream shares a queue with one of the four:
    profiles/r06_graph_streams.md; eager launches cannot feed more than two, profiles/r05r_compute_streams.txt) — else 1."""
    return 4 if default_compute_streams(model, cfg) > 1 else 1


_DEALER_TLS = threading.local()      # .dealer: the StepStreams whose next() context the calling host thread is inside


def streams_overlap_ratio(s0, s1, micros: int = 200) -> float:
    """(time of a spin kernel on s0 and then one on s1, each alone) / (time of both launched together): ~2 when the two streams
    execute concurrently, ~1 when they share a hardware queue and run back to back.  ~1 ms of device time.  The spin kernel is
    this library's (gdrnpp_debug_spin: one wave waiting on the wall clock)."""
    dev = s0.device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s0):
        hip_lib.spin(micros)               # warm both paths (first launch on a fresh stream creates its queue)
    with torch.cuda.stream(s1):
        hip_lib.spin(micros)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s0):                  # alone
        ev[0].record()
        hip_lib.spin(micros)
        ev[1].record()
    torch.cuda.synchronize(dev)
    alone = ev[0].elapsed_time(ev[1])
    with torch.cuda.stream(s0):                  # together: s1's kernel is launched while s0's spins
        ev[2].record()
        hip_lib.spin(micros)
    with torch.cuda.stream(s1):
        hip_lib.spin(micros)
        ev[3].record()
    torch.cuda.synchronize(dev)
    together = ev[2].elapsed_time(ev[3])
    return 2.0 * alone / max(together, 1e-6)


class StepStreams:
    """Consecutive steps are independent (each batch its own ROIs, its own records), so they need not queue behind each other
    on ONE stream: dealt round-robin to ``n`` compute streams, the second step's GEMMs fill the chip while the first one is in
    its narrow tail (8x8 stage, Patch-PnP, pose heads, depth refine: launches of a few workgroups each) — two steps in flight
    instead of one.  Measured at the headline batch: 25.0 -> 23.3 ms per 128-ROI step, records bit-equal to the single-stream
    schedule (profiles/r05q_two_streams.txt).

        streams = StepStreams(2)
        with streams.next():
            handle = inference_step_async(model, post, batch)     # launched on the dealt stream; handle.result() from anywhere

    Everything a step allocates comes from its stream's pool and its range words are that stream's (hip_lib.x3_flags), so two
    steps share nothing but the read-only weights.  What must NOT share the chip with the split GEMMs is packed fp32 code with
    op_sel swizzles (a hardware hazard, csrc/Makefile): the library is built without it and checked at link time."""

    def __init__(self, n: int = 2, device=None, priorities=None, allow_foreign: bool = False):
        if n < 1:
            raise ValueError("StepStreams needs at least one stream")
        self.allow_foreign = bool(allow_foreign)   # A/B only: keep sharing the chip although a step launched kernels this library cannot check
        self.stopped_sharing = None                # reason, once a step with foreign launches made this dealer fall back to ONE stream
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        pr = list(priorities) if priorities is not None else [0] * n     # (A/B only: equal priorities are what was measured best)
        self.streams = [None]
        self.overlap_probe = None               # [(candidates tried, overlap ratio)] per stream after the first: what the choice was based on
        if n > 1:
            # HIP multiplexes its streams over a few hardware queues; two streams that land on the SAME queue run one after the
            # other, and "two steps in flight" silently becomes the one-stream schedule (measured: a pair drawn later in a
            # process gave 24.97 instead of 23.49 ms per step, profiles/r05last_two_stream_soak.txt).  So every further stream is
            # drawn from torch's pool until a pair of spin kernels really overlaps with the first one.
            self.streams = [torch.cuda.Stream(self.device, priority=int(pr[0]))]
            self.overlap_probe = []
            for i in range(1, n):
                best = None
                for attempt in range(8):
                    cand = torch.cuda.Stream(self.device, priority=int(pr[i % len(pr)]))
                    ratio = min(streams_overlap_ratio(s_, cand) for s_ in self.streams)
                    if best is None or ratio > best[1]:
                        best = (cand, ratio)
                    if ratio > 1.6:
                        break
                self.streams.append(best[0])
                self.overlap_probe.append((attempt + 1, round(best[1], 2)))
        self._i = 0
        self.sync_with_current()

    def sync_with_current(self) -> None:
        """Work queued on the caller's stream so far (weights, resident batches) is visible to every compute stream."""
        cur = torch.cuda.current_stream(self.device)
        for s_ in self.streams:
            if s_ is not None:
                s_.wait_stream(cur)

    def sharing(self) -> bool:
        """Are consecutive steps of this dealer really dealt to different streams (and must therefore launch nothing foreign)?"""
        return len(self.streams) > 1 and self.stopped_sharing is None and not self.allow_foreign

    def stop_sharing(self, reason: str) -> None:
        """From now on every step goes to the FIRST stream (one step at a time on the device): a step launched kernels that are
        not this library's.  Loud: a RuntimeWarning naming the launch."""
        import warnings

        if self.stopped_sharing is None:
            self.stopped_sharing = reason
            warnings.warn("StepStreams: two steps in flight switched OFF for this dealer — " + reason + ".  Foreign arithmetic kernels "
                          "must not run beside another stream's MFMAs on MI355X (packed-fp32 hazard); steps now queue on one stream.",
                          RuntimeWarning, stacklevel=3)

    def shared_min_tiles(self) -> int:
        """Tile count from which a launch takes the three-product 256-row form while this dealer's streams share the chip: a
        launch need not give every CU a workgroup when a second step runs beside it (hip_lib.split2_tiles_ok; 0 = rule off).
        Unchanged by ``stop_sharing``: the kernel choice (and with it every bit of the records) stays what it was."""
        n = len(self.streams)
        return hip_lib.SPLIT2_MIN_TILES // n if n > 1 else 0

    def shared_min_rows(self):
        """Fewest rows of a launch under that rule: the process default (4 096) for two streams — the eager schedule of rounds 5 / 6,
        whose records this keeps — and 2 048 from three streams on (four hipGraphs in flight: 8 / 16 / 32 ROIs 3 305 -> 3 592,
        4 533 -> 4 561, 5 107 -> 5 172 ROIs/s with 64 tiles, profiles/r06_graph_streams.md)."""
        return 2048 if len(self.streams) > 2 else None

    def next(self):
        """Context manager: the body's launches go to the next compute stream (with n = 1: the caller's current stream) and, with
        n > 1, choose their GEMM kernels for a shared chip (``shared_min_tiles``: 4 248 -> 4 525 ROIs/s at 32 ROIs, neutral at 8 and
        128, profiles/r05y_shared_chip_tile_rule.txt)."""
        idx = self._i % len(self.streams)
        self._i += 1
        return self.on(idx)

    def on(self, index: int):
        """Context manager like ``next()`` for a GIVEN stream of the dealer, without advancing the round-robin (a hipGraph slot is
        bound to the stream it was captured on)."""
        import contextlib

        s_ = self.streams[0 if self.stopped_sharing is not None else index % len(self.streams)]

        @contextlib.contextmanager
        def ctx():
            # the rule belongs to the calling HOST THREAD for the duration of this step's launches (hip_lib.shared_min_tiles_scope):
            # two threads with their own dealers do not see each other's; an explicit setting (tests, A/B runs, env var) wins
            explicit = hip_lib.shared_min_tiles() != 0
            rule, rows = (None, None) if explicit else (self.shared_min_tiles(), self.shared_min_rows())
            prev = getattr(_DEALER_TLS, "dealer", None), getattr(_DEALER_TLS, "foreign_at_entry", None)
            _DEALER_TLS.dealer, _DEALER_TLS.foreign_at_entry = self, hip_layers.fallback_launches()
            try:
                with hip_lib.shared_min_tiles_scope(rule, rows), torch.cuda.stream(s_):    # torch.cuda.stream(None) is a no-op context
                    yield s_
            finally:
                _DEALER_TLS.dealer, _DEALER_TLS.foreign_at_entry = prev
        return ctx()


class GraphHandle:
    """A replayed hipGraph whose range words have not been looked at yet (``GraphedInference.replay_async``).  ``result()``
    waits for the replay (one event), and — when a three-product kernel of the graph left its range — repeats the step eagerly
    with six products and has the graph captured again.  Must be resolved before the same graph is replayed again (the graph's
    static buffers are reused; ``replay_async`` resolves a forgotten handle itself)."""

    def __init__(self, owner, event, rec):
        self._owner, self._event, self._rec = owner, event, rec
        self.stream = owner.stream              # the stream the graph was replayed on (None: the caller's current one)
        self.reran = False                      # result() repeated the step eagerly with six products

    def result(self) -> torch.Tensor:
        if self._owner is not None:
            owner, self._owner = self._owner, None
            n0 = owner.reruns
            self._rec = owner._resolve(self._event, self._rec)
            self.reran = owner.reruns != n0
            self._event = None
        return self._rec


class GraphedInference:
    """The whole hot path (forward + HIP post-processing + record packing) captured once into a hipGraph and
    replayed per batch.  At the reference's own batch sizes (one image = a few to ~30 ROIs, gdrn_evaluator.py:702)
    the ~150 launches of a step are launch-bound (3.2 ms of host time per 8-ROI step through ctypes); a graph replay removes the
    per-launch host cost.  Shapes are fixed at capture time: batches are copied into static device buffers (pad the ROI
    dimension to the captured size; padded rows are ordinary ROIs whose records the caller ignores).

    ``stream``: the HIP stream the graph is captured and replayed on (default: the caller's current stream).  Two graphs on the
    two streams of a ``StepStreams`` dealer are TWO STEPS IN FLIGHT without any per-launch host work (``GraphedStepStreams``).
    ``shared_min_tiles``: the kernel rule of a shared chip (StepStreams.shared_min_tiles) the graph's launches are chosen by —
    captured with the rule of the eager two-stream schedule a graph replays the same kernels and gives the same bits.
    ``sharing``: the graph is going to run beside another stream's step: a captured step that launched anything outside this
    library raises (hip_layers.fallback_launches; the packed-fp32 hazard of MI355X, profiles/r05p_two_stream_hazard.md).

    Three-product kernels inside the graph write their range words to a buffer the graph owns; every replay copies it to pinned
    host memory behind the graph (asynchronously — ``replay_async`` returns at once, ``GraphHandle.result()`` looks).  When a
    layer left the range the step is repeated eagerly with six products, its records are copied into the static output, the
    layer is demoted and the graph is captured again with it on the six-product kernels — so a flagged layer is paid for once,
    not on every replay."""

    def __init__(self, model, post: GdrnHipPost, example_batch: dict, roi_ids: torch.Tensor | None = None,
                 warmup: int = 3, stream=None, shared_min_tiles=None, sharing: bool = False, shared_min_rows=None, body=None):
        self.model, self.post = model, post
        self.body = body                                      # callable(static) -> records: a step that is more than forward + post
        self.reruns = 0                                       # (RoiStreamScheduler(graph_steps=True): crop + forward + post)
        self.stream = stream                                  # None = whatever stream is current when replay is called
        self.shared_min_tiles, self.shared_min_rows, self.sharing = shared_min_tiles, shared_min_rows, bool(sharing)
        self.static = ({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in example_batch.items()} if body is None
                       else example_batch)                    # with a body the caller owns the static inputs and fills them itself
        self.roi_ids = roi_ids.clone() if roi_ids is not None else None
        self.captures = 0
        self._pending = None                                  # the unresolved GraphHandle of the latest replay
        dev = next(v.device for v in self.static.values() if isinstance(v, torch.Tensor))
        for _ in range(max(warmup, 1)):                       # MIOpen find, hipFuncSetAttribute, allocator warm-up, weight packing and the
            self._eager_pass()                                # first range verdicts (demotions) happen outside capture
        self.x3_flag = torch.zeros((hip_lib.X3_SLOTS,), dtype=torch.int32, device=dev)   # the graph's own range words
        self._host_words = torch.zeros((hip_lib.X3_SLOTS,), dtype=torch.int32, pin_memory=True)
        self._capture()

    def _on_stream(self):
        """Context: the graph's stream is current (no-op when the graph follows the caller's stream)."""
        return torch.cuda.stream(self.stream)

    @torch.no_grad()
    def _eager_pass(self):
        """One eager step on a side stream with the CURRENT demotions / products, range check included (it may demote further
        layers): everything a capture must not do — packing a weight for the first time (a block that left the fused MLP kernel
        has never packed its two unfused images), ``packed_rows_in_range``'s host read, hipFuncSetAttribute — happens here."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        if self.stream is not None:
            side.wait_stream(self.stream)
        with torch.cuda.stream(side), hip_lib.shared_min_tiles_scope(self.shared_min_tiles, self.shared_min_rows):
            run_with_range_check(torch.no_grad()(self._step))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _step(self):
        """The work of one replay, as a callable of no arguments (eager passes, capture, the six-product repeat)."""
        if self.body is not None:
            return self.body(self.static)
        return _step_closure(self.model, self.post, self.static, self.roi_ids)()

    def _recapture(self):
        for _ in range(4):          # an eager pass may itself demote a layer: repeat until the set is stable
            before = (x3_policy.demoted(), x3_policy.gemm_products())
            self._eager_pass()
            if (x3_policy.demoted(), x3_policy.gemm_products()) == before:
                break
        self._capture()

    @torch.no_grad()
    def _capture(self):
        run = self._step
        self.graph = torch.cuda.CUDAGraph()
        n_x3, n_foreign = hip_lib.x3_launch_count(), hip_layers.fallback_launches()
        self.x3_flag.zero_()
        torch.cuda.synchronize()
        with hip_lib.x3_flag_scope(self.x3_flag), hip_lib.shared_min_tiles_scope(self.shared_min_tiles, self.shared_min_rows), \
                torch.cuda.graph(self.graph, stream=self.stream):
            self.records = run()
        self.uses_x3 = hip_lib.x3_launch_count() != n_x3     # the captured step holds three-product kernels
        self.foreign_launches = hip_layers.fallback_launches() - n_foreign
        if self.sharing and self.foreign_launches:
            raise RuntimeError(f"GraphedInference(sharing=True): the captured step launched {self.foreign_launches} kernel(s) outside this "
                               f"library (last: {hip_layers.last_fallback()}); such a graph must not run beside another stream's MFMAs on "
                               "MI355X — replay it on ONE stream (sharing=False)")
        self._demoted_at_capture = x3_policy.demoted()
        self._products_at_capture = x3_policy.gemm_products()
        self.captures += 1

    @torch.no_grad()
    def replay_async(self) -> GraphHandle:
        """Replay on the static buffers and return without waiting for the device; ``.result()`` -> the records f32[b,16] — a copy
        of the graph's static output made on the graph's stream right behind the replay (64 B per ROI), so the next replay of this
        graph cannot overwrite what the caller still reads on another stream."""
        if self._pending is not None:
            self._pending.result()
        if self.uses_x3 and (x3_policy.demoted() != self._demoted_at_capture or x3_policy.gemm_products() != self._products_at_capture):
            self._recapture()      # another step demoted a layer this graph still runs on three products
        with self._on_stream():
            self.graph.replay()
            if self.uses_x3:
                self._host_words.copy_(self.x3_flag, non_blocking=True)
            rec = self.records.clone()
            ev = torch.cuda.Event()
            ev.record()
        self._pending = GraphHandle(self, ev, rec)
        return self._pending

    @torch.no_grad()
    def _resolve(self, event, rec) -> torch.Tensor:
        self._pending = None
        caller = torch.cuda.current_stream()
        if self.uses_x3:
            event.synchronize()
            words = hip_lib.range_words_of(self._host_words)
            if words:
                with self._on_stream(), hip_lib.shared_min_tiles_scope(self.shared_min_tiles, self.shared_min_rows):
                    rec = _six_product_rerun(self._step, words)
                    self.reruns += 1
                    self._recapture()
                    self.records.copy_(rec)
                    event = torch.cuda.Event()
                    event.record()
        if self.stream is not None and self.stream != caller:
            caller.wait_event(event)            # the caller's stream reads the records behind the replay ...
            rec.record_stream(caller)           # ... and their memory (the graph stream's pool) is not handed out under it
        return rec

    @torch.no_grad()
    def replay(self) -> torch.Tensor:
        """Replay on the static buffers, then the range check of the graph's three-product kernels (synchronous form)."""
        return self.replay_async().result()

    @torch.no_grad()
    def load(self, batch: dict) -> None:
        """Copy a batch into the graph's static buffers on the graph's stream (behind the previous replay, which is resolved
        first: its inputs must not change under it)."""
        if self._pending is not None:
            self._pending.result()
        caller = torch.cuda.current_stream()
        with self._on_stream():
            if self.stream is not None and self.stream != caller:
                self.stream.wait_stream(caller)       # the batch was produced on the caller's stream
            for k, v in batch.items():
                if isinstance(v, torch.Tensor) and k in self.static:
                    self.static[k].copy_(v, non_blocking=True)
            if self.roi_ids is not None and isinstance(batch.get("roi_id"), torch.Tensor):
                self.roi_ids.copy_(batch["roi_id"], non_blocking=True)      # the ids the records carry travel with the batch

    @torch.no_grad()
    def __call__(self, batch: dict) -> torch.Tensor:
        self.load(batch)
        return self.replay()


class GraphedStepStreams:
    """Two hipGraphs in flight: the small-batch form of ``StepStreams``.  One ``GraphedInference`` per SLOT (a resident batch, or a
    static buffer batches are copied into), slots dealt round-robin to the dealer's compute streams and captured there with the
    dealer's shared-chip kernel rule — the kernels, and therefore every bit of the records, are those of the eager two-stream
    schedule; what disappears is the host's ~150 launches per step, which is what bounds 8-32 ROIs (the reference's own regime:
    one image per forward, gdrn_evaluator.py:697-750, demo/predictor_gdrn.py:133-143).

        gs = GraphedStepStreams(model, post, [batch0, batch1, batch2, batch3])   # default_graph_streams(model) = 4 streams
        h0 = gs.launch(0); h1 = gs.launch(1); ...                       # four steps in flight, ~0.1 ms of host time each
        rec0 = h0.result(); h2 = gs.launch(0, new_batch) ...            # (launching a slot again resolves its previous handle first)

    A model whose step launches kernels outside this library gets ONE stream (the static gate), and a capture that does so all
    the same raises (``GraphedInference(sharing=True)``)."""

    def __init__(self, model, post: GdrnHipPost, slot_batches, roi_ids=None, compute_streams=None, warmup: int = 2, device=None):
        slot_batches = list(slot_batches)
        if not slot_batches:
            raise ValueError("GraphedStepStreams needs at least one slot batch")
        dev = slot_batches[0]["roi_img"].device if device is None else torch.device(device)
        if isinstance(compute_streams, StepStreams):
            self.dealer = compute_streams
        else:
            n = default_graph_streams(model) if compute_streams is None else max(1, int(compute_streams))
            self.dealer = StepStreams(n, dev)
        streams = self.dealer.streams
        multi = len(streams) > 1
        rule, rows = ((self.dealer.shared_min_tiles(), self.dealer.shared_min_rows()) if multi and hip_lib.shared_min_tiles() == 0
                      else (None, None))
        ids = roi_ids if isinstance(roi_ids, (list, tuple)) else [roi_ids] * len(slot_batches)
        self.graphs = []
        for i, (bt, rid) in enumerate(zip(slot_batches, ids)):
            st = streams[i % len(streams)]      # None (StepStreams(1)): captured on a side stream, replayed on the caller's current one
            self.graphs.append(GraphedInference(model, post, bt, rid if rid is not None else bt.get("roi_id"), warmup=warmup, stream=st,
                                                shared_min_tiles=rule, shared_min_rows=rows, sharing=self.dealer.sharing()))

    def launch(self, slot: int, batch: dict | None = None) -> GraphHandle:
        g = self.graphs[slot % len(self.graphs)]
        if batch is not None:
            g.load(batch)
        return g.replay_async()
