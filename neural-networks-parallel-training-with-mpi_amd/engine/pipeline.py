"""The bucket pipeline of the comm-overlapped schedules (plain overlap, grouped with per-bucket
collectives, overlapped row-band): as soon as a bucket's last gradient is written its
all-reduce starts on the comm stream, followed there by that bucket's SGD update (gated on the
last reader of its weights, ``ev_wfree``), so only the final bucket's all-reduce + update remain
on the critical path.  With one rank the update of the whole arena runs once at the end.
Under gradient clipping (engine/optimizer.py) the collectives overlap the backward all the same,
but no update is issued before the join: the clip coefficient needs the whole reduced gradient,
so one norm, one finalize and one update of the whole arena follow the join.

Invariants (docs/ARCHITECTURE.md §1 records the hang at P = 2 and the capture crash at P = 3
that breaking them caused):

* every collective of a communicator is issued on the comm stream (GradSync.launch_bucket);
* bucket updates stay on the comm stream itself, gated on ``ev_wfree``: a third stream in a step
  graph whose capture origin is the comm stream (GradSync.capture_origin) crashes hipGraph
  instantiation on ROCm 7 (measured at 1 and 2 ranks: docs/PERF.md §3).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from ..utils.knobs import knob


class BucketPipeline:
    def __init__(self, spec, arena, ops, sync, opt, stream, *, grad16, bf16: bool, defer: bool):
        """``opt``: the optimizer every update goes through (engine/optimizer.py);
        ``grad16``: the bf16 payload the per-bucket updates read (None: the fp32 gradient);
        ``bf16``: bf16 compute; ``defer``: the schedule launches the chunk weight gradients that
        can carry deferred updates."""
        self.spec, self.arena, self.ops, self.sync = spec, arena, ops, sync
        self.opt, self.stream = opt, stream
        self.sharded = sync.sharded
        # ev_wfree[l]: the last reader of layer l's weights has been issued
        self.ev_wfree = ([torch.cuda.Event(enable_timing=False) for _ in range(spec.n_layers)]
                         if stream is not None else [])
        # bf16-payload overlapped schedule: per-bucket updates read the bf16 payload ...
        self.upd_grad = grad16
        # ... and the chunked weight gradients store that bf16 payload themselves
        self.w16 = grad16 is not None and bf16 and ops.can_write_bf16_wgrad()
        # Deferred updates (several ranks, bf16 payload written by the chunk weight gradients):
        # the SGD of chunk bucket (layer i+1, rows r0:r1) runs in the epilogue of the weight
        # gradient of chunk (layer i, rows r0:r1) -- same [rows, in] shape -- once its all-reduce
        # has completed (the compute stream waits for that collective's event), instead of as a
        # separate memory-bound pass next to compute-bound GEMMs.  defer_plan: chunk bucket
        # index -> the partner bucket it updates.
        # (not for the row-band schedules: they never launch the chunk weight gradients whose
        # epilogues would apply these updates, so every target bucket would fall to join())
        self.defer_plan: Dict[int, object] = {}
        # (only an optimizer the epilogues can apply: linear_wgrad_defer runs sgd_elem)
        if (self.w16 and defer and not self.sharded and self.opt.fusable
                and knob("NNMPI_DEFER", "1") != "0"):
            for i in range(spec.n_layers - 2):
                if spec.layer_shape(i) != spec.layer_shape(i + 1):
                    continue
                nxt = {b.rows: b for b in arena.chunk_buckets(i + 1)}
                for b in arena.chunk_buckets(i):
                    if b.rows in nxt:
                        self.defer_plan[b.index] = nxt[b.rows]
        self.defer_targets = {b.index for b in self.defer_plan.values()}
        # NNMPI_DEFER_WAIT=chunk: every deferred update waits on its own partner's collective
        # (default: one wait per partner layer, see defer_update)
        self.defer_wait_layer = knob("NNMPI_DEFER_WAIT", "layer") != "chunk"
        self.ev_ar = {b.index: torch.cuda.Event(enable_timing=False)
                      for b in self.defer_plan.values()}
        self._reset(True, None)

    def _reset(self, first: bool, images):
        self.first = first
        self.sgd_done = set()                 # buckets whose update is queued or issued
        self.reduced = {}                     # bucket index -> stream its collective completes on
        self.pending: List[Tuple[object, object]] = []   # (bucket, stream) updates not issued yet
        self.held: List[object] = []          # clipping: reduced buckets, updated behind the join
        self.written16: List[Tuple[int, int]] = []       # arena ranges stored as bf16 payload
        self.waited = set()                   # partner layers the compute stream has waited for
        # keywords of every bucket update: the bf16 payload, the row-band images to refresh
        self.upd_kw = {} if self.upd_grad is None else {"grad_bf16": self.upd_grad}
        if images is not None:
            self.upd_kw["images"] = images

    def begin(self, first: bool, images=None):
        """Start a step: the sync's begin and the only reset of the per-step state.  ``images``:
        {layer: (forward, dgrad)} row-band weight images the updates refresh."""
        self.sync.begin()
        self._reset(first, images)

    def sgd(self, offset: int, numel: int):
        self.opt.apply(self.first, offset=offset, numel=numel, **self.upd_kw)

    def update_all(self, first: bool):
        """Optimizer update of the whole arena (or, sharded, of this rank's slice + gathers)."""
        if self.sharded:
            # (its clip follows the reduce-scatter, inside update())
            self.sync.update(self.opt, first)
        else:
            self.opt.clip()        # (clipping off: launches nothing)
            self.opt.apply(first)

    def bucket_reduce(self, b, stream):
        """Launch bucket b's collective (once); returns the stream it completes on.  One queued
        bucket update is issued behind every new collective, so the comm stream alternates
        collectives and updates instead of parking a later collective behind an update that
        waits for its weights' last reader."""
        if b.index not in self.reduced:
            # bf16 payload: the bucket's update reads the reduced bf16 gradient directly
            kw = ({} if self.upd_grad is None else
                  {"cast_back": False, "written": self.written16})
            rs = self.reduced[b.index] = self.sync.launch_bucket(b, stream, **kw)
            if b.index in self.ev_ar and rs is not None:
                rs.record_event(self.ev_ar[b.index])
            self.flush(1)
        return self.reduced[b.index]

    def layer_done(self, layer: int, stream, record: bool = True):
        """Layer ``layer``'s gradient is final and its weights' last reader issued on ``stream``
        (``record``: record ev_wfree[layer] there now): reduce every bucket the layer completes
        and queue each bucket's SGD (on the stream its collective completes on, behind the last
        reader of its weights)."""
        if record:
            stream.record_event(self.ev_wfree[layer])
        for b in self.arena.buckets_completed_by(layer):
            rs = self.bucket_reduce(b, stream)
            if rs is None or rs is stream:
                continue   # reduced on this stream already (single rank): update once at the end
            if self.opt.clipping:
                # the clip coefficient needs the whole reduced gradient: the collectives still
                # overlap the backward, every update waits for join()
                self.held.append(b)
                continue
            self.pending.append((b, rs))
            self.sgd_done.add(b.index)

    def flush(self, n: Optional[int] = None):
        # (updates planned into a later weight-gradient epilogue stay queued for it;
        # join() runs whatever is left)
        while n is None or n > 0:
            k = next((k for k, (pb, _) in enumerate(self.pending)
                      if pb.index not in self.defer_targets), None)
            if k is None:
                break
            b, rs = self.pending.pop(k)
            with torch.cuda.stream(rs):
                for l in b.layers:
                    rs.wait_event(self.ev_wfree[l])
                self.sgd(b.offset, b.numel)
            if n is not None:
                n -= 1

    def defer_update(self, b, i: int, dz, x_in, g16) -> bool:
        """Launch chunk bucket b's weight gradient (layer i, bf16 payload) with the pending SGD
        of its partner bucket fused into the epilogue; False when there is nothing to fuse."""
        part = self.defer_plan.get(b.index)
        if part is None:
            return False
        k = next((n for n, (pb, _) in enumerate(self.pending) if pb.index == part.index), None)
        out_f, in_f = self.spec.layer_shape(i)
        r0, r1 = b.rows
        if k is None or not self.ops.wgrad_defer_ok(dz.shape[0], r1 - r0, in_f):
            return False
        self.pending.pop(k)
        ar, main = self.arena, self.stream
        if self.defer_wait_layer:
            # ONE cross-queue wait per layer: on the collective of the partner layer's last
            # chunk (the comm stream runs its collectives in order, so all earlier chunks of that
            # layer are reduced too) -- issued a whole dgrad earlier, so already complete unless
            # the links are slower than a dgrad; every cross-queue edge in a replayed graph costs
            # 5-10 us whether or not its event has completed (docs/PERF.md)
            li = part.layers[0]
            if li not in self.waited:
                last = max(b.index for b in ar.chunk_buckets(li))
                main.wait_event(self.ev_ar[last])
                self.waited.add(li)
        else:
            main.wait_event(self.ev_ar[part.index])      # the partner's all-reduce has completed
        woff = ar.by_name[f"layers.{2 * (i + 1)}.weight"].offset + part.rows[0] * in_f
        self.ops.linear_wgrad_defer(dz, x_in, ar.weight(i, g16)[r0:r1], ar.bias(i, g16)[r0:r1],
                                    ar, woff, g16, self.opt.fusion(self.first, offset=woff))
        # the rest of the partner bucket (its layer's bias and padding, in the last chunk)
        wend = woff + (r1 - r0) * in_f
        rest = part.offset + part.numel - wend
        if rest > 0:
            self.sgd(wend, rest)
        return True

    def join(self, joined=None):
        """Join the comm stream into the compute stream.  Updates still queued at this point
        (the last buckets) run after the join on the compute stream, merged into one SGD launch
        per contiguous range, instead of as a serial tail of small launches on the comm stream
        in front of the join; then (``joined()``, the engine's phase mark, in between) the
        buckets the comm stream did not update -- all of them on one rank: one pass."""
        tail, self.pending = self.pending, []
        self.sync.finish()   # joins the comm stream into the compute stream
        if self.held:
            # clipping, per-bucket collectives: one norm of the whole reduced gradient (of the
            # bf16 payload when that is what the update reads), one finalize, one update
            self.held = []
            if joined is not None:
                joined()
            self.opt.clip(grad_bf16=self.upd_grad)
            self.sgd(0, self.arena.numel)
            return
        runs: List[List[int]] = []           # [start, end) of each contiguous range
        for b in sorted((b for b, _ in tail), key=lambda b: b.offset):
            if runs and runs[-1][1] == b.offset:
                runs[-1][1] += b.numel
            else:
                runs.append([b.offset, b.offset + b.numel])
        for s, e in runs:
            self.sgd(s, e - s)
        if joined is not None:
            joined()
        if not self.sgd_done:
            self.update_all(self.first)                   # one pass over the whole arena
        else:
            for b in self.arena.buckets:
                if b.index not in self.sgd_done:
                    self.sgd(b.offset, b.numel)
