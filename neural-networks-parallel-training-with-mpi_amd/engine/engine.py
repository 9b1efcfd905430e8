"""Explicit data-parallel MLP training engine.

One step (per rank), replacing the reference's hot loop ``ref.py:155-211`` (DataLoader ->
``.float()`` -> forward -> MSELoss -> autograd backward -> gather/average/send -> SGD):

    forward   h_i = act(h_{i-1} W_i^T + b_i)                  hidden layers (GEMM + epilogue)
    head      logits, loss, dlogits, dZ_{L-2}, dW_{L-1}, db   fused output layer + loss
              -> grad bucket(s) of layer L-1 ready -> all-reduce starts on the comm stream
    backward  for i = L-2 .. 0:
                 dW_i, db_i = dZ_i^T h_{i-1}, sum(dZ_i)       wgrad (+ fused bias grad)
                 -> bucket ready -> all-reduce overlaps the rest of backward
                 dZ_{i-1} = (dZ_i W_i) * act'(h_{i-1})        dgrad + activation backward
    join      compute stream waits for the comm stream
    update    fused SGD-momentum over the whole arena (1/P folded in, bf16 shadow refreshed,
              gradients zeroed for the next step); or Adam / AdamW, one pass of the same shape
              behind a one-thread launch that advances the device step number (optimizer.py);
              with clip_grad_norm, the gradient's norm and a one-block launch that rewrites
              the gradient-scale slot run right before it

All buffers are allocated once (rows capacity), so on the GPU the steady-state step is
allocation-free and is captured into ONE hipGraph (kernels + RCCL + cross-stream events) that
is replayed every step.  The same schedule runs with :class:`~nnmpi_amd.ops.torch_ops.TorchOps`
on the CPU (gloo) — that is the reference-semantics path and the test oracle.

Layout: :meth:`MLPEngine._schedule` alone decides which ``_step_*`` body a batch runs; the
comm-overlapped bodies share :class:`~.pipeline.BucketPipeline`; :class:`WeightImages` holds the
row-band weight images.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple

import torch
from ..utils.knobs import knob

from ..models.mlp import MLPSpec
from ..parallel.sync import NativeRcclSync, NoSync, TorchDistSync
from .arena import Arena
from .optimizer import adam_hparams, make_optimizer, sgd_hparams
from .pipeline import BucketPipeline

TINY_MAX_WIDTH = 16
TINY_MAX_LAYERS = 4
LOSS_HIST_MAX = 1024   # steps per loss-recording graph (run_steps(..., losses=...))


class WeightImages:
    """v2 row-band kernel: the weights also live in fragment-major images (one global load per
    MFMA operand, no LDS staging -- rowband.hip).  The images must hold the CURRENT weights: the
    single-rank fused combine and the optimizer passes given ``images`` rewrite them from the
    updated weights; every other update path (ZeRO-1, other schedules, a reload of the arena
    -- Arena.version) leaves them stale and the next row-band step rebuilds them first."""

    def __init__(self, ops, arena, n_hidden: int, buf=None, views=None):
        self.ops, self.arena, self.n_hidden = ops, arena, n_hidden
        self.buf, self.views = buf, views     # one bf16 buffer; per layer (forward, dgrad) views
        self.fresh, self.ver = False, -1

    def by_layer(self):
        """{layer: (forward image, dgrad image)} for an optimizer pass that refreshes them."""
        return None if self.views is None else dict(enumerate(self.views))

    def current(self) -> bool:
        return self.fresh and self.ver == self.arena.version

    def mark(self, fresh: bool):
        """The weights were just updated with (``fresh``) or without the images."""
        self.fresh, self.ver = bool(fresh), self.arena.version

    def pack(self):
        """Rebuild the images from the bf16 shadow (one launch, on the current stream)."""
        self.ops.rowband_pack([self.arena.compute_weight(i) for i in range(self.n_hidden)],
                              self.views)
        self.mark(True)

    def snapshot(self):
        return self.fresh, self.ver

    def restore(self, state):
        self.fresh, self.ver = state


class MLPEngine:
    def __init__(self, spec: MLPSpec, arena: Arena, ops, sync, *, device, dtype: torch.dtype,
                 rows_capacity: int, lr: float, momentum: float, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, use_graph: bool = True,
                 use_tiny: Optional[bool] = None, overlap: bool = True, fuse_sgd: bool = True,
                 grouped: bool = True, rowband_overlap: bool = False,
                 rowband_plan: Optional[int] = None, optimizer: str = "sgd", beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-8,
                 clip_grad_norm: Optional[float] = None):
        """``optimizer``: ``sgd`` (momentum / dampening / nesterov apply), ``adam`` or ``adamw``
        (beta1 / beta2 / eps apply; ``momentum`` is ignored).  ``weight_decay`` is shared.
        ``clip_grad_norm``: clip the (reduced, averaged) gradient to this global L2 norm before
        every update, as ``torch.nn.utils.clip_grad_norm_`` does -- norm and coefficient are
        computed on the device inside the step (engine/optimizer.py); None: off."""
        self.spec, self.arena, self.ops, self.sync = spec, arena, ops, sync
        self.device = torch.device(device)
        self.dtype = dtype
        self.R = max(1, int(rows_capacity))
        self.is_cuda = self.device.type == "cuda"
        L = self.L = spec.n_layers
        w = spec.widths
        self.act, self.loss_kind = spec.activation, spec.loss
        bf16 = dtype == torch.bfloat16
        if use_tiny is None:
            # GPU: tiny_mlp.hip; CPU: the host twin when the op set has it (ops/host_ops.py)
            use_tiny = ((self.is_cuda or ops.tiny_supported()) and dtype == torch.float32
                        and L <= TINY_MAX_LAYERS and max(w) <= TINY_MAX_WIDTH)
        self.use_tiny = bool(use_tiny)
        # host-driven torch.distributed transports (gloo copies device tensors through the host;
        # torch's nccl runs on its own side stream) cannot live inside a replayed hipGraph
        self.use_graph = (bool(use_graph) and self.is_cuda
                          and not (isinstance(sync, TorchDistSync) and sync.world > 1))
        self._validate()
        dev, R = self.device, self.R
        self.stream = torch.cuda.Stream(device=dev) if self.is_cuda else None
        # persistent buffers
        self.X = torch.zeros(R, w[0], dtype=dtype, device=dev)
        mse = spec.loss == "mse"
        self.Y = torch.zeros(R, w[-1], dtype=torch.float32, device=dev) if mse else None
        self.labels = None if mse else torch.zeros(R, dtype=torch.int64, device=dev)
        self.acts = [torch.zeros(R, w[i + 1], dtype=dtype, device=dev) for i in range(L - 1)]
        self.dzl = [torch.zeros(R, w[i + 1], dtype=dtype, device=dev) for i in range(L - 1)]
        self.dlogits = torch.zeros(R, w[-1], dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=dev)
        adam = optimizer != "sgd"
        if adam and (nesterov or dampening):
            raise ValueError("nesterov / dampening are SGD options: not with " + str(optimizer))
        self.hp = (adam_hparams(lr, beta1, beta2, eps, weight_decay, dev) if adam else
                   sgd_hparams(lr, momentum, dampening, weight_decay, dev))
        # every update site goes through this object (engine/optimizer.py)
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0:    # (also NaN)
            raise ValueError(f"clip_grad_norm must be > 0, got {clip_grad_norm}")
        self.opt = make_optimizer(optimizer, ops, arena, self.hp, nesterov,
                                  clip_grad_norm=clip_grad_norm)
        # Adam cannot ride in the kernels' fused epilogues (SgdFuse: one state buffer, the SGD
        # formula): every schedule runs in its unfused form, the update a separate pass.  So
        # does a clipped step: its coefficient needs the whole reduced gradient
        fuse_sgd = bool(fuse_sgd) and self.opt.fusable
        # ---- what the configuration allows; _schedule() picks per batch from these ----------
        self.overlap = bool(overlap) and self.is_cuda and not self.use_tiny
        local = isinstance(sync, NoSync)
        self.fuse_sgd = bool(fuse_sgd) and self.overlap and local and bf16 and ops.can_fuse_sgd()
        # tiny single-rank model: the one-block kernel applies SGD itself (one launch per step)
        self.tiny_fused = (bool(fuse_sgd) and self.use_tiny and local
                           and ops.tiny_can_fuse_sgd(self.R))
        self._first = True
        self.ws = torch.zeros(max(1, self._workspace_bytes() // 4 + 64), dtype=torch.float32,
                              device=dev)
        self.sharded = bool(sync.sharded)
        inline_sync = local or self.sharded or (isinstance(sync, NativeRcclSync) and sync.inline)
        # per-bucket collectives on the native comm stream, each bucket's SGD behind them
        self.comm_overlap = isinstance(sync, NativeRcclSync) and not sync.inline
        # grouped backward (bf16 GPU): dgrad_i + wgrad_i + combine_{i+1} in one launch.  Layer
        # i's slabs live in ws_pair[(L-1-i) % 2] so they never alias the pending combine's.
        # (shapes the grouped kernel does not cover -- e.g. the 256x256-tile 8192-wide layers --
        # take the sequential fused schedule, whose un-split wgrads apply SGD in their epilogue)
        # (layers cut into output-row chunk buckets are reduced chunk by chunk behind their own
        # weight-gradient launches: the sequential schedule, never the grouped one)
        self.grouped = (bool(grouped) and self.overlap and bf16
                        and (inline_sync or self.comm_overlap)
                        and not any(b.rows is not None for b in arena.buckets) and L > 1
                        and all(ops.bwd_group_supported(self.R, *spec.layer_shape(i))
                                for i in range(L - 1)))
        self.ws_pair = [self.ws, torch.zeros_like(self.ws)] if self.grouped else [self.ws, self.ws]
        # Row-band step (narrow square MSE regressor, e.g. the 512-wide proxy): the forward, the
        # head and every activation gradient in ONE launch, all weight gradients in one more and
        # every combine (+ the fused update on one rank) in a third -- see rowband.hip.  Taken
        # whenever the gradient is reduced after the backward (one rank, the inline all-reduce,
        # ZeRO-1): it produces every layer's gradient at once, so there is nothing for a
        # per-bucket overlapped schedule to hide.  NNMPI_EXPERIMENTS=1 NNMPI_ROWBAND=0 keeps the grouped schedule
        # (proxy step 0.082 vs 0.094 ms, profiles/r3s2_rowband_*).
        # rowband_overlap: also with per-bucket collectives on the comm stream -- the band launch
        # and the last hidden layer's + the head's weight gradients first, their bucket's
        # all-reduce overlapping the other layers' weight gradients (_step_rowband_overlap)
        self.rb_overlap = bool(rowband_overlap) and self.comm_overlap
        self.rowband = (self.overlap and bf16 and (inline_sync or self.rb_overlap)
                        and knob("NNMPI_ROWBAND", "1") != "0"
                        and ops.rowband_ok(self.R, w, self.act, spec.loss))
        # split-K plan of the weight gradients (RowbandStep::plan): the overlapped schedule's
        # phased plan, else one launch filling the chip with every layer
        if rowband_plan is None:
            rowband_plan = int(knob("NNMPI_RB_PLAN", "1" if self.rb_overlap else "0"))
        self.rb_plan = int(rowband_plan)
        self.ws_rb = (torch.zeros(ops.rowband_workspace_bytes(self.R, w[1], L - 1, in_=w[0]) // 4 + 64,
                                  dtype=torch.float32, device=dev) if self.rowband else None)
        self.rb_version = ops.rowband_version(self.R, w, self.act, spec.loss) if self.rowband else 0
        self.images = WeightImages(ops, arena, L - 1, *(
            ops.rowband_packed(w[1], w[0], L - 1, dev) if self.rb_version == 2 else ()))
        # A band's passes cost the same whatever the number of bands (per-CU bound: 47 us at
        # 1,024 rows as at 8,192, profiles/r3s2_rowband_pmc.txt), so below this the band kernel
        # is not taken; small batches (strong-scaling shards: up to 4,096 rows of the 512-wide
        # proxy) run the column-split form instead (rowband.hip rowband_split_kernel: each band
        # over 2-8 CUs, activations exchanged per layer), everything else the grouped schedule.
        # 512-wide shards of 4,097-6,143 rows: the band kernel (the column-split form stops at
        # 4,096 rows) -- 0.0629 / 0.0641 / 0.0670 ms at 4,500 / 5,000 / 6,000 rows vs the grouped
        # schedule's 0.0811 / 0.0822 / 0.0868 (profiles/r6_rowband_threshold.txt); other widths
        # keep the measured 6,144
        self.rowband_min_rows = int(knob("NNMPI_ROWBAND_MIN_ROWS", "4097" if w[1] == 512 else "6144"))
        self._rb_split: Dict[int, bool] = {}
        # the per-bucket collectives and updates of the comm-overlapped bodies
        self.pipe = BucketPipeline(
            spec, arena, ops, sync, self.opt, self.stream, bf16=bf16,
            grad16=sync.update_grad() if self.comm_overlap else None, defer=not self.rb_overlap)
        self.rows = 0
        self._steps = 0
        self._graphs: Dict[tuple, object] = {}
        self.inv_count = 1.0
        self.loss_scale = 1.0
        self.timer = None   # utils.metrics.EventTimer: per-phase breakdown (steps run eagerly)
        self._acc = self._eval_gw = self._loss_hist = self._clip_hist = self._ev = None   # allocated on first use
        self._n_acc = 0

    @property
    def steps_done(self) -> int:
        """Optimizer steps taken.  Assigning it (a resume) also sets the optimizer's device-side
        step number; the engine's own bookkeeping advances ``_steps`` -- the device counter
        advances by itself, once per step, inside the step (Adam.tick)."""
        return self._steps

    @steps_done.setter
    def steps_done(self, n: int):
        self._steps = int(n)
        with self._on_stream():
            self.opt.set_step(self._steps)

    # names the tests, the trainer and the scripts read
    rb_packed = property(lambda self: self.images.views)
    _rb_buf = property(lambda self: self.images.buf)
    _defer_plan = property(lambda self: self.pipe.defer_plan)
    _rb_pack = property(lambda self: self.images.pack)

    def _mark(self, name: str = "comm"):
        # (the default is the mark the pipeline's join() places: pipe.join(self._mark))
        if self.timer is not None:
            self.timer.mark(name, self.stream)

    def _on_stream(self):
        """Context: the engine's stream is current (CPU: nothing)."""
        return torch.cuda.stream(self.stream) if self.is_cuda else contextlib.nullcontext()

    def _targets(self, rows: int):
        """(Y[:rows], labels[:rows]) of the loaded batch; the one the loss does not use is None."""
        return (self.Y[:rows] if self.Y is not None else None,
                self.labels[:rows] if self.labels is not None else None)

    # ------------------------------------------------------------------------------------
    def _validate(self):
        w = self.spec.widths
        # (any output layer: heads beyond the skinny kernels run on the general path)
        if self.is_cuda and not self.use_tiny and self.dtype == torch.bfloat16:
            if any(w[i] % 8 or w[i + 1] % 8 for i in range(self.L - 1)):
                raise ValueError(f"bf16 GPU path needs hidden/input widths % 8 == 0: {w}")

    def _workspace_bytes(self) -> int:
        ops, R, w = self.ops, self.R, self.spec.widths
        if self.use_tiny:
            return ops.tiny_workspace_bytes(R, self.arena.numel)
        need = ops.head_workspace_bytes(R, w[-2], w[-1])
        for i in range(self.L - 1):
            need = max(need, ops.wgrad_workspace_bytes(R, w[i + 1], w[i], self.dtype))
            # an output-row chunk is its own GEMM: fewer tiles than the whole layer, so it
            # may split K where the layer does not (1024 of 2048 rows at K = 1024: 2 splits)
            for b in self.arena.chunk_buckets(i):
                need = max(need, ops.wgrad_workspace_bytes(R, b.rows[1] - b.rows[0], w[i],
                                                           self.dtype))
        return need

    # ------------------------------------------------------------------------------------
    def set_hparams(self, lr=None, momentum=None, grad_scale=None):
        # written on the engine's stream: the kernels that read hp (SGD, fused combines) run
        # there, so the write is ordered before the next step and after the previous one
        if momentum is not None and self.opt.name != "sgd":
            raise ValueError("momentum is an SGD hyper-parameter (slot 1 holds Adam's beta1)")
        with self._on_stream(), torch.no_grad():
            # fill_ with a scalar is a kernel launch (capturable inside a graph, e.g. the
            # per-step scales of run_epoch); item assignment would copy a host tensor
            for k, v in ((0, lr), (1, momentum), (4, grad_scale)):
                if v is not None:
                    self.hp[k:k + 1].fill_(float(v))
            if grad_scale is not None and self.opt.clipping:
                # clip_finalize rewrites slot 4 every step as this base scale x the coefficient
                self.opt.clip_state[1:2].fill_(float(grad_scale))

    def set_scales(self, inv_count: float, loss_scale: float, grad_scale: float):
        """Loss-gradient scale (1/count), reported-loss scale, optimizer gradient scale (1/P)."""
        self.inv_count, self.loss_scale = float(inv_count), float(loss_scale)
        self.set_hparams(grad_scale=grad_scale)

    def load_batch(self, X: torch.Tensor, Y: Optional[torch.Tensor] = None,
                   labels: Optional[torch.Tensor] = None):
        """Copy a batch into the persistent (graph-stable) input buffers."""
        n = X.shape[0]
        if n > self.R:
            raise ValueError(f"batch of {n} rows exceeds capacity {self.R}")
        with self._on_stream(), torch.no_grad():
            self.X[:n].copy_(X, non_blocking=True)
            if self.Y is not None and Y is not None:
                self.Y[:n].copy_(Y.reshape(n, self.Y.shape[1]), non_blocking=True)
            if self.labels is not None and labels is not None:
                self.labels[:n].copy_(labels, non_blocking=True)
        self.rows = n

    def _load_rows(self, X, Y, labels, lo: int, hi: int):
        """load_batch of rows lo:hi of X and of whichever targets are given."""
        self.load_batch(X[lo:hi], *(t if t is None else t[lo:hi] for t in (Y, labels)))

    def _row_chunks(self, n: int):
        """(lo, hi) of the row-capacity chunks of n rows, in order."""
        return ((lo, min(n, lo + self.R)) for lo in range(0, n, self.R))

    def load_batch_indexed(self, X: torch.Tensor, Y: Optional[torch.Tensor],
                           labels: Optional[torch.Tensor], idx: torch.Tensor):
        """Mini-batch ``idx`` (int64, on the engine's device) of a resident shard, gathered
        straight into the persistent input buffers (HIP: one gather launch per tensor; the
        reference's DataLoader shuffle + per-row __getitem__ + collate, ref.py:146,155)."""
        n = idx.numel()
        if n > self.R:
            raise ValueError(f"batch of {n} rows exceeds capacity {self.R}")
        if n == 0:   # empty micro-batch of a short shard: zero gradient, still steps
            self.rows = 0
            return
        with self._on_stream(), torch.no_grad():
            self.ops.gather_rows(X, idx, self.X)
            if self.Y is not None and Y is not None:
                self.ops.gather_rows(Y.reshape(Y.shape[0], self.Y.shape[1]), idx, self.Y)
            if self.labels is not None and labels is not None:
                self.ops.gather_rows(labels, idx, self.labels)
        self.rows = n

    # ------------------------------------------------------------------------------------
    def _dzl(self, layer: int, rows: int) -> torch.Tensor:
        """Gradient w.r.t. the pre-activation of hidden layer ``layer`` (own buffer per layer,
        so a concurrent wgrad(layer) never races with the next dgrad's output)."""
        return self.dzl[layer][:rows]

    # ---------------- sequential schedule (CPU path, and the no-overlap debug mode) ----------
    def forward_backward(self):
        rows, ops, ar, L = self.rows, self.ops, self.arena, self.L
        if rows == 0 or self.use_tiny:
            if rows == 0:  # empty shard: contributes a zero gradient, still joins every collective
                self.loss_out.zero_()
                ar.grad.zero_()
            else:
                fz = self.opt.fusion(self._first) if self.tiny_fused else None
                ops.tiny_step(self.spec, ar, self.X[:rows], *self._targets(rows), self.inv_count,
                              self.loss_out, self.ws, sgd=fz, loss_scale=self.loss_scale)
            for i in reversed(range(L)):
                self.sync.ready(i)
            return
        x = self.X[:rows]
        h = self._forward(x)
        self._mark("fwd")
        last = L - 1
        dz = self._dzl(last - 1, rows) if L > 1 else None
        self._head(h, dz)
        self._mark("head")
        self.sync.ready(last)
        for i in range(L - 2, -1, -1):
            x_in = self.acts[i - 1][:rows] if i > 0 else x
            for _ in self._wgrad_chunks(i, dz, x_in):
                pass
            self.sync.ready(i)
            if i > 0:
                dz_next = self._dzl(i - 1, rows)
                ops.linear_dgrad(dz, ar.compute_weight(i), self.acts[i - 1][:rows], self.act, dz_next)
                dz = dz_next
        self._mark("bwd")

    def _wgrad_chunks(self, i: int, dz, x_in, bf16_out: bool = False):
        """Weight gradient of layer i; a layer cut into output-row chunk buckets (Arena
        .layer_chunks) is computed chunk by chunk, yielding each chunk's bucket as soon as its
        launch is queued (so its all-reduce can start while the next chunk computes).  Every
        output tile is the same GEMM tile over the same K either way: the result is bitwise
        independent of the chunking.

        ``bf16_out`` (bf16-payload overlapped schedule): the chunks' GEMM epilogues store the
        gradient straight into the bf16 payload buffer -- no fp32 gradient write and no cast
        pass; the layer's arena range is recorded in the pipeline's ``written16`` so its buckets
        skip the cast.  Same rounding as the cast: bitwise identical payload."""
        ar, pipe = self.arena, self.pipe
        gW, gb = ar.grad_weight(i), ar.grad_bias(i)
        chunks = ar.chunk_buckets(i)
        if not chunks:
            self.ops.linear_wgrad(dz, x_in, gW, gb, ws=self.ws)
            return
        g16 = pipe.upd_grad if bf16_out else None
        if g16 is not None:
            out_f, in_f = self.spec.layer_shape(i)
            if all(self.ops.wgrad_can_write_bf16(dz.shape[0], b.rows[1] - b.rows[0], in_f)
                   for b in chunks):
                pipe.written16.append(ar.layer_range[i])
            else:
                g16 = None
        for b in chunks:
            r0, r1 = b.rows
            if g16 is not None:
                if not pipe.defer_update(b, i, dz[:, r0:r1], x_in, g16):
                    self.ops.linear_wgrad(dz[:, r0:r1], x_in, None, None, out_bf16=(
                        ar.weight(i, g16)[r0:r1], ar.bias(i, g16)[r0:r1]))
            else:
                self.ops.linear_wgrad(dz[:, r0:r1], x_in, gW[r0:r1], gb[r0:r1], ws=self.ws)
            yield b

    def _forward(self, x):
        h = x
        for i in range(self.L - 1):
            out = self.acts[i][:self.rows]
            self.ops.linear_act(h, self.arena.compute_weight(i), self.arena.bias(i), self.act, out)
            h = out
        return h

    def _head(self, h, dz, sgd=None):
        rows, ar, last = self.rows, self.arena, self.L - 1
        kw = {"sgd": sgd} if sgd is not None else {}
        self.ops.head(h, ar.weight(last), ar.bias(last), *self._targets(rows),
                      self.loss_kind, self.inv_count, self.act if self.L > 1 else "none", dz,
                      ar.grad_weight(last), ar.grad_bias(last), self.dlogits[:rows], self.loss_out,
                      self.loss_scale, ws=self.ws, **kw)

    # ---------------- the schedule decision ----------------------------------------------------
    def _schedule(self, rows: Optional[int] = None) -> Tuple[str, bool]:
        """(body, split): the ``_BODIES`` entry a step of ``rows`` rows (default: the loaded
        batch) runs, and whether its row-band launches take the column-split kernel.  The only
        place a schedule is chosen: the step, schedule_name(), uses_rowband*() and the weight
        images' invalidation all read it.

        ``rows == 0`` always takes the sequential body (a short shard's empty mini-batch, a rank
        without rows): forward_backward zeroes the gradient and still issues every bucket's
        collective in backward order, so this rank joins the same collective sequence as its
        peers, whatever schedule they run."""
        rows = self.rows if rows is None else rows
        if not self.overlap or rows <= 0:
            return "sequential", False          # also CPU and the tiny one-launch step
        if self.rowband:
            split = rows < max(1, self.rowband_min_rows) and self._rb_split_ok(rows)
            if split or rows >= max(1, self.rowband_min_rows):
                return ("rowband_overlap" if self.rb_overlap else "rowband"), split
        if self.grouped:
            return "grouped", False
        return ("fused" if self.fuse_sgd else "overlap"), False

    def _rb_split_ok(self, rows: int) -> bool:
        if rows not in self._rb_split:
            w = self.spec.widths
            self._rb_split[rows] = bool(self.ops.rowband_split_ok(rows, w[1], w[0], self.L - 1,
                                                                  self.act))
        return self._rb_split[rows]

    def uses_rowband(self, rows: Optional[int] = None) -> bool:
        """True when a step of ``rows`` rows (default: the loaded batch) runs the row-band step."""
        return self._schedule(rows)[0].startswith("rowband")

    def uses_rowband_split(self, rows: Optional[int] = None) -> bool:
        """True when a step of ``rows`` rows runs the column-split row-band kernel (small batches
        below the band kernel's threshold)."""
        return self._schedule(rows)[1]

    def schedule_name(self) -> str:
        """The step schedule a batch of the loaded size runs (bench / result reports)."""
        return self._BODIES[self._schedule()[0]][1]

    def _step_body(self, first: bool):
        # Adam: the device step number advances and the bias corrections are refreshed first, on
        # the compute stream -- behind the previous step's join, ahead of every update of this
        # step on either stream (they wait for events recorded after it).  SGD launches nothing.
        self.opt.tick()
        self._mark("start")
        body = self._schedule()[0]
        if not body.startswith("rowband"):
            self.images.mark(False)       # this step updates the weights without the images
        self._BODIES[body][0](self, first)
        self._mark("update")

    def _step_sequential(self, first: bool):
        self._first = first
        self.sync.begin()
        self.forward_backward()
        self.sync.finish()
        self._mark("comm")
        if not self.tiny_fused or self.rows == 0:
            self.pipe.update_all(first)

    def _inline_tail(self, first: bool, zero_grad: bool = True, images=None):
        """The gradient is complete: reduce every bucket on the compute stream and update the
        whole arena in one pass (ZeRO-1: its reduce-scatter / owner update / all-gather).
        ``images``: row-band weight images the pass refreshes from the updated weights."""
        if self.sharded:
            return self.pipe.update_all(first)
        self.sync.begin()
        for b in self.arena.buckets:
            self.sync.launch_bucket(b, self.stream)
        self.sync.finish()
        self._mark("comm")
        self.opt.clip()            # (clipping off: launches nothing)
        self.opt.apply(first, zero_grad=zero_grad, images=images)
        if images is not None:
            self.images.mark(True)

    # ---------------- comm-overlapped schedule (GPU) -----------------------------------------
    # Compute stays on ONE stream (measured: splitting wgrad onto a side stream only adds
    # cross-stream waits — every GEMM already fills all 256 CUs, so nothing overlaps).  What runs
    # concurrently is communication: see engine/pipeline.py.
    def _step_overlap(self, first: bool):
        rows, ops, ar, L, main, pipe = self.rows, self.ops, self.arena, self.L, self.stream, self.pipe
        pipe.begin(first)
        x = self.X[:rows]
        h = self._forward(x)
        self._mark("fwd")
        last = L - 1
        dz = self._dzl(last - 1, rows) if L > 1 else None
        self._head(h, dz)
        self._mark("head")
        pipe.layer_done(last, main)
        for i in range(L - 2, -1, -1):
            x_in = self.acts[i - 1][:rows] if i > 0 else x
            for b in self._wgrad_chunks(i, dz, x_in, bf16_out=pipe.w16):
                pipe.bucket_reduce(b, main)      # chunk's all-reduce starts right away
            if i > 0:
                dz_next = self._dzl(i - 1, rows)
                ops.linear_dgrad(dz, ar.compute_weight(i), self.acts[i - 1][:rows], self.act, dz_next)
                dz = dz_next
            pipe.layer_done(i, main)
        self._mark("bwd")
        pipe.join(self._mark)

    # Single rank: a layer's gradient is final as soon as its split-K partials are combined, so
    # the reducer applies the SGD update itself (no gradient round trip through HBM, no separate
    # optimizer pass).  dgrad_i runs BEFORE wgrad_i here: it is the last reader of W_i.
    def _step_fused(self, first: bool):
        rows, ops, ar, L = self.rows, self.ops, self.arena, self.L
        fz = self.opt.fusion(first)
        x = self.X[:rows]
        h = self._forward(x)
        self._mark("fwd")
        last = L - 1
        dz = self._dzl(last - 1, rows) if L > 1 else None
        unfused = []
        if ops.head_can_fuse_sgd(self.spec.widths[-1], self.spec.widths[-2], self.loss_kind):
            self._head(h, dz, sgd=fz)
        else:
            self._head(h, dz)
            unfused.append(last)
        self._mark("head")
        # Wide layers (256x256-tile, un-split weight gradients): wgrad_i + its SGD epilogue runs
        # in ONE launch with dgrad_{i-1} (or, last, with wgrad_0) -- ops.wide_pair -- so the
        # memory-bound SGD epilogues overlap compute-bound main loops.  `pend` is the weight
        # gradient waiting for its partner; every hazard is as in the sequential order: W_i's
        # last reader dgrad_i ran in an earlier launch, dgrad_{i-1} reads only W_{i-1}.
        pend = None

        def wg_of(i, dz_i, x_in):
            return (dz_i, x_in, ar.grad_weight(i), ar.grad_bias(i))

        def pair_wg_ok(i, dz_i):
            out_f, in_f = self.spec.layer_shape(i)
            return ops.wide_pair_wgrad_ok(dz_i.shape[0], out_f, in_f)

        def issue_wgrad(i, dz_i, x_in):
            out_f, in_f = self.spec.layer_shape(i)
            # dgrad_i was issued before: nothing reads W_i any more, so even an un-split wgrad
            # may update it in its epilogue
            if ops.wgrad_can_fuse_sgd(rows, out_f, in_f, self.dtype, epilogue=True):
                ops.linear_wgrad(dz_i, x_in, ar.grad_weight(i), ar.grad_bias(i), ws=self.ws, sgd=fz)
            else:
                ops.linear_wgrad(dz_i, x_in, ar.grad_weight(i), ar.grad_bias(i), ws=self.ws)
                unfused.append(i)

        for i in range(L - 2, -1, -1):
            x_in = self.acts[i - 1][:rows] if i > 0 else x
            dz_i = dz
            if i > 0:
                dz_next = self._dzl(i - 1, rows)
                dg = (dz_i, ar.compute_weight(i), self.acts[i - 1][:rows], self.act, dz_next)
                out_f, in_f = self.spec.layer_shape(i)
                if pend is not None and pair_wg_ok(pend[0], pend[1]) and \
                        ops.wide_pair_dgrad_ok(rows, out_f, in_f):
                    ops.wide_pair(wg_of(*pend), fz, dgrad=dg)
                else:
                    if pend is not None:
                        issue_wgrad(*pend)
                    ops.linear_dgrad(*dg)
                pend = None
                dz = dz_next
            if pend is not None:            # i == 0: the last two weight gradients
                if pair_wg_ok(pend[0], pend[1]) and pair_wg_ok(i, dz_i):
                    ops.wide_pair(wg_of(*pend), fz, wgrad2=wg_of(i, dz_i, x_in), sgd2=fz)
                    pend = None
                    continue
                issue_wgrad(*pend)
            pend = (i, dz_i, x_in)
        if pend is not None:
            issue_wgrad(*pend)
        self._mark("bwd")
        self._sgd_layers(unfused, first)

    def _sgd_layers(self, layers, first: bool):
        """Separate optimizer passes for the layers whose kernels could not apply the update."""
        for i in layers:
            s, e = self.arena.layer_range[i]
            self.opt.apply(first, offset=s, numel=e - s)

    def check_device_errors(self):
        """Raise if a column-split row-band step gave up a bounded wait (a band's blocks were not
        all resident within 2 ms: its results are invalid).  Reads one device word (host sync)."""
        if self.ws_rb is not None and any(self._rb_split.values()):
            i = self.ops.rowband_error_word()
            word = self.ws_rb[i:i + 1].view(torch.int32)
            if int(word.item()) != 0:
                # sticky until read: clear it so one timed-out step is reported once
                with torch.no_grad():
                    word.zero_()
                torch.cuda.synchronize(self.device)
                raise RuntimeError("row-band split step: a band's hand-off wait timed out (results invalid)")

    # Row-band schedule (see rowband.hip): three launches per step.  One rank: the combine
    # applies the SGD update; several ranks: the combine writes the gradient, then the inline
    # all-reduce (or ZeRO-1's reduce-scatter / all-gather) and the update follow.
    def _rb_layers(self):
        rows, ar = self.rows, self.arena
        # (the last hidden layer's activations are consumed inside the band -- head and its
        # weight-gradient partials -- so the hot path does not copy them out; evaluation and the
        # other schedules recompute or write their own)
        last = self.L - 2
        return [(ar.compute_weight(i), ar.bias(i), self.acts[i][:rows] if i < last else None,
                 self._dzl(i, rows), ar.grad_weight(i), ar.grad_bias(i))
                for i in range(self.L - 1)]

    def _rb_launch(self, sgd=None, phase: int = 0):
        rows, ar, last = self.rows, self.arena, self.L - 1
        kw = {}
        if self.images.views is not None:
            if phase <= 1 and not self.images.current():
                self.images.pack()
            kw["packed"] = self.images.views
        self.ops.rowband_step(self.X[:rows], self._rb_layers(), ar.weight(last), ar.bias(last),
                              self.Y[:rows], self.inv_count, ar.grad_weight(last),
                              ar.grad_bias(last), self.ws_rb, self.loss_scale, self.loss_out,
                              self.act, sgd=sgd, phase=phase, plan=self.rb_plan,
                              split=1 if self._schedule(rows)[1] else 0, **kw)

    # Row-band step with per-bucket collectives on the comm stream (several ranks): the band
    # launch and the last hidden layer's + the head's weight gradients first (phase 1); their
    # bucket's all-reduce -- and its SGD, which also refreshes that layer's v2 images -- run on
    # the comm stream while the other layers' weight gradients compute (phase 2); the buckets
    # those complete follow.  Every weight's last reader is the band launch.
    def _step_rowband_overlap(self, first: bool):
        L, main, pipe = self.L, self.stream, self.pipe
        pipe.begin(first, images=self.images.by_layer())
        self._rb_launch(phase=1)
        for l in range(L):
            main.record_event(pipe.ev_wfree[l])
        self._mark("bwd_tail")
        pipe.layer_done(L - 1, main, record=False)
        pipe.layer_done(L - 2, main, record=False)
        if L > 2:
            self._rb_launch(phase=2)
            for i in range(L - 3, -1, -1):
                pipe.layer_done(i, main, record=False)
        self._mark("bwd")
        pipe.join(self._mark)
        self.images.mark(self.images.views is not None)

    def _step_rowband(self, first: bool):
        fz = self.opt.fusion(first) if self.fuse_sgd else None
        self._rb_launch(sgd=fz)
        # the fused combine rewrote the images from the updated weights; of the multi-rank
        # updates below only the inline tail's optimizer pass does
        self.images.mark(fz is not None)
        self._mark("bwd")
        if fz is None:
            # (every gradient element the pass reads is rewritten by the next step's launches --
            # the combines store whole layer gradients, the arena's padding is never written and
            # stays zero -- so the pass does not zero the gradient behind itself: 3 MB less to
            # write on the 512-wide proxy)
            self._inline_tail(first, zero_grad=False, images=self.images.by_layer())

    # Grouped schedule: the backward of layer i is ONE launch holding three independent jobs —
    # dgrad_i, wgrad_i (split-K partial slabs) and the slab combine of layer i+1 (with the SGD
    # update fused on a single rank) — so each job's tail is filled by the others' blocks and
    # the step has L+1 fewer launch gaps.  Hazards: combine_{i+1} updates W_{i+1}, which no job
    # of the group reads (dgrad_i reads W_i); the two slab workspaces alternate.
    def _step_grouped(self, first: bool):
        rows, ops, ar, L, main, pipe = self.rows, self.ops, self.arena, self.L, self.stream, self.pipe
        fz = self.opt.fusion(first) if self.fuse_sgd else None
        comm = self.comm_overlap
        if comm:
            # several ranks, per-bucket collectives: each combine's finished layer gradient goes
            # straight to its bucket's all-reduce on the comm stream (its SGD follows there)
            # while the next grouped launch computes
            pipe.begin(first)
        x = self.X[:rows]
        h = self._forward(x)
        self._mark("fwd")
        last = L - 1
        dz = self._dzl(last - 1, rows)
        unfused = []
        pending_layer = last
        if ops.head_can_fuse_sgd(self.spec.widths[-1], self.spec.widths[-2], self.loss_kind):
            y, labels = self._targets(rows)
            pending = ops.head_deferred(
                h, ar.weight(last), ar.bias(last), y, self.inv_count, self.act, dz,
                ar.grad_weight(last), ar.grad_bias(last), self.loss_out, self.loss_scale,
                self.ws_pair[0], sgd=fz, labels=labels, loss=self.loss_kind,
                dlogits=self.dlogits[:rows])
        else:
            self._head(h, dz)
            pending = None
            pending_layer = None          # the head's gradient is already final
            unfused.append(last)
            if comm:
                pipe.layer_done(last, main)
        self._mark("head")
        for i in range(L - 2, -1, -1):
            x_in = self.acts[i - 1][:rows] if i > 0 else x
            dgrad = None
            dz_i = dz
            if i > 0:
                dz = self._dzl(i - 1, rows)
                dgrad = (dz_i, ar.compute_weight(i), self.acts[i - 1][:rows], self.act, dz)
            out_f, in_f = self.spec.layer_shape(i)
            fuse = fz is not None and ops.wgrad_can_fuse_sgd(rows, out_f, in_f, self.dtype)
            if not fuse:
                unfused.append(i)
            pending = ops.bwd_group(dgrad, (dz_i, x_in, ar.grad_weight(i), ar.grad_bias(i),
                                            self.ws_pair[(last - i) % 2]),
                                    fz if fuse else None, pending)
            if comm and pending_layer == i + 1:
                # this launch held combine_{i+1}: layer i+1's gradient is final, and its
                # weights' last reader (dgrad_{i+1} / the head) ran in an earlier launch
                pipe.layer_done(i + 1, main)
            pending_layer = i
        ops.slab_reduce(pending)
        self._mark("bwd")
        if comm:
            pipe.layer_done(0, main)
            pipe.join(self._mark)
        elif fz is not None:
            self._sgd_layers(unfused, first)
        else:
            self._inline_tail(first)

    # body -> (function, the name schedule_name() reports).  The single-rank fused schedule
    # reports "overlap"; tiny, CPU and empty batches run -- and report -- the sequential body.
    _BODIES = {"sequential": (_step_sequential, "sequential"),
               "rowband": (_step_rowband, "rowband"),
               "rowband_overlap": (_step_rowband_overlap, "rowband_overlap"),
               "grouped": (_step_grouped, "grouped"),
               "fused": (_step_fused, "overlap"),
               "overlap": (_step_overlap, "overlap")}

    def step(self):
        """One optimizer step on the loaded batch.  Asynchronous on the GPU."""
        first = self.steps_done == 0
        with self._on_stream():
            if first or not self.use_graph or self.timer is not None:   # (CPU: never a graph)
                self._step_body(first)
            else:
                # scales are baked into the captured launches -> part of the key
                key = (self.rows, self.inv_count, self.loss_scale)
                g = self._graphs.get(key)
                if g is None:
                    try:
                        g = self._capture()
                    except RuntimeError as e:   # e.g. a collective that cannot be captured
                        import sys
                        print(f"[nnmpi] hipGraph capture failed ({e}); running eagerly",
                              file=sys.stderr, flush=True)
                        self.use_graph = False
                        self._step_body(False)
                        self._steps += 1
                        return
                    self._graphs[key] = g
                g.launch(int(self.stream.cuda_stream))
        self._steps += 1

    # ---------------- multi-step graphs ------------------------------------------------------
    # A hipGraph replay has a fixed cost (~8 us measured between consecutive replays on MI355X,
    # MI355X_MICROARCH.md "graph-replay-floor"), which is ~8 % of a 512-wide step.  When the
    # host has nothing to do between steps (a timed loop, full-batch epochs without per-step
    # output) the engine can replay graphs holding `chunk` complete consecutive steps.
    def _chunks(self, n: int, chunk: int):
        return [min(chunk, n - k) for k in range(0, n, chunk)]

    def _keep_clip(self, dst: torch.Tensor):
        """dst[0, :] = (norm, coefficient) of the step just issued (a copy on the stream)."""
        dst.view(-1)[:2].copy_(self.opt.clip_state[2:4])

    def prepare_steps(self, n: int, chunk: int = 16, losses: bool = False):
        """Capture (without running) every graph that run_steps(n, chunk) will replay
        (``losses``: the form that records every step's loss, see run_steps)."""
        if not (self.is_cuda and self.use_graph and self.timer is None and self.steps_done > 0):
            return
        with torch.cuda.stream(self.stream):
            for c in set(self._chunks(n, chunk)):
                key = (self.rows, self.inv_count, self.loss_scale, c, losses)
                if key not in self._graphs:
                    self._graphs[key] = self._capture(c, hist=losses)

    def run_steps(self, n: int, chunk: int = 16, losses: Optional[torch.Tensor] = None,
                  clips: Optional[torch.Tensor] = None):
        """n optimizer steps (asynchronous on the GPU).  In graph mode the steps are replayed as
        graphs of up to `chunk` consecutive steps; results are identical to n step() calls.

        ``losses``: a device fp32 tensor of >= n entries; step k's loss (what loss() would
        return right after it) lands in losses[k] -- per-step losses without a host sync per
        step (the compat trainer's full-batch epochs).  Written on the engine's stream:
        synchronize() before reading them on the host.  ``clips`` (with ``losses``, under
        clip_grad_norm): a device fp32 tensor [>= n, 2]; step k's pre-clip gradient norm and
        clip coefficient land in clips[k] the same way."""
        k0 = 0
        if clips is not None and (losses is None or not self.opt.clipping):
            raise ValueError("run_steps(clips=) needs losses= and an engine with clip_grad_norm")

        def keep(k):
            if losses is not None:
                with self._on_stream():
                    losses[k:k + 1].copy_(self.loss_out[:1])
                    if clips is not None:
                        self._keep_clip(clips[k])
        if not (self.is_cuda and self.use_graph and self.timer is None):
            for k in range(n):
                self.step()
                keep(k)
            return
        if n > 0 and self.steps_done == 0:
            self.step()          # eager first step (momentum initialisation semantics)
            keep(0)
            n -= 1
            k0 = 1
        hist = losses is not None
        try:
            self.prepare_steps(n, chunk, losses=hist)
        except RuntimeError:
            for k in range(n):   # capture unavailable: step() falls back to eager by itself
                self.step()
                keep(k0 + k)
            return
        with torch.cuda.stream(self.stream):
            for c in self._chunks(n, chunk):
                self._graphs[(self.rows, self.inv_count, self.loss_scale, c, hist)].launch(
                    int(self.stream.cuda_stream))
                if hist:
                    losses[k0:k0 + c].copy_(self._loss_hist[:c])
                    if clips is not None:
                        clips[k0:k0 + c, :2].copy_(self._clip_hist[:c])
                self._steps += c
                k0 += c

    def run_epoch(self, X: torch.Tensor, Y: Optional[torch.Tensor],
                  labels: Optional[torch.Tensor], perm: torch.Tensor, plan) -> None:
        """One mini-batch epoch as ONE graph replay: for every ``(lo, hi, inv_count, loss_scale,
        grad_scale)`` of ``plan`` the rows ``perm[lo:hi]`` of the resident shard are gathered
        into the input buffers and a step is taken with those scales -- exactly what
        load_batch_indexed + set_scales + step() do per step, with the per-step host work
        gone.  ``perm`` must be the same device buffer every epoch (rewrite its contents; the
        graph holds its address).  Falls back to those per-step calls when graphs are off or
        no step has run yet."""
        plan = [tuple(p) for p in plan]

        def body(step):
            for lo, hi, inv, lsc, gsc in plan:
                self.load_batch_indexed(X, Y, labels, perm[lo:hi])
                self.set_scales(inv, lsc, gsc)
                step()
        if not (self.is_cuda and self.use_graph and self.timer is None and self.steps_done > 0):
            return body(self.step)
        key = ("epoch", tuple(plan), X.data_ptr(), perm.data_ptr(),
               None if Y is None else Y.data_ptr(), None if labels is None else labels.data_ptr())
        with torch.cuda.stream(self.stream):
            g = self._graphs.get(key)
            if g is None:
                g = self._capture_fn(lambda: body(lambda: self._step_body(False)))
                self._graphs[key] = g
            else:
                # the host-side state the per-step calls would leave behind (rows, scales)
                lo, hi, inv, lsc, gsc = plan[-1]
                self.rows = hi - lo
                self.inv_count, self.loss_scale = float(inv), float(lsc)
            g.launch(int(self.stream.cuda_stream))
        self._steps += len(plan)

    def _capture(self, nsteps: int = 1, hist: bool = False):
        """One graph of ``nsteps`` consecutive steps; ``hist``: step k also copies its loss into
        self._loss_hist[k] (a node inside the graph)."""
        if hist:
            # allocated once: captured graphs keep writing to this address
            if self._loss_hist is None:
                self._loss_hist = torch.zeros(LOSS_HIST_MAX, dtype=torch.float32, device=self.device)
            if nsteps > LOSS_HIST_MAX:
                raise ValueError(f"loss-recording graphs hold at most {LOSS_HIST_MAX} steps")
            # under clipping each step's (norm, coefficient) is recorded the same way
            if self.opt.clipping and self._clip_hist is None:
                self._clip_hist = torch.zeros(LOSS_HIST_MAX, 2, dtype=torch.float32,
                                              device=self.device)

        def body():
            for k in range(nsteps):
                self._step_body(False)
                if hist:
                    self._loss_hist[k:k + 1].copy_(self.loss_out[:1])
                    if self.opt.clipping:
                        self._keep_clip(self._clip_hist[k])
        return self._capture_fn(body)

    def _capture_fn(self, body):
        """Capture ``body()`` (work on the engine's streams) as one replayable graph."""
        from .. import native
        g = native.lib().GraphRunner()
        # the row-band image state the captured body assumes at its start, and leaves behind
        rb_pre, rb_pre_current = self.images.snapshot(), self.images.current()
        # collectives live on the comm stream: it is the capture origin, the compute stream
        # forks from it here and joins back below (see GradSync.capture_origin)
        origin = self.sync.capture_origin()
        if origin is None:
            origin = self.stream
        g.begin(int(origin.cuda_stream))
        self.sync.record(True)
        try:
            if origin is not self.stream:
                self.stream.wait_stream(origin)
            body()
            if origin is not self.stream:
                origin.wait_stream(self.stream)
        except Exception:
            self.sync.record(False)
            g.cancel()    # leave the stream out of capture mode, drop the partial graph
            self.images.restore(rb_pre)
            raise
        # (record(False) rolls the sequence number and the signature back: the capture issued
        # these collectives once, but every launch runs them, and the launch adds them to the
        # collective signature -- utils/seqcheck.py)
        notes = self.sync.record(False)
        g.end()
        rb_post = self.images.fresh
        self.images.restore(rb_pre)     # nothing ran yet
        return _Graph(g, self.sync, notes, self.images, self.stream, rb_pre_current, rb_post)

    # ---------------- gradient accumulation ----------------------------------------------------
    # Not in the reference (one backward per step, SURVEY.md §2.3 "optional").  A step over more
    # rows than fit the activation buffers is cut into micro-batches: each runs the sequential
    # forward/backward kernels with communication and the optimizer switched off and its
    # gradient is added into an fp32 accumulation arena; the step's gradient synchronisation
    # and update then run ONCE on the sum.  set_scales() must carry the row count of the whole
    # step (inv_count = 1/rows_step), so the sum is the step's mean gradient and the summed
    # micro-batch losses are the step's mean loss.
    def accumulate(self):
        """Forward + backward of the loaded micro-batch; gradient and loss are added to the
        accumulators (asynchronous on the GPU)."""
        ar = self.arena
        if self._acc is None:
            self._acc = torch.zeros_like(ar.grad)
            self._acc_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        with self._on_stream(), torch.no_grad():
            sync, tiny_fused = self.sync, self.tiny_fused
            self.sync, self.tiny_fused = _SilentSync(), False
            try:
                self.forward_backward()
            finally:
                self.sync, self.tiny_fused = sync, tiny_fused
            if self._n_acc == 0:
                self._acc.copy_(ar.grad)
                self._acc_loss.copy_(self.loss_out[:1])
            else:
                self._acc.add_(ar.grad)
                self._acc_loss.add_(self.loss_out[:1])
        self._n_acc += 1

    def apply_accumulated(self):
        """Gradient synchronisation + optimizer update on the accumulated gradient: one optimizer
        step (steps_done += 1).  The accumulators restart empty."""
        if not self._n_acc:
            raise RuntimeError("apply_accumulated() without a preceding accumulate()")
        first = self.steps_done == 0
        ar = self.arena
        with self._on_stream(), torch.no_grad():
            self.opt.tick()      # once per optimizer step, however many micro-batches it summed
            ar.grad.copy_(self._acc)
            self.loss_out[:1].copy_(self._acc_loss)
            self._first = first
            self.sync.begin()
            for i in reversed(range(self.L)):
                self.sync.ready(i)
            self.sync.finish()
            self.pipe.update_all(first)      # (clips once, on the accumulated sum)
        self.images.mark(False)
        self._n_acc = 0
        self._steps += 1

    # ---------------- evaluation (forward only) ---------------------------------------------
    def evaluate(self, X: torch.Tensor, Y: Optional[torch.Tensor] = None,
                 labels: Optional[torch.Tensor] = None):
        """Forward-only loss over held-out rows, chunked by the row capacity.  Parameters and
        optimizer state are untouched (the head's gradient outputs go to scratch buffers and no
        optimizer fusion is requested).  The training batch in the input buffers is overwritten:
        reload it before the next step.  Returns (sum of per-row losses, rows); the reference's
        validation/test hooks are dead code (ref.py:213-236)."""
        n = X.shape[0]
        if n == 0:
            return 0.0, 0
        out_f = self.spec.widths[-1]
        per = out_f if self.loss_kind == "mse" else 1
        last = self.L - 1
        if self._eval_gw is None:
            self._eval_gw = torch.zeros_like(self.arena.grad_weight(last))
            self._eval_gb = torch.zeros_like(self.arena.grad_bias(last))
        total = 0.0
        for lo, hi in self._row_chunks(n):
            self._load_rows(X, Y, labels, lo, hi)
            rows = self.rows
            with self._on_stream(), torch.no_grad():
                if self.use_tiny:
                    # the one-block kernel's mean loss (its gradient output is rewritten by the
                    # next training step; no optimizer fusion here)
                    self.ops.tiny_step(self.spec, self.arena, self.X[:rows], *self._targets(rows),
                                       1.0 / (rows * per), self.loss_out, self.ws, sgd=None)
                    scale = rows * per
                else:
                    h = self._forward(self.X[:rows])
                    self.ops.head(h, self.arena.weight(last), self.arena.bias(last),
                                  *self._targets(rows), self.loss_kind, 0.0,
                                  self.act if self.L > 1 else "none", None,
                                  self._eval_gw, self._eval_gb, self.dlogits[:rows], self.loss_out,
                                  1.0, ws=self.ws)
                    scale = 1.0
            total += self.loss() * scale
        return total, n

    # ---------------- prediction / metrics (forward only, head_eval.hip) -----------------------
    # Both run the hidden layers with the sequential GEMMs (_forward: the compute weights a
    # training step would use; a tiny-path engine takes them too, in fp32) and then the
    # forward-only head on the fp32 master of the last layer -- what evaluate() passes.  Neither
    # is captured into a graph.  They leave parameters, optimizer state, gradients, dlogits,
    # loss_out, the clip state and the step counters alone; like evaluate() they OVERWRITE the
    # input and activation buffers: reload the training batch before the next step.
    def _eval_buffers(self):
        if self._ev is None:
            w, dev = self.spec.widths, self.device
            nws = max(1, self.ops.head_eval_workspace_bytes(self.R, w[-2], w[-1]) // 4 + 16)
            with self._on_stream():     # filled on the stream that uses them
                self._ev = {
                    "metrics": torch.zeros(4, dtype=torch.float64, device=dev),
                    "logits": torch.zeros(self.R, w[-1], dtype=torch.float32, device=dev),
                    "pred": torch.zeros(self.R, dtype=torch.int32, device=dev),
                    "ws": torch.zeros(nws, dtype=torch.float32, device=dev)}
        return self._ev

    def _eval_chunk(self, X, Y, labels, lo: int, hi: int, loss=None, **outputs):
        """Rows lo..hi through the hidden layers and the forward-only head (on the stream);
        ``loss``: the loss whose targets (loaded with the rows) the head reads, None: neither."""
        self._load_rows(X, Y, labels, lo, hi)
        rows, last = self.rows, self.L - 1
        y, lab = self._targets(rows) if loss is not None else (None, None)
        with self._on_stream(), torch.no_grad():
            h = self._forward(self.X[:rows])
            self.ops.head_eval(h, self.arena.weight(last), self.arena.bias(last), y, lab, loss,
                               **outputs)

    def predict(self, X: torch.Tensor, classes: bool = False) -> torch.Tensor:
        """The model's outputs for the rows of ``X`` with the current parameters: fp32
        ``[n, out]`` (logits under cross-entropy, the regression output under MSE), or with
        ``classes=True`` the int64 argmax ``[n]`` (``torch.argmax``'s rule).  Chunked by the
        row capacity; ``n == 0`` returns an empty tensor without a launch.  Overwrites the input
        and activation buffers (see above); synchronises the engine's stream before returning."""
        n, out_f = X.shape[0], self.spec.widths[-1]
        res = (torch.empty(n, dtype=torch.int64, device=self.device) if classes else
               torch.empty(n, out_f, dtype=torch.float32, device=self.device))
        if n == 0:
            return res
        ev = self._eval_buffers()
        for lo, hi in self._row_chunks(n):
            rows = hi - lo
            if classes:
                self._eval_chunk(X, None, None, lo, hi, pred_out=ev["pred"][:rows])
            else:
                self._eval_chunk(X, None, None, lo, hi, logits_out=ev["logits"][:rows])
            with self._on_stream(), torch.no_grad():
                res[lo:hi].copy_(ev["pred"][:rows] if classes else ev["logits"][:rows])
        self.synchronize()
        return res

    def evaluate_metrics(self, X: torch.Tensor, Y: Optional[torch.Tensor] = None,
                         labels: Optional[torch.Tensor] = None) -> dict:
        """Forward-only metrics over held-out rows, chunked by the row capacity: ``loss_sum``
        (the per-row sums evaluate() returns), ``rows``, ``correct`` (cross-entropy: rows whose
        argmax is the label, else 0) and ``abs_err_sum`` (MSE: sum of |output - target|, else 0)
        as Python numbers.  Every chunk accumulates on the device (float64, fixed order): ONE host
        synchronisation at the end.  Overwrites the input and activation buffers (see above)."""
        n = X.shape[0]
        if n == 0:
            return {"loss_sum": 0.0, "rows": 0, "correct": 0, "abs_err_sum": 0.0}
        ev = self._eval_buffers()
        for lo, hi in self._row_chunks(n):
            self._eval_chunk(X, Y, labels, lo, hi, loss=self.loss_kind,
                             metrics=ev["metrics"], accumulate=lo > 0, ws=ev["ws"])
        self.synchronize()      # (also check_device_errors, as loss() does)
        m = ev["metrics"].tolist()
        return {"loss_sum": float(m[0]), "rows": int(m[3]), "correct": int(m[1]),
                "abs_err_sum": float(m[2])}

    def loss(self) -> float:
        """Local (this rank's) mean loss of the last step (host sync)."""
        if self.is_cuda:
            self.stream.synchronize()
        self.check_device_errors()
        return float(self.loss_out[0].item())

    def _clip_slot(self, k: int) -> float:
        if not self.opt.clipping:
            raise RuntimeError("gradient clipping is off (MLPEngine(clip_grad_norm=...))")
        if self.is_cuda:
            self.stream.synchronize()
        return float(self.opt.clip_state[k].item())

    def grad_norm(self) -> float:
        """Global L2 norm of the last step's reduced, averaged gradient, before clipping (host
        sync).  Raises when clipping is off: nothing computes a norm then."""
        return self._clip_slot(2)

    def clip_coef(self) -> float:
        """The last step's clip coefficient min(1, max_norm / (norm + 1e-6)) (host sync)."""
        return self._clip_slot(3)

    def synchronize(self, check: bool = True):
        """Wait for the engine's stream.  ``check``: then raise if a column-split row-band step
        gave up a hand-off wait since the last check (one device word read; only once a split
        step has run) -- every host sync of the training paths sees a timed-out step instead of
        training on.  A timed region passes check=False and calls check_device_errors() after
        its clock stops."""
        if self.is_cuda:
            self.stream.synchronize()
            if check:
                self.check_device_errors()

    @property
    def flops_per_step(self) -> float:
        return float(self.spec.flops_per_sample()) * self.rows


class _Graph:
    """A captured graph plus the collectives it issues per launch (for the signature) and the
    row-band weight-image state it was captured under: a body captured with current images
    skips their rebuild, so before it replays on stale images they are rebuilt eagerly.
    (It holds the images and the stream, not the engine: engine -> _graphs -> graph -> engine
    would be a cycle, freed by the garbage collector in arbitrary order at teardown -- a graph
    holding RCCL kernels then outlives its communicator, and the teardown of the two hung a
    2-rank RCCL job.)"""

    def __init__(self, runner, sync, notes, images, stream, rb_pre: bool, rb_post: bool):
        self.runner, self.sync, self.notes = runner, sync, notes
        self.images, self.stream = images, stream
        self.rb_pre, self.rb_post = rb_pre, rb_post

    def launch(self, stream_handle: int):
        im = self.images
        if im.views is not None and self.rb_pre and not im.current():
            with torch.cuda.stream(self.stream):
                im.pack()
        self.runner.launch(stream_handle)
        self.sync.replay(self.notes)
        im.mark(self.rb_post)


class _SilentSync:
    """Stand-in for the gradient sync while a micro-batch's gradient is produced."""

    def ready(self, layer: int):
        pass
