"""What every op set answers when the engine asks what it can do: the engine picks its schedule
from these predicates and size queries.  An op set overrides the ones whose kernels it has;
everything else keeps the "not supported" answer declared here (TorchOps keeps all of them)."""
from __future__ import annotations


def _no(*args, **kw) -> bool:
    return False


def _zero(*args, **kw) -> int:
    return 0


def yes(*args, **kw) -> bool:
    return True


class LambState:
    """What a LAMB optimizer keeps on the device besides exp_avg / exp_avg_sq (layout: the top of
    csrc/kernels/optim.hip).  One tensor per ``Arena.slots`` entry, in arena order."""

    def __init__(self, ops, arena):
        import torch
        self.names = [s.name for s in arena.slots]
        self.ranges = [(s.offset, s.numel) for s in arena.slots]
        self.T, self.chunk = len(self.ranges), int(ops.lamb_chunk)
        first, self.nchunks = ops.lamb_layout([n for _, n in self.ranges], self.chunk)
        dev = arena.master.device
        self.table = torch.tensor([[o, n, f] for (o, n), f in zip(self.ranges, first)],
                                  dtype=torch.int64, device=dev).reshape(-1)
        self.part = torch.zeros(2 * max(1, self.nchunks), dtype=torch.float64, device=dev)
        self.trust = torch.ones(self.T, dtype=torch.float32, device=dev)
        self.norms = torch.zeros(2 * self.T, dtype=torch.float32, device=dev)
        self._sums = None

    def sums(self, sets: int = 1):
        """float64 [sets][T][2]: per-tensor (sum p^2, sum u^2) of ``sets`` ranks or ranges
        (allocated on first use -- a first step runs eagerly, ahead of any capture)."""
        if self._sums is None or self._sums.shape[0] != sets:
            import torch
            self._sums = torch.zeros(sets, self.T, 2, dtype=torch.float64,
                                     device=self.table.device)
        return self._sums


class OpSet:
    # the op set has tiny_step / sgd_fusion / the weight gradients that store the bf16
    # all-reduce payload themselves (linear_wgrad(out_bf16=), linear_wgrad_defer)
    tiny_supported = can_fuse_sgd = can_write_bf16_wgrad = _no
    # per-shape predicates
    tiny_can_fuse_sgd = bwd_group_supported = wide_pair_wgrad_ok = rowband_split_ok = _no
    # workspace sizes in bytes; the row-band kernel version that runs a model (0: none)
    tiny_workspace_bytes = wgrad_workspace_bytes = head_workspace_bytes = rowband_version = _zero

    # ---- global-norm gradient clipping (csrc/kernels/optim.hip; TorchOps is the oracle) ----
    def grad_sumsq(self, arena, part, offset: int = 0, numel=None, grad_bf16=None) -> int:
        """Sum of squares of ``[offset, offset + numel)`` of the gradient (``grad_bf16``: of that
        bf16 buffer instead of ``arena.grad``) as float64 partials in ``part``; returns how many
        partials were written."""
        raise NotImplementedError(f"{type(self).__name__}: grad_sumsq is not supported")

    def sumsq_reduce(self, part, nparts: int, out):
        """``out[0]`` = the fixed-order sum of ``part[:nparts]`` (float64)."""
        raise NotImplementedError(f"{type(self).__name__}: sumsq_reduce is not supported")

    def clip_finalize(self, hp, clip_state, part, nparts: int):
        """From the summed partials: ``hp[4]`` = base scale x clip coefficient, and the norm and
        the coefficient into ``clip_state`` ([max_norm, base_gs, last_norm, last_coef])."""
        raise NotImplementedError(f"{type(self).__name__}: clip_finalize is not supported")

    # ---- LAMB (csrc/kernels/optim.hip; TorchOps is the CPU training path) ----
    lamb_chunk = 4096       # elements per chunk of the per-tensor reduction (HipOps: measured)

    def lamb_layout(self, lens, chunk: int):
        """(first chunk of every tensor, number of chunks) of tensors of ``lens`` elements."""
        first, c = [], 0
        for n in lens:
            first.append(c)
            c += (n + chunk - 1) // chunk
        return first, c

    def lamb_state(self, arena) -> "LambState":
        """The device state of a LAMB optimizer over ``arena``, allocated once (captured graphs
        keep its addresses)."""
        return LambState(self, arena)

    def lamb(self, arena, hp, t, zero_grad: bool = True, offset: int = 0, numel=None,
             grad_bf16=None, images=None, gather=None, state=None):
        """LAMB over ``[offset, offset + numel)`` (multiples of 64), the keywords of ``adam``.
        Per arena tensor: ``u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p``, ``r = |p| / |u|``
        where both norms are non-zero (else 1), ``p -= lr * r * u``; the norms cover the
        tensor's elements inside the range.  ``gather = (world, rank, allgather)`` (ZeRO-1: the
        range is this rank's slice): ``allgather(buf)`` gathers the ``world`` equal parts of the
        float64 ``buf`` in place, bitwise (part ``rank`` is this rank's); the per-rank sums are
        then added in rank order, so every rank holds the same ratios.  ``state``: the
        optimizer's :class:`LambState` (default: one kept with the arena)."""
        raise NotImplementedError(f"{type(self).__name__}: lamb is not supported")

    # ---- layer / RMS normalisation of hidden layers (csrc/kernels/norm.hip; TorchOps: CPU path) ----
    def norm_act(self, z, norm: str, act: str, out, stats, eps: float = 1e-5):
        """``out = act(x)`` with ``x`` the rows of ``z`` [rows, H] normalised without scale or
        shift: ``norm = "layer"``: ``(z - mu) * rstd``, ``rstd = 1 / sqrt(mean((z - mu)^2) + eps)``;
        ``"rms"``: the same with ``mu = 0``.  ``stats`` (fp32 [rows, 2]) receives ``(mu, rstd)``.
        ``out`` is another buffer than ``z``: :meth:`norm_bwd` reads ``z`` again."""
        raise NotImplementedError(f"{type(self).__name__}: norm_act is not supported")

    def norm_bwd(self, dn, z, stats, norm: str):
        """``dn`` (the loss gradient w.r.t. ``x``) becomes the gradient w.r.t. ``z``, in place:
        ``rstd * (dn - mean(dn) - x * mean(dn * x))`` (``"rms"``: without the ``mean(dn)`` term),
        ``x`` recomputed from the saved ``z`` and the ``stats`` of :meth:`norm_act`."""
        raise NotImplementedError(f"{type(self).__name__}: norm_bwd is not supported")

    # ---- dropout of hidden activations (csrc/kernels/dropout.hip; TorchOps: CPU path, oracle) ----
    # The mask is never stored: logical element e = r * H + c of a [rows, H] operand takes word
    # e & 3 of the Philox4x32-10 call with counter (g lo32, g hi32, pass, (rank << 8) | layer),
    # g = e >> 2, and key (seed lo32, seed hi32); it is kept iff word >= T.  ``state`` is the
    # int32[4] tensor (seed lo32, seed hi32, pass, 0) of torch_ops.dropout_state, read where the
    # op runs; (T, scale) come from torch_ops.dropout_consts(p).
    def dropout(self, a, out, state, p: float, layer: int, rank: int):
        """``out = float(a) * scale`` where kept (one fp32 multiply, rounded once to the element
        type), ``+0`` where dropped.  ``out`` is another buffer than ``a``: the backward reads the
        undropped ``a``."""
        raise NotImplementedError(f"{type(self).__name__}: dropout is not supported")

    def dropout_bwd(self, dd, a, state, p: float, act: str, layer: int, rank: int):
        """``dd`` (the loss gradient w.r.t. the dropped activations) becomes the gradient w.r.t.
        the activation's input, in place: with ``g = float(dd) * scale``, ``relu``: ``g`` where
        ``a > 0`` else 0; ``none``: ``g``; ``tanh``: ``dd * scale * (1 - a^2)`` formed in double
        and rounded once (three fp32 roundings stray up to 1.9 ulp); ``+0`` where dropped.
        ``a`` is the UNDROPPED activation :meth:`dropout` read; the mask is regenerated."""
        raise NotImplementedError(f"{type(self).__name__}: dropout_bwd is not supported")

    def dropout_tick(self, state):
        """``state[2] += 1`` where the ops run: the next pass draws another mask."""
        raise NotImplementedError(f"{type(self).__name__}: dropout_tick is not supported")

    # ---- forward-only output layer (csrc/kernels/head_eval.hip; TorchOps is the oracle) ----
    def head_eval(self, a, W, b, y=None, labels=None, loss=None, logits_out=None, pred_out=None,
                  metrics=None, accumulate: bool = False, ws=None):
        """Logits ``a @ W^T + b`` of the output layer, without any gradient.  ``loss``: ``"mse"``
        (targets ``y`` [rows, out]), ``"xent"`` (``labels`` [rows] int64, only compared with the
        output index: an out-of-range label counts as a wrong row) or None (no target is read).
        Optional outputs: ``logits_out`` (fp32, rows x >= out, row stride >= out), ``pred_out``
        (int32 [rows], ``torch.argmax``'s rule: first maximum, a NaN is the maximum) and
        ``metrics`` (float64 [4] = loss_sum, correct, abs_err_sum, rows; per-row fp32 values
        summed in float64; ``accumulate``: added to instead of overwritten; the slot the loss
        does not define is 0).  ``ws``: ``head_eval_workspace_bytes`` (with ``metrics``)."""
        raise NotImplementedError(f"{type(self).__name__}: head_eval is not supported")

    def head_eval_workspace_bytes(self, rows, in_f, out_f) -> int:
        return 0

    def rowband_ok(self, rows, widths, act, loss) -> bool:
        """The whole forward + head + activation-gradient chain runs as one launch per step
        (see rowband.hip)."""
        return self.rowband_version(rows, widths, act, loss) > 0
