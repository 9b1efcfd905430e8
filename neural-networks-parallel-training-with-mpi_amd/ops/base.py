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
