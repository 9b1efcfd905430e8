"""The optimizer behind every update site of the engine.

The update is issued from five places -- the inline tail, the per-layer passes behind the fused
schedules, the bucket pipeline, the ZeRO-1 owner update and (SGD only) the deferred weight-gradient
epilogue.  They all hold one of these objects and call :meth:`apply`; which formula runs, which
state buffers exist and whether a step counter has to advance is decided here alone.  So are the
operands: the object holds the op set, the arena, the hyper-parameter tensor and the formula's
flags, and no site passes any of them -- a kernel that applies the update itself (the fused
combines, the tiny step, the deferred epilogue) gets its operand tuple from :meth:`Sgd.fusion`.

* :class:`Sgd` -- ``ops.sgd``, and ``ops.sgd_fusion`` for the kernels' fused epilogues.
* :class:`Adam` -- ``ops.adam`` (torch.optim.Adam, or AdamW when ``decoupled``).  It cannot ride
  in the fused epilogues (SgdFuse carries one state buffer and the SGD formula), so the engine
  takes the unfused form of every schedule under it.  Its step number lives on the device:
  :meth:`tick`, the first launch of every optimizer step, advances it and refreshes the bias
  corrections in the hyper-parameter tensor, so a replayed graph of N steps counts N steps.

Hyper-parameter tensor: slots 0 / 3 / 4 (lr, weight decay, gradient scale) mean the same under
both, so ``MLPEngine.set_hparams`` / ``set_scales`` do not care which one is active.  The Adam
layout (12 slots) is documented at the top of ``csrc/kernels/optim.hip``.

Global-norm gradient clipping (:class:`_Clipped`, ``clip_grad_norm=``) belongs to both: slot 4 is
rewritten on the device every step as base scale x clip coefficient, ahead of the update.
"""
from __future__ import annotations

import struct
from typing import List, Optional

import torch

SGD_HP_LEN = 8
ADAM_HP_LEN = 12
CLIP_MAX_PARTS = 1024     # float64 partials of grad_sumsq (kernels.h)
OPTIMIZERS = ("sgd", "adam", "adamw")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def sgd_hparams(lr, momentum, dampening, weight_decay, device) -> torch.Tensor:
    return torch.tensor([lr, momentum, dampening, weight_decay, 1.0, 0, 0, 0],
                        dtype=torch.float32, device=device)


def adam_hparams(lr, beta1, beta2, eps, weight_decay, device, grad_scale: float = 1.0,
                 step: int = 0) -> torch.Tensor:
    """The Adam layout: 1 - beta rounded from the doubles, the betas' fp32 remainders (adam_tick
    rebuilds the doubles from them) and the bias corrections of step ``step`` (0: not ticked)."""
    b1, b2 = float(beta1), float(beta2)
    return torch.tensor([lr, b1, b2, weight_decay, grad_scale, eps,
                         1.0 - b1 ** step, 1.0 - b2 ** step, 1.0 - b1, 1.0 - b2,
                         b1 - _f32(b1), b2 - _f32(b2)], dtype=torch.float32, device=device)


class _Clipped:
    """Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_), shared by both optimizers.

    Every update kernel multiplies the gradient by slot 4 of the hyper-parameter tensor, read
    from device memory.  :meth:`clip` -- called by every site that applies a whole-gradient
    update, right before it -- launches the norm of the reduced gradient and one tiny kernel
    that writes ``slot 4 = base scale x min(1, max_norm / (norm + 1e-6))``; no update kernel
    changes.  The coefficient needs the whole reduced gradient, so a clipping optimizer is not
    ``fusable``: the engine takes the unfused form of every schedule, as under Adam.  Clip-state
    layout (documented at the top of ``csrc/kernels/optim.hip``): ``[max_norm, base_gs,
    last_norm, last_coef]``.  Both buffers are allocated once: captured graphs keep their
    addresses.  With clipping off nothing is allocated and :meth:`clip` launches nothing."""
    clip_state = clip_part = _clip_gather = None

    def _init_clip(self, max_norm: Optional[float]):
        if max_norm is None:
            return
        max_norm = float(max_norm)
        if not max_norm > 0:      # (also NaN)
            raise ValueError(f"clip_grad_norm must be > 0, got {max_norm}")
        dev = self.hp.device
        self.fusable = False
        self.clip_state = torch.tensor([max_norm, 1.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        with torch.no_grad():
            self.clip_state[1:2].copy_(self.hp[4:5])
        self.clip_part = torch.zeros(CLIP_MAX_PARTS, dtype=torch.float64, device=dev)

    @property
    def clipping(self) -> bool:
        return self.clip_state is not None

    def clip(self, offset: int = 0, numel: Optional[int] = None, grad_bf16=None, gather=None):
        """Norm of ``[offset, offset + numel)`` of the reduced gradient (``grad_bf16``: of the
        bf16 payload the update will read) and the finalize, on the current stream.

        ``gather = (world, rank, allgather)`` (ZeRO-1 over RCCL: the range is this rank's
        slice): the rank's partials are reduced to one double, ``allgather(buf)`` gathers the
        ``world`` doubles of ``buf`` in place (entry ``rank`` is this rank's) bitwise, and the
        finalize sums them in rank order -- every rank computes the same coefficient."""
        if not self.clipping:
            return
        part = self.clip_part
        n = self.ops.grad_sumsq(self.arena, part, offset=offset, numel=numel, grad_bf16=grad_bf16)
        if gather is not None:
            world, rank, allgather = gather
            if self._clip_gather is None:     # (first step: eager, so ahead of any capture)
                self._clip_gather = torch.zeros(world, dtype=torch.float64, device=part.device)
            self.ops.sumsq_reduce(part, n, self._clip_gather[rank:rank + 1])
            allgather(self._clip_gather)
            part, n = self._clip_gather, world
        self.ops.clip_finalize(self.hp, self.clip_state, part, n)


class Sgd(_Clipped):
    name = "sgd"
    fusable = True     # the kernels' fused epilogues (SgdFuse) apply this formula

    def __init__(self, ops, arena, hp, nesterov: bool = False, clip_grad_norm=None):
        self.ops, self.arena, self.hp, self.nesterov = ops, arena, hp, bool(nesterov)
        self._init_clip(clip_grad_norm)

    def apply(self, first: bool, offset: int = 0, numel: Optional[int] = None,
              zero_grad: bool = True, grad_bf16=None, images=None):
        self.ops.sgd(self.arena, self.hp, self.nesterov, first, zero_grad=zero_grad,
                     offset=offset, numel=numel, grad_bf16=grad_bf16, images=images)

    def fusion(self, first: bool, offset: int = 0):
        """The SgdFuse operands of a kernel that applies this update itself (``offset``: to the
        arena elements from there on -- the deferred weight-gradient epilogue)."""
        return self.ops.sgd_fusion(self.arena, self.hp, self.nesterov, first, offset)

    def tick(self):
        """SGD has no step number: nothing is launched."""

    def set_step(self, steps: int):
        pass

    def state_buffers(self) -> List[torch.Tensor]:
        return [self.arena.momentum]


class Adam(_Clipped):
    fusable = False    # no fused epilogue: always a separate pass behind the gradient

    def __init__(self, ops, arena, hp, decoupled: bool, clip_grad_norm=None):
        if hp.numel() < ADAM_HP_LEN:
            raise ValueError(f"Adam needs the {ADAM_HP_LEN}-slot hyper-parameter tensor")
        self.ops, self.arena, self.hp, self.decoupled = ops, arena, hp, bool(decoupled)
        self.name = "adamw" if decoupled else "adam"
        arena.ensure_exp_avg_sq()
        # the optimizer step number, on the device (an int32: a float stops counting at 2^24)
        self.t = torch.zeros(1, dtype=torch.int32, device=hp.device)
        self._init_clip(clip_grad_norm)

    def apply(self, first: bool, offset: int = 0, numel: Optional[int] = None,
              zero_grad: bool = True, grad_bf16=None, images=None):
        # (``first`` is SGD's momentum initialisation; Adam starts from zero state)
        self.ops.adam(self.arena, self.hp, self.t, self.decoupled, zero_grad=zero_grad,
                      offset=offset, numel=numel, grad_bf16=grad_bf16, images=images)

    def fusion(self, first: bool, offset: int = 0):
        raise RuntimeError("Adam has no fused epilogue (fusable is False): nothing may ask")

    def tick(self):
        self.ops.adam_tick(self.hp, self.t)

    def set_step(self, steps: int):
        """Resume: the device counter continues from ``steps`` optimizer steps."""
        with torch.no_grad():
            self.t.fill_(int(steps))

    def state_buffers(self) -> List[torch.Tensor]:
        return [self.arena.momentum, self.arena.exp_avg_sq]


def make_optimizer(name: str, ops, arena, hp, nesterov: bool = False,
                   clip_grad_norm: Optional[float] = None):
    """``clip_grad_norm``: clip the gradient to this global L2 norm (None: off)."""
    if name == "sgd":
        return Sgd(ops, arena, hp, nesterov, clip_grad_norm)
    if name in ("adam", "adamw"):
        return Adam(ops, arena, hp, decoupled=name == "adamw", clip_grad_norm=clip_grad_norm)
    raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {name!r}")
