"""The optimizer behind every update site of the engine.

The update is issued from five places -- the inline tail, the per-layer passes behind the fused
schedules, the bucket pipeline, the ZeRO-1 owner update and (SGD only) the deferred weight-gradient
epilogue.  They all hold one of these objects and call :meth:`apply`; which formula runs, which
state buffers exist and whether a step counter has to advance is decided here alone.

* :class:`Sgd` -- ``ops.sgd`` with the arguments the sites passed before this module existed.
* :class:`Adam` -- ``ops.adam`` (torch.optim.Adam, or AdamW when ``decoupled``).  It cannot ride
  in the fused epilogues (SgdFuse carries one state buffer and the SGD formula), so the engine
  takes the unfused form of every schedule under it.  Its step number lives on the device:
  :meth:`tick`, the first launch of every optimizer step, advances it and refreshes the bias
  corrections in the hyper-parameter tensor, so a replayed graph of N steps counts N steps.

Hyper-parameter tensor: slots 0 / 3 / 4 (lr, weight decay, gradient scale) mean the same under
both, so ``MLPEngine.set_hparams`` / ``set_scales`` do not care which one is active.  The Adam
layout (12 slots) is documented at the top of ``csrc/kernels/optim.hip``.
"""
from __future__ import annotations

import struct
from typing import List, Optional

import torch

SGD_HP_LEN = 8
ADAM_HP_LEN = 12
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


class Sgd:
    name = "sgd"
    fusable = True     # the kernels' fused epilogues (SgdFuse) apply this formula

    def __init__(self, ops, arena, hp, nesterov: bool = False):
        self.ops, self.arena, self.hp, self.nesterov = ops, arena, hp, bool(nesterov)

    def apply(self, first: bool, offset: int = 0, numel: Optional[int] = None,
              zero_grad: bool = True, grad_bf16=None, images=None):
        kw = {}
        if offset or numel is not None:
            kw.update(offset=offset, numel=numel)
        if not zero_grad:
            kw["zero_grad"] = False
        if grad_bf16 is not None:
            kw["grad_bf16"] = grad_bf16
        if images is not None:
            kw["images"] = images
        self.ops.sgd(self.arena, self.hp, self.nesterov, first, **kw)

    def tick(self):
        """SGD has no step number: nothing is launched."""

    def set_step(self, steps: int):
        pass

    def state_buffers(self) -> List[torch.Tensor]:
        return [self.arena.momentum]


class Adam:
    fusable = False    # no fused epilogue: always a separate pass behind the gradient

    def __init__(self, ops, arena, hp, decoupled: bool):
        if hp.numel() < ADAM_HP_LEN:
            raise ValueError(f"Adam needs the {ADAM_HP_LEN}-slot hyper-parameter tensor")
        self.ops, self.arena, self.hp, self.decoupled = ops, arena, hp, bool(decoupled)
        self.name = "adamw" if decoupled else "adam"
        arena.ensure_exp_avg_sq()
        # the optimizer step number, on the device (an int32: a float stops counting at 2^24)
        self.t = torch.zeros(1, dtype=torch.int32, device=hp.device)

    def apply(self, first: bool, offset: int = 0, numel: Optional[int] = None,
              zero_grad: bool = True, grad_bf16=None, images=None):
        # (``first`` is SGD's momentum initialisation; Adam starts from zero state)
        self.ops.adam(self.arena, self.hp, self.t, self.decoupled, zero_grad=zero_grad,
                      offset=offset, numel=numel, grad_bf16=grad_bf16, images=images)

    def tick(self):
        self.ops.adam_tick(self.hp, self.t)

    def set_step(self, steps: int):
        """Resume: the device counter continues from ``steps`` optimizer steps."""
        with torch.no_grad():
            self.t.fill_(int(steps))

    def state_buffers(self) -> List[torch.Tensor]:
        return [self.arena.momentum, self.arena.exp_avg_sq]


def make_optimizer(name: str, ops, arena, hp, nesterov: bool = False):
    if name == "sgd":
        return Sgd(ops, arena, hp, nesterov)
    if name in ("adam", "adamw"):
        return Adam(ops, arena, hp, decoupled=name == "adamw")
    raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {name!r}")
