"""Plain-PyTorch implementation of the engine's op set.

This is (a) the CPU compute path (BASELINE config 1 runs on CPU with gloo, like the
reference's CPU-only script) and (b) the numerics oracle every HIP kernel is tested against.
It computes in fp32 (upcasting bf16 operands) and rounds results to the destination dtype,
which is exactly the contract of the HIP kernels (bf16 in, fp32 accumulate, bf16/fp32 out).

The forward uses ``torch.addmm(b, x, W.t())`` and the backward the same products autograd's
``AddmmBackward0``/``MseLossBackward0`` use, so in fp32 the CPU path
reproduces the reference's golden losses to reorder tolerance.
"""
from __future__ import annotations

import torch

from .base import OpSet

ACT_CODES = {"none": 0, "relu": 1, "tanh": 2}


def act_fwd(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "relu":
        return torch.relu(z)
    if act == "tanh":
        return torch.tanh(z)
    return z


def act_bwd_from_out(a: torch.Tensor, act: str) -> torch.Tensor:
    if act == "relu":
        return (a > 0).to(torch.float32)
    if act == "tanh":
        return 1.0 - a * a
    return torch.ones_like(a)


class TorchOps(OpSet):
    name = "torch"

    def __init__(self, device="cpu"):
        self.device = torch.device(device)

    # y = act(x @ W^T + b)
    def linear_act(self, x, W, b, act: str, out):
        z = torch.addmm(b.float(), x.float(), W.float().t())
        out.copy_(act_fwd(z, act))

    # out = (dz @ W) * act'(a_prev)
    def linear_dgrad(self, dz, W, a_prev, act: str, out):
        g = dz.float().mm(W.float())
        out.copy_(g * act_bwd_from_out(a_prev.float(), act))

    # gW = dz^T @ x ; gb = sum(dz, 0)
    def linear_wgrad(self, dz, x, gW, gb, ws=None, out_bf16=None):
        if out_bf16 is not None:
            gW, gb = out_bf16
        gW.copy_(dz.float().t().mm(x.float()))
        if gb is not None:
            gb.copy_(dz.float().sum(0))

    def head(self, a, W, b, y, labels, loss: str, inv_count: float, act_prev: str, dz_out,
             gW, gb, dlogits, loss_out, loss_scale: float, ws=None):
        """Output layer + loss fwd/bwd.  Writes gW, gb, dz_out (if not None), loss_out[0]."""
        af = a.float()
        logits = torch.addmm(b.float(), af, W.float().t())
        if loss == "mse":
            d = logits - y.float()
            total = (d * d).sum()
            dl = 2.0 * d * inv_count
        else:
            lse = torch.logsumexp(logits, dim=1, keepdim=True)
            total = (lse.squeeze(1) - logits.gather(1, labels.view(-1, 1)).squeeze(1)).sum()
            p = torch.exp(logits - lse)
            p[torch.arange(p.shape[0], device=p.device), labels] -= 1.0
            dl = p * inv_count
        if dlogits is not None:
            dlogits.copy_(dl)
        loss_out.fill_(0.0)
        loss_out.add_(total * loss_scale)
        gW.copy_(dl.t().mm(af))
        gb.copy_(dl.sum(0))
        if dz_out is not None:
            dz_out.copy_(dl.mm(W.float()) * act_bwd_from_out(af, act_prev))

    def head_eval(self, a, W, b, y=None, labels=None, loss=None, logits_out=None, pred_out=None,
                  metrics=None, accumulate: bool = False, ws=None):
        """The contract of OpSet.head_eval in plain torch (CPU path and the kernel's oracle)."""
        rows, out_f = a.shape[0], W.shape[0]
        if loss not in (None, "mse", "xent"):
            raise ValueError(f"head_eval: unknown loss {loss!r}")
        if (loss == "mse" and y is None) or (loss == "xent" and labels is None):
            raise ValueError(f"head_eval: loss {loss!r} needs its targets")
        with torch.no_grad():
            logits = torch.addmm(b.float(), a.float(), W.float().t())
            pred = (torch.argmax(logits, dim=1) if rows else
                    torch.zeros(0, dtype=torch.int64, device=logits.device))
            if logits_out is not None:
                logits_out[:rows, :out_f].copy_(logits)
            if pred_out is not None:
                pred_out[:rows].copy_(pred)
            if metrics is None:
                return
            vals = torch.zeros(4, dtype=torch.float64, device=metrics.device)
            vals[3] = rows
            if loss == "xent" and rows:
                lab = labels.view(-1)
                ok = (lab >= 0) & (lab < out_f)
                zl = logits.gather(1, lab.clamp(0, out_f - 1).view(-1, 1)).squeeze(1)
                zl = torch.where(ok, zl, torch.zeros_like(zl))
                vals[0] = (torch.logsumexp(logits, dim=1) - zl).double().sum()
                vals[1] = (pred == lab).sum()
            elif loss == "mse" and rows:
                d = logits - y.float().reshape(rows, out_f)
                vals[0] = (d * d).sum(1).double().sum()
                vals[2] = d.abs().sum(1).double().sum()
            if accumulate:
                metrics.add_(vals)
            else:
                metrics.copy_(vals)

    def gather_rows(self, src, idx, dst):
        dst[:idx.numel()].copy_(src.index_select(0, idx))

    def sgd(self, arena, hp, nesterov: bool, first: bool, zero_grad: bool = True, offset: int = 0,
            numel: int = None, grad_bf16=None, images=None):
        # (``images``: ignored -- the row-band weight images are a HIP path, there are none here)
        lr, mom, damp, wd, gs = [float(v) for v in hp.tolist()[:5]]
        n = arena.numel - offset if numel is None else numel
        sl = slice(offset, offset + n)
        p, g, buf = arena.master[sl], arena.grad[sl], arena.momentum[sl]
        if grad_bf16 is not None:
            g = grad_bf16[sl].float()
            zero_grad = False
        with torch.no_grad():
            d = g * gs
            if wd != 0:
                d = d + wd * p
            if mom != 0:
                if first:
                    buf.copy_(d)
                else:
                    buf.mul_(mom).add_(d, alpha=1.0 - damp)
                d = d + mom * buf if nesterov else buf
            p.sub_(lr * d)
            if arena.shadow is not None:
                arena.shadow[sl].copy_(p)
            if zero_grad:
                g.zero_()

    # ---- global-norm clipping: the float64 oracle of grad_sumsq / clip_finalize (optim.hip) -----
    def grad_sumsq(self, arena, part, offset: int = 0, numel: int = None, grad_bf16=None) -> int:
        n = arena.numel - offset if numel is None else numel
        g = (arena.grad if grad_bf16 is None else grad_bf16)[offset:offset + n]
        with torch.no_grad():
            g = g.double()
            part[:1].copy_((g * g).sum().reshape(1))
        return 1

    def sumsq_reduce(self, part, nparts: int, out):
        with torch.no_grad():
            out[:1].copy_(part[:nparts].sum().reshape(1))

    def clip_finalize(self, hp, clip_state, part, nparts: int):
        """The kernel's formula in Python doubles: the partials summed in index order (ZeRO-1:
        rank order), min(1, .) that keeps a NaN as torch.clamp(max=1) does, and ``hp[4]`` = the
        base scale bit for bit when the coefficient is 1."""
        total = 0.0
        for v in part[:nparts].tolist():
            total += v
        max_norm, base = [float(v) for v in clip_state[:2].tolist()]
        norm = base * (total ** 0.5 if total == total and total >= 0 else float("nan"))
        coef = max_norm / (norm + 1e-6)
        coef = coef if coef < 1.0 else (1.0 if coef >= 1.0 else coef)
        # (rounded as the kernel's (float) casts round: a double beyond fp32 becomes inf)
        out = torch.tensor([base * coef, norm, coef], dtype=torch.float64).to(torch.float32)
        with torch.no_grad():
            hp[4:5].copy_(out[0:1])
            clip_state[2:4].copy_(out[1:3])

    # ---- Adam / AdamW: hp in the Adam layout (engine/optimizer.py ADAM_*, optim.hip) ----------
    def adam_tick(self, hp, t):
        """t += 1 (int32 tensor of one element); hp[6], hp[7] = 1 - beta1^t, 1 - beta2^t, computed
        in double from the betas the host stored (slot + remainder slot) -- as adam_tick_kernel."""
        with torch.no_grad():
            t.add_(1)
            step = int(t.item())
            h = hp.tolist()
            b1, b2 = h[1] + h[10], h[2] + h[11]
            hp[6:8].copy_(torch.tensor([1.0 - b1 ** step, 1.0 - b2 ** step], dtype=torch.float32))

    def adam(self, arena, hp, t, decoupled: bool, zero_grad: bool = True, offset: int = 0,
             numel: int = None, grad_bf16=None, images=None):
        """The update of adam_kernel in plain torch: the same operations in fp32, in its order
        (``t`` is not read: the bias corrections come from ``hp``, as in the kernel)."""
        if images:
            raise ValueError("TorchOps.adam: the row-band weight images are a HIP path")
        f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=hp.device)  # noqa: E731
        h = hp.detach()
        lr, b1, b2, wd, gs, eps, bc1, bc2, omb1, omb2 = [h[k] for k in range(10)]
        n = arena.numel - offset if numel is None else numel
        sl = slice(offset, offset + n)
        p, g, m, v = arena.master[sl], arena.grad[sl], arena.exp_avg[sl], arena.exp_avg_sq[sl]
        if grad_bf16 is not None:
            g = grad_bf16[sl].float()
            zero_grad = False
        with torch.no_grad():
            d = g * gs
            if decoupled:
                p.mul_(f32(1.0) - lr * wd)
            elif float(wd) != 0:
                d = d + wd * p
            m.mul_(b1).add_(omb1 * d)
            v.mul_(b2).add_((omb2 * d) * d)
            p.sub_((lr / bc1) * (m / (v.sqrt() / bc2.sqrt() + eps)))
            if arena.shadow is not None:
                arena.shadow[sl].copy_(p)
            if zero_grad:
                g.zero_()
