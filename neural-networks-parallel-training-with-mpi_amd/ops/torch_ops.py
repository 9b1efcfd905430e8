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
NORM_CODES = {"layer": 1, "rms": 2}     # (kernels.h Norm; "none" is no launch at all)
NORM_EPS = 1e-5                         # torch.nn.LayerNorm's default


# ---- dropout: the Philox4x32-10 mask of csrc/kernels/dropout.hip, bit for bit, in numpy ----
PHILOX_M = (0xD2511F53, 0xCD9E8D57)     # multipliers
PHILOX_W = (0x9E3779B9, 0xBB67AE85)     # Weyl key increments


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ``ctr`` four and ``key`` two arrays (or ints) of
    32-bit values -> four uint64 arrays holding the 32-bit output words."""
    import numpy as np
    u, lo32 = np.uint64, np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=u) for x in ctr]
    k = [np.asarray(x, dtype=u) for x in key]
    for _ in range(10):
        p0, p1 = u(PHILOX_M[0]) * c[0], u(PHILOX_M[1]) * c[2]      # 32 x 32 -> 64 bits: exact
        c = [(p1 >> u(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> u(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + u(PHILOX_W[0])) & lo32, (k[1] + u(PHILOX_W[1])) & lo32]
    return c


def dropout_consts(p: float):
    """(T, scale) of drop probability ``p``: an element is kept iff its mask word >= T =
    min(2^32 - 1, round(p * 2^32)); kept values are multiplied by scale = float32(1 / (1 - p)).
    Both op sets take them from here."""
    import numpy as np
    if not 0.0 < p < 1.0:
        raise ValueError(f"dropout: 0 < p < 1, got {p}")
    return min(2 ** 32 - 1, int(round(p * 2 ** 32))), float(np.float32(1.0 / (1.0 - p)))


def dropout_state(seed: int, step: int, device) -> torch.Tensor:
    """The int32[4] device state the dropout kernels read: (seed lo32, seed hi32, pass, 0)."""
    words = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, step & 0xFFFFFFFF, 0]
    return torch.tensor([w - 2 ** 32 if w >= 2 ** 31 else w for w in words], dtype=torch.int32,
                        device=device)


def dropout_keep(state, p: float, layer: int, rank: int, rows: int, H: int) -> torch.Tensor:
    """bool [rows, H]: the kept elements.  Logical element e = r * H + c takes word e & 3 of the
    call with counter (g lo32, g hi32, pass, (rank << 8) | layer), g = e >> 2, key = the seed."""
    import numpy as np
    lo, hi, step = (int(v) & 0xFFFFFFFF for v in state[:3].tolist())
    n = rows * H
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), step,
                           ((rank << 8) | layer) & 0xFFFFFFFF), (lo, hi))
    flat = np.stack(words, 1).reshape(-1)[:n]
    return torch.from_numpy(flat >= np.uint64(dropout_consts(p)[0])).reshape(rows, H)


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

    # ---- layer / RMS normalisation (the contract of OpSet.norm_act / norm_bwd in fp32 torch) ----
    def norm_act(self, z, norm: str, act: str, out, stats, eps: float = NORM_EPS):
        if norm not in NORM_CODES:
            raise ValueError(f"norm_act: norm layer | rms, got {norm!r}")
        zf = z.float()
        mu = zf.mean(1, keepdim=True) if norm == "layer" else torch.zeros_like(zf[:, :1])
        rstd = 1.0 / torch.sqrt(((zf - mu) ** 2).mean(1, keepdim=True) + eps)
        out.copy_(act_fwd((zf - mu) * rstd, act))
        stats.copy_(torch.cat([mu, rstd], 1))

    def norm_bwd(self, dn, z, stats, norm: str):
        if norm not in NORM_CODES:
            raise ValueError(f"norm_bwd: norm layer | rms, got {norm!r}")
        g, mu, rstd = dn.float(), stats[:, :1], stats[:, 1:2]
        x = (z.float() - mu) * rstd
        d = g - x * (g * x).mean(1, keepdim=True)
        if norm == "layer":
            d = d - g.mean(1, keepdim=True)
        dn.copy_(rstd * d)

    # ---- dropout (the contract of OpSet.dropout / dropout_bwd; the mask is the kernels' own) ----
    def dropout(self, a, out, state, p: float, layer: int, rank: int):
        keep = dropout_keep(state, p, layer, rank, *a.shape).to(a.device)
        scale = torch.tensor(dropout_consts(p)[1], dtype=torch.float32, device=a.device)
        out.copy_(torch.where(keep, a.float() * scale, torch.zeros((), device=a.device)))

    def dropout_bwd(self, dd, a, state, p: float, act: str, layer: int, rank: int):
        keep = dropout_keep(state, p, layer, rank, *dd.shape).to(dd.device)
        zero = torch.zeros((), device=dd.device)
        g = dd.float() * torch.tensor(dropout_consts(p)[1], dtype=torch.float32, device=dd.device)
        if act == "relu":
            g = torch.where(a.float() > 0, g, zero)
        elif act == "tanh":
            g = (dd.double() * dropout_consts(p)[1] * (1.0 - a.double() ** 2)).float()
        dd.copy_(torch.where(keep, g, zero))

    def dropout_tick(self, state):
        state[2] += 1

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

    def lamb(self, arena, hp, t, zero_grad: bool = True, offset: int = 0, numel: int = None,
             grad_bf16=None, images=None, gather=None, state=None):
        """LAMB in plain torch (see :meth:`OpSet.lamb`): the kernels' element formula in fp32,
        the per-tensor sums of squares in float64, tensor by tensor over the parts inside the
        range; padding is left alone."""
        if images:
            raise ValueError("TorchOps.lamb: the row-band weight images are a HIP path")
        st = state
        if st is None:
            st = getattr(arena, "_lamb_state", None)
            if st is None:
                st = arena._lamb_state = self.lamb_state(arena)
        n = arena.numel - offset if numel is None else numel
        if offset % 64 or n % 64 or offset < 0 or n < 0 or offset + n > arena.numel:
            raise ValueError(f"lamb: offset and numel % 64 == 0 inside the arena ({offset}, {n})")
        lr, b1, b2, wd, gs, eps, bc1, bc2, omb1, omb2 = [hp.detach()[k] for k in range(10)]
        parts = []          # (tensor, slice, u) of every tensor with elements in the range
        sums = torch.zeros(st.T, 2, dtype=torch.float64, device=hp.device)
        with torch.no_grad():
            for k, (o, ln) in enumerate(st.ranges):
                lo, hi = max(o, offset), min(o + ln, offset + n)
                if lo >= hi:
                    continue
                sl = slice(lo, hi)
                p, m, v = arena.master[sl], arena.exp_avg[sl], arena.exp_avg_sq[sl]
                d = (grad_bf16[sl].float() if grad_bf16 is not None else arena.grad[sl]) * gs
                m.mul_(b1).add_(omb1 * d)
                v.mul_(b2).add_((omb2 * d) * d)
                u = (m / bc1) / ((v / bc2).sqrt() + eps)
                if float(wd) != 0:
                    u = u + wd * p
                sums[k, 0] = (p.double() ** 2).sum()
                sums[k, 1] = (u.double() ** 2).sum()
                parts.append((k, sl, u))
            if gather is not None:
                world, rank, allgather = gather
                buf = st.sums(world)
                buf[rank].copy_(sums)
                allgather(buf)
                sums = torch.zeros_like(sums)
                for q in range(world):      # rank order, as lamb_trust_kernel adds them
                    sums = sums + buf[q]
            pn, un = sums[:, 0].sqrt(), sums[:, 1].sqrt()
            r = torch.where((pn == 0) | (un == 0), torch.ones_like(pn), pn / un)
            st.trust.copy_(r)
            st.norms.copy_(torch.stack([pn, un], 1).reshape(-1))
            for k, sl, u in parts:
                p = arena.master[sl]
                p.sub_((lr * st.trust[k]) * u)
                if arena.shadow is not None:
                    arena.shadow[sl].copy_(p)
                if zero_grad and grad_bf16 is None:
                    arena.grad[sl].zero_()
