"""Shared by the Adam tests: the kernel-test inputs and the float64 oracle -- torch.optim.Adam /
AdamW run in float64 on the CPU from the same fp32 inputs (the gradient scale folded into the
gradient it is given, exactly: a power of two)."""
import torch

LR, B1, B2, EPS, GS = 1e-2, 0.9, 0.999, 1e-8, 0.5
# t = 1 from zero state and t = 7 from random state x weight decay 0 / 1e-2 x adam / adamw
CASES = [(t, wd, name) for t in (1, 7) for wd in (0.0, 1e-2) for name in ("adam", "adamw")]
TOL = dict(rtol=1e-6, atol=1e-6)     # the project's own bound (test_sgd_matches_torch_optim)


def _rand(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, generator=g)


def inputs(numel: int, t: int, seed: int = 50):
    """fp32 CPU (p, g, m, v): zero state at t = 1, else random state with v built from squares."""
    p, g = _rand(numel, seed), _rand(numel, seed + 1)
    if t == 1:
        return p, g, torch.zeros(numel), torch.zeros(numel)
    return p, g, _rand(numel, seed + 2) * 0.5, (_rand(numel, seed + 3) ** 2) * 0.25


def oracle(p, g, m, v, t: int, name: str, wd: float, dtype=torch.float64):
    """(p, m, v) after step ``t`` of torch.optim.Adam / AdamW in ``dtype`` on the CPU."""
    q = torch.nn.Parameter(p.to(dtype).clone())
    cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    opt = cls([q], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    if t > 1:
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.to(dtype).clone(),
                        "exp_avg_sq": v.to(dtype).clone()}
    q.grad = g.to(dtype) * GS
    opt.step()
    st = opt.state[q]
    assert int(st["step"]) == t
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def max_err(got, want):
    """Largest |got - want| / (1 + |want|) over the three tensors: the figure the tolerance
    (rtol = atol) bounds."""
    return max(float(((a.double() - b.double()).abs() / (1.0 + b.double().abs())).max())
               for a, b in zip(got, want))


def fill(ar, p, g, m, v):
    """Load the inputs into an arena (and its bf16 shadow)."""
    ar.ensure_exp_avg_sq()
    ar.master.copy_(p)
    ar.grad.copy_(g)
    ar.momentum.copy_(m)
    ar.exp_avg_sq.copy_(v)
    if ar.shadow is not None:
        ar.shadow.copy_(ar.master)
