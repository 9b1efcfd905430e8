"""Shared by the LAMB tests: the formula of the issue written once in float64, tensor by tensor
over an arena's slots (padding is left alone), from the fp32 inputs of ``_adam_oracle.inputs``."""
import torch

from _adam_oracle import B1, B2, EPS, GS, LR, TOL, fill, inputs, max_err  # noqa: F401

CASES = [(t, wd) for t in (1, 7) for wd in (0.0, 1e-2)]


def oracle(slots, p, g, m, v, t, wd, gs=GS, lr=LR, dtype=torch.float64):
    """((p, m, v) after step ``t``, {slot name: (ratio, |p|, |u|)})."""
    p, g, m, v = [x.detach().cpu().to(dtype).clone() for x in (p, g, m, v)]
    ratios = {}
    for s in slots:
        sl = slice(s.offset, s.offset + s.numel)
        d = g[sl] * gs
        m[sl] = B1 * m[sl] + (1 - B1) * d
        v[sl] = B2 * v[sl] + (1 - B2) * d * d
        u = (m[sl] / (1 - B1 ** t)) / ((v[sl] / (1 - B2 ** t)).sqrt() + EPS) + wd * p[sl]
        pn, un = float(p[sl].double().norm()), float(u.double().norm())
        r = pn / un if pn > 0 and un > 0 else 1.0
        ratios[s.name] = (r, pn, un)
        p[sl] -= lr * r * u
    return (p, m, v), ratios


def check_ratios(got, want):
    """{name: (ratio, |p|, |u|)} against the oracle's within TOL."""
    assert set(got) == set(want)
    for k in want:
        torch.testing.assert_close(torch.tensor(got[k], dtype=torch.float64),
                                   torch.tensor(want[k], dtype=torch.float64), **TOL)
