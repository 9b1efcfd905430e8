"""LAMB on the MI355X: lamb_moments / lamb_trust / lamb_apply against the float64 formula, the
bf16-gradient, ranged and image-refreshing forms, and the engine (graphs, schedules, clipping)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _lamb_oracle import (B1, B2, CASES, EPS, GS, LR, TOL, check_ratios, fill, inputs,  # noqa: E402
                          max_err, oracle)
from test_adam_gpu import _data, _engine, _full_state, _load, _same, _three_steps  # noqa: E402

DEV = "cuda"


def _arena(dev=DEV):     # tensors of 1 element, 64 (< a chunk), 8,192 (two chunks), 12,800 (ragged)
    from nnmpi_amd.engine.arena import Arena
    return Arena([(64, 200), (128, 64), (1, 64)], dev, shadow_dtype=torch.bfloat16)


def _opt(ar, wd, t, ops=None):
    from nnmpi_amd.engine.optimizer import Lamb, adam_hparams
    from nnmpi_amd.ops.hip_ops import HipOps
    hp = adam_hparams(LR, B1, B2, EPS, wd, ar.master.device, grad_scale=GS, step=t)
    return Lamb(ops or HipOps(), ar, hp)


def _filled(t, wd, p, g, m, v, dev=DEV, ops=None):
    ar = _arena(dev)
    fill(ar, *[x.to(dev) for x in (p, g, m, v)])
    return ar, _opt(ar, wd, t, ops)


def _state(ar):
    return [x.clone() for x in (ar.master, ar.momentum, ar.exp_avg_sq, ar.shadow)]


@pytest.mark.parametrize("t,wd", CASES)
def test_lamb_kernels_match_float64_oracle(t, wd):
    """Master, moments, ratios and norms within rtol = atol = 1e-6 of the float64 formula; padding
    untouched, shadow == bf16(master), gradients zeroed.  Edge tensors: layer 1's bias all zero
    (ratio 1); layer 0's bias with g = m = v = 0 (wd = 0: ratio 1, bitwise unchanged).  Measured
    max |err| / (1 + |ref|): kernels 4.4e-8, TorchOps fp32 on the CPU 6.3e-8 (docs/PERF.md §6)."""
    from nnmpi_amd.ops.torch_ops import TorchOps
    lay = _arena("cpu")
    p, g, m, v = inputs(lay.numel, t)
    zero, still = lay.by_name["layers.2.bias"], lay.by_name["layers.0.bias"]
    p[zero.offset:zero.offset + zero.numel] = 0
    for x in (g, m, v):
        x[still.offset:still.offset + still.numel] = 0
    ar, opt = _filled(t, wd, p, g, m, v)
    want, ratios = oracle(ar.slots, p, g, m, v, t, wd)
    opt.apply(False)
    got = [x.cpu() for x in (ar.master, ar.momentum, ar.exp_avg_sq)]
    cpu, copt = _filled(t, wd, p, g, m, v, "cpu", TorchOps())
    copt.apply(False)
    print("LAMB_ERR kernel", t, wd, max_err(got, want), "TorchOps fp32 cpu",
          max_err((cpu.master, cpu.momentum, cpu.exp_avg_sq), want))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b.float(), **TOL)
    rr = opt.trust_ratios()
    check_ratios(rr, ratios)
    assert rr[zero.name][0] == 1.0
    if wd == 0:
        assert rr[still.name][0] == 1.0
        assert torch.equal(ar.bias(0).cpu(), p[still.offset:still.offset + still.numel])
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    assert all(torch.count_nonzero(ar.grad[s.offset:s.offset + s.numel]) == 0 for s in ar.slots)


def test_lamb_bf16_gradient_form_and_determinism():
    """The bf16 payload as the gradient == the fp32 form fed g16.float(), bit for bit, the fp32
    gradient arena untouched; two runs from the same inputs are bitwise equal."""
    t, wd = 7, 1e-2
    p, g, m, v = inputs(_arena("cpu").numel, t)
    g16 = inputs(p.numel(), t, seed=60)[1].to(torch.bfloat16)
    a, oa = _filled(t, wd, p, g, m, v)
    oa.apply(False, grad_bf16=g16.to(DEV))
    assert torch.equal(a.grad.cpu(), g), "the fp32 gradient arena must stay untouched"
    out = []
    for _ in range(2):
        b, ob = _filled(t, wd, p, g16.float(), m, v)
        ob.apply(False)
        out.append(_state(b) + [ob.state.trust.clone(), ob.state.norms.clone()])
    _same(_state(a) + [oa.state.trust, oa.state.norms], out[0])
    _same(out[0], out[1])


def test_lamb_ranges():
    """Pass 1 on [0, h) and [h, n), h mid-chunk inside the ragged tensor: the per-tensor sums
    added in that order match the one-pass sums to 1e-13 relative (exact squares, regrouped) and
    the update from them is within TOL of the one-pass one.  A bad range raises, changing nothing."""
    t, wd = 7, 1e-2
    p, g, m, v = inputs(_arena("cpu").numel, t)
    one, o1 = _filled(t, wd, p, g, m, v)
    two, o2 = _filled(t, wd, p, g, m, v)
    ops, s1, s2 = o1.ops, o1.state, o2.state
    ops.lamb_moments(one, o1.hp, s1)
    whole = torch.zeros(s1.T, 2, dtype=torch.float64, device=DEV)
    ops.lamb_trust(s1, sums_out=whole)
    ops.lamb_apply(one, o1.hp, s1)
    h = two.by_name["layers.0.weight"].offset + 4096 + 640
    halves = s2.sums(2)
    for k, (lo, n) in enumerate(((0, h), (h, two.numel - h))):
        ops.lamb_moments(two, o2.hp, s2, offset=lo, numel=n)
        ops.lamb_trust(s2, sums_out=halves[k], ratios=False)
    ops.lamb_trust(s2, gathered=halves)
    ops.lamb_apply(two, o2.hp, s2, offset=0, numel=h)
    ops.lamb_apply(two, o2.hp, s2, offset=h, numel=two.numel - h)
    torch.testing.assert_close(halves[0] + halves[1], whole, rtol=1e-13, atol=0)
    for x, y in zip(_state(two)[:3], _state(one)[:3]):
        torch.testing.assert_close(x, y, **TOL)
    before = _state(two) + [two.grad.clone()]
    for bad in (dict(numel=two.numel - 32), dict(offset=32, numel=two.numel - 32),
                dict(offset=0, numel=two.numel + 64)):
        with pytest.raises((ValueError, RuntimeError)):
            o2.apply(False, **bad)
    torch.cuda.synchronize()
    _same(before, _state(two) + [two.grad])


def test_lamb_pass_refreshes_the_weight_images():
    """512-512-512-1: after lamb(..., images=) both images of every hidden layer equal a fresh
    rowband_pack of the updated shadow, bit for bit."""
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.ops.hip_ops import HipOps
    ops, t = HipOps(), 7
    ar = Arena([(512, 512), (512, 512), (1, 512)], DEV, shadow_dtype=torch.bfloat16)
    p, g, m, v = [x.to(DEV) for x in inputs(ar.numel, t)]
    fill(ar, p * 0.05, g, m, v)
    buf, views = ops.rowband_packed(512, 512, 2, DEV)
    _opt(ar, 1e-2, t, ops).apply(False, images=dict(enumerate(views)))
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    fbuf, fresh = ops.rowband_packed(512, 512, 2, DEV)
    ops.rowband_pack([ar.compute_weight(i) for i in range(2)], fresh)
    torch.cuda.synchronize()
    assert torch.count_nonzero(fbuf) > 0 and torch.equal(buf, fbuf)


def test_lamb_engine_graphs_count_steps():
    """run_steps(6, chunk=5) -- one eager step and one graph of five -- is bitwise six eager
    steps, and the device step counter reads 6."""
    widths, rows = [64, 64, 1], 48
    X, Y = _data(rows, widths)
    out = []
    for graph in (True, False):
        ar, eng = _engine(widths, rows, optimizer="lamb", use_graph=graph)
        _load(eng, X, Y, rows)
        if graph:
            eng.run_steps(6, chunk=5)
        else:
            for _ in range(6):
                eng.step()
        out.append(_full_state(ar, eng) + [eng.opt.state.trust.clone()])
        assert int(eng.opt.t.item()) == 6 and eng.steps_done == 6 and not eng.fuse_sgd
    _same(*out)


@pytest.mark.parametrize("body", ["grouped", "overlap"])
def test_lamb_schedules_bitwise_equal_to_sequential(body):
    widths, rows = [128, 128, 128, 1], 96
    X, Y = _data(rows, widths)
    name, got, gl, eng = _three_steps(widths, rows, X, Y, optimizer="lamb", grouped=body == "grouped")
    assert name == body and not eng.fuse_sgd and not eng._defer_plan
    sname, want, wl, _ = _three_steps(widths, rows, X, Y, optimizer="lamb", overlap=False)
    assert sname == "sequential" and gl == wl
    _same(got, want)


def test_lamb_engine_clipped_step_matches_oracle():
    """One clipped step of [64, 64, 1] at 48 rows: clip_coef() < 1; master, moments and
    trust_ratios() equal the oracle fed the gradient the update saw, scaled by slot 4 (TOL)."""
    widths, rows = [64, 64, 1], 48
    X, Y = _data(rows, widths)
    ar, eng = _engine(widths, rows, optimizer="lamb", use_graph=False, overlap=False,
                      clip_grad_norm=1e-3)
    _load(eng, X, Y, rows)
    seen, apply = [], eng.opt.apply

    def spy(*a, **kw):
        eng.stream.synchronize()
        seen.append([x.clone() for x in (ar.master, ar.grad, ar.momentum, ar.exp_avg_sq)])
        return apply(*a, **kw)
    eng.opt.apply = spy
    eng.step()
    assert eng.clip_coef() < 1.0 and len(seen) == 1
    want, ratios = oracle(ar.slots, *seen[0], 1, 1e-2, gs=float(eng.hp[4]), lr=1e-3)
    for a, b in zip(_full_state(ar, eng), want):
        torch.testing.assert_close(a.cpu(), b.float(), **TOL)
    check_ratios(eng.trust_ratios(), ratios)
