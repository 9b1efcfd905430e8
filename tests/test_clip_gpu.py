"""Global-norm gradient clipping on the MI355X: grad_sumsq exact on integers and within the
summation bound on Gaussians, deterministic, its launcher's refusals; clip_finalize's semantics;
and the engine: the tiny step against the TorchOps engine, every one-rank schedule bit for bit
against the sequential body, the coefficient recomputed inside replayed graphs."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = dict(rtol=1e-6, atol=1e-6)     # the project's bound (tests/_adam_oracle.py)
GRID_SPAN = 1024 * 256 * 4           # elements one pass of the capped grid covers


def _ops():
    from nnmpi_amd.ops.hip_ops import HipOps
    return HipOps(DEV)


def _part():
    return torch.full((1024,), float("nan"), dtype=torch.float64, device=DEV)


def _holder(g):
    """What grad_sumsq reads of an arena: the gradient buffer and its length."""
    return types.SimpleNamespace(grad=g, numel=g.numel())


def _total(ops, part, n):
    """The fixed-order sum of the first n partials (sumsq_reduce)."""
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.sumsq_reduce(part, n, out)
    torch.cuda.synchronize()
    return out.item()


def _ints(n, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, size=n).astype(np.int64)
    want = int((g * g).sum())
    assert int(np.abs(g).max()) <= 8 and want < 2 ** 53
    return torch.from_numpy(g).to(torch.float32).to(DEV), want


# ---------------------------------------------------------------- 1. grad_sumsq
@pytest.mark.parametrize("n,parts", [(4, 1), (1020, 1), (GRID_SPAN + 4, 1024)])
def test_grad_sumsq_exact_on_integers(n, parts):
    """Integer gradients, |g| <= 8: every square and every partial sum is an integer below 2^53,
    so the result must be the integer sum of squares exactly, fp32 and bf16 form alike.  n = 4:
    one float4; 1020: less than one block; 1,048,580: the capped grid of 1024 blocks wraps once
    plus one float4, so the stride loop runs twice for one thread only."""
    ops = _ops()
    assert int(ops.lib.CLIP_MAX_PARTS) == 1024 and int(ops.lib.sumsq_parts(n)) == parts
    g, want = _ints(n)
    for kw in ({}, {"grad_bf16": g.to(torch.bfloat16)}):
        part = _part()
        got_parts = ops.grad_sumsq(_holder(g), part, **kw)
        assert got_parts == parts
        assert _total(ops, part, parts) == float(want)
        assert float(part[:parts].cpu().sum()) == float(want)    # (integers: any order)
        assert bool(torch.isnan(part[parts:]).all()), "wrote past its partials"


def test_grad_sumsq_range_inside_a_nan_filled_buffer():
    """A range at a non-zero offset of a NaN-filled buffer: any read outside it poisons the sum."""
    ops = _ops()
    n, off = 2052, 1028
    g, want = _ints(n, seed=3)
    for dt in (torch.float32, torch.bfloat16):
        buf = torch.full((off + n + 1024,), float("nan"), dtype=dt, device=DEV)
        buf[off:off + n] = g.to(dt)
        part = _part()
        kw = {} if dt == torch.float32 else {"grad_bf16": buf}
        h = _holder(buf if dt == torch.float32 else torch.zeros(buf.numel(), device=DEV))
        k = ops.grad_sumsq(h, part, offset=off, numel=n, **kw)
        assert k == int(ops.lib.sumsq_parts(n)) == 3
        assert _total(ops, part, k) == float(want)
    # an empty range writes one zero partial
    part = _part()
    assert ops.grad_sumsq(_holder(buf.float()), part, offset=8, numel=0) == 1
    assert _total(ops, part, 1) == 0.0


@pytest.mark.parametrize("n", [1020, GRID_SPAN + 4])
def test_grad_sumsq_gaussian_within_the_summation_bound_and_deterministic(n):
    """fp32 squares are exact in double, so the only error is in the additions of non-negative
    terms: relative error <= n * 2^-53 in any order.  The reference is the exactly rounded sum
    (math.fsum) of the exact squares.  Two runs give identical partials."""
    ops = _ops()
    g = torch.randn(n, generator=torch.Generator().manual_seed(5)) * 3.0
    g64 = g.double()
    want = math.fsum((g64 * g64).tolist())
    gd = g.to(DEV)
    a, b = _part(), _part()
    k = ops.grad_sumsq(_holder(gd), a)
    ops.grad_sumsq(_holder(gd), b)
    got = _total(ops, a, k)
    rel = abs(got - want) / want
    print("SUMSQ_GAUSS n", n, "rel err", rel, "bound", n * 2.0 ** -53)
    assert rel <= n * 2.0 ** -53
    assert torch.equal(a[:k].view(torch.int64), b[:k].view(torch.int64))


def test_grad_sumsq_launcher_refusals():
    ops = _ops()
    g = torch.zeros(64, device=DEV)
    g16 = g.to(torch.bfloat16)
    part = _part()
    s = torch.cuda.current_stream().cuda_stream
    for fn, p in ((ops.lib.grad_sumsq, g.data_ptr()), (ops.lib.grad_sumsq_bf16, g16.data_ptr())):
        for args in ((p, 6, part.data_ptr()), (p, -4, part.data_ptr()), (0, 8, part.data_ptr()),
                     (p, 8, 0)):
            with pytest.raises(RuntimeError):
                fn(*args, s)
    with pytest.raises(ValueError):
        ops.grad_sumsq(_holder(g), part, offset=2, numel=8)
    with pytest.raises(ValueError):
        ops.grad_sumsq(_holder(g), part, offset=60, numel=8)
    with pytest.raises(RuntimeError):
        ops.lib.clip_finalize(0, part.data_ptr(), part.data_ptr(), 1, s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all())


# ---------------------------------------------------------------- 2. clip_finalize
@pytest.mark.parametrize("case", ["zero", "nan", "inf", "clipped", "unclipped"])
def test_clip_finalize_semantics(case):
    """300 partials (more than the block's 256 threads) summed in fixed order; norm = base *
    sqrt(total), coef = min(1, max_norm / (norm + 1e-6)) keeping NaN.  Unclipped: slot 4 is the
    base scale bit for bit.  last_norm / last_coef against the same formula in float64."""
    ops = _ops()
    base = torch.tensor(0.3, dtype=torch.float32).item()      # the fp32 value, as a double
    max_norm = 2.0
    parts = torch.arange(1, 301, dtype=torch.float64)          # total 45150, exact in any order
    if case == "zero":
        parts.zero_()
    elif case == "nan":
        parts[17] = float("nan")
    elif case == "inf":
        parts[299] = float("inf")
    elif case == "unclipped":
        parts.zero_()
        parts[0], parts[299] = 3.0, 1.0                        # norm 0.6 < max_norm
    hp = torch.tensor([0.1, 0.9, 0, 0, 7.0, 0, 0, 0], dtype=torch.float32, device=DEV)
    cs = torch.tensor([max_norm, 0.3, -1.0, -1.0], dtype=torch.float32, device=DEV)
    ops.clip_finalize(hp, cs, parts.to(DEV), 300)
    torch.cuda.synchronize()
    norm, coef, slot4 = cs[2].item(), cs[3].item(), hp[4].item()
    total = float(parts.sum())
    assert cs[0].item() == max_norm and cs[1].item() == base and hp[0].item() == pytest.approx(0.1)
    if case == "nan":
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(slot4)
        return
    if case == "inf":
        assert norm == math.inf and coef == 0.0 and slot4 == 0.0
        return
    wnorm = base * math.sqrt(total)
    wcoef = min(1.0, max_norm / (wnorm + 1e-6))
    assert norm == pytest.approx(wnorm, rel=2e-7, abs=0) and coef == pytest.approx(wcoef, rel=2e-7)
    assert slot4 == pytest.approx(base * wcoef, rel=2e-7)
    if case in ("zero", "unclipped"):
        assert coef == 1.0 and slot4 == base, "unclipped: slot 4 must be the base scale bitwise"
        assert (norm == 0.0) == (case == "zero")
    else:
        assert coef < 1.0


# ---------------------------------------------------------------- engines
def _engine(widths, rows, *, dtype=torch.bfloat16, dev=DEV, ops=None, optimizer="adamw", lr=1e-3,
            seed=3, cap=None, clip=None, **kw):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec(tuple(widths), "relu", "mse")
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev,
               shadow_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None)
    ar.bind_model(reference_init(widths, "relu", seed=seed))
    eng = MLPEngine(spec, ar, ops or HipOps(dev), NoSync(ar), device=dev, dtype=dtype,
                    rows_capacity=cap or rows, lr=lr, momentum=0.9, weight_decay=1e-2,
                    optimizer=optimizer, clip_grad_norm=clip, **kw)
    return ar, eng


def _data(rows, widths, dtype=torch.bfloat16):
    from nnmpi_amd.data import synth
    X, Y = synth.chunked_regression(0, rows, widths[0], out=1, device=DEV)
    return X.to(dtype), Y


def _load(eng, X, Y, rows):
    eng.load_batch(X.to(eng.device), Y.to(eng.device))
    eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)


def _full_state(ar, eng):
    eng.synchronize()
    out = [ar.master.clone(), ar.momentum.clone()]
    if ar.exp_avg_sq is not None:
        out.append(ar.exp_avg_sq.clone())
    return out + ([ar.shadow.clone()] if ar.shadow is not None else [])


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"tensor {k} differs"


def _half_norm(widths, rows, X, Y, **kw):
    """A max_norm that clips: half the first step's gradient norm (read from an engine whose
    max_norm is too large to clip)."""
    _, probe = _engine(widths, rows, use_graph=False, clip=1e30, **kw)
    _load(probe, X, Y, rows)
    probe.step()
    assert probe.clip_coef() == 1.0
    return 0.5 * probe.grad_norm()


# ---------------------------------------------------------------- 3. tiny step
@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
def test_clipped_tiny_fp32_matches_torch_ops_engine(optimizer):
    """fp32 2-3-1 at 16 rows (the one-launch tiny step; its fused SGD form is off under clipping)
    against a TorchOps engine on the CPU, three clipped steps: parameters, state and every
    step's norm within rtol = atol = 1e-6.  The norm over the whole arena equals the norm over
    the parameters' own gradient views: the arena's padding holds zeros."""
    from nnmpi_amd.ops.torch_ops import TorchOps
    widths, rows, max_norm = [2, 3, 1], 16, 0.05
    X, Y = _data(rows, widths, torch.float32)
    out, norms = [], []
    for dev, ops in ((DEV, None), ("cpu", TorchOps("cpu"))):
        ar, eng = _engine(widths, rows, dtype=torch.float32, dev=dev, ops=ops, use_graph=False,
                          optimizer=optimizer, clip=max_norm,
                          **({} if dev == DEV else {"use_tiny": False}))
        assert not eng.tiny_fused and (eng.use_tiny or dev == "cpu")
        views = []
        if dev == DEV:
            clip = eng.opt.clip

            def spy(*a, _clip=clip, _ar=ar, _eng=eng, **kw):
                _eng.stream.synchronize()
                sq = sum(float((_ar.grad_weight(i).double() ** 2).sum() +
                               (_ar.grad_bias(i).double() ** 2).sum()) for i in range(2))
                views.append(math.sqrt(sq))
                return _clip(*a, **kw)
            eng.opt.clip = spy
        _load(eng, X.to(dev), Y.to(dev), rows)
        ns = []
        for _ in range(3):
            eng.step()
            ns.append(eng.grad_norm())
            assert eng.clip_coef() < 1.0
        out.append([x.cpu() for x in _full_state(ar, eng)])
        norms.append(ns)
        if dev == DEV:
            assert len(views) == 3
            print("CLIP_TINY", optimizer, "norms", ns, "over the views", views)
            for a, b in zip(ns, views):
                assert a == pytest.approx(b, rel=1e-6)
    for a, b in zip(*out):
        torch.testing.assert_close(a, b, **TOL)
    torch.testing.assert_close(torch.tensor(norms[0]), torch.tensor(norms[1]), **TOL)


# ---------------------------------------------------------------- 4. schedules
def _three_steps(widths, rows, X, Y, **kw):
    ar, eng = _engine(widths, rows, use_graph=False, **kw)
    _load(eng, X, Y, rows)
    name = eng.schedule_name()
    losses, norms = [], []
    for _ in range(3):
        eng.step()
        losses.append(eng.loss())
        norms.append(eng.grad_norm())
        assert eng.clip_coef() < 1.0, "every step must be a clipped one"
    return name, _full_state(ar, eng), losses, norms, eng


@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
@pytest.mark.parametrize("body", ["grouped", "overlap"])
def test_clipped_schedules_bitwise_equal_to_sequential(body, optimizer):
    """bf16 512-512-512-1 at 256 rows under the grouped and the overlapped body, three clipped
    steps, against overlap=False (the sequential body): bitwise-equal parameters, state, shadow,
    losses and norms.  The fused-update forms are off under clipping."""
    widths, rows = [512, 512, 512, 1], 256
    X, Y = _data(rows, widths)
    clip = _half_norm(widths, rows, X, Y, optimizer=optimizer, overlap=False)
    kw = dict(optimizer=optimizer, clip=clip)
    name, got, gl, gn, eng = _three_steps(widths, rows, X, Y, grouped=body == "grouped", **kw)
    assert name == body and not eng.fuse_sgd and not eng._defer_plan
    sname, want, wl, wn, _ = _three_steps(widths, rows, X, Y, overlap=False, **kw)
    assert sname == "sequential"
    _same(got, want)
    assert gl == wl and gn == wn


@pytest.mark.rowband
@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
@pytest.mark.parametrize("rows,split", [(8191, False), (64, True)])
def test_clipped_rowband_bodies(rows, split, optimizer, monkeypatch):
    """The row-band body under clipping (band kernel at 8,191 rows, column-split kernel at 64;
    512-512-512-1): its launches sum the gradient in another order than the sequential kernels,
    so what is bitwise is the optimizer side, checked against the same gradient launch driven by
    hand -- tick, gradient, norm + finalize, one whole-arena pass that knows nothing of the
    images: state, losses and norms equal bit for bit after three steps, images current."""
    monkeypatch.setenv("NNMPI_ROWBAND_MIN_ROWS", "6144")     # (the production threshold)
    widths = [512, 512, 512, 1]
    X, Y = _data(rows, widths)
    clip = _half_norm(widths, rows, X, Y, optimizer=optimizer)
    name, got, gl, gn, eng = _three_steps(widths, rows, X, Y, optimizer=optimizer, clip=clip)
    assert name == "rowband" and eng.uses_rowband_split(rows) == split and not eng.fuse_sgd
    assert eng.images.current()
    eng.check_device_errors()
    fbuf, fresh = eng.ops.rowband_packed(512, 512, 2, DEV)
    eng.ops.rowband_pack([eng.arena.compute_weight(i) for i in range(2)], fresh)
    torch.cuda.synchronize()
    assert torch.equal(eng._rb_buf, fbuf), "images differ from a fresh pack of the new weights"
    ar2, ref = _engine(widths, rows, use_graph=False, optimizer=optimizer, clip=clip)
    _load(ref, X, Y, rows)
    rl, rn = [], []
    for k in range(3):
        with torch.cuda.stream(ref.stream):
            ref.opt.tick()
            ref._rb_launch(sgd=None)
            ref.opt.clip()
            ref.opt.apply(k == 0)
            ref.images.mark(False)
        rl.append(ref.loss())
        rn.append(ref.grad_norm())
    _same(got, _full_state(ar2, ref))
    assert gl == rl and gn == rn


def test_clipped_bf16_payload_overlap_reads_the_payload_bitwise_equal_to_inline():
    """8192-wide layers in chunk buckets, bf16 all-reduce payload written by the weight gradients
    themselves, per-bucket collectives on the comm stream (a one-rank RCCL communicator): under
    clipping every bucket update waits for the join, the norm reads the bf16 payload and one
    update of the whole arena reads it too -- bitwise equal, norms included, to the inline bf16
    path (fp32 gradient -> cast -> all-reduce -> cast back -> norm of the fp32 gradient ->
    update).  134 M elements: every thread of the capped grid runs its stride loop 128 times."""
    from nnmpi_amd.engine import trainer
    from nnmpi_amd.utils.config import TrainConfig
    base = dict(widths=[8192, 8192, 8192, 1], n_features=8192, n_samples=512, dtype="bf16",
                nepochs=3, lr=1e-4, data_gen="device", data_dist="local", scaling="none",
                print_rank="none", device="cuda", comm="native", grad_dtype="bf16",
                clip_grad_norm=1.0)
    a = trainer.run_worker(TrainConfig(comm_mode="overlap", bucket_mb=16, **base))
    b = trainer.run_worker(TrainConfig(comm_mode="inline", **base))
    assert not a.schedule["inline"] and b.schedule["inline"]
    assert a.schedule["grad_dtype"] == "bf16" and a.schedule["deferred_updates"] == 0
    print("CLIP_WIDE norms", a.grad_norms, "coefs", a.clip_coefs)
    assert len(a.clip_coefs) == 3 and all(0 < c < 1.0 for c in a.clip_coefs)
    assert a.grad_norms == b.grad_norms and a.clip_coefs == b.clip_coefs
    assert a.losses == b.losses
    assert torch.equal(a.final_params, b.final_params)


# ---------------------------------------------------------------- 5. replayed graphs
def test_clip_coefficient_recomputed_inside_replayed_graphs():
    """run_steps(6, chunk=3, losses=, clips=) -- one eager step, a graph of three steps and one of
    two -- ends bitwise where six eager steps without graphs do; the recorded per-step norms and
    coefficients equal the eager ones and are not all equal to each other: the coefficient is
    recomputed by every replayed step, not baked into the graph."""
    widths, rows = [64, 64, 1], 48
    X, Y = _data(rows, widths)
    clip = _half_norm(widths, rows, X, Y)
    ar, eng = _engine(widths, rows, clip=clip)
    assert eng.use_graph and not eng.fuse_sgd
    _load(eng, X, Y, rows)
    losses = torch.zeros(6, device=DEV)
    clips = torch.zeros(6, 2, device=DEV)
    eng.run_steps(6, chunk=3, losses=losses, clips=clips)
    got = _full_state(ar, eng)
    assert eng.steps_done == 6 and len(eng._graphs) == 2
    last = (eng.grad_norm(), eng.clip_coef())
    ar2, ref = _engine(widths, rows, clip=clip, use_graph=False)
    _load(ref, X, Y, rows)
    wl, wc = [], []
    for _ in range(6):
        ref.step()
        wl.append(ref.loss())
        wc.append([ref.grad_norm(), ref.clip_coef()])
    _same(got, _full_state(ar2, ref))
    assert losses.tolist() == wl
    assert clips.tolist() == wc and tuple(wc[-1]) == last
    norms = [c[0] for c in wc]
    print("CLIP_REPLAY norms", norms, "coefs", [c[1] for c in wc])
    assert len(set(norms)) > 1 and all(c[1] < 1.0 for c in wc)
    with pytest.raises(ValueError):
        eng.run_steps(1, clips=clips)
