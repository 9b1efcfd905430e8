"""Adam / AdamW on the MI355X: adam_kernel and adam_tick against the float64 oracle
(torch.optim.Adam / AdamW in float64 on the CPU), the ranged / bf16-gradient / image-refreshing
forms bit for bit, and the engine: the device step counter inside replayed graphs, every step
schedule of one rank, gradient accumulation."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _adam_oracle import B1, B2, CASES, EPS, GS, LR, TOL, fill, inputs, max_err, oracle  # noqa: E402

DEV = "cuda"


def _arena():
    from nnmpi_amd.engine.arena import Arena
    # (the SGD kernel tests' shape: padding gaps, a length that ends a grid-stride loop mid-grid)
    return Arena([(64, 200), (1, 64)], DEV, shadow_dtype=torch.bfloat16)


def _hp(wd, step=0):
    from nnmpi_amd.engine.optimizer import adam_hparams
    return adam_hparams(LR, B1, B2, EPS, wd, DEV, grad_scale=GS, step=step)


def _t(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _state(ar):
    return [x.clone() for x in (ar.master, ar.momentum, ar.exp_avg_sq, ar.shadow)]


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"tensor {k} differs"


# ---------------------------------------------------------------- 1. kernel vs float64 oracle
@pytest.mark.parametrize("t,wd,name", CASES)
def test_adam_kernel_matches_float64_oracle(t, wd, name):
    """adam_tick (from t - 1) + adam_kernel against torch.optim.Adam / AdamW in float64 from the
    same fp32 inputs, gradient scale 0.5: master, exp_avg, exp_avg_sq within rtol = atol = 1e-6
    (the bound of test_sgd_matches_torch_optim); shadow == bf16(master) exactly; gradient zeroed.
    Measured max |err| / (1 + |ref|): the kernel 8.2e-8, torch.optim in fp32 on the CPU against
    the same oracle 8.2e-8 (docs/PERF.md §6) -- 1e-6 holds with a decade to spare, so the
    4x-of-torch fallback bound is not needed."""
    from nnmpi_amd.ops.hip_ops import HipOps
    ar = _arena()
    p, g, m, v = inputs(ar.numel, t)
    fill(ar, p.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV))
    want = oracle(p, g, m, v, t, name, wd)
    ops, hp, tt = HipOps(), _hp(wd), _t(t - 1)
    ops.adam_tick(hp, tt)
    assert int(tt.item()) == t
    assert hp[6].item() == pytest.approx(1 - B1 ** t, rel=1e-7)
    assert hp[7].item() == pytest.approx(1 - B2 ** t, rel=1e-7)
    ops.adam(ar, hp, tt, name == "adamw")
    got = [x.cpu() for x in (ar.master, ar.momentum, ar.exp_avg_sq)]
    ref32 = oracle(p, g, m, v, t, name, wd, dtype=torch.float32)
    print("ADAM_ERR kernel", t, wd, name, max_err(got, want), "torch fp32", max_err(ref32, want))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b.float(), **TOL)
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    assert torch.count_nonzero(ar.grad) == 0


# ---------------------------------------------------------------- 2. bf16-gradient form
@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_adam_bf16_gradient_form(name):
    """The bf16 all-reduce payload as the gradient: the oracle fed the bf16 values in fp32; the
    fp32 gradient arena bit for bit untouched; bitwise the fp32-gradient kernel fed g16.float()."""
    from nnmpi_amd.ops.hip_ops import HipOps
    t, wd = 7, 1e-2
    ar, ar2 = _arena(), _arena()
    p, g, m, v = inputs(ar.numel, t)
    g16 = inputs(ar.numel, t, seed=60)[1].to(torch.bfloat16)
    fill(ar, p.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV))
    want = oracle(p, g16.float(), m, v, t, name, wd)
    ops, hp, tt = HipOps(), _hp(wd, step=t), _t(t)
    ops.adam(ar, hp, tt, name == "adamw", grad_bf16=g16.to(DEV))
    for a, b in zip((ar.master, ar.momentum, ar.exp_avg_sq), want):
        torch.testing.assert_close(a.cpu(), b.float(), **TOL)
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    assert torch.equal(ar.grad.cpu(), g), "the fp32 gradient arena must stay untouched"
    fill(ar2, p.to(DEV), g16.float().to(DEV), m.to(DEV), v.to(DEV))
    ops.adam(ar2, hp, tt, name == "adamw")
    _same(_state(ar), _state(ar2))


# ---------------------------------------------------------------- 3. ranges
def test_adam_ranges_zero_grad_and_bad_length():
    """[0, h) + [h, numel) == one pass, bit for bit (fp32 and bf16 gradient); zero_grad=False
    leaves the gradient; a length or offset that is no multiple of 4 raises."""
    from nnmpi_amd.ops.hip_ops import HipOps
    t, wd = 7, 1e-2
    ops, hp, tt = HipOps(), _hp(wd, step=t), _t(t)
    p, g, m, v = [x.to(DEV) for x in inputs(_arena().numel, t)]
    g16 = g.to(torch.bfloat16)
    for kw in ({}, {"grad_bf16": g16}):
        one, two = _arena(), _arena()
        fill(one, p, g, m, v)
        fill(two, p, g, m, v)
        ops.adam(one, hp, tt, True, **kw)
        h = (two.numel // 2) // 4 * 4
        ops.adam(two, hp, tt, True, offset=0, numel=h, **kw)
        ops.adam(two, hp, tt, True, offset=h, numel=two.numel - h, **kw)
        _same(_state(one), _state(two))
        assert torch.equal(one.grad, two.grad)
    keep = _arena()
    fill(keep, p, g, m, v)
    ops.adam(keep, hp, tt, False, zero_grad=False)
    assert torch.equal(keep.grad, g)
    before = _state(keep)
    for bad in (dict(numel=keep.numel - 2), dict(offset=2, numel=keep.numel - 2),
                dict(offset=0, numel=keep.numel + 4)):
        with pytest.raises((ValueError, RuntimeError)):
            ops.adam(keep, hp, tt, False, **bad)
    with pytest.raises(RuntimeError):    # the host entry point's own check
        ops.lib.adam_update(keep.master.data_ptr(), keep.grad.data_ptr(), keep.momentum.data_ptr(),
                            keep.exp_avg_sq.data_ptr(), keep.shadow.data_ptr(), keep.numel - 2,
                            hp.data_ptr(), 0, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(before, _state(keep))


# ---------------------------------------------------------------- 4. row-band weight images
@pytest.mark.parametrize("split_pass", [False, True])
def test_adam_pass_refreshes_the_weight_images(split_pass):
    """512-512-512-1 (the v2 shape rowband_packed takes): after an Adam pass with ``images=`` both
    images of every hidden layer equal a fresh rowband_pack of the updated shadow, bit for bit.
    ``split_pass``: two ranged launches, the second beginning inside a weight matrix."""
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.ops.hip_ops import HipOps
    widths, t = [512, 512, 512, 1], 7
    ops = HipOps()
    ar = Arena([(widths[i + 1], widths[i]) for i in range(3)], DEV, shadow_dtype=torch.bfloat16)
    p, g, m, v = [x.to(DEV) for x in inputs(ar.numel, t)]
    fill(ar, p * 0.05, g, m, v)
    buf, views = ops.rowband_packed(512, 512, 2, DEV)
    images = dict(enumerate(views))
    hp, tt = _hp(1e-2, step=t), _t(t)
    if split_pass:
        # mid-row of layer 1, the layer that has both a forward and a dgrad image
        h = ar.by_name["layers.2.weight"].offset + 37 * 512 + 128
        ops.adam(ar, hp, tt, True, offset=0, numel=h, images=images)
        ops.adam(ar, hp, tt, True, offset=h, numel=ar.numel - h, images=images)
    else:
        ops.adam(ar, hp, tt, True, images=images)
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    fbuf, fresh = ops.rowband_packed(512, 512, 2, DEV)
    ops.rowband_pack([ar.compute_weight(i) for i in range(2)], fresh)
    torch.cuda.synchronize()
    assert torch.count_nonzero(fbuf) > 0
    for l, ((pf, pd), (qf, qd)) in enumerate(zip(views, fresh)):
        assert torch.equal(pf, qf), f"forward image of layer {l}"
        if pd is not None:
            assert torch.equal(pd, qd), f"dgrad image of layer {l}"


# ---------------------------------------------------------------- engines
def _engine(widths, rows, *, dtype=torch.bfloat16, dev=DEV, ops=None, optimizer="adamw", lr=1e-3,
            seed=3, cap=None, **kw):
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
                    optimizer=optimizer, **kw)
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
    out = [x.clone() for x in (ar.master, ar.momentum, ar.exp_avg_sq)]
    return out + ([ar.shadow.clone()] if ar.shadow is not None else [])


# ---------------------------------------------------------------- 5. step counter in graphs
def test_adam_step_counter_inside_replayed_graphs():
    """The trap: Adam's step number cannot be a host value baked into a captured launch.
    run_steps(6, chunk=5) -- one eager step + ONE graph of five steps -- ends bitwise where six
    eager step() calls do and the device t reads 6; replaying the same graph once more gives
    t = 11 and the state of eleven eager steps."""
    widths, rows = [64, 64, 1], 48
    X, Y = _data(rows, widths)
    ar, eng = _engine(widths, rows)
    assert eng.use_graph and not eng.fuse_sgd
    _load(eng, X, Y, rows)
    eng.run_steps(6, chunk=5)
    got6 = _full_state(ar, eng)
    assert int(eng.opt.t.item()) == 6 and eng.steps_done == 6
    n_graphs = len(eng._graphs)
    eng.run_steps(5, chunk=5)
    got11 = _full_state(ar, eng)
    assert len(eng._graphs) == n_graphs == 1, "the second run must replay the captured graph"
    assert int(eng.opt.t.item()) == 11 and eng.steps_done == 11
    ar2, ref = _engine(widths, rows, use_graph=False)
    _load(ref, X, Y, rows)
    for _ in range(6):
        ref.step()
    want6 = _full_state(ar2, ref)
    for _ in range(5):
        ref.step()
    want11 = _full_state(ar2, ref)
    assert int(ref.opt.t.item()) == 11
    _same(got6, want6)
    _same(got11, want11)
    assert not torch.equal(want6[0], want11[0])


# ---------------------------------------------------------------- 6. schedules
def _three_steps(widths, rows, X, Y, **kw):
    ar, eng = _engine(widths, rows, use_graph=False, **kw)
    _load(eng, X, Y, rows)
    name = eng.schedule_name()
    losses = []
    for _ in range(3):
        eng.step()
        losses.append(eng.loss())
    assert int(eng.opt.t.item()) == 3
    return name, _full_state(ar, eng), losses, eng


@pytest.mark.parametrize("body", ["grouped", "overlap"])
def test_adamw_schedules_bitwise_equal_to_sequential(body):
    """AdamW under the grouped and the overlapped body, three steps, against overlap=False (the
    sequential body): bitwise-equal master, exp_avg, exp_avg_sq, shadow and losses.  128-wide at
    96 rows: the narrowest hidden width bwd_group_supported takes (it refuses 64)."""
    from nnmpi_amd.ops.hip_ops import HipOps
    widths, rows = [128, 128, 128, 1], 96
    ops = HipOps(DEV)
    assert not ops.bwd_group_supported(rows, 64, 64) and ops.bwd_group_supported(rows, 128, 128)
    X, Y = _data(rows, widths)
    name, got, gl, eng = _three_steps(widths, rows, X, Y, grouped=body == "grouped")
    assert name == body and not eng.fuse_sgd and not eng._defer_plan
    sname, want, wl, _ = _three_steps(widths, rows, X, Y, overlap=False)
    assert sname == "sequential"
    _same(got, want)
    assert gl == wl


@pytest.mark.rowband
@pytest.mark.parametrize("rows,split", [(8191, False), (64, True)])
def test_adamw_rowband_bodies(rows, split, monkeypatch):
    """AdamW under the row-band body (band kernel at 8,191 rows, column-split kernel at 64; 512-
    512-512-1, the row counts test_rowband_gpu.py uses for this model).  The row-band launches
    sum the gradient in another order than the sequential kernels (test_rowband_gpu.py: "close,
    not bitwise"), so a bitwise comparison against overlap=False cannot hold for any optimizer;
    what is bitwise is the optimizer side, checked against the same row-band gradient launch
    driven by hand -- tick, gradient, one whole-arena Adam pass that zeroes the gradient and
    knows nothing of the images, images rebuilt by the next step: master, exp_avg, exp_avg_sq,
    shadow and losses equal bit for bit after three steps, the engine's images equal a fresh
    pack, t = 3.  Against the sequential body the losses agree to 2e-3 relative (the bound of
    test_rowband_engine_is_taken_and_trains_like_grouped)."""
    monkeypatch.setenv("NNMPI_ROWBAND_MIN_ROWS", "6144")     # (the production threshold)
    widths = [512, 512, 512, 1]
    X, Y = _data(rows, widths)
    name, got, gl, eng = _three_steps(widths, rows, X, Y)
    assert name == "rowband" and eng.uses_rowband_split(rows) == split and not eng.fuse_sgd
    assert eng.images.current()
    eng.check_device_errors()
    ops = eng.ops
    fbuf, fresh = ops.rowband_packed(512, 512, 2, DEV)
    ops.rowband_pack([eng.arena.compute_weight(i) for i in range(2)], fresh)
    torch.cuda.synchronize()
    assert torch.equal(eng._rb_buf, fbuf), "images differ from a fresh pack of the new weights"
    # the same gradient launches, the optimizer applied by hand
    ar2, ref = _engine(widths, rows, use_graph=False)
    _load(ref, X, Y, rows)
    rl = []
    for _ in range(3):
        with torch.cuda.stream(ref.stream):
            ref.opt.tick()
            ref._rb_launch(sgd=None)
            ref.opt.apply(False)
            ref.images.mark(False)
        rl.append(ref.loss())
    _same(got, _full_state(ar2, ref))
    assert gl == rl
    monkeypatch.setenv("NNMPI_ROWBAND", "0")
    sname, _, sl, _ = _three_steps(widths, rows, X, Y, overlap=False)
    assert sname == "sequential"
    for a, b in zip(gl, sl):
        assert a == pytest.approx(b, rel=2e-3)


def test_adamw_tiny_fp32_matches_torch_ops_engine():
    """fp32 2-3-1 at 16 rows (the one-launch tiny step; its fused SGD form is off under Adam)
    against a TorchOps engine on the CPU, three steps: parameters and both states within the
    kernel test's rtol = atol = 1e-6."""
    from nnmpi_amd.ops.torch_ops import TorchOps
    widths, rows = [2, 3, 1], 16
    X, Y = _data(rows, widths, torch.float32)
    out = []
    for dev, ops in ((DEV, None), ("cpu", TorchOps("cpu"))):
        ar, eng = _engine(widths, rows, dtype=torch.float32, dev=dev, ops=ops, use_graph=False,
                          **({} if dev == DEV else {"use_tiny": False}))
        assert not eng.tiny_fused and (eng.use_tiny or dev == "cpu")
        _load(eng, X, Y, rows)
        for _ in range(3):
            eng.step()
        out.append([x.cpu() for x in _full_state(ar, eng)])
        assert int(eng.opt.t.item()) == 3
    for a, b in zip(*out):
        torch.testing.assert_close(a, b, **TOL)
    assert torch.count_nonzero(out[0][2]) > 0


# ---------------------------------------------------------------- 7. gradient accumulation
def test_adam_grad_accum_ticks_once_per_optimizer_step():
    """K = 2 micro-batches per optimizer step: t counts optimizer steps, not micro-batches; an
    empty batch still ticks (the rank stays in step with its peers)."""
    widths, rows = [64, 64, 1], 48
    X, Y = _data(rows, widths)
    ar, eng = _engine(widths, rows, cap=24, use_graph=False)
    for _ in range(3):
        eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
        for lo in (0, 24):
            eng.load_batch(X[lo:lo + 24], Y[lo:lo + 24])
            eng.accumulate()
        eng.apply_accumulated()
    eng.synchronize()
    assert int(eng.opt.t.item()) == 3 and eng.steps_done == 3
    assert torch.count_nonzero(ar.exp_avg_sq) > 0 and torch.count_nonzero(ar.momentum) > 0
    # the same three steps on whole batches: same t, same bias corrections
    ar2, ref = _engine(widths, rows, use_graph=False)
    _load(ref, X, Y, rows)
    for _ in range(3):
        ref.step()
    ref.synchronize()
    assert torch.equal(eng.hp[6:8], ref.hp[6:8])
    eng.load_batch(X[:0], Y[:0])
    eng.step()
    eng.synchronize()
    assert int(eng.opt.t.item()) == 4 and eng.steps_done == 4
