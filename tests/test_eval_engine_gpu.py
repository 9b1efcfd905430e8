"""MLPEngine.predict / evaluate_metrics on the GPU: exact against a float64 oracle on integer
weights, free of side effects on the training state, reading the current weights, agreeing with
evaluate(), and the trainer's --val_metrics against the CPU run."""
import pytest
import torch

import _exact as ex

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _build(widths, loss, R, dtype, sd=None, seed=3, **kw):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec(tuple(widths), "relu", loss)
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], DEV,
               shadow_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None)
    ar.bind_model(reference_init(widths, seed=seed))
    if sd is not None:
        ar.load_state_dict(sd)
        ar.sync_shadow()
    kw.setdefault("lr", 0.05)
    kw.setdefault("momentum", 0.9)
    eng = MLPEngine(spec, ar, HipOps(DEV), NoSync(ar), device=DEV, dtype=dtype, rows_capacity=R, **kw)
    return eng, ar


def _int_state_dict(widths, seed):
    """Integer weights that keep every hidden activation an integer <= 256 (bf16-exact): full
    {-1, 0, 1} first layer on inputs in [-2, 2]; later hidden layers four nonzeros per row; the
    head (fp32 master) in [-2, 2]."""
    sd = {}
    L = len(widths) - 1
    for i in range(L):
        o, k = widths[i + 1], widths[i]
        hi = 2 if i == L - 1 else 1
        W = ex.ints((o, k), -hi, hi, seed + 10 * i, dtype=torch.float32)
        if 0 < i < L - 1:
            keep = (torch.arange(k).view(1, k) % 8) == (torch.arange(o).view(o, 1) % 8)
            W = W * keep
        sd[f"layers.{2 * i}.weight"] = W
        sd[f"layers.{2 * i}.bias"] = ex.ints(o, -2, 2, seed + 10 * i + 1, dtype=torch.float32)
    return sd


def _oracle(sd, X, L):
    """float64 forward; asserts every layer meets the 2^24 precondition and every hidden
    activation is exactly representable in bf16."""
    h = ex.d(X)
    for i in range(L):
        W, b = sd[f"layers.{2 * i}.weight"], sd[f"layers.{2 * i}.bias"]
        ex.assert_exact_ok(h, W.t(), b)
        z = ex.preact(h, W, b)
        if i == L - 1:
            return z
        h = torch.relu(z)
        assert torch.equal(ex.bf16_rne(h).double(), h), "hidden activations are not bf16-exact"


@pytest.mark.parametrize("widths,loss", [([16, 32, 32, 10], "xent"), ([16, 32, 1], "mse")])
def test_predict_exact_bf16(widths, loss):
    sd = _int_state_dict(widths, 5)
    eng, _ = _build(widths, loss, 64, torch.bfloat16, sd=sd)
    assert not eng.use_tiny
    X = ex.ints((150, widths[0]), -2, 2, 9)                    # n = 150 with R = 64: three chunks
    z = _oracle(sd, X, len(widths) - 1)
    got = eng.predict(X.to(DEV))
    assert ex.same(got, ex.f32(z))
    cls = eng.predict(X.to(DEV), classes=True)
    assert cls.dtype == torch.int64 and torch.equal(cls.cpu(), torch.argmax(z, 1))
    assert eng.predict(X[:0].to(DEV)).shape == (0, widths[-1])
    # metrics on the same exact outputs
    if loss == "mse":
        y64 = z + ex.ints((150, widths[-1]), -3, 3, 11, dtype=torch.float64)
        m = eng.evaluate_metrics(X.to(DEV), Y=ex.f32(y64).to(DEV))
        d = z - y64
        assert m == {"loss_sum": float((d * d).sum()), "rows": 150, "correct": 0,
                     "abs_err_sum": float(d.abs().sum())}
    else:
        labels = torch.argmax(z, 1)
        labels[::3] = 0
        m = eng.evaluate_metrics(X.to(DEV), labels=labels.to(DEV))
        assert m["rows"] == 150 and m["correct"] == int((torch.argmax(z, 1) == labels).sum())
        want = float((torch.logsumexp(z, 1) - z.gather(1, labels.view(-1, 1)).squeeze(1)).sum())
        assert m["loss_sum"] == pytest.approx(want, rel=1e-5) and m["abs_err_sum"] == 0.0


def test_predict_exact_tiny_fp32():
    """The reference 2-3-1 model: the engine is on the tiny path; predict takes the sequential
    fp32 forward and the scalar form of the head (in = 3)."""
    widths = [2, 3, 1]
    sd = {"layers.0.weight": ex.ints((3, 2), -3, 3, 1, dtype=torch.float32),
          "layers.0.bias": ex.ints(3, -3, 3, 2, dtype=torch.float32),
          "layers.2.weight": ex.ints((1, 3), -3, 3, 3, dtype=torch.float32),
          "layers.2.bias": ex.ints(1, -3, 3, 4, dtype=torch.float32)}
    eng, _ = _build(widths, "mse", 16, torch.float32, sd=sd)
    assert eng.use_tiny
    X = ex.ints((37, 2), -9, 9, 5, dtype=torch.float32)
    z = ex.preact(torch.relu(ex.preact(X, sd["layers.0.weight"], sd["layers.0.bias"])),
                  sd["layers.2.weight"], sd["layers.2.bias"])
    assert ex.same(eng.predict(X.to(DEV)), ex.f32(z))
    y64 = z + ex.ints((37, 1), -3, 3, 6, dtype=torch.float64)
    m = eng.evaluate_metrics(X.to(DEV), Y=ex.f32(y64).to(DEV))
    assert m == {"loss_sum": float(((z - y64) ** 2).sum()), "rows": 37, "correct": 0,
                 "abs_err_sum": float((z - y64).abs().sum())}


def _state(eng, ar):
    t = [ar.master, ar.momentum, ar.grad, eng.dlogits, eng.loss_out, eng.hp]
    if ar.shadow is not None:
        t.append(ar.shadow)
    if ar.exp_avg_sq is not None:
        t.append(ar.exp_avg_sq)
    if eng.opt.clipping:
        t.append(eng.opt.clip_state)
    eng.synchronize()
    return [x.clone() for x in t]


@pytest.mark.parametrize("opt", [dict(), dict(optimizer="adam", clip_grad_norm=1.0, lr=0.01)])
def test_no_side_effects_and_next_step_bitwise(opt):
    """predict / evaluate_metrics after a step leave every training buffer bitwise alone, and
    (the batch reloaded) the next step -- a graph replay -- is bitwise the second step of an
    engine that never evaluated."""
    widths = [16, 32, 32, 10]
    g = torch.Generator().manual_seed(2)
    X = torch.randn(64, 16, generator=g).to(DEV).to(torch.bfloat16)
    L = torch.randint(0, 10, (64,), generator=g).to(DEV)
    Xv = torch.randn(100, 16, generator=g).to(DEV).to(torch.bfloat16)
    Lv = torch.randint(0, 10, (100,), generator=g).to(DEV)

    def run(evaluate):
        eng, ar = _build(widths, "xent", 64, torch.bfloat16, use_graph=True, **opt)
        eng.load_batch(X, None, L)
        eng.set_scales(1 / 64, 1 / 64, 1.0)
        eng.step()
        if evaluate:
            before, steps = _state(eng, ar), eng.steps_done
            eng.predict(Xv)
            eng.predict(Xv, classes=True)
            m = eng.evaluate_metrics(Xv, labels=Lv)
            assert m["rows"] == 100
            for a, b in zip(before, _state(eng, ar)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert eng.steps_done == steps
            eng.load_batch(X, None, L)
        eng.step()
        eng.step()
        return _state(eng, ar), eng.loss()

    (a, la), (b, lb) = run(True), run(False)
    assert la == lb
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.rowband
def test_predict_reads_current_weights_rowband():
    """512-wide row-band engine: after two steps predict equals a plain-PyTorch forward over the
    CURRENT compute weights and master head (within bf16 activation rounding) -- a predict that
    read stale weights or weight images would be off by the two updates."""
    from nnmpi_amd.data import synth
    from nnmpi_amd.ops.torch_ops import TorchOps
    widths, rows = [512, 512, 512, 1], 1024
    eng, ar = _build(widths, "mse", rows, torch.bfloat16, lr=0.01, momentum=0.9, use_graph=False)
    assert eng.uses_rowband(rows)
    X, Y = synth.chunked_regression(0, rows, 512, out=1, device=DEV)
    X = X.to(torch.bfloat16)
    w0 = ar.master.clone()
    eng.load_batch(X, Y)
    eng.set_scales(1 / rows, 1 / rows, 1.0)
    eng.step()
    eng.step()
    eng.synchronize()
    assert not torch.equal(w0, ar.master)
    got = eng.predict(X).cpu()
    t = TorchOps("cpu")
    h = X.cpu()
    for i in range(2):
        out = torch.empty(rows, 512, dtype=torch.bfloat16)
        t.linear_act(h, ar.compute_weight(i).cpu(), ar.bias(i).cpu(), "relu", out)
        h = out
    want = torch.addmm(ar.bias(2).cpu().float(), h.float(), ar.weight(2).cpu().float().t())
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)
    # and not the initial weights' outputs (the two updates move the outputs by about 100)
    eng0, _ = _build(widths, "mse", rows, torch.bfloat16, use_graph=False)
    assert float((eng0.predict(X).cpu() - want).abs().max()) > 10.0


@pytest.mark.parametrize("widths,loss", [([16, 32, 32, 10], "xent"), ([16, 32, 1], "mse"),
                                         ([24, 40, 37], "xent")])
def test_evaluate_metrics_vs_evaluate(widths, loss):
    eng, _ = _build(widths, loss, 64, torch.bfloat16)
    g = torch.Generator().manual_seed(8)
    n = 150
    X = torch.randn(n, widths[0], generator=g).to(DEV).to(torch.bfloat16)
    Y = torch.randn(n, widths[-1], generator=g).to(DEV) if loss == "mse" else None
    L = None if loss == "mse" else torch.randint(0, widths[-1], (n,), generator=g).to(DEV)
    tot, rows = eng.evaluate(X, Y, L)
    m = eng.evaluate_metrics(X, Y, L)
    assert rows == m["rows"] == n
    assert m["loss_sum"] == pytest.approx(tot, rel=1e-5)
    if loss == "xent":
        assert m["correct"] == int((eng.predict(X, classes=True) == L).sum())
    else:
        assert m["abs_err_sum"] == pytest.approx(float((eng.predict(X) - Y).abs().sum()), rel=1e-5)
    # the same call again: the same bits
    assert eng.evaluate_metrics(X, Y, L) == m


def test_trainer_val_metrics_gpu_matches_cpu(monkeypatch):
    """The mnist preset's shape scaled down, trained on the GPU and on the CPU.  The synthetic
    classification rows come from the generator of the device they are made on, so both runs are
    given the CPU generator's rows (moved to the device): the same data, as the comparison needs."""
    from nnmpi_amd.data import synth
    from nnmpi_amd.engine import trainer
    from nnmpi_amd.utils.config import TrainConfig
    orig = synth.chunked_classification

    def cpu_rows(row_start, n_rows, n_features, n_classes, seed=7, noise=1.0, device="cpu",
                 dtype=torch.float32):
        X, lab = orig(row_start, n_rows, n_features, n_classes, seed=seed, noise=noise,
                      device="cpu", dtype=dtype)
        return X.to(device), lab.to(device)
    monkeypatch.setattr(synth, "chunked_classification", cpu_rows)
    kw = dict(print_rank="none", widths=[16, 32, 10], n_features=16, loss="xent", n_samples=256,
              nepochs=3, lr=0.05, val_fraction=0.25, val_metrics=True)
    a = trainer.run_worker(TrainConfig(device="cuda", **kw))
    b = trainer.run_worker(TrainConfig(device="cpu", **kw))
    val_rows = 64
    print("val_accs gpu", a.val_accs, "cpu", b.val_accs)
    print("val_losses gpu", a.val_losses, "cpu", b.val_losses)
    assert len(a.val_accs) == 3 and len(b.val_accs) == 3
    for x, y in zip(a.val_accs, b.val_accs):
        assert abs(x - y) <= 1.0 / val_rows
    assert a.val_losses == pytest.approx(b.val_losses, rel=1e-5)
