"""Forward-only evaluation on the CPU: TorchOps.head_eval against the float64 oracle,
MLPEngine.predict / evaluate_metrics, Predictor, and the trainer's --val_metrics."""
import json

import pytest
import torch

import _exact as ex
from _mp import run_ranks

import nnmpi_amd  # noqa: F401
from nnmpi_amd import Predictor
from nnmpi_amd.engine import trainer
from nnmpi_amd.engine.arena import Arena
from nnmpi_amd.engine.engine import MLPEngine
from nnmpi_amd.models.mlp import MLP, MLPSpec, reference_init
from nnmpi_amd.ops.torch_ops import TorchOps
from nnmpi_amd.parallel.sync import NoSync
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args, validate


def _engine(widths, loss, R, seed=0, sd=None):
    spec = MLPSpec(tuple(widths), "relu", loss)
    arena = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], "cpu")
    arena.bind_model(reference_init(widths, seed=seed))
    if sd is not None:
        arena.load_state_dict(sd)
    return MLPEngine(spec, arena, TorchOps("cpu"), NoSync(arena), device="cpu",
                     dtype=torch.float32, rows_capacity=R, lr=0.1, momentum=0.9), arena


def _xent_oracle(z, labels):
    out = z.shape[1]
    ok = (labels >= 0) & (labels < out)
    zl = z.gather(1, labels.clamp(0, out - 1).view(-1, 1)).squeeze(1)
    return torch.logsumexp(z, 1) - torch.where(ok, zl, torch.zeros_like(zl))


# ---------------- TorchOps.head_eval ----------------------------------------------------------
@pytest.mark.parametrize("rows,in_f,out", [(1, 3, 1), (17, 7, 10), (33, 24, 37)])
def test_torch_head_eval_exact(rows, in_f, out):
    a = ex.ints((rows, in_f), -3, 3, 1, dtype=torch.float32)
    W = ex.ints((out, in_f), -2, 2, 2, dtype=torch.float32)
    b = ex.ints(out, -5, 5, 3, dtype=torch.float32)
    ex.assert_exact_ok(a, W.t(), b)
    z = ex.preact(a, W, b)
    ops = TorchOps("cpu")
    logits = torch.full((rows, out + 3), 9.0)
    pred = torch.full((rows,), -7, dtype=torch.int32)
    m = torch.full((4,), float("nan"), dtype=torch.float64)
    y64 = z + ex.ints((rows, out), -3, 3, 4, dtype=torch.float64)
    ops.head_eval(a, W, b, ex.f32(y64), None, "mse", logits_out=logits, pred_out=pred, metrics=m)
    assert torch.equal(logits[:, :out].double(), z) and bool((logits[:, out:] == 9.0).all())
    assert torch.equal(pred.long(), torch.argmax(z, 1))
    d = z - y64
    assert m.tolist() == [float((d * d).sum()), 0.0, float(d.abs().sum()), float(rows)]
    labels = torch.argmax(z, 1)
    labels[::2] = 0
    ops.head_eval(a, W, b, None, labels, "xent", metrics=m, accumulate=True)
    want = _xent_oracle(z, labels)
    assert m[1].item() == float((torch.argmax(z, 1) == labels).sum()) and m[3].item() == 2 * rows
    assert m[0].item() - float((d * d).sum()) == pytest.approx(float(want.sum()), rel=1e-6)
    ops.head_eval(a[:0], W, b, None, labels[:0], "xent", metrics=m)
    assert m.tolist() == [0.0, 0.0, 0.0, 0.0]
    ops.head_eval(a, W, b, metrics=m)          # no loss: counts only
    assert m.tolist() == [0.0, 0.0, 0.0, float(rows)]


def test_torch_head_eval_ties_nan_labels():
    ops = TorchOps("cpu")
    W, zero = torch.eye(4), torch.zeros(4)
    a = torch.tensor([[1.0, 0.0, 3.0, 0.0], [2.0, 5.0, 5.0, 1.0], [0.0, 0.0, 0.0, 7.0]])
    pred = torch.zeros(3, dtype=torch.int32)
    ops.head_eval(a, W, zero, pred_out=pred)
    assert pred.tolist() == [2, 1, 3]                    # [2, 5, 5, 1]: the first maximum
    # a NaN bias on outputs 1 and 3: row 0's logits are [1, nan, 3, nan] -- the first NaN wins
    nb = torch.tensor([0.0, float("nan"), 0.0, float("nan")])
    ops.head_eval(a, W, nb, pred_out=pred)
    assert pred.tolist() == [1, 1, 1]
    assert torch.argmax(torch.tensor([1.0, float("nan"), 3.0, float("nan")])).item() == 1
    # out-of-range labels: wrong rows, the label's logit counts as 0
    m = torch.zeros(4, dtype=torch.float64)
    labels = torch.tensor([-1, 4, 3])
    ops.head_eval(a, W, zero, None, labels, "xent", metrics=m)
    assert m[1].item() == 1.0
    assert m[0].item() == pytest.approx(float(_xent_oracle(a.double(), labels).sum()), rel=1e-6)
    # a NaN activation: loss NaN, prediction torch.argmax's, the other rows' logits untouched
    an = a.clone()
    an[1, 2] = float("nan")
    logits = torch.zeros(3, 4)
    ops.head_eval(an, W, zero, None, labels, "xent", logits_out=logits, pred_out=pred, metrics=m)
    assert m[0].isnan().item() and pred.tolist() == torch.argmax(an @ W.t(), 1).tolist()
    assert torch.equal(logits[0], a[0]) and torch.equal(logits[2], a[2])
    with pytest.raises(ValueError):
        ops.head_eval(a, W, zero, None, None, "xent", metrics=m)
    from nnmpi_amd.ops.base import OpSet
    with pytest.raises(NotImplementedError):
        OpSet().head_eval(a, W, zero)


# ---------------- engine ----------------------------------------------------------------------
@pytest.mark.parametrize("widths,loss", [([2, 3, 1], "mse"), ([8, 16, 4], "xent"), ([5, 2], "mse")])
def test_predict_matches_module(widths, loss):
    eng, arena = _engine(widths, loss, R=7)
    m = MLP(widths)
    m.load_state_dict(arena.state_dict())
    X = torch.randn(19, widths[0], generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = m(X)
    torch.testing.assert_close(eng.predict(X), want)
    assert torch.equal(eng.predict(X, classes=True), torch.argmax(eng.predict(X), 1))
    assert eng.predict(X, classes=True).dtype == torch.int64
    e0 = eng.predict(X[:0])
    assert e0.shape == (0, widths[-1]) and e0.dtype == torch.float32
    assert eng.predict(X[:0], classes=True).shape == (0,)


@pytest.mark.parametrize("loss", ["mse", "xent"])
def test_evaluate_metrics_matches_evaluate(loss):
    widths = [8, 16, 4]
    eng, _ = _engine(widths, loss, R=16)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(40, 8, generator=g)
    Y = torch.randn(40, 4, generator=g) if loss == "mse" else None
    L = None if loss == "mse" else torch.randint(0, 4, (40,), generator=g)
    tot, n = eng.evaluate(X, Y, L)
    m = eng.evaluate_metrics(X, Y, L)
    assert m["rows"] == n == 40 and m["loss_sum"] == pytest.approx(tot, rel=1e-6)
    if loss == "xent":
        assert m["correct"] == int((eng.predict(X, classes=True) == L).sum()) and m["abs_err_sum"] == 0.0
    else:
        assert m["abs_err_sum"] == pytest.approx(float((eng.predict(X) - Y).abs().sum()), rel=1e-6)
        assert m["correct"] == 0
    assert eng.evaluate_metrics(X[:0], None if Y is None else Y[:0], None if L is None else L[:0]) == {
        "loss_sum": 0.0, "rows": 0, "correct": 0, "abs_err_sum": 0.0}


def test_chunking_is_exact_on_integer_data():
    """n = 2.5 R equals one chunk with a larger R: integer weights and inputs, exact sums."""
    widths = [8, 16, 4]
    sd = {"layers.0.weight": ex.ints((16, 8), -2, 2, 1, dtype=torch.float32),
          "layers.0.bias": ex.ints(16, -3, 3, 2, dtype=torch.float32),
          "layers.2.weight": ex.ints((4, 16), -2, 2, 3, dtype=torch.float32),
          "layers.2.bias": ex.ints(4, -3, 3, 4, dtype=torch.float32)}
    X = ex.ints((50, 8), -3, 3, 5, dtype=torch.float32)
    Y = ex.ints((50, 4), -9, 9, 6, dtype=torch.float32)
    small, _ = _engine(widths, "mse", R=20, sd=sd)
    big, _ = _engine(widths, "mse", R=64, sd=sd)
    assert torch.equal(small.predict(X), big.predict(X))
    assert small.evaluate_metrics(X, Y) == big.evaluate_metrics(X, Y)


def test_side_effects_cpu():
    eng, arena = _engine([8, 16, 4], "xent", R=16)
    g = torch.Generator().manual_seed(7)
    X, L = torch.randn(16, 8, generator=g), torch.randint(0, 4, (16,), generator=g)
    eng.load_batch(X, None, L)
    eng.set_scales(1 / 16, 1 / 16, 1.0)
    eng.step()
    keep = [t.clone() for t in (arena.master, arena.momentum, arena.grad, eng.dlogits, eng.loss_out)]
    steps = eng.steps_done
    eng.predict(X[:5])
    eng.evaluate_metrics(X, None, L)
    for a, b in zip(keep, (arena.master, arena.momentum, arena.grad, eng.dlogits, eng.loss_out)):
        assert torch.equal(a, b)
    assert eng.steps_done == steps


# ---------------- Predictor -------------------------------------------------------------------
def test_predictor_from_checkpoint(tmp_path):
    ck = str(tmp_path / "m.pt")
    trainer.run_worker(TrainConfig(device="cpu", print_rank="none", nepochs=2, checkpoint=ck))
    p = Predictor.from_checkpoint(ck, device="cpu")
    assert p.widths == [2, 3, 1]
    m = MLP()
    m.load_state_dict(torch.load(ck, weights_only=True))
    X = torch.randn(9, 2, generator=torch.Generator().manual_seed(1))
    y = torch.randn(9, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = m(X)
    torch.testing.assert_close(p.predict(X), want)
    r = p.evaluate(X, y)
    assert r["rows"] == 9
    assert r["loss"] == pytest.approx(float(((want.squeeze(1) - y) ** 2).mean()), rel=1e-5)
    assert r["mae"] == pytest.approx(float((want.squeeze(1) - y).abs().mean()), rel=1e-5)


def test_predictor_xent_and_bad_state_dicts(tmp_path):
    ck = str(tmp_path / "c.pt")
    cfg = TrainConfig(device="cpu", print_rank="none", widths=[8, 16, 4], n_features=8, loss="xent",
                      n_samples=64, nepochs=2, lr=0.1, checkpoint=ck)
    trainer.run_worker(cfg)
    p = Predictor.from_checkpoint(ck, loss="xent", device="cpu", batch_rows=10)
    assert p.widths == [8, 16, 4]
    sd = torch.load(ck, weights_only=True)
    m = MLP([8, 16, 4])
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(4)
    X, L = torch.randn(33, 8, generator=g), torch.randint(0, 4, (33,), generator=g)
    with torch.no_grad():
        want = m(X)
    torch.testing.assert_close(p.predict(X), want)
    assert torch.equal(p.predict(X, classes=True), torch.argmax(p.predict(X), 1))
    r = p.evaluate(X, L)
    assert r["accuracy"] == pytest.approx(int((torch.argmax(want, 1) == L).sum()) / 33, abs=1e-12)
    assert r["loss"] == pytest.approx(float(torch.nn.functional.cross_entropy(want, L)), rel=1e-5)
    q = Predictor.from_state_dict(sd, loss="xent", device="cpu")
    assert torch.equal(q.predict(X), p.predict(X))
    missing = {k: v for k, v in sd.items() if k != "layers.2.bias"}
    with pytest.raises(ValueError, match="layers.2.bias"):
        Predictor.from_state_dict(missing, loss="xent", device="cpu")
    bad = dict(sd)
    bad["layers.2.weight"] = torch.zeros(4, 15)
    with pytest.raises(ValueError, match="layers.2.weight"):
        Predictor.from_state_dict(bad, loss="xent", device="cpu")
    bad = dict(sd)
    bad["layers.0.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match="layers.0.bias"):
        Predictor.from_state_dict(bad, loss="xent", device="cpu")


# ---------------- trainer: --val_metrics ------------------------------------------------------
XENT = dict(device="cpu", print_rank="all", widths=[8, 16, 4], n_features=8, loss="xent",
            n_samples=64, nepochs=3, lr=0.1, scaling="none", val_fraction=0.25)


def _held_out_accuracy(res, cfg):
    """Accuracy of the final model on the held-out tail, recomputed with torch."""
    from nnmpi_amd.data import synth
    X, lab = synth.chunked_classification(0, cfg.n_samples, cfg.n_features, cfg.widths[-1],
                                          seed=cfg.data_seed)
    nv = int(round(cfg.n_samples * cfg.val_fraction))
    m = MLP(cfg.widths)
    m.load_state_dict(res.state_dict)
    with torch.no_grad():
        return int((torch.argmax(m(X[-nv:]), 1) == lab[-nv:]).sum()) / nv


def test_trainer_val_metrics_xent(tmp_path, capsys):
    mj = str(tmp_path / "m.jsonl")
    cfg = TrainConfig(val_metrics=True, metrics_json=mj, **XENT)
    res = trainer.run_worker(cfg)
    out = capsys.readouterr().out
    assert len(res.val_accs) == 3 and all(0.0 <= a <= 1.0 for a in res.val_accs)
    assert res.val_maes == [] and len(res.val_losses) == 3
    assert res.val_accs[-1] == pytest.approx(_held_out_accuracy(res, cfg), abs=1e-12)
    assert out.count("validation accuracy: ") == 3 and out.count("validation loss: ") == 3
    recs = [json.loads(l) for l in open(mj)]
    assert [r["val_acc"] for r in recs] == res.val_accs and all("val_mae" not in r for r in recs)
    # the flag off: evaluate() is still the path -- no new line, no new key, and the validation
    # losses agree with the metrics path (same forward, another head)
    mj2 = str(tmp_path / "m2.jsonl")
    off = trainer.run_worker(TrainConfig(metrics_json=mj2, **XENT))
    out = capsys.readouterr().out
    assert "validation accuracy" not in out and "validation mae" not in out
    assert off.val_accs == [] and off.val_maes == []
    recs = [json.loads(l) for l in open(mj2)]
    assert all("val_acc" not in r and "val_mae" not in r for r in recs)
    assert off.val_losses == pytest.approx(res.val_losses, rel=1e-5)
    again = trainer.run_worker(TrainConfig(**XENT))
    capsys.readouterr()
    assert again.val_losses == off.val_losses               # bitwise: the default path
    assert torch.equal(again.final_params, res.final_params)   # evaluation never touches training


def test_flag_off_path_is_evaluate(monkeypatch):
    """Without the flag the trainer calls evaluate() and never evaluate_metrics()."""
    calls = []
    orig_e, orig_m = MLPEngine.evaluate, MLPEngine.evaluate_metrics
    monkeypatch.setattr(MLPEngine, "evaluate", lambda s, *a, **k: calls.append("e") or orig_e(s, *a, **k))
    monkeypatch.setattr(MLPEngine, "evaluate_metrics",
                        lambda s, *a, **k: calls.append("m") or orig_m(s, *a, **k))
    trainer.run_worker(TrainConfig(**dict(XENT, print_rank="none", nepochs=2)))
    assert calls == ["e", "e"]
    calls.clear()
    trainer.run_worker(TrainConfig(val_metrics=True, **dict(XENT, print_rank="none", nepochs=2)))
    assert calls == ["m", "m"]


def test_trainer_val_metrics_mse(tmp_path, capsys):
    mj = str(tmp_path / "m.jsonl")
    res = trainer.run_worker(TrainConfig(device="cpu", print_rank="all", val_fraction=0.25,
                                         val_metrics=True, nepochs=3, metrics_json=mj))
    out = capsys.readouterr().out
    assert len(res.val_maes) == 3 and res.val_accs == [] and out.count("validation mae: ") == 3
    recs = [json.loads(l) for l in open(mj)]
    assert [r["val_mae"] for r in recs] == res.val_maes and all("val_acc" not in r for r in recs)
    off = trainer.run_worker(TrainConfig(device="cpu", print_rank="none", val_fraction=0.25, nepochs=3))
    assert off.val_losses == pytest.approx(res.val_losses, rel=1e-5)
    # MAE of the final model on the held-out rows, recomputed as test_parallel_cpu does the loss
    import numpy as np
    from sklearn.preprocessing import StandardScaler
    from nnmpi_amd.data import synth
    X, y = synth.reference_regression()
    Xs = StandardScaler().fit_transform(X)
    Xv = torch.from_numpy(np.ascontiguousarray(Xs[-4:])).float()
    yv = torch.from_numpy(np.ascontiguousarray(y[-4:])).float().reshape(-1, 1)
    m = MLP()
    m.load_state_dict(res.state_dict)
    with torch.no_grad():
        assert res.val_maes[-1] == pytest.approx(float((m(Xv) - yv).abs().mean()), rel=1e-5)


def test_val_metrics_two_ranks_global():
    base = dict(XENT, print_rank="none", nepochs=2)
    on = run_ranks(TrainConfig(val_metrics=True, **base), 2)
    off = run_ranks(TrainConfig(**base), 2)
    assert on[0]["val"] == on[1]["val"] and len(on[0]["val"]) == 2
    assert on[0]["val"] == pytest.approx(off[0]["val"], rel=1e-5)
    assert torch.equal(on[0]["final"], off[0]["final"])


def test_val_metrics_needs_val_fraction():
    with pytest.raises(ValueError, match="val_fraction"):
        validate(TrainConfig(val_metrics=True))
    with pytest.raises(ValueError, match="val_fraction"):
        config_from_args(build_parser().parse_args(["--val_metrics"]))
    cfg = config_from_args(build_parser().parse_args(["--val_metrics", "--val_fraction", "0.25"]))
    assert cfg.val_metrics and not TrainConfig().val_metrics
