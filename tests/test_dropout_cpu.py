"""--dropout on the CPU: the numpy Philox4x32-10 against known answers, the kept share, and one
TorchOps engine step against float64 autograd with the reference mask multiplied in."""
import copy

import pytest
import torch

import nnmpi_amd  # noqa: F401
from nnmpi_amd.engine.arena import Arena
from nnmpi_amd.engine.engine import MLPEngine
from nnmpi_amd.models.mlp import MLP, MLPSpec, reference_init
from nnmpi_amd.ops.torch_ops import (TorchOps, dropout_consts, dropout_keep, dropout_state,
                                     philox4x32_10)
from nnmpi_amd.parallel.sync import NoSync
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args, validate

SEED, WIDTHS = 1234, (5, 13, 12, 1)


@pytest.mark.parametrize("ctr,key,want", [
    ([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, want):
    """Random123's known-answer vectors for philox4x32-10 (zeros, ones, digits of pi)."""
    assert " ".join(f"{int(w):08x}" for w in philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_share(p):
    """64 x 512, seed 1234: |kept / n - (1 - p)| < 5 sqrt(p (1 - p) / n)."""
    keep = dropout_keep(dropout_state(SEED, 3, "cpu"), p, 1, 2, 64, 512)
    assert abs(float(keep.sum()) / 32768 - (1 - p)) < 5 * (p * (1 - p) / 32768) ** 0.5


def make_engine(widths, act, norm, p, ops=None, dtype=torch.float32, rows=9, **kw):
    """(arena, engine with a loaded batch, the initial model, X, Y) on the device of ``ops``."""
    ops = ops or TorchOps("cpu")
    spec = MLPSpec(tuple(widths), act, "mse", norm, p)
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], ops.device,
               shadow_dtype=dtype if dtype == torch.bfloat16 else None)
    model = reference_init(widths, act, seed=1, norm=norm, dropout=p)
    init = copy.deepcopy(model)
    ar.bind_model(model)
    eng = MLPEngine(spec, ar, ops, NoSync(ar), device=ops.device, dtype=dtype, rows_capacity=rows,
                    lr=0.05, momentum=0.9, dropout_seed=SEED, **kw)
    g = torch.Generator().manual_seed(3)
    X, Y = torch.randn(rows, widths[0], generator=g).to(dtype), torch.randn(rows, 1, generator=g)
    eng.load_batch(X.to(ops.device), Y.to(ops.device))
    eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
    return ar, eng, init, X, Y


def reference_step(init, X, Y, act, norm, p, step=0, rank=0):
    """(loss, parameters after the first SGD step) of the float64 model, reference masks."""
    lins = [copy.deepcopy(m).double() for m in init.linears()]
    h = X.double()
    for i, lin in enumerate(lins[:-1]):
        z = lin(h)
        if norm == "layer":
            z = torch.nn.functional.layer_norm(z, z.shape[1:], eps=1e-5)
        a = torch.relu(z) if act == "relu" else torch.tanh(z)
        keep = dropout_keep(dropout_state(SEED, step, "cpu"), p, i, rank, *a.shape)
        h = a * keep * float(dropout_consts(p)[1])
    loss = torch.nn.functional.mse_loss(lins[-1](h), Y.double())
    params = [q for lin in lins for q in lin.parameters()]
    grads = torch.autograd.grad(loss, params)
    return float(loss.detach()), torch.cat(
        [(q - 0.05 * g).detach().reshape(-1) for q, g in zip(params, grads)])


@pytest.mark.parametrize("norm", ["none", "layer"])
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_cpu_engine_step_vs_float64_autograd(act, norm):
    """p = 0.5, fp32 TorchOps: loss and parameters after one step to rtol = atol = 1e-5 (the
    bound of test_norm_cpu.py's fp32-against-float64 comparison); the second pass draws
    another mask, the one of pass 1."""
    ar, eng, init, X, Y = make_engine(WIDTHS, act, norm, 0.5)
    eng.step()
    want_loss, want = reference_step(init, X, Y, act, norm, 0.5)
    assert eng.loss() == pytest.approx(want_loss, rel=1e-5, abs=1e-5)
    torch.testing.assert_close(ar.flat_params_forward_order().double(), want, rtol=1e-5, atol=1e-5)
    assert eng.dropout_step == 1
    if act == "tanh":       # (tanh is never exactly 0: the zeros of drop[] are the mask)
        first = eng.drop[0] != 0
        eng.step()
        keep = [dropout_keep(dropout_state(SEED, k, "cpu"), 0.5, 0, 0, 9, WIDTHS[1]) for k in (0, 1)]
        assert torch.equal(first, keep[0]) and torch.equal(eng.drop[0] != 0, keep[1])
        assert not torch.equal(keep[0], keep[1])


def test_evaluate_ignores_dropout_and_the_option_surface():
    """evaluate() == the p = 0 engine with the same weights, bitwise, no pass counted; CLI, keys."""
    _, eng, _, X, Y = make_engine(WIDTHS, "relu", "none", 0.5)
    _, plain, _, _, _ = make_engine(WIDTHS, "relu", "none", 0.0, use_tiny=False)
    assert eng.evaluate(X, Y) == plain.evaluate(X, Y) and eng.dropout_step == 0
    assert config_from_args(build_parser().parse_args(["--dropout", "0.25"])).dropout == 0.25
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            validate(TrainConfig(dropout=bad))
    plain, dropped = MLP([8, 16, 16, 1]), MLP([8, 16, 16, 1], norm="layer", dropout=0.5)
    assert list(dropped.state_dict()) == list(plain.state_dict()) and dropped.spec.dropout == 0.5
