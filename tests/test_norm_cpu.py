"""--norm on the CPU: TorchOps.norm_act / norm_bwd against float64 autograd, the CLI and the model
surface, and a 2-rank gloo run against one rank on the same rows."""
import pytest
import torch

from _mp import run_ranks

import nnmpi_amd  # noqa: F401
from nnmpi_amd.engine import trainer
from nnmpi_amd.models.mlp import MLP
from nnmpi_amd.ops.torch_ops import TorchOps
from nnmpi_amd.predictor import Predictor
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args, validate


@pytest.mark.parametrize("H", [3, 24])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_torch_ops_norm_vs_float64_autograd(norm, act, H):
    """fp32 torch against the float64 definitions, 67 rows: rtol = atol = 1e-5 (a few fp32
    roundings on values of order 1; H-term means)."""
    g = torch.Generator().manual_seed(H)
    z, dn = 1.5 * torch.randn(67, H, generator=g) + 0.3, torch.randn(67, H, generator=g)
    z64 = z.double().requires_grad_()
    mu = z64.mean(1, keepdim=True) if norm == "layer" else torch.zeros(67, 1, dtype=torch.float64)
    rstd = 1 / torch.sqrt(((z64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    n = (z64 - mu) * rstd
    (dz,) = torch.autograd.grad(n, z64, dn.double())
    a, stats, d = torch.empty(67, H), torch.empty(67, 2), dn.clone()
    ops = TorchOps()
    ops.norm_act(z, norm, act, a, stats)
    ops.norm_bwd(d, z, stats, norm)
    want_a = torch.relu(n) if act == "relu" else torch.tanh(n)
    for got, want in ((a, want_a), (stats, torch.cat([mu, rstd], 1)), (d, dz)):
        torch.testing.assert_close(got.double(), want.detach(), rtol=1e-5, atol=1e-5)


def test_cli_and_state_dict_keys():
    assert config_from_args(build_parser().parse_args(["--norm", "rms"])).norm == "rms"
    assert config_from_args(build_parser().parse_args([])).norm == "none"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--norm", "batch"])
    with pytest.raises(ValueError):
        validate(TrainConfig(norm="batch"))
    plain, normed = MLP([8, 16, 16, 1]), MLP([8, 16, 16, 1], "tanh", norm="layer")
    assert list(normed.state_dict()) == list(plain.state_dict())
    assert normed.spec.norm == "layer" and plain.spec.norm == "none"
    # the state dict cannot tell: the predictor is told, and then computes the module's forward
    X = torch.randn(5, 8, generator=torch.Generator().manual_seed(0))
    pred = Predictor.from_state_dict(normed.state_dict(), activation="tanh", norm="layer",
                                     device="cpu")
    torch.testing.assert_close(pred.predict(X), normed(X).detach(), rtol=1e-5, atol=1e-6)


def test_two_ranks_equal_one_rank_on_the_same_rows():
    """--norm rms over 2 gloo ranks == 1 rank on the concatenated rows (global scaling, weighted
    averaging), to test_parallel_cpu.py's bounds for that comparison."""
    cfg = TrainConfig(device="cpu", print_rank="none", scaling="global", averaging="weighted",
                      nepochs=6, n_samples=48, lr=0.01, widths=[2, 8, 8, 1], norm="rms")
    single = trainer.run_worker(cfg)
    assert single.losses[-1] < single.losses[0]
    for o in run_ranks(cfg, 2):
        torch.testing.assert_close(o["final"], single.final_params, rtol=1e-5, atol=2e-6)
