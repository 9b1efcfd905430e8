"""LAMB on the CPU path: the plain-torch update against the float64 oracle, training through
dist_train, checkpoint / resume, ZeRO-1 over gloo and the flags the configuration rejects."""
import pytest
import torch

import nnmpi_amd  # noqa: F401
from nnmpi_amd.engine import trainer
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args

from _lamb_oracle import B1, B2, CASES, EPS, GS, LR, TOL, check_ratios, fill, inputs, max_err, oracle
from _mp import run_ranks

KW = dict(device="cpu", print_rank="none", lr=0.02, weight_decay=0.01)


@pytest.mark.parametrize("t,wd", CASES)
def test_torch_ops_lamb_matches_float64_oracle(t, wd):
    """TorchOps.lamb (fp32 elements, float64 norms) against the float64 formula: master, exp_avg,
    exp_avg_sq, ratios and norms within rtol = atol = 1e-6; padding untouched (the whole arena is
    compared), shadow == bf16(master), every tensor's gradient zeroed."""
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.optimizer import Lamb, adam_hparams
    from nnmpi_amd.ops.torch_ops import TorchOps
    ar = Arena([(64, 200), (128, 64), (1, 64)], "cpu", shadow_dtype=torch.bfloat16)
    p, g, m, v = inputs(ar.numel, t)
    fill(ar, p, g, m, v)
    want, ratios = oracle(ar.slots, p, g, m, v, t, wd)
    opt = Lamb(TorchOps(), ar, adam_hparams(LR, B1, B2, EPS, wd, "cpu", grad_scale=GS, step=t))
    opt.apply(False)
    got = (ar.master, ar.momentum, ar.exp_avg_sq)
    print("LAMB_ERR torch_ops", t, wd, max_err(got, want))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b.float(), **TOL)
    check_ratios(opt.trust_ratios(), ratios)
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    assert all(torch.count_nonzero(ar.grad[s.offset:s.offset + s.numel]) == 0 for s in ar.slots)


def test_dist_train_lamb_trains_and_is_its_own_update():
    """--optimizer lamb on the reference config: the loss falls, the result carries one trust
    ratio per tensor, and sgd / adam / lamb end in three different states."""
    out = {o: trainer.run_worker(TrainConfig(nepochs=8, optimizer=o, **KW))
           for o in ("sgd", "adam", "lamb")}
    lamb = out["lamb"]
    assert lamb.schedule["optimizer"] == "lamb" and lamb.steps == 8
    assert lamb.losses[-1] < lamb.losses[0]
    assert set(lamb.schedule["trust_ratios"]) == set(lamb.state_dict)
    assert all(r > 0 for r, _, _ in lamb.schedule["trust_ratios"].values())
    finals = [out[o].final_params for o in ("sgd", "adam", "lamb")]
    assert not any(torch.equal(finals[i], finals[j]) for i, j in ((0, 1), (0, 2), (1, 2)))


def test_lamb_checkpoint_resume_is_exact_and_adam_refuses_it(tmp_path):
    ck = str(tmp_path / "lamb.pt")
    full = trainer.run_worker(TrainConfig(nepochs=4, optimizer="lamb", **KW))
    trainer.run_worker(TrainConfig(nepochs=1, checkpoint=ck, optimizer="lamb", **KW))
    st = torch.load(ck + ".train", weights_only=True)
    assert st["optimizer"] == "lamb" and st["steps"] == 1
    assert set(st["exp_avg_sq_by_name"]) == set(st["momentum_by_name"])
    res = trainer.run_worker(TrainConfig(nepochs=4, resume=ck, optimizer="lamb", **KW))
    assert res.steps == 4 and torch.equal(res.final_params, full.final_params)
    with pytest.raises(ValueError, match="optimizer"):
        trainer.run_worker(TrainConfig(nepochs=2, resume=ck, optimizer="adam", **KW))


def test_lamb_sharded_optimizer_close_to_allreduce(world=2):
    """ZeRO-1 over gloo: each rank's per-tensor sums all-gathered and added in rank order -- the
    same doubles grouped differently than the replicated path's, so close (TOL), not bitwise;
    replicas equal within each run."""
    cfg = dict(nepochs=4, n_samples=17, optimizer="lamb", **KW)
    a = run_ranks(TrainConfig(shard_optimizer=True, **cfg), world)
    b = run_ranks(TrainConfig(**cfg), world)
    assert a[0]["schedule"]["sync"] == "ShardedSync"
    for out in (a, b):
        assert torch.equal(out[0]["final"], out[1]["final"])
        assert out[0]["losses"][-1] < out[0]["losses"][0]
    torch.testing.assert_close(a[0]["final"], b[0]["final"], **TOL)


def test_lamb_cli_flags():
    cfg = config_from_args(build_parser().parse_args(["--optimizer", "lamb", "--beta2", "0.99"]))
    assert (cfg.optimizer, cfg.beta2, cfg.momentum) == ("lamb", 0.99, 0.9)
    for bad in (["--nesterov"], ["--dampening", "0.1"]):
        with pytest.raises(ValueError):
            config_from_args(build_parser().parse_args(["--optimizer", "lamb"] + bad))
