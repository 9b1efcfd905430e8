"""Adam / AdamW on the CPU path: the plain-torch update against the float64 oracle, training
through dist_train at one and two ranks, ZeRO-1, checkpoint / resume (the step number included)
and the flag combinations the configuration rejects."""
import pytest
import torch

import nnmpi_amd  # noqa: F401
from nnmpi_amd.engine import trainer
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args

from _adam_oracle import CASES, GS, LR, B1, B2, EPS, TOL, fill, inputs, max_err, oracle
from _mp import run_ranks


def _arena(shadow=True):
    from nnmpi_amd.engine.arena import Arena
    return Arena([(64, 200), (1, 64)], "cpu", shadow_dtype=torch.bfloat16 if shadow else None)


@pytest.mark.parametrize("t,wd,name", CASES)
def test_torch_ops_adam_matches_float64_oracle(t, wd, name):
    """TorchOps.adam (fp32, the kernel's operation order) after TorchOps.adam_tick against
    torch.optim.Adam / AdamW in float64: master, exp_avg, exp_avg_sq within rtol = atol = 1e-6;
    the shadow is the bf16 of the master and the gradient is zeroed.  (Measured here:
    max |err| / (1 + |ref|) = 8.2e-8 over the eight cases; torch.optim in fp32 gives 8.2e-8.)"""
    from nnmpi_amd.engine.optimizer import adam_hparams
    from nnmpi_amd.ops.torch_ops import TorchOps
    ar = _arena()
    p, g, m, v = inputs(ar.numel, t)
    fill(ar, p, g, m, v)
    want = oracle(p, g, m, v, t, name, wd)
    hp = adam_hparams(LR, B1, B2, EPS, wd, "cpu", grad_scale=GS)
    tt = torch.tensor([t - 1], dtype=torch.int32)
    ops = TorchOps()
    ops.adam_tick(hp, tt)
    assert int(tt) == t
    assert hp[6].item() == pytest.approx(1 - B1 ** t, rel=1e-7)
    assert hp[7].item() == pytest.approx(1 - B2 ** t, rel=1e-7)
    ops.adam(ar, hp, tt, name == "adamw")
    got = (ar.master, ar.momentum, ar.exp_avg_sq)
    ref32 = oracle(p, g, m, v, t, name, wd, dtype=torch.float32)
    print("ADAM_ERR torch_ops", t, wd, name, max_err(got, want), "torch fp32", max_err(ref32, want))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b.float(), **TOL)
    assert torch.equal(ar.shadow, ar.master.to(torch.bfloat16))
    assert torch.count_nonzero(ar.grad) == 0


def test_torch_ops_adam_ranges_and_bf16_gradient():
    """Two ranges == one pass, bit for bit; the bf16-gradient form leaves the fp32 gradient alone
    and equals the fp32 form fed the same values; zero_grad=False keeps the gradient."""
    from nnmpi_amd.engine.optimizer import adam_hparams
    from nnmpi_amd.ops.torch_ops import TorchOps
    ops = TorchOps()
    hp = adam_hparams(LR, B1, B2, EPS, 1e-2, "cpu", grad_scale=GS, step=7)
    tt = torch.tensor([7], dtype=torch.int32)
    a, b, c, d = _arena(), _arena(), _arena(), _arena()
    p, g, m, v = inputs(a.numel, 7)
    g16 = g.to(torch.bfloat16)
    for ar in (a, b):
        fill(ar, p, g, m, v)
    ops.adam(a, hp, tt, True)
    h = (b.numel // 2) // 4 * 4
    ops.adam(b, hp, tt, True, offset=0, numel=h, zero_grad=False)
    assert torch.equal(b.grad, g)
    ops.adam(b, hp, tt, True, offset=h, numel=b.numel - h, zero_grad=False)
    for x, y in ((a.master, b.master), (a.momentum, b.momentum), (a.exp_avg_sq, b.exp_avg_sq),
                 (a.shadow, b.shadow)):
        assert torch.equal(x, y)
    fill(c, p, g, m, v)
    ops.adam(c, hp, tt, False, grad_bf16=g16)
    assert torch.equal(c.grad, g)
    fill(d, p, g16.float(), m, v)
    ops.adam(d, hp, tt, False)
    assert torch.equal(c.master, d.master) and torch.equal(c.exp_avg_sq, d.exp_avg_sq)


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_dist_train_adam_loss_decreases(name):
    """The reference config under Adam / AdamW, one rank and two (gloo / shared memory): the loss
    goes down on every rank and the replicas stay equal."""
    cfg = TrainConfig(device="cpu", print_rank="none", nepochs=8, optimizer=name, lr=0.01,
                      weight_decay=0.01)
    one = trainer.run_worker(cfg)
    assert one.schedule["optimizer"] == name and one.steps == 8
    assert one.losses[-1] < one.losses[0]
    two = run_ranks(cfg, 2)
    for r in two:
        assert r["losses"][-1] < r["losses"][0]
    assert torch.equal(two[0]["final"], two[1]["final"])


def test_adam_differs_from_adamw_and_sgd():
    """The three optimizers are three different updates (a flag that selected nothing would pass
    the loss test above)."""
    out = [trainer.run_worker(TrainConfig(device="cpu", print_rank="none", nepochs=3, lr=0.01,
                                          weight_decay=0.1, optimizer=o)).final_params
           for o in ("sgd", "adam", "adamw")]
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])


def test_engine_step_matches_torch_optim_adamw():
    """A TorchOps engine (fp32, 2-3-1, 16 rows) under AdamW for 4 steps against autograd +
    torch.optim.AdamW on the same model and data: the whole step wiring (tick once per step,
    bias corrections from the device counter), not just the element formula."""
    from nnmpi_amd.data import synth
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.torch_ops import TorchOps
    from nnmpi_amd.parallel.sync import NoSync
    widths, rows = [2, 3, 1], 16
    spec = MLPSpec(tuple(widths), "relu", "mse")
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], "cpu")
    ar.bind_model(reference_init(widths, "relu", seed=0))
    eng = MLPEngine(spec, ar, TorchOps(), NoSync(ar), device="cpu", dtype=torch.float32,
                    rows_capacity=rows, lr=0.01, momentum=0.9, weight_decay=0.01,
                    optimizer="adamw", use_tiny=False)
    X, Y = synth.chunked_regression(0, rows, 2, device="cpu")
    model = reference_init(widths, "relu", seed=0)
    opt = torch.optim.AdamW(model.parameters(), lr=0.01, weight_decay=0.01)
    eng.load_batch(X, Y)
    eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
    for _ in range(4):
        eng.step()
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(X), Y).backward()
        opt.step()
    assert int(eng.opt.t) == 4 and eng.steps_done == 4
    want = torch.cat([q.detach().reshape(-1) for q in model.parameters()])
    torch.testing.assert_close(ar.flat_params_forward_order(), want, rtol=1e-5, atol=1e-6)


def test_adam_sharded_optimizer_matches_allreduce_bitwise(world=2):
    """ZeRO-1 under AdamW: the owner slices' exp_avg / exp_avg_sq give exactly the all-reduce
    path's parameters (uneven data split, padded arena).  Two ranks: a two-term fp32 sum has one
    order; at three the gloo ring and the shared-memory transport sum in different orders, and
    Adam -- unlike SGD at a small learning rate -- turns a last-bit gradient difference into a
    visible parameter difference (the GPU test compares P = 3 under the ordered reduction)."""
    cfg = dict(print_rank="none", nepochs=4, n_samples=17, optimizer="adamw", lr=0.01,
               weight_decay=0.01)
    a = run_ranks(TrainConfig(device="cpu", shard_optimizer=True, **cfg), world)
    b = run_ranks(TrainConfig(device="cpu", **cfg), world)
    for x, y in zip(a, b):
        assert x["losses"] == y["losses"]
        assert torch.equal(x["final"], y["final"])


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_adam_checkpoint_resume_is_exact(tmp_path, name):
    """Checkpoint after epoch 1, resume in a fresh job: bitwise the uninterrupted run -- exp_avg,
    exp_avg_sq AND the step number come back (a restart at t = 0 changes the bias corrections
    of every later step)."""
    ck = str(tmp_path / "adam.pt")
    kw = dict(device="cpu", print_rank="none", optimizer=name, lr=0.01, weight_decay=0.01)
    full = trainer.run_worker(TrainConfig(nepochs=4, **kw))
    trainer.run_worker(TrainConfig(nepochs=1, checkpoint=ck, **kw))
    st = torch.load(ck + ".train", weights_only=True)
    assert st["optimizer"] == name and st["steps"] == 1
    assert set(st["exp_avg_sq_by_name"]) == set(st["momentum_by_name"])
    assert st["exp_avg_sq_by_name"]["layers.0.weight"].shape == (3, 2)      # unpadded views
    assert all(float(v.min()) >= 0 for v in st["exp_avg_sq_by_name"].values())
    res = trainer.run_worker(TrainConfig(nepochs=4, resume=ck, **kw))
    assert res.steps == 4
    assert torch.equal(res.final_params, full.final_params)


def test_adam_sharded_checkpoint_holds_both_states(tmp_path):
    """A ZeRO-1 AdamW run at P = 2 checkpoints the re-assembled exp_avg and exp_avg_sq: resumed,
    it ends bitwise where the uninterrupted run does."""
    ck = str(tmp_path / "z.pt")
    cfg = dict(device="cpu", print_rank="none", shard_optimizer=True, n_samples=32,
               optimizer="adamw", lr=0.01)
    full = run_ranks(TrainConfig(nepochs=4, **cfg), 2)
    run_ranks(TrainConfig(nepochs=2, checkpoint=ck, **cfg), 2)
    res = run_ranks(TrainConfig(nepochs=4, resume=ck, **cfg), 2)
    assert torch.equal(res[0]["final"], full[0]["final"])


def test_resume_with_another_optimizer_raises(tmp_path):
    sgd, adamw = str(tmp_path / "sgd.pt"), str(tmp_path / "adamw.pt")
    base = dict(device="cpu", print_rank="none")
    trainer.run_worker(TrainConfig(nepochs=1, checkpoint=sgd, **base))
    trainer.run_worker(TrainConfig(nepochs=1, checkpoint=adamw, optimizer="adamw", **base))
    assert "optimizer" in torch.load(sgd + ".train", weights_only=True)
    with pytest.raises(ValueError, match="optimizer"):
        trainer.run_worker(TrainConfig(nepochs=2, resume=sgd, optimizer="adamw", **base))
    with pytest.raises(ValueError, match="optimizer"):
        trainer.run_worker(TrainConfig(nepochs=2, resume=adamw, **base))
    with pytest.raises(ValueError, match="optimizer"):
        trainer.run_worker(TrainConfig(nepochs=2, resume=adamw, optimizer="adam", **base))
    # a .train file from before the field existed is SGD state
    st = torch.load(sgd + ".train", weights_only=True)
    del st["optimizer"]
    torch.save(st, sgd + ".train")
    trainer.run_worker(TrainConfig(nepochs=2, resume=sgd, **base))
    with pytest.raises(ValueError, match="optimizer"):
        trainer.run_worker(TrainConfig(nepochs=2, resume=sgd, optimizer="adam", **base))


@pytest.mark.parametrize("argv", [["--optimizer", "adam", "--beta1", "1.0"],
                                  ["--optimizer", "adam", "--beta1", "-0.1"],
                                  ["--optimizer", "adamw", "--beta2", "1.0"],
                                  ["--optimizer", "adamw", "--beta2=-1e-3"],
                                  ["--optimizer", "adam", "--eps", "0"],
                                  ["--optimizer", "adamw", "--eps=-1e-8"],
                                  ["--optimizer", "adam", "--nesterov"],
                                  ["--optimizer", "adamw", "--nesterov"],
                                  ["--optimizer", "adam", "--dampening", "0.1"],
                                  ["--optimizer", "adamw", "--dampening", "0.1"]])
def test_rejected_flag_combinations(argv):
    with pytest.raises(ValueError):
        config_from_args(build_parser().parse_args(argv))


def test_cli_flags_and_defaults():
    cfg = config_from_args(build_parser().parse_args([]))
    assert (cfg.optimizer, cfg.beta1, cfg.beta2, cfg.eps) == ("sgd", 0.9, 0.999, 1e-8)
    # --momentum keeps its default of 0.9 under Adam: ignored, not rejected
    cfg = config_from_args(build_parser().parse_args(
        ["--optimizer", "adamw", "--beta1", "0.8", "--beta2", "0.99", "--eps", "1e-6",
         "--weight_decay", "0.05"]))
    assert (cfg.optimizer, cfg.beta1, cfg.beta2, cfg.eps) == ("adamw", 0.8, 0.99, 1e-6)
    assert cfg.momentum == 0.9 and cfg.weight_decay == 0.05
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--optimizer", "lion"])
    from nnmpi_amd.utils.config import validate
    with pytest.raises(ValueError):
        validate(TrainConfig(optimizer="lion"))
    with pytest.raises(ValueError):     # and the engine refuses a name it does not know
        trainer.run_worker(TrainConfig(device="cpu", print_rank="none", optimizer="lion"))


def test_engine_rejects_sgd_only_options_under_adam():
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec
    from nnmpi_amd.ops.torch_ops import TorchOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec((2, 3, 1), "relu", "mse")
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], "cpu")
    kw = dict(device="cpu", dtype=torch.float32, rows_capacity=4, lr=0.01, momentum=0.9)
    for bad in (dict(nesterov=True), dict(dampening=0.1)):
        with pytest.raises(ValueError):
            MLPEngine(spec, ar, TorchOps(), NoSync(ar), optimizer="adam", **kw, **bad)
    eng = MLPEngine(spec, ar, TorchOps(), NoSync(ar), optimizer="adam", **kw)
    assert not eng.fuse_sgd and not eng.tiny_fused and eng.opt.name == "adam"
    assert [b.data_ptr() for b in eng.opt.state_buffers()] == [ar.momentum.data_ptr(),
                                                               ar.exp_avg_sq.data_ptr()]
    eng.steps_done = 5      # a resume sets the device step number too
    assert int(eng.opt.t) == 5 and eng.steps_done == 5
