"""Global-norm gradient clipping (--clip_grad_norm) on the CPU path: a TorchOps engine against
autograd + torch.nn.utils.clip_grad_norm_ + torch.optim in fp32 and in float64, the unclipped
step bit for bit, gradient accumulation, ZeRO-1 over gloo, the configuration and the finalize
semantics (zero / NaN / inf gradients)."""
import copy
import json
import math

import pytest
import torch

import nnmpi_amd  # noqa: F401
from nnmpi_amd.engine import trainer
from nnmpi_amd.utils.config import TrainConfig, build_parser, config_from_args, validate

from _mp import run_ranks

TOL = dict(rtol=1e-6, atol=1e-6)     # the project's bound (tests/_adam_oracle.py)
LR, WD = 0.01, 0.01


def _engine(widths, loss, rows, optimizer="sgd", clip=None, cap=None, seed=0):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.torch_ops import TorchOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec(tuple(widths), "relu", loss)
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], "cpu")
    ar.bind_model(reference_init(widths, "relu", seed=seed))
    eng = MLPEngine(spec, ar, TorchOps(), NoSync(ar), device="cpu", dtype=torch.float32,
                    rows_capacity=cap or rows, lr=LR, momentum=0.9, weight_decay=WD,
                    optimizer=optimizer, use_tiny=False, clip_grad_norm=clip)
    return ar, eng


def _data(widths, loss, rows):
    from nnmpi_amd.data import synth
    if loss == "xent":
        X, labels = synth.chunked_classification(0, rows, widths[0], widths[-1], device="cpu")
        return X, None, labels
    X, Y = synth.chunked_regression(0, rows, widths[0], device="cpu")
    return X, Y, None


def _torch_optim(name, params):
    if name == "sgd":
        return torch.optim.SGD(params, lr=LR, momentum=0.9, weight_decay=WD)
    cls = torch.optim.AdamW if name == "adamw" else torch.optim.Adam
    return cls(params, lr=LR, weight_decay=WD)


def _torch_run(widths, loss, X, Y, labels, name, max_norm, steps, dtype):
    """Autograd + clip_grad_norm_ + torch.optim in ``dtype`` from the same fp32 inputs: the final
    flat parameters, the pre-clip norms and the coefficients of every step."""
    from nnmpi_amd.models.mlp import reference_init
    model = copy.deepcopy(reference_init(widths, "relu", seed=0)).to(dtype)
    opt = _torch_optim(name, model.parameters())
    Xd = X.to(dtype)
    norms, coefs = [], []
    for _ in range(steps):
        opt.zero_grad()
        out = model(Xd)
        if loss == "xent":
            torch.nn.functional.cross_entropy(out, labels).backward()
        else:
            torch.nn.functional.mse_loss(out, Y.to(dtype)).backward()
        n = float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm))
        norms.append(n)
        coefs.append(max_norm / (n + 1e-6))
        opt.step()
    return torch.cat([q.detach().reshape(-1) for q in model.parameters()]), norms, coefs


# (the smallest gradient norm over the three steps of either model is above 0.05: printed below)
@pytest.mark.parametrize("name", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("widths,loss,rows,max_norm", [([2, 3, 1], "mse", 16, 0.05),
                                                        ([8, 16, 16, 4], "xent", 32, 0.05)])
def test_clipped_engine_matches_torch_clip_grad_norm(widths, loss, rows, max_norm, name):
    """Three clipped steps of a TorchOps engine against clip_grad_norm_ + torch.optim on the same
    model and data, once in fp32 and once in float64 built from the same inputs, both at
    rtol = atol = 1e-6: parameters and every step's pre-clip norm.  The coefficient is below 1
    on every step (asserted), so every update is a clipped one."""
    X, Y, labels = _data(widths, loss, rows)
    ar, eng = _engine(widths, loss, rows, name, clip=max_norm)
    assert not eng.opt.fusable and not eng.fuse_sgd and not eng.tiny_fused
    eng.load_batch(X, Y, labels)
    eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
    got_n, got_c = [], []
    for _ in range(3):
        eng.step()
        got_n.append(eng.grad_norm())
        got_c.append(eng.clip_coef())
    got = ar.flat_params_forward_order()
    for dtype in (torch.float32, torch.float64):
        want, norms, coefs = _torch_run(widths, loss, X, Y, labels, name, max_norm, 3, dtype)
        print("CLIP_CPU", name, widths, dtype, "norms", norms, "engine", got_n, "coefs", coefs)
        assert all(c < 1.0 for c in coefs), coefs
        torch.testing.assert_close(got, want.float(), **TOL)
        torch.testing.assert_close(torch.tensor(got_n), torch.tensor(norms), **TOL)
        torch.testing.assert_close(torch.tensor(got_c), torch.tensor(coefs), **TOL)
    assert all(c < 1.0 for c in got_c)
    assert len(set(got_n)) == 3      # (a fresh norm every step)


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_huge_max_norm_is_bitwise_the_unclipped_run(name):
    """max_norm far above the norm: the coefficient is exactly 1, slot 4 stays the base scale
    bit for bit and the parameters equal a run without the flag, bit for bit."""
    widths, rows = [2, 3, 1], 16
    X, Y, _ = _data(widths, "mse", rows)
    out = []
    for clip in (1e30, None):
        ar, eng = _engine(widths, "mse", rows, name, clip=clip)
        eng.load_batch(X, Y)
        eng.set_scales(1.0 / rows, 1.0 / rows, 0.5)
        for _ in range(3):
            eng.step()
            if clip is not None:
                assert eng.clip_coef() == 1.0 and eng.grad_norm() > 0
                assert eng.hp[4].item() == 0.5
        out.append((ar.master.clone(), ar.momentum.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    with pytest.raises(RuntimeError):       # nothing computes a norm without the flag
        eng.grad_norm()
    with pytest.raises(RuntimeError):
        eng.clip_coef()
    assert eng.opt.clip_state is None and eng.opt.clip_part is None and eng.opt.fusable == (
        name == "sgd")


def test_grad_accumulation_clips_once_on_the_sum():
    """K = 3 micro-batches per optimizer step: ONE norm and ONE finalize per step, taken on the
    accumulated sum -- the norm and the parameters of the same steps on whole batches."""
    widths, rows, max_norm = [8, 16, 16, 4], 30, 0.05
    X, Y, labels = _data(widths, "xent", rows)
    ar, eng = _engine(widths, "xent", rows, "adamw", clip=max_norm, cap=10)
    calls = {"sumsq": 0, "fin": 0}
    for key, name in (("sumsq", "grad_sumsq"), ("fin", "clip_finalize")):
        fn = getattr(eng.ops, name)

        def counted(*a, _fn=fn, _k=key, **kw):
            calls[_k] += 1
            return _fn(*a, **kw)
        setattr(eng.ops, name, counted)
    ar2, ref = _engine(widths, "xent", rows, "adamw", clip=max_norm)
    ref.load_batch(X, None, labels)
    ref.set_scales(1.0 / rows, 1.0 / rows, 1.0)
    for s in range(3):
        eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
        for lo in (0, 10, 20):
            eng.load_batch(X[lo:lo + 10], None, labels[lo:lo + 10])
            eng.accumulate()
        eng.apply_accumulated()
        ref.step()
        assert calls == {"sumsq": s + 1, "fin": s + 1}
        assert eng.clip_coef() < 1.0
        assert eng.grad_norm() == pytest.approx(ref.grad_norm(), rel=1e-6)
    torch.testing.assert_close(ar.master, ar2.master, **TOL)


def test_zero1_over_gloo_is_bitwise_the_allreduce_path_under_clipping():
    """P = 2 on the CPU: the sharded path all-reduces the full gradient and takes the norm over
    it, so ZeRO-1 stays bitwise equal to the plain all-reduce path, clipped on every step."""
    cfg = dict(device="cpu", print_rank="none", nepochs=4, n_samples=17, optimizer="adamw",
               lr=0.01, weight_decay=0.01, clip_grad_norm=0.05)
    a = run_ranks(TrainConfig(shard_optimizer=True, **cfg), 2)
    b = run_ranks(TrainConfig(**cfg), 2)
    for x, y in zip(a, b):
        assert x["losses"] == y["losses"]
        assert torch.equal(x["final"], y["final"])
        assert x["schedule"]["grad_norms"] == y["schedule"]["grad_norms"]
        assert len(x["schedule"]["clip_coefs"]) == 4
        assert all(c < 1.0 for c in x["schedule"]["clip_coefs"]), x["schedule"]
    assert a[0]["schedule"]["grad_norms"] == a[1]["schedule"]["grad_norms"]
    assert torch.equal(a[0]["final"], a[1]["final"])
    # and the flag does something: the unclipped run ends elsewhere
    c = run_ranks(TrainConfig(**dict(cfg, clip_grad_norm=None)), 2)
    assert not torch.equal(c[0]["final"], b[0]["final"])
    assert "grad_norms" not in c[0]["schedule"]


@pytest.mark.parametrize("argv", [["--clip_grad_norm", "0"], ["--clip_grad_norm=-1.5"],
                                  ["--clip_grad_norm", "nan"]])
def test_config_rejects_bad_clip_values(argv):
    with pytest.raises(ValueError):
        config_from_args(build_parser().parse_args(argv))


def test_config_default_and_engine_validation():
    assert config_from_args(build_parser().parse_args([])).clip_grad_norm is None
    cfg = config_from_args(build_parser().parse_args(["--clip_grad_norm", "1.5",
                                                      "--optimizer", "adam"]))
    assert cfg.clip_grad_norm == 1.5 and isinstance(cfg.clip_grad_norm, float)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            validate(TrainConfig(clip_grad_norm=bad))
        with pytest.raises(ValueError):
            _engine([2, 3, 1], "mse", 4, clip=bad)


def test_metrics_json_records_norm_and_coefficient_only_with_the_flag(tmp_path):
    recs = {}
    for clip in (0.05, None):
        path = str(tmp_path / f"m{clip}.jsonl")
        res = trainer.run_worker(TrainConfig(device="cpu", print_rank="none", nepochs=3,
                                             clip_grad_norm=clip, metrics_json=path))
        recs[clip] = [json.loads(l) for l in open(path) if l.strip()]
        assert len(res.grad_norms) == (3 if clip else 0)
    assert all("grad_norm" not in r and "clip_coef" not in r for r in recs[None])
    ep = [r for r in recs[0.05] if "epoch" in r]
    assert len(ep) == 3
    for r in ep:
        assert r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1.0
        assert r["clip_coef"] == pytest.approx(min(1.0, 0.05 / (r["grad_norm"] + 1e-6)), rel=1e-6)


@pytest.mark.parametrize("fill,coef_is", [(0.0, "one"), (float("nan"), "nan"),
                                          (float("inf"), "zero")])
def test_finalize_semantics_through_torch_ops(fill, coef_is):
    """A zero gradient: coefficient exactly 1 and slot 4 bitwise the base scale; a NaN gradient:
    NaN norm and coefficient (torch.clamp(max=1) keeps a NaN); an inf gradient: coefficient 0."""
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.ops.torch_ops import TorchOps
    ops = TorchOps()
    ar = Arena([(3, 2), (1, 3)], "cpu")
    ar.grad.fill_(1.0)
    ar.grad[5] = fill
    if fill == 0.0:
        ar.grad.zero_()
    hp = torch.tensor([0.1, 0.9, 0, 0, 7.0, 0, 0, 0], dtype=torch.float32)
    base = 0.3
    cs = torch.tensor([2.0, base, -1.0, -1.0], dtype=torch.float32)
    part = torch.zeros(1024, dtype=torch.float64)
    n = ops.grad_sumsq(ar, part)
    ops.clip_finalize(hp, cs, part, n)
    norm, coef = cs[2].item(), cs[3].item()
    if coef_is == "one":
        assert norm == 0.0 and coef == 1.0
        assert hp[4].item() == cs[1].item()          # bitwise the fp32 base scale
    elif coef_is == "nan":
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(hp[4].item())
    else:
        assert norm == math.inf and coef == 0.0 and hp[4].item() == 0.0
    assert cs[0].item() == 2.0 and cs[1].item() == torch.tensor(base).item()


def test_torch_ops_sumsq_range_bf16_and_rank_ordered_finalize():
    """The ranged and the bf16-payload forms against float64, and a finalize over P gathered
    per-rank sums: norm = base * sqrt(sum in rank order)."""
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.ops.torch_ops import TorchOps
    ops = TorchOps()
    ar = Arena([(16, 12), (4, 16)], "cpu")
    g = torch.Generator().manual_seed(1)
    ar.grad.copy_(torch.randn(ar.numel, generator=g))
    part = torch.zeros(1024, dtype=torch.float64)
    assert ops.grad_sumsq(ar, part, offset=8, numel=64) == 1
    assert part[0].item() == float((ar.grad[8:72].double() ** 2).sum())
    g16 = ar.grad.to(torch.bfloat16)
    ops.grad_sumsq(ar, part, grad_bf16=g16)
    assert part[0].item() == float((g16.double() ** 2).sum())
    sums = torch.tensor([1.5, 2.25, 0.25], dtype=torch.float64)
    out = torch.zeros(1, dtype=torch.float64)
    ops.sumsq_reduce(sums, 3, out)
    assert out.item() == 4.0
    hp = torch.ones(8, dtype=torch.float32)
    cs = torch.tensor([1.0, 0.5, 0, 0], dtype=torch.float32)
    ops.clip_finalize(hp, cs, sums, 3)
    assert cs[2].item() == 1.0 and cs[3].item() == pytest.approx(1.0 / (1.0 + 1e-6), rel=1e-7)
    assert hp[4].item() == pytest.approx(0.5 / (1.0 + 1e-6), rel=1e-7)
