"""Cost of global-norm gradient clipping (``--clip_grad_norm``; docs/PERF.md §6).

Two measurements on one MI355X, each timed with device events, the variants alternated inside
one process and the median of the repeats reported with their spread (the method of
scripts/adam_perf.py):

* the norm + finalize pair alone over the proxy512 arena (512-512-512-512-1): ``grad_sumsq`` (a
  read-only pass, 4 B per element) followed by the one-block ``clip_finalize``, as a hipGraph of
  back-to-back pairs, next to the SGD-momentum pass;
* the proxy512 training step (8,192 rows, graphs of 16 steps): SGD-momentum fused (the default)
  and with ``fuse_sgd=False`` -- the schedule a clipped step takes -- against
  ``clip_grad_norm=1.0``; the same pair under AdamW.

Usage: python scripts/clip_perf.py [--out FILE] [--reps 7] [--passes 200] [--steps 1600]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from adam_perf import ROWS, WIDTHS, _alternate, _graph, _time_ms  # noqa: E402


def passes(reps: int, n: int):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.optimizer import CLIP_MAX_PARTS, sgd_hparams
    from nnmpi_amd.ops.hip_ops import HipOps
    dev = torch.device("cuda", 0)
    ops = HipOps(dev)
    ar = Arena([(WIDTHS[i + 1], WIDTHS[i]) for i in range(len(WIDTHS) - 1)], dev,
               shadow_dtype=torch.bfloat16)
    gen = torch.Generator(device="cpu").manual_seed(0)
    ar.grad.copy_(torch.randn(ar.numel, generator=gen) * 0.05)
    g16 = ar.grad.to(torch.bfloat16)
    hp = sgd_hparams(1e-6, 0.9, 0.0, 0.0, dev)
    cs = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    part = torch.zeros(CLIP_MAX_PARTS, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)

    def rep(f):
        def body():
            for _ in range(n):
                f()
        return body

    def pair(**kw):
        ops.clip_finalize(hp, cs, part, ops.grad_sumsq(ar, part, **kw))
    graphs = {
        "sumsq": _graph(stream, rep(lambda: ops.grad_sumsq(ar, part))),
        "sumsq_finalize": _graph(stream, rep(pair)),
        "sumsq_bf16_finalize": _graph(stream, rep(lambda: pair(grad_bf16=g16))),
        "sgd_pass": _graph(stream, rep(lambda: ops.sgd(ar, hp, False, False, zero_grad=False))),
    }
    h = int(stream.cuda_stream)
    res = _alternate({k: (lambda g=g: _time_ms(stream, lambda: g.launch(h), 50) / n * 1e3)
                      for k, g in graphs.items()}, reps)
    out = {k + "_us": {"median": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3)}
           for k, v in res.items()}
    out["arena_elements"] = ar.numel
    out["sumsq_TBps"] = round(ar.numel * 4 / (res["sumsq"][0] * 1e-6) / 1e12, 3)
    return out


def steps(reps: int, n: int):
    from nnmpi_amd.data import synth
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    dev = torch.device("cuda", 0)
    spec = MLPSpec(tuple(WIDTHS), "relu", "mse")
    X, Y = synth.chunked_regression(0, ROWS, WIDTHS[0], device=dev)
    engines = {}
    for name, kw in (("sgd_fused", dict()), ("sgd_unfused", dict(fuse_sgd=False)),
                     ("sgd_clip", dict(clip_grad_norm=1.0)),
                     ("adamw", dict(optimizer="adamw")),
                     ("adamw_clip", dict(optimizer="adamw", clip_grad_norm=1.0))):
        ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev,
                   shadow_dtype=torch.bfloat16)
        ar.bind_model(reference_init(WIDTHS))
        eng = MLPEngine(spec, ar, HipOps(dev), NoSync(ar), device=dev, dtype=torch.bfloat16,
                        rows_capacity=ROWS, lr=1e-5, momentum=0.9, **kw)
        eng.load_batch(X.to(torch.bfloat16), Y)
        eng.set_scales(1.0 / ROWS, 1.0 / ROWS, 1.0)
        eng.run_steps(1 + 16, 16)
        eng.synchronize()
        engines[name] = eng

    def timed(eng):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(eng.stream)
        eng.run_steps(n, 16)
        b.record(eng.stream)
        b.synchronize()
        eng.check_device_errors()
        return a.elapsed_time(b) / n
    res = _alternate({k: (lambda e=e: timed(e)) for k, e in engines.items()}, reps)
    out = {k + "_step_ms": {"median": round(v[0], 5), "min": round(v[1], 5), "max": round(v[2], 5)}
           for k, v in res.items()}
    out["schedule"] = {k: e.schedule_name() for k, e in engines.items()}
    out["clip_coef"] = {k: e.clip_coef() for k, e in engines.items() if e.opt.clipping}
    out["sgd_clip_minus_unfused_us"] = round(
        (res["sgd_clip"][0] - res["sgd_unfused"][0]) * 1e3, 3)
    out["adamw_clip_minus_adamw_us"] = round((res["adamw_clip"][0] - res["adamw"][0]) * 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--steps", type=int, default=1600)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_perf.py measures on the GPU: no device visible")
    import nnmpi_amd  # noqa: F401
    out = {"passes": passes(a.reps, a.passes), "steps": steps(a.reps, a.steps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
