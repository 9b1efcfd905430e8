"""Cost of the Adam / AdamW optimizer pass next to the SGD-momentum pass (docs/PERF.md §6).

Three measurements on one MI355X, each a hipGraph of back-to-back launches timed with device
events, the variants alternated inside one process and the median of the repeats reported with
their spread:

* the optimizer pass alone over the proxy512 arena (512-512-512-512-1, bf16 shadow, gradient
  zeroed behind the pass): ``sgd_momentum`` vs ``adam_update``, and the bytes each moves;
* ``adam_tick`` inside a replayed graph: the pass with and without the tick in front of it, and
  a chain of ticks alone;
* the proxy512 training step (8,192 rows, graphs of 16 steps): ``--optimizer adamw`` vs
  SGD-momentum with ``fuse_sgd=False`` -- the same unfused schedule, only the pass differs.

Usage: python scripts/adam_perf.py [--out FILE] [--reps 7] [--passes 200] [--steps 1600]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WIDTHS = [512, 512, 512, 512, 1]
ROWS = 8192


def _graph(stream, body):
    from nnmpi_amd import native
    g = native.lib().GraphRunner()
    with torch.cuda.stream(stream):
        g.begin(int(stream.cuda_stream))
        body()
        g.end()
    return g


def _time_ms(stream, launch, inner: int) -> float:
    """Milliseconds per replay of ``launch`` (``inner`` replays between two device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        for _ in range(inner):
            launch()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / inner


def _alternate(variants, reps):
    """{name: (median, min, max)} of ``reps`` alternated timings of every variant."""
    for fn in variants.values():       # warm-up: code objects, graph upload
        fn()
    got = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            got[k].append(fn())
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def passes(reps: int, n: int):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.optimizer import adam_hparams, sgd_hparams
    from nnmpi_amd.ops.hip_ops import HipOps
    dev = torch.device("cuda", 0)
    ops = HipOps(dev)
    ar = Arena([(WIDTHS[i + 1], WIDTHS[i]) for i in range(len(WIDTHS) - 1)], dev,
               shadow_dtype=torch.bfloat16)
    ar.ensure_exp_avg_sq()
    gen = torch.Generator(device="cpu").manual_seed(0)
    ar.master.copy_(torch.randn(ar.numel, generator=gen) * 0.05)
    ar.sync_shadow()
    hp_s = sgd_hparams(1e-6, 0.9, 0.0, 0.0, dev)
    hp_a = adam_hparams(1e-6, 0.9, 0.999, 1e-8, 1e-2, dev, step=1)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    images = dict(enumerate(ops.rowband_packed(WIDTHS[1], WIDTHS[0], len(WIDTHS) - 2, dev)[1]))

    def rep(f):
        def body():
            for _ in range(n):
                f()
        return body
    graphs = {
        "sgd_pass": _graph(stream, rep(lambda: ops.sgd(ar, hp_s, False, False))),
        "adam_pass": _graph(stream, rep(lambda: ops.adam(ar, hp_a, t, True))),
        "tick_adam_pass": _graph(stream, rep(lambda: (ops.adam_tick(hp_a, t),
                                                      ops.adam(ar, hp_a, t, True)))),
        "tick_chain": _graph(stream, rep(lambda: ops.adam_tick(hp_a, t))),
        # with the row-band weight images refreshed by the pass (SGD: the tiled kernel; Adam:
        # element-wise, rb_pack_store4)
        "sgd_pass_images": _graph(stream, rep(lambda: ops.sgd(ar, hp_s, False, False,
                                                              images=images))),
        "adam_pass_images": _graph(stream, rep(lambda: ops.adam(ar, hp_a, t, True,
                                                                images=images))),
    }
    h = int(stream.cuda_stream)
    res = _alternate({k: (lambda g=g: _time_ms(stream, lambda: g.launch(h), 50) / n * 1e3)
                      for k, g in graphs.items()}, reps)
    out = {k + "_us": {"median": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3)}
           for k, v in res.items()}
    out["arena_elements"] = ar.numel
    # p, g, m (+ v) read; p, m (+ v), the zeroed g and the bf16 shadow written
    out["sgd_bytes_per_element"], out["adam_bytes_per_element"] = 26, 34
    for k, b in (("sgd_pass", 26), ("adam_pass", 34)):
        out[k + "_TBps"] = round(ar.numel * b / (res[k][0] * 1e-6) / 1e12, 3)
    out["adam_over_sgd"] = round(res["adam_pass"][0] / res["sgd_pass"][0], 3)
    out["tick_in_graph_us"] = round(res["tick_adam_pass"][0] - res["adam_pass"][0], 3)
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
    for name, kw in (("sgd_unfused", dict(fuse_sgd=False)), ("adamw", dict(optimizer="adamw")),
                     ("sgd_fused", dict())):
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
    out["adamw_over_sgd_unfused"] = round(res["adamw"][0] / res["sgd_unfused"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--steps", type=int, default=1600)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_perf.py measures on the GPU: no device visible")
    import nnmpi_amd  # noqa: F401
    out = {"passes": passes(a.reps, a.passes), "steps": steps(a.reps, a.steps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
