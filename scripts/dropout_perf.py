"""Cost of --dropout (docs/PERF.md §6), measured as norm_perf.py measures: hipGraphs of
back-to-back launches timed with device events, every variant alternated inside one process,
medians of 7 with their spread.

* ``dropout_fwd`` and ``dropout_bwd`` (relu) alone at 8192 x 512 and 4096 x 8192 in bf16 with
  p = 0.5, next to ``norm_act_fwd`` and ``norm_bwd`` (layer) at the same shapes: the norm kernels
  move the same bytes per element (forward 4 B, backward 6 B), so the ratio shows whether the
  Philox rounds have made the dropout kernels ALU-bound;
* the proxy512 step (8,192 rows) and the wide8192 step (4,096 rows) with ``--dropout 0.5``
  against the same model without it on the sequential schedule (``--no_overlap``: with
  ``--dropout 0`` that body runs the launches it ran before the option existed) and on the
  default schedule.

Usage: python scripts/dropout_perf.py [--out FILE] [--reps 7] [--steps 1600] [--skip_wide]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_perf import _alternate, _graph, _time_ms  # noqa: E402

import torch  # noqa: E402

SHAPES = {"8192x512": (8192, 512, 100), "4096x8192": (4096, 8192, 20)}
MODELS = {"proxy512": ([512, 512, 512, 512, 1], 8192),
          "wide8192": ([8192, 8192, 8192, 8192, 8192, 1], 4096)}
P = 0.5


def kernels(reps: int):
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.ops.torch_ops import dropout_state
    dev = torch.device("cuda", 0)
    ops, stream, out = HipOps(dev), torch.cuda.Stream(device=dev), {}
    h = int(stream.cuda_stream)
    state = dropout_state(1, 0, dev)
    for name, (rows, H, n) in SHAPES.items():
        z = (1.5 * torch.randn(rows, H, device=dev) + 0.3).to(torch.bfloat16)
        a, dn = torch.empty_like(z), torch.randn(rows, H, device=dev).to(torch.bfloat16)
        stats = torch.zeros(rows, 2, device=dev)
        launches = {"dropout_fwd": lambda: ops.dropout(z, a, state, P, 1, 0),
                    "dropout_bwd": lambda: ops.dropout_bwd(dn, z, state, P, "relu", 1, 0),
                    "norm_fwd": lambda: ops.norm_act(z, "layer", "relu", a, stats),
                    "norm_bwd": lambda: ops.norm_bwd(dn, z, stats, "layer")}

        def rep(f):
            def body():
                for _ in range(n):
                    f()
            return body
        graphs = {k: _graph(stream, rep(f)) for k, f in launches.items()}
        res = _alternate({k: (lambda g=g: _time_ms(stream, lambda: g.launch(h), 10) / n * 1e3)
                          for k, g in graphs.items()}, reps)
        out[name] = {}
        for k, v in res.items():
            nbytes = rows * H * (4 if k.endswith("fwd") else 6)
            out[name][k] = {"us": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3),
                            "TBps": round(nbytes / (v[0] * 1e-6) / 1e12, 3)}
        for d in ("fwd", "bwd"):
            out[name][f"dropout_over_norm_{d}"] = round(res[f"dropout_{d}"][0] / res[f"norm_{d}"][0], 3)
    return out


def steps(model: str, reps: int, n: int):
    from nnmpi_amd.data import synth
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    widths, rows = MODELS[model]
    dev = torch.device("cuda", 0)
    X, Y = synth.chunked_regression(0, rows, widths[0], device=dev)
    engines = {}
    for name, p, kw in (("dropout", P, {}), ("sequential", 0.0, {"overlap": False}),
                        ("default", 0.0, {})):
        spec = MLPSpec(tuple(widths), "relu", "mse", "none", p)
        ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev,
                   shadow_dtype=torch.bfloat16)
        ar.bind_model(reference_init(widths, device=dev))
        eng = MLPEngine(spec, ar, HipOps(dev), NoSync(ar), device=dev, dtype=torch.bfloat16,
                        rows_capacity=rows, lr=1e-5, momentum=0.9, **kw)
        eng.load_batch(X.to(torch.bfloat16), Y)
        eng.set_scales(1.0 / rows, 1.0 / rows, 1.0)
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
    out["dropout_over_sequential"] = round(res["dropout"][0] / res["sequential"][0], 4)
    out["dropout_over_default"] = round(res["dropout"][0] / res["default"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--skip_wide", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropout_perf.py measures on the GPU: no device visible")
    import nnmpi_amd  # noqa: F401
    out = {"kernels": kernels(a.reps)}
    for m in MODELS:
        if not (a.skip_wide and m == "wide8192"):
            out[m] = steps(m, a.reps, a.steps if m == "proxy512" else max(16, a.steps // 10))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
