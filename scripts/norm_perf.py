"""Cost of --norm (docs/PERF.md §7), measured as lamb_perf.py measures: hipGraphs of back-to-back
launches timed with device events, every variant alternated inside one process, medians with
their spread.

* ``norm_act_fwd`` and ``norm_bwd`` alone at 8192 x 512 and 4096 x 8192 in bf16, against the
  bytes each moves (forward: z read, a written = 4 B / element; backward: dn and z read, dz
  written = 6 B / element; the statistics are 8 B / row);
* the proxy512 step (8,192 rows) and the wide8192 step (4,096 rows) with ``--norm layer`` against
  the same model without a norm on the sequential schedule (``--no_overlap``: with ``--norm
  none`` that body runs the launches it ran before the option existed, so the difference is
  the two kernels and the un-fused activation) and on the default schedule (what giving up the
  fused / row-band bodies costs).

Usage: python scripts/norm_perf.py [--out FILE] [--reps 7] [--steps 1600] [--skip_wide]
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


def kernels(reps: int):
    from nnmpi_amd.ops.hip_ops import HipOps
    dev = torch.device("cuda", 0)
    ops, stream, out = HipOps(dev), torch.cuda.Stream(device=dev), {}
    h = int(stream.cuda_stream)
    for name, (rows, H, n) in SHAPES.items():
        z = (1.5 * torch.randn(rows, H, device=dev) + 0.3).to(torch.bfloat16)
        a, dn = torch.empty_like(z), torch.randn(rows, H, device=dev).to(torch.bfloat16)
        stats = torch.zeros(rows, 2, device=dev)

        def rep(f):
            def body():
                for _ in range(n):
                    f()
            return body
        graphs = {f"{k}_{norm}": _graph(stream, rep(f))
                  for norm in ("layer", "rms")
                  for k, f in (("fwd", lambda norm=norm: ops.norm_act(z, norm, "relu", a, stats)),
                               ("bwd", lambda norm=norm: ops.norm_bwd(dn, z, stats, norm)))}
        res = _alternate({k: (lambda g=g: _time_ms(stream, lambda: g.launch(h), 10) / n * 1e3)
                          for k, g in graphs.items()}, reps)
        out[name] = {}
        for k, v in res.items():
            nbytes = rows * H * (4 if k.startswith("fwd") else 6) + rows * 8
            out[name][k] = {"us": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3),
                            "TBps": round(nbytes / (v[0] * 1e-6) / 1e12, 3)}
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
    for name, norm, kw in (("norm_layer", "layer", {}), ("sequential", "none", {"overlap": False}),
                           ("default", "none", {})):
        spec = MLPSpec(tuple(widths), "relu", "mse", norm)
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
    out["norm_over_sequential"] = round(res["norm_layer"][0] / res["sequential"][0], 4)
    out["norm_over_default"] = round(res["norm_layer"][0] / res["default"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--skip_wide", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_perf.py measures on the GPU: no device visible")
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
