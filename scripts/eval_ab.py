"""Forward-only evaluation A/B (docs/PERF.md "Forward-only evaluation"): ``MLPEngine.evaluate``
(the training head: dlogits, dZ and a discarded weight gradient, one host synchronisation per
row chunk) against ``MLPEngine.evaluate_metrics`` (head_eval.hip, one synchronisation in all).

One MI355X, three configurations:

    mnist   784-1024-1024-10, cross-entropy, bf16, R = 8192     8,192 validation rows
    mnist   the same                                            65,536 rows (eight chunks)
    proxy   512-512-512-512-1, MSE, bf16, R = 8192              8,192 rows

Both paths are warmed up, then alternated in one process; every window is a host clock around
``inner`` calls (each call ends in a device synchronise), ``inner`` chosen so that a window lasts
at least 0.2 s.  Reported per path: median, min and max of ``--reps`` windows, in microseconds per
call, and whether evaluate_metrics is slower than evaluate by more than evaluate's own spread.

``--trace`` runs a few evaluate_metrics calls only (for ``rocprofv3 --kernel-trace --stats --
python scripts/eval_ab.py --trace``, a run of its own).

Usage: python scripts/eval_ab.py [--out profiles/eval_ab.txt] [--reps 5] [--window 0.25]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CONFIGS = [
    ("mnist_8192", [784, 1024, 1024, 10], "xent", 8192),
    ("mnist_65536", [784, 1024, 1024, 10], "xent", 65536),
    ("proxy512_8192", [512, 512, 512, 512, 1], "mse", 8192),
]
R = 8192


def build(widths, loss, n, dev):
    from nnmpi_amd.data import synth
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec(tuple(widths), "relu", loss)
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev, shadow_dtype=torch.bfloat16)
    ar.bind_model(reference_init(widths))
    eng = MLPEngine(spec, ar, HipOps(dev), NoSync(ar), device=dev, dtype=torch.bfloat16,
                    rows_capacity=R, lr=1e-3, momentum=0.9, use_graph=False)
    if loss == "xent":
        X, labels = synth.chunked_classification(0, n, widths[0], widths[-1], device=dev)
        Y = None
    else:
        X, Y = synth.chunked_regression(0, n, widths[0], out=widths[-1], device=dev)
        labels = None
    return eng, X.to(torch.bfloat16), Y, labels


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    return (time.perf_counter() - t0) / inner * 1e6


def measure(name, widths, loss, n, dev, reps, min_window):
    eng, X, Y, labels = build(widths, loss, n, dev)
    paths = {"evaluate": lambda: eng.evaluate(X, Y, labels),
             "evaluate_metrics": lambda: eng.evaluate_metrics(X, Y, labels)}
    for f in paths.values():          # warm-up: code objects, lazily allocated buffers
        for _ in range(5):
            f()
    ref, _ = eng.evaluate(X, Y, labels)
    got = eng.evaluate_metrics(X, Y, labels)
    inner = {k: max(3, math.ceil(min_window * 1e6 / window(f, 5))) for k, f in paths.items()}
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():    # alternated
            times[k].append(window(f, inner[k]))
    out = {"config": name, "widths": widths, "loss": loss, "rows": n, "R": R, "inner": inner,
           "loss_sum_evaluate": ref, "loss_sum_metrics": got["loss_sum"],
           "rel_diff": abs(got["loss_sum"] - ref) / max(abs(ref), 1e-30)}
    for k, v in times.items():
        out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                          "max": round(max(v), 2), "window_s": round(min(v) * inner[k] * 1e-6, 3)}
    e, m = out["evaluate_us"], out["evaluate_metrics_us"]
    out["spread_evaluate_us"] = round(e["max"] - e["min"], 2)
    out["metrics_minus_evaluate_us"] = round(m["median"] - e["median"], 2)
    out["within_spread"] = bool(m["median"] - e["median"] <= e["max"] - e["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ab.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_ab.py measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    if args.trace:
        for name, widths, loss, n in CONFIGS[::2]:
            eng, X, Y, labels = build(widths, loss, n, dev)
            for _ in range(20):
                eng.evaluate_metrics(X, Y, labels)
                eng.evaluate(X, Y, labels)
        return
    lines = []
    for name, widths, loss, n in CONFIGS:
        r = measure(name, widths, loss, n, dev, args.reps, args.window)
        print(json.dumps(r), flush=True)
        lines.append(r)
    with open(args.out, "w") as fh:
        fh.write("# scripts/eval_ab.py: us per call, median [min, max] of %d alternated windows "
                 ">= %.2f s, host clock around calls that end in a synchronise\n"
                 % (args.reps, args.window))
        for r in lines:
            e, m = r["evaluate_us"], r["evaluate_metrics_us"]
            fh.write("%-14s rows %6d  evaluate %9.2f [%9.2f, %9.2f]  evaluate_metrics %9.2f "
                     "[%9.2f, %9.2f]  diff %+8.2f  evaluate spread %7.2f  within spread: %s\n"
                     % (r["config"], r["rows"], e["median"], e["min"], e["max"], m["median"],
                        m["min"], m["max"], r["metrics_minus_evaluate_us"],
                        r["spread_evaluate_us"], r["within_spread"]))
        for r in lines:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
