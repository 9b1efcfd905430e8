"""Cost of the LAMB update next to the Adam pass (docs/PERF.md §6), measured as adam_perf.py
measures: hipGraphs of back-to-back launches timed with device events, every variant alternated
inside one process, medians with their spread.

* the three launches (lamb_moments, lamb_trust, lamb_apply) at each chunk size (2,048 / 4,096 /
  8,192) and ``adam_update`` over the proxy512 arena and the wide8192 arena (bf16 shadow,
  gradient zeroed behind the pass);
* the proxy512 training step (8,192 rows, graphs of 16 steps): ``--optimizer lamb`` vs ``adam``.

Usage: python scripts/lamb_perf.py [--out FILE] [--reps 7] [--steps 1600] [--skip_wide]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_perf import ROWS, WIDTHS, _alternate, _graph, _time_ms  # noqa: E402

import torch  # noqa: E402

ARENAS = {"proxy512": (WIDTHS, 200), "wide8192": ([8192, 8192, 8192, 8192, 8192, 1], 4)}
CHUNKS = (2048, 4096, 8192)


def passes(name: str, reps: int):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.optimizer import adam_hparams
    from nnmpi_amd.ops.hip_ops import HipOps
    widths, n = ARENAS[name]
    dev = torch.device("cuda", 0)
    ops = HipOps(dev)
    ar = Arena([(widths[i + 1], widths[i]) for i in range(len(widths) - 1)], dev,
               shadow_dtype=torch.bfloat16)
    ar.ensure_exp_avg_sq()
    ar.master.normal_(0.0, 0.05)
    ar.grad.normal_(0.0, 1e-3)
    ar.sync_shadow()
    hp = adam_hparams(1e-6, 0.9, 0.999, 1e-8, 1e-2, dev, step=1)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    os.environ["NNMPI_EXPERIMENTS"] = "1"        # the chunk size is an experiment knob
    states = {}
    for c in CHUNKS:
        os.environ["NNMPI_LAMB_CHUNK"] = str(c)
        states[c] = ops.lamb_state(ar)
        assert states[c].chunk == c
    del os.environ["NNMPI_LAMB_CHUNK"], os.environ["NNMPI_EXPERIMENTS"]

    def rep(f):
        def body():
            for _ in range(n):
                f()
        return body
    graphs = {"adam_pass": _graph(stream, rep(lambda: ops.adam(ar, hp, t, False)))}
    for c, st in states.items():
        graphs[f"moments_{c}"] = _graph(stream, rep(lambda st=st: ops.lamb_moments(ar, hp, st)))
        graphs[f"trust_{c}"] = _graph(stream, rep(lambda st=st: ops.lamb_trust(st)))
        graphs[f"apply_{c}"] = _graph(stream, rep(lambda st=st: ops.lamb_apply(ar, hp, st)))
    h = int(stream.cuda_stream)
    res = _alternate({k: (lambda g=g: _time_ms(stream, lambda: g.launch(h), 10) / n * 1e3)
                      for k, g in graphs.items()}, reps)
    out = {k + "_us": {"median": round(v[0], 3), "min": round(v[1], 3), "max": round(v[2], 3)}
           for k, v in res.items()}
    out["arena_elements"], out["chunks_4096"] = ar.numel, states[4096].nchunks
    for c in CHUNKS:
        tot = sum(res[f"{k}_{c}"][0] for k in ("moments", "trust", "apply"))
        out[f"lamb_{c}_us"] = round(tot, 3)
        out[f"lamb_{c}_over_adam"] = round(tot / res["adam_pass"][0], 3)
    # pass 1: p, g, m, v read, m, v written (24); pass 2: p, m, v read, p, g, shadow written (22)
    out["lamb_4096_TBps"] = round(ar.numel * 46 / (out["lamb_4096_us"] * 1e-6) / 1e12, 3)
    out["adam_TBps"] = round(ar.numel * 34 / (res["adam_pass"][0] * 1e-6) / 1e12, 3)
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
    for name in ("adam", "lamb"):
        ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev,
                   shadow_dtype=torch.bfloat16)
        ar.bind_model(reference_init(WIDTHS))
        eng = MLPEngine(spec, ar, HipOps(dev), NoSync(ar), device=dev, dtype=torch.bfloat16,
                        rows_capacity=ROWS, lr=1e-5, momentum=0.9, optimizer=name)
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
    out["lamb_over_adam"] = round(res["lamb"][0] / res["adam"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--skip_wide", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lamb_perf.py measures on the GPU: no device visible")
    import nnmpi_amd  # noqa: F401
    out = {k: passes(k, a.reps) for k in ARENAS if not (a.skip_wide and k == "wide8192")}
    out["steps"] = steps(a.reps, a.steps)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
