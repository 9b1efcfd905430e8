"""The launch trace of every step schedule: which kernels and collectives one step issues, and in
which order.  The bitwise tests pin what a step computes; this pins the structure that sets its
speed.  The op set's launching methods and the gradient sync's calls are recorded by patching
the bound methods on the engine's own instances (the engine dispatches on ``isinstance(sync,
...)``, so the objects are not wrapped) and the second and third step -- the third is the first
steady-state one: the row-band weight images are built -- are compared against literal lists."""
import json

import pytest

pytestmark = pytest.mark.gpu

import nnmpi_amd  # noqa: E402,F401
from nnmpi_amd.engine import trainer  # noqa: E402
from nnmpi_amd.utils.config import TrainConfig  # noqa: E402
from test_engine_gpu import _cfg, _wide_cfg  # noqa: E402

# every HipOps method that launches (predicates and size queries are not recorded)
LAUNCHES = ("linear_act", "linear_dgrad", "linear_wgrad", "linear_wgrad_defer", "head",
            "head_deferred", "wide_pair", "bwd_group", "slab_reduce", "rowband_pack",
            "rowband_step", "tiny_step", "gather_rows", "sgd")
SYNC_CALLS = ("begin", "ready", "launch_bucket", "finish", "update")


class _Recorder:
    def __init__(self):
        self.steps, self.cur, self.engine = [], None, None

    def add(self, what):
        if self.cur is not None:
            self.cur.append(what)

    def install(self, eng):
        self.engine = eng

        def wrap(obj, name, label):
            fn = getattr(obj, name, None)
            if fn is None:
                return

            def call(*a, **kw):
                self.add(label(a, kw))
                return fn(*a, **kw)
            setattr(obj, name, call)
        for name in LAUNCHES:
            if name == "rowband_step":
                wrap(eng.ops, name, lambda a, kw: "rowband_step(phase=%d,split=%d)" % (
                    kw.get("phase", 0), kw.get("split", -1)))
            else:
                wrap(eng.ops, name, lambda a, kw, n=name: n)
        for name in SYNC_CALLS:
            if name == "launch_bucket":
                wrap(eng.sync, name, lambda a, kw: "sync.launch_bucket(%d)" % a[0].index)
            else:
                wrap(eng.sync, name, lambda a, kw, n=name: "sync." + n)
        step = eng.step

        def traced_step():
            self.cur = []
            self.steps.append(self.cur)
            try:
                return step()
            finally:
                self.cur = None
        eng.step = traced_step


def _run_recorded(cfg, grouped=None):
    """Run ``cfg`` eagerly with a recording engine; the recorder (its ``engine`` stays usable)."""
    import nnmpi_amd.engine.engine as eng_mod
    rec = _Recorder()
    orig = eng_mod.MLPEngine.__init__

    def init(self, *args, **kw):
        kw["use_graph"] = False
        if grouped is not None:
            kw["grouped"] = grouped
        orig(self, *args, **kw)
        rec.install(self)
    eng_mod.MLPEngine.__init__ = init
    try:
        trainer.run_worker(cfg)
    finally:
        eng_mod.MLPEngine.__init__ = orig
    return rec


def _trace(cfg, grouped=None, empty_third=False):
    """The per-step traces of ``cfg``."""
    rec = _run_recorded(cfg, grouped)
    if empty_third:
        eng = rec.engine
        eng.load_batch(eng.X[:0], eng.Y[:0])
        eng.step()
        eng.synchronize()
    return rec.steps


RB = pytest.mark.rowband

# The steady-state step of every case (the second and the third step are equal, except for the
# empty batch), recorded on the engine before its schedules were gathered into one decision
# (MLPEngine._schedule) and one bucket pipeline (engine/pipeline.py).
FWD = ["linear_act", "linear_act"]
GROUPED = FWD + ["head_deferred", "bwd_group", "bwd_group", "slab_reduce"]
EXPECTED = {
    "tiny": ["sync.begin", "tiny_step", "sync.ready", "sync.ready", "sync.finish"],
    "sequential": ["sync.begin"] + FWD + [
        "head", "sync.ready", "linear_wgrad", "sync.ready", "linear_dgrad", "linear_wgrad",
        "sync.ready", "sync.finish", "sgd"],
    "grouped": GROUPED,
    "fused_ungrouped": FWD + ["head", "linear_dgrad", "linear_wgrad", "linear_wgrad"],
    "grouped_inline_rccl": GROUPED + ["sync.begin", "sync.launch_bucket(0)", "sync.finish", "sgd"],
    "grouped_comm_overlap": ["sync.begin"] + GROUPED + ["sync.launch_bucket(0)", "sync.finish",
                                                        "sgd"],
    "small_buckets_overlap": ["sync.begin"] + FWD + [
        "head", "linear_wgrad", "linear_dgrad", "sync.launch_bucket(0)", "linear_wgrad",
        "sync.launch_bucket(1)", "sgd", "sync.finish", "sgd"],
    "zero1": GROUPED + ["sync.update", "sgd"],
    "rowband": ["rowband_step(phase=0,split=0)"],
    "rowband_split": ["rowband_step(phase=0,split=1)"],
    "rowband_overlap": [
        "sync.begin", "rowband_step(phase=1,split=0)", "sync.launch_bucket(0)",
        "rowband_step(phase=2,split=0)", "sync.launch_bucket(1)", "sgd", "sync.launch_bucket(2)",
        "sgd", "sync.finish", "sgd"],
    "chunk_buckets_deferred": ["sync.begin"] + FWD + [
        "head", "sync.launch_bucket(0)", "linear_wgrad", "sync.launch_bucket(1)", "sgd",
        "linear_wgrad", "sync.launch_bucket(2)", "linear_wgrad", "sync.launch_bucket(3)",
        "linear_wgrad", "sync.launch_bucket(4)", "linear_dgrad", "linear_wgrad_defer",
        "sync.launch_bucket(5)", "linear_wgrad_defer", "sync.launch_bucket(6)",
        "linear_wgrad_defer", "sync.launch_bucket(7)", "linear_wgrad_defer", "sgd",
        "sync.launch_bucket(8)", "sync.finish", "sgd"],
}
# a grouped engine's empty batch runs the sequential body: every bucket's collective is still
# issued in backward order and the update runs, so the rank stays in step with its peers
EMPTY = ["sync.begin", "sync.ready", "sync.ready", "sync.ready", "sync.finish", "sgd"]


def _rb512(widths, rows, **kw):
    return _cfg(device="cuda", widths=widths, n_features=512, n_samples=rows, lr=1e-5,
                nepochs=3, **kw)


CASES = {
    "tiny": (lambda: TrainConfig(device="cuda", print_rank="none", nepochs=3), {}),
    "sequential": (lambda: _cfg(device="cuda", overlap=False, nepochs=3), {}),
    "grouped": (lambda: _cfg(device="cuda", nepochs=3), {}),
    "fused_ungrouped": (lambda: _cfg(device="cuda", nepochs=3), dict(grouped=False)),
    "grouped_inline_rccl": (lambda: _cfg(device="cuda", comm="native", comm_mode="inline",
                                         nepochs=3), {}),
    "grouped_comm_overlap": (lambda: _cfg(device="cuda", comm="native", comm_mode="overlap",
                                          nepochs=3), {}),
    "small_buckets_overlap": (lambda: _cfg(device="cuda", comm="native", comm_mode="overlap",
                                           bucket_mb=0.01, nepochs=3), dict(grouped=False)),
    "zero1": (lambda: _cfg(device="cuda", comm="native", shard_optimizer=True, nepochs=3), {}),
    "rowband": (lambda: _rb512([512, 512, 1], 4097), {}),
    "rowband_split": (lambda: _rb512([512, 512, 512, 1], 64), {}),
    "rowband_overlap": (lambda: _rb512([512, 512, 512, 512, 1], 4097, comm="native",
                                       comm_mode="overlap_rowband"), {}),
    "chunk_buckets_deferred": (lambda: _wide_cfg(comm="native", comm_mode="overlap", bucket_mb=16,
                                                 grad_dtype="bf16", nepochs=3), {}),
    "empty_batch": (lambda: _cfg(device="cuda", nepochs=2), dict(empty_third=True)),
}


@pytest.mark.parametrize("case", [pytest.param(c, marks=RB) if c.startswith("rowband") else c
                                  for c in CASES])
def test_step_launch_trace(case, monkeypatch):
    # (the row-band cases run under the production thresholds: 4,097 rows is the smallest batch
    # of a 512-wide model that takes the band kernel, 64 rows the column-split one)
    monkeypatch.delenv("NNMPI_ROWBAND_MIN_ROWS", raising=False)
    make, kw = CASES[case]
    steps = _trace(make(), **kw)
    assert len(steps) == 3
    print("TRACE", json.dumps({case: [steps[1], steps[2]]}))
    if case == "empty_batch":
        assert steps[1] == EXPECTED["grouped"] and steps[2] == EMPTY
    else:
        assert steps[1] == EXPECTED[case]
        assert steps[2] == EXPECTED[case]


# The communicator calls of the inline native sync: bench.py times ``comm_only()`` as "exactly the
# collectives of one step", so both must put the same calls on the communicator.
class _CommProxy:
    """Forwards to the communicator and records (call, elements, dtype code) of its collectives
    (dtype codes: 0 fp32, 1 bf16; the two scratch-buffer all-reduces have theirs in the name)."""
    # call -> (position of the element count, position of the dtype code or the fixed code)
    CALLS = {"allreduce": (1, 2), "reduce": (1, 2), "broadcast": (1, 2),
             "allreduce_bf16_acc32": (2, None), "allreduce_f32_ordered": (2, None)}
    FIXED = {"allreduce_bf16_acc32": 1, "allreduce_f32_ordered": 0}

    def __init__(self, comm):
        self._comm, self.calls = comm, []

    def __getattr__(self, name):
        fn = getattr(self._comm, name)
        if name not in self.CALLS:
            return fn
        n_at, dt_at = self.CALLS[name]

        def call(*a):
            dt = self.FIXED[name] if dt_at is None else int(a[dt_at])
            self.calls.append((name, int(a[n_at]), dt))
            return fn(*a)
        return call


INLINE_SYNCS = {
    "fp32": (dict(), lambda n: [("allreduce", n, 0)]),
    "bf16": (dict(grad_dtype="bf16"), lambda n: [("allreduce_bf16_acc32", n, 1)]),
    "root": (dict(sync="root"), lambda n: [("reduce", n, 0), ("broadcast", n, 0)]),
}


@pytest.mark.parametrize("kind", sorted(INLINE_SYNCS))
def test_inline_sync_comm_only_issues_the_steps_collectives(kind):
    """Inline NativeRcclSync over a 1-rank communicator (fp32 payload, bf16 payload, the root
    pattern): the calls one eager step makes on the communicator equal those of comm_only() --
    one sequence over the single whole-arena bucket -- and comm_only() leaves the collective
    signature alone."""
    kw, want = INLINE_SYNCS[kind]
    rec = _run_recorded(_cfg(device="cuda", comm="native", comm_mode="inline", nepochs=2, **kw))
    eng = rec.engine
    sync = eng.sync
    assert sync.inline and len(eng.arena.buckets) == 1
    proxy = sync.comm = _CommProxy(sync.comm)
    eng.step()
    eng.synchronize()
    step, proxy.calls = proxy.calls, []
    seq, sig = sync.seq, sync.sig
    with eng._on_stream():
        sync.comm_only()
    eng.synchronize()
    print("COMM", json.dumps({kind: [step, proxy.calls]}))
    assert step == proxy.calls
    assert step == want(eng.arena.numel)
    assert (sync.seq, sync.sig) == (seq, sig)
