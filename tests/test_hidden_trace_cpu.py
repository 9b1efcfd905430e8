"""The op calls of one sequential step with --norm / --dropout on, in order, on TorchOps: which
hidden-layer transform runs where.  The numeric tests pin what such a step computes; this pins
that the norm and the dropout sit between the same launches, that dropout_bwd runs before
norm_bwd on every dZ, and that exactly one dropout_tick closes every training pass.  The op set's
methods are recorded by patching them on the engine's own instance, as test_schedule_trace_gpu.py
does."""
import pytest

import nnmpi_amd  # noqa: F401
from test_dropout_cpu import make_engine

WIDTHS, ROWS, P = (8, 16, 16, 1), 8, 0.25
CALLS = ("linear_act", "norm_act", "dropout", "head", "dropout_bwd", "norm_bwd", "linear_wgrad",
         "linear_dgrad", "dropout_tick", "sgd", "head_eval")

# one step() of the sequential body with both on
FULL = ["linear_act", "norm_act", "dropout", "linear_act", "norm_act", "dropout",
        "head", "dropout_bwd", "norm_bwd",
        "linear_wgrad", "linear_dgrad", "dropout_bwd", "norm_bwd", "linear_wgrad",
        "dropout_tick", "sgd"]
NORM_ONLY = ["linear_act", "norm_act", "linear_act", "norm_act",
             "head", "norm_bwd",
             "linear_wgrad", "linear_dgrad", "norm_bwd", "linear_wgrad",
             "sgd"]
DROP_ONLY = ["linear_act", "dropout", "linear_act", "dropout",
             "head", "dropout_bwd",
             "linear_wgrad", "linear_dgrad", "dropout_bwd", "linear_wgrad",
             "dropout_tick", "sgd"]
PLAIN = ["linear_act", "linear_act", "head", "linear_wgrad", "linear_dgrad", "linear_wgrad", "sgd"]


def _engine(norm, p):
    """The (8, 16, 16, 1) fp32 MSE engine with 8 rows loaded, and the list its op calls land in
    as (name, positional arguments)."""
    _, eng, _, X, Y = make_engine(WIDTHS, "tanh", norm, p, rows=ROWS, use_tiny=False)
    trace = []
    for name in CALLS:
        def call(*a, _fn=getattr(eng.ops, name), _name=name, **kw):
            trace.append((_name, a))
            return _fn(*a, **kw)
        setattr(eng.ops, name, call)
    return eng, trace, X, Y


def _names(trace):
    return [name for name, _ in trace]


@pytest.mark.parametrize("norm,p,want", [("layer", P, FULL), ("layer", 0.0, NORM_ONLY),
                                         ("none", P, DROP_ONLY), ("none", 0.0, PLAIN)])
def test_step_op_order(norm, p, want):
    eng, trace, _, _ = _engine(norm, p)
    assert eng.schedule_name() == "sequential"
    eng.step()
    assert _names(trace) == want
    assert eng.hidden.active == (want is not PLAIN)
    if want is PLAIN:
        assert eng.drop == [] and eng.dropout_step == 0


def test_dropout_operands():
    """dropout(layer i) reads acts[i] and writes drop[i]; dropout_bwd(layer i) rewrites dzl[i]
    through the UNDROPPED acts[i]; the backward visits the layers last first."""
    eng, trace, _, _ = _engine("layer", P)
    eng.step()
    ptr = lambda bufs: [t.data_ptr() for t in bufs]   # noqa: E731
    acts, drop, dzl = ptr(eng.acts), ptr(eng.drop), ptr(eng.dzl)
    assert len(set(acts + drop + dzl)) == 6
    fwd = [a for name, a in trace if name == "dropout"]
    bwd = [a for name, a in trace if name == "dropout_bwd"]
    # dropout(a, out, state, p, layer, rank); dropout_bwd(dd, a, state, p, act, layer, rank)
    assert [(a[0].data_ptr(), a[1].data_ptr(), a[4]) for a in fwd] == [
        (acts[0], drop[0], 0), (acts[1], drop[1], 1)]
    assert [(a[0].data_ptr(), a[1].data_ptr(), a[5]) for a in bwd] == [
        (dzl[1], acts[1], 1), (dzl[0], acts[0], 0)]
    assert all(a[0].shape[0] == ROWS and a[1].shape[0] == ROWS for a in fwd + bwd)
    # what the next layer, the head and the weight gradients read is the dropped copy
    reads = {name: [a for n, a in trace if n == name] for name in ("linear_act", "head",
                                                                   "linear_wgrad")}
    assert reads["linear_act"][1][0].data_ptr() == drop[0]
    assert reads["head"][0][0].data_ptr() == drop[1]
    assert reads["linear_wgrad"][0][1].data_ptr() == drop[0]


def test_forward_only_paths_leave_dropout_alone():
    eng, trace, X, Y = _engine("layer", P)
    eng.evaluate(X, Y)
    eng.predict(X)
    names = _names(trace)
    assert names == ["linear_act", "norm_act"] * 2 + ["head"] + ["linear_act", "norm_act"] * 2 + [
        "head_eval"]
    assert not any(n.startswith("dropout") for n in names) and eng.dropout_step == 0


def test_empty_batch_is_one_pass():
    eng, trace, _, _ = _engine("layer", P)
    eng.load_batch(eng.X[:0], eng.Y[:0])
    eng.step()
    assert _names(trace) == ["dropout_tick", "sgd"] and eng.dropout_step == 1
