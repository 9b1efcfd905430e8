"""LAMB at P = 2 over RCCL -- rank processes sharing one MI355X, each with its own ``NCCL_HOSTID``
(see test_multirank_gpu.py): the inline all-reduce, the per-bucket overlap and ZeRO-1."""
import pytest
import torch

from _mp import run_ranks_proc
from test_adam_multirank_gpu import _cfg, _replicas_equal, rccl_env

pytestmark = pytest.mark.gpu

LR, EPOCHS = 1e-3, 2


def test_lamb_two_ranks_inline_overlap_bitwise_zero1_close():
    """Inline and overlap (updates held until the join, then one whole-arena LAMB update) end
    bitwise equal, replicas equal in every run.  ZeRO-1 adds the same exact squares per slice and
    then in rank order: its trust ratios differ from the replicated path's by the regrouping of
    double additions, ~1e-13 relative, so a parameter differs by fp32 rounding of one update per
    step at most: atol = rtol = 1e-5 for >= 99 % of the elements.  No element can part by more
    than the steps themselves, lr x ratio x |u| with |u| <= 1 over the first steps (Adam's
    bound), in either run: 2 * lr * epochs * max_ratio."""
    kw = dict(optimizer="lamb", lr=LR, nepochs=EPOCHS, scaling="global", averaging="weighted")
    a = run_ranks_proc(_cfg(comm_mode="inline", **kw), 2, env_per_rank=rccl_env)
    b = run_ranks_proc(_cfg(comm_mode="overlap", **kw), 2, env_per_rank=rccl_env)
    c = run_ranks_proc(_cfg(comm_mode="inline", shard_optimizer=True, **kw), 2,
                       env_per_rank=rccl_env)
    for out in (a, b, c):
        assert out[0]["schedule"]["optimizer"] == "lamb" and out[0]["steps"] == EPOCHS
        _replicas_equal(out)
        assert out[0]["schedule"]["trust_ratios"] == out[1]["schedule"]["trust_ratios"]
    assert a[0]["schedule"]["inline"] and not b[0]["schedule"]["inline"]
    assert c[0]["schedule"]["sync"] == "ShardedSync"
    assert torch.equal(a[0]["final"], b[0]["final"])
    assert a[0]["losses"] == b[0]["losses"] and a[0]["losses"][0] != a[0]["losses"][-1]
    x, y = c[0]["final"], a[0]["final"]
    max_ratio = max(r for out in (a, c) for r, _, _ in out[0]["schedule"]["trust_ratios"].values())
    d = (x - y).abs()
    frac = float((d <= 1e-5 + 1e-5 * y.abs()).float().mean())
    print("LAMB_ZERO1_VS_INLINE max", float(d.max()), "frac within 1e-5", frac, "max ratio",
          max_ratio)
    assert frac >= 0.99
    assert float(d.max()) <= 2 * LR * EPOCHS * max_ratio
