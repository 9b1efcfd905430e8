"""Adam / AdamW at P = 2 and 3 over RCCL -- rank processes sharing one MI355X, each with its own
``NCCL_HOSTID`` (see test_multirank_gpu.py): the inline all-reduce, the per-bucket overlap on the
comm stream and ZeRO-1 apply the same update, step graphs (the device step counter ticking
inside them) included."""
import pytest
import torch

from _mp import run_ranks_proc

pytestmark = pytest.mark.gpu

LR, EPOCHS = 1e-3, 2


def rccl_env(rank):
    return {"NCCL_HOSTID": f"nnmpi-test-host-{rank}", "NCCL_SOCKET_IFNAME": "lo",
            "NCCL_IB_DISABLE": "1", "PYTHONFAULTHANDLER": "1", "NCCL_DEBUG": "WARN"}


def _cfg(**kw):
    base = dict(device="cuda", print_rank="none", widths=[64, 64, 1], n_features=64,
                n_samples=512, dtype="bf16", nepochs=EPOCHS, lr=LR, data_gen="device",
                data_dist="local", scaling="none", optimizer="adamw", weight_decay=1e-2,
                comm="native")
    base.update(kw)
    return base


def _replicas_equal(out):
    for r in range(1, len(out)):
        assert torch.equal(out[r]["final"], out[0]["final"]), f"rank {r} diverged"


def test_adamw_two_ranks_inline_overlap_zero1_bitwise_and_close_to_one_rank():
    """P = 2: the inline all-reduce, the per-bucket overlap (the bucket's AdamW pass on the comm
    stream behind its collective) and --shard_optimizer end with bitwise-equal parameters and
    losses, replicas equal across ranks.  Against P = 1 on the concatenated shard (global
    scaling, weighted averaging: the same global gradient) the difference is fp32 summation
    order only.  Adam divides the gradient by its own magnitude, so that reaches a parameter as
    2 * lr * eps_g per step, eps_g the relative difference of that gradient element: 256-term
    fp32 sums agree to about 256 * 2^-24 * kappa, i.e. 1e-3 at a condition number kappa of 60 ->
    4e-6 over the two steps, asserted for 99 % of the elements as atol = rtol = 1e-5; an element
    whose gradient cancels to nothing can take steps of opposite sign, which bounds the rest by
    the steps themselves: |m^ / sqrt(v^)| <= 1 over the first two steps (Cauchy-Schwarz on the
    bias-corrected weights), so the two runs part by at most 2 * lr per step."""
    kw = dict(scaling="global", averaging="weighted")
    a = run_ranks_proc(_cfg(comm_mode="inline", **kw), 2, env_per_rank=rccl_env)
    b = run_ranks_proc(_cfg(comm_mode="overlap", **kw), 2, env_per_rank=rccl_env)
    c = run_ranks_proc(_cfg(comm_mode="inline", shard_optimizer=True, **kw), 2,
                       env_per_rank=rccl_env)
    one = run_ranks_proc(_cfg(comm="none", **kw), 1)
    for out in (a, b, c):
        assert out[0]["schedule"]["optimizer"] == "adamw" and out[0]["steps"] == EPOCHS
        _replicas_equal(out)
    assert a[0]["schedule"]["inline"] and not b[0]["schedule"]["inline"]
    assert c[0]["schedule"]["sync"] == "ShardedSync"
    assert b[0]["schedule"]["deferred_updates"] == 0
    for r in range(2):
        assert a[r]["losses"] == b[r]["losses"] == c[r]["losses"], r
    assert torch.equal(a[0]["final"], b[0]["final"])
    assert torch.equal(a[0]["final"], c[0]["final"])
    x, y = a[0]["final"], one[0]["final"]
    assert one[0]["losses"][0] != one[0]["losses"][-1]      # (it trained)
    d = (x - y).abs()
    print("ADAM_P2_VS_P1 max", float(d.max()), "frac within 1e-5",
          float((d <= 1e-5 + 1e-5 * y.abs()).float().mean()))
    assert float((d <= 1e-5 + 1e-5 * y.abs()).float().mean()) >= 0.99
    assert float(d.max()) <= 2 * LR * EPOCHS * 1.01


def _saved(path):
    sd = torch.load(path, weights_only=True)
    st = torch.load(path + ".train", weights_only=True)
    assert st["optimizer"] == "adamw"
    return sd, st["momentum_by_name"], st["exp_avg_sq_by_name"]


def test_adamw_three_ranks_zero1_state_equals_inline_bitwise(tmp_path):
    """P = 3, an uneven split, rank-ordered fp32 sums for both runs (NNMPI_F32_REDUCE=ordered:
    the ordered all-reduce, and ZeRO-1's reduce-scatter with the same sums): the master, exp_avg
    and exp_avg_sq that gather_state re-assembles from the three owner slices -- read from the
    checkpoint rank 0 writes -- equal the inline run's, bit for bit and parameter by parameter
    (the two arenas are padded differently)."""
    env = lambda r: dict(rccl_env(r), NNMPI_F32_REDUCE="ordered")  # noqa: E731
    kw = dict(n_samples=287, comm_mode="inline")
    za, ia = str(tmp_path / "zero.pt"), str(tmp_path / "inline.pt")
    z = run_ranks_proc(_cfg(shard_optimizer=True, checkpoint=za, **kw), 3, env_per_rank=env)
    i = run_ranks_proc(_cfg(checkpoint=ia, **kw), 3, env_per_rank=env)
    _replicas_equal(z)
    _replicas_equal(i)
    assert torch.equal(z[0]["final"], i[0]["final"])
    for got, want, what in zip(_saved(za), _saved(ia), ("master", "exp_avg", "exp_avg_sq")):
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (what, k)
    assert all(float(v.abs().max()) > 0 for v in _saved(za)[2].values())
