"""--clip_grad_norm at P = 2 and 3 over RCCL -- rank processes sharing one MI355X, each with its
own ``NCCL_HOSTID`` (see test_multirank_gpu.py): the inline and the overlapped all-reduce apply
the same clipped update bit for bit, ZeRO-1 keeps its replicas bitwise equal through the
rank-ordered gather of the per-rank sums, and every rank reports the same norm."""
import pytest
import torch

from _mp import run_ranks_proc

pytestmark = pytest.mark.gpu

LR, EPOCHS = 1e-3, 2
# the gradient norm of this model and data is about 170 (its first steps, measured on the CPU
# path): a max_norm of 10 clips every step -- asserted from the recorded coefficients
MAX_NORM = 10.0


def rccl_env(rank):
    return {"NCCL_HOSTID": f"nnmpi-test-host-{rank}", "NCCL_SOCKET_IFNAME": "lo",
            "NCCL_IB_DISABLE": "1", "PYTHONFAULTHANDLER": "1", "NCCL_DEBUG": "WARN"}


def _cfg(**kw):
    base = dict(device="cuda", print_rank="none", widths=[64, 64, 1], n_features=64,
                n_samples=512, dtype="bf16", nepochs=EPOCHS, lr=LR, data_gen="device",
                data_dist="local", scaling="none", optimizer="adamw", weight_decay=1e-2,
                comm="native", clip_grad_norm=MAX_NORM)
    base.update(kw)
    return base


def _check_clipped(out, world):
    """Every rank: one (norm, coefficient) per epoch, every coefficient below 1, the replicas
    and the reported norms equal across ranks bit for bit."""
    for r in range(world):
        s = out[r]["schedule"]
        assert s["clip_grad_norm"] == MAX_NORM and out[r]["steps"] == EPOCHS
        assert len(s["grad_norms"]) == len(s["clip_coefs"]) == EPOCHS
        assert all(0 < c < 1.0 for c in s["clip_coefs"]), s["clip_coefs"]
        assert s["grad_norms"] == out[0]["schedule"]["grad_norms"], f"rank {r}: another norm"
        assert s["clip_coefs"] == out[0]["schedule"]["clip_coefs"]
        assert torch.equal(out[r]["final"], out[0]["final"]), f"rank {r} diverged"


@pytest.fixture(scope="module")
def inline2():
    return run_ranks_proc(_cfg(comm_mode="inline"), 2, env_per_rank=rccl_env)


def test_two_ranks_inline_and_overlap_bitwise_equal_under_clipping(inline2):
    """P = 2: the inline all-reduce and the per-bucket overlap -- whose bucket updates all wait
    for the join under clipping: one norm, one finalize, one update -- end with bitwise-equal
    parameters, losses and norms; the step graph of the second epoch included."""
    a = inline2
    b = run_ranks_proc(_cfg(comm_mode="overlap"), 2, env_per_rank=rccl_env)
    for out in (a, b):
        _check_clipped(out, 2)
    assert a[0]["schedule"]["inline"] and not b[0]["schedule"]["inline"]
    assert a[0]["schedule"]["graph"] and b[0]["schedule"]["graph"]
    assert b[0]["schedule"]["deferred_updates"] == 0
    for r in range(2):
        assert a[r]["losses"] == b[r]["losses"], r
    assert torch.equal(a[0]["final"], b[0]["final"])
    assert a[0]["schedule"]["grad_norms"] == b[0]["schedule"]["grad_norms"]


def test_two_ranks_zero1_replicas_bitwise_equal_and_close_to_allreduce(inline2):
    """P = 2 ZeRO-1: each rank's sum of squares of its reduced slice, gathered bitwise and added
    in rank order -- the replicas are bitwise equal across ranks.  Against the all-reduce run the
    same double sum is grouped differently (about 1e-13 relative in the norm, so possibly the
    last bit of the fp32 coefficient): parameters within rtol = atol = 1e-6, not bitwise."""
    z = run_ranks_proc(_cfg(comm_mode="inline", shard_optimizer=True), 2, env_per_rank=rccl_env)
    _check_clipped(z, 2)
    assert z[0]["schedule"]["sync"] == "ShardedSync"
    torch.testing.assert_close(z[0]["final"], inline2[0]["final"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(torch.tensor(z[0]["schedule"]["grad_norms"]),
                               torch.tensor(inline2[0]["schedule"]["grad_norms"]),
                               rtol=1e-6, atol=1e-6)
    assert z[0]["losses"][0] != z[0]["losses"][-1]      # (it trained)


def test_three_ranks_uneven_split_report_one_norm():
    """P = 3, 287 samples (96 / 96 / 95 rows), ZeRO-1: every rank reports the same grad_norm and
    coefficient bit for bit and holds the same parameters."""
    z = run_ranks_proc(_cfg(comm_mode="inline", shard_optimizer=True, n_samples=287), 3,
                       env_per_rank=rccl_env)
    assert len({z[r]["rows"] for r in range(3)}) > 1      # (an uneven split)
    _check_clipped(z, 3)
