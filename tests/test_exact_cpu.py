"""The exact-integer GEMM oracle (tests/_exact.py) checked on the CPU: the precondition holds at
the shapes the GPU tests use it for, and the comparison is sharp -- the REFERENCE is damaged in
the ways a kernel goes wrong (negative controls) and the bitwise comparison must fail each time.
"""
import pytest
import torch

import _exact as ex

M, N, K = 136, 200, 2050


@pytest.fixture(scope="module")
def case():
    x = ex.ints((M, K), -4, 4, 1)
    W = ex.ints((N, K), -4, 4, 2)
    b = ex.ints(N, -64, 64, 3, dtype=torch.float32)
    bound = ex.assert_exact_ok(x, W.t(), b)
    z = ex.preact(x, W, b)
    return x, W, b, z, bound


def test_precondition_bound_and_two_fp32_orders_equal_float64(case):
    x, W, b, z, bound = case
    assert 8000 < bound < ex.TWO24
    xf, Wf = x.float(), W.float()
    fwd_order = torch.zeros(M, N)
    for k0 in range(0, K, 64):                      # 64-deep k-steps, ascending
        fwd_order = fwd_order + xf[:, k0:k0 + 64] @ Wf[:, k0:k0 + 64].t()
    halves = torch.zeros(M, N)
    for part in (slice(1025, K), slice(0, 1025)):   # two uneven "splits", the later one first
        acc = torch.zeros(M, N)
        for k in reversed(range(part.start, part.stop)):
            acc = acc + xf[:, k:k + 1] * Wf[:, k].unsqueeze(0)
        halves = halves + acc
    for got in (fwd_order, halves):
        assert ex.same(got + b, ex.f32(z))


def test_precondition_refuses_operands_that_can_round():
    big = ex.ints((4, 2050), 100, 128, 5)
    with pytest.raises(AssertionError, match="2\\^24"):
        ex.assert_exact_ok(big, big.t())
    with pytest.raises(AssertionError, match="grid"):
        ex.assert_exact_ok(ex.ints((4, 8), -4, 4, 6, scale=0.5), ex.ints((8, 4), -4, 4, 7))
    ex.assert_exact_ok(ex.ints((4, 8), -4, 4, 6, scale=0.5), ex.ints((8, 4), -4, 4, 7), ua=0.5)
    with pytest.raises(AssertionError, match="not exact"):
        ex.ints((4, 4), 0, 300, 8)                  # bf16 holds integers only up to 256


def test_control_dropped_k_tail(case):
    x, W, b, z, _ = case
    bad = ex.preact(x[:, :-8], W[:, :-8], b)
    assert not ex.same(ex.bf16_rne(bad), ex.bf16_rne(z))
    assert not ex.same(ex.f32(bad), ex.f32(z))


def test_control_transposed_fragment(case):
    *_, z, _ = case
    bad = z.clone()
    bad[16:32, 32:48] = z[16:32, 32:48].t()
    assert not ex.same(ex.bf16_rne(bad), ex.bf16_rne(z))


def test_control_truncation_instead_of_rne(case):
    *_, z, _ = case
    rne, trunc = ex.bf16_rne(z), ex.bf16_trunc(z)
    share = float((rne != trunc).double().mean())
    assert share >= 0.10, f"only {share:.3f} of the outputs tell RNE from truncation: inputs too tame"
    assert not ex.same(trunc, rne)
    # exact ties (the low 16 bits are 0x8000) are where round-half-up and RNE part
    ties = (ex.f32(z).view(torch.int32) & 0xFFFF) == 0x8000
    assert float(ties.double().mean()) > 0.0


def test_control_bias_shifted_in_the_n_tail(case):
    x, W, b, z, _ = case
    bad_b = b.clone()
    bad_b[192:] = torch.roll(b[192:], 1)            # the last, partial column chunk of N = 200
    assert not torch.equal(bad_b, b)
    assert not ex.same(ex.bf16_rne(ex.preact(x, W, bad_b)), ex.bf16_rne(z))


@pytest.mark.parametrize("S", [2, 7, 65])
def test_control_slab_sum_missing_one_split(S):
    ws = ex.ints((S, 5, 8), -1000, 1000, 10 + S, dtype=torch.float32)
    assert float(ws.abs().sum(0).max()) < ex.TWO24
    full = ex.f32(ex.slab_sum(ws))
    for leave in (0, S - 1):
        keep = [s for s in range(S) if s != leave]
        assert not ex.same(ex.f32(ex.slab_sum(ws[keep])), full)


def test_relu_and_tanh_derivative_oracles_are_fp32_exact():
    dz = ex.ints((40, 72), -2, 2, 20)
    W = ex.ints((72, 136), -2, 2, 21)
    assert ex.assert_exact_ok(dz, W) <= 1000
    a = ex.tanh_grid((40, 136), 22)
    want = ex.dgrad(dz, W, a, "tanh")
    acc, af = ex.f32(ex.gemm(dz, W)), a.float()
    # three associations of acc (1 - a^2) in fp32, all exact
    for got in (acc * (1 - af * af), acc - acc * af * af, acc * ((1 - af) * (1 + af))):
        assert ex.same(got, ex.f32(want))
    r = ex.dgrad(dz, W, torch.relu(a), "relu")
    assert ex.same(ex.f32(r), acc * (a > 0).float())


def test_tanh_forward_cpu_reference_stays_inside_both_conditions():
    """fp32 torch.tanh on the exact pre-activations of the GPU test's tanh case: every output
    within 1 bf16 ulp of bf16(tanh_f64(z)), at most 1e-3 of them not identical."""
    x = ex.ints((200, 72), -4, 4, 30)
    W = ex.ints((136, 72), -4, 4, 31, scale=2.0 ** -6)
    b = ex.ints(136, -64, 64, 32, scale=2.0 ** -6, dtype=torch.float32)
    ex.assert_exact_ok(x, W.t(), b, ub=2.0 ** -6)
    z = ex.preact(x, W, b)
    assert float(z.abs().max()) > 3 and float((z.abs() < 1).double().mean()) > 0.2
    want = torch.tanh(z).to(torch.bfloat16)
    got = torch.tanh(ex.f32(z)).to(torch.bfloat16)
    assert float(ex.bf16_ulp_apart(got, want).max()) <= 1.0
    share = float((got != want).double().mean())
    print(f"\nTANH_SHARE cpu fp32 reference: {share:.2e}")
    assert share <= 1e-3


def test_embed_and_guards():
    t = ex.ints((5, 16), -4, 4, 40)
    buf, v = ex.embed(t, 2, 4, ex.NAN)
    assert v.stride(0) == 24 and v.storage_offset() == 2 * 24 + 4 and torch.equal(v, t)
    assert torch.isnan(buf[:2]).all() and torch.isnan(buf[:, :4]).all() and torch.isnan(buf[:, 20:]).all()
    assert ex.guards_intact(buf, v)
    out, ov = ex.embed(torch.zeros(5, 16), 1, 2, ex.SENTINEL_F32, pad_right=3)
    assert ov.stride(0) == 21 and ex.guards_intact(out, ov)
    ov.fill_(7.0)                                   # writing the view is fine
    assert ex.guards_intact(out, ov)
    for hit in ((0, 5), (3, 1), (3, 18), (6, 20)):  # above, left, right, below
        o2 = out.clone()
        o2.poison_bits = out.poison_bits
        o2[hit] = 7.0
        v2 = o2[1:6, 2:18]
        assert not ex.guards_intact(o2, v2), hit
    b1, v1 = ex.embed(torch.zeros(12, dtype=torch.bfloat16), 0, 4, ex.SENTINEL_BF16)
    assert v1.storage_offset() == 4 and ex.guards_intact(b1, v1)
    b1[2] = 0.0
    assert not ex.guards_intact(b1, v1)
    # a NaN from the padding reaches whatever sums it
    assert torch.isnan(buf[2, 4:28].float().sum())
