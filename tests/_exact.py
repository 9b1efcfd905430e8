"""Exact-integer operands and float64 oracles for the GEMM family (no GPU needed).

The 2^24 precondition (tests/test_tiny_mlp.py uses the same idea): when every operand is a small
integer -- or a dyadic multiple ``unit`` of one -- and sum_k |a_k| |b_k| + |bias|, counted in
units, stays below 2^24, every product and every partial sum of the dot product is an integer
below 2^24 times a power of two, hence exact in fp32, in ANY summation order, tile shape or
split-K count.  An fp32 kernel result must then equal the float64 matmul bit for bit, and a bf16
output must equal its round-to-nearest-even cast.

``embed`` places an operand or an output inside a larger poisoned allocation (a view with
ld > width and an offset base pointer); ``guards_intact`` compares the poison around the view
bit for bit afterwards.  Inputs are poisoned with NaN -- a read past a K, M or N tail that the
kernel's predicate should have turned into zero then yields NaN -- outputs with a sentinel bit
pattern.
"""
import torch

TWO24 = float(2 ** 24)
NAN = float("nan")
SENTINEL_F32 = 0x4B5A5A5A    # 14309978.0 as fp32
SENTINEL_BF16 = 0x4B5A       # 14286848.0 as bf16

_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}

# the largest sum |a||b| + |bias| (in units) any caller has checked in this process
largest_bound = 0.0


def ints(shape, lo, hi, seed, scale=1.0, dtype=torch.bfloat16):
    """Integers drawn uniformly from [lo, hi], times ``scale`` (a power of two), as ``dtype``;
    asserts the values are representable (bf16 holds integers up to 256 exactly)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if isinstance(shape, int):
        shape = (shape,)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g).double() * scale
    out = v.to(dtype)
    assert torch.equal(out.double(), v), f"[{lo}, {hi}] x {scale} is not exact in {dtype}"
    return out


def assert_exact_ok(A, B, bias=None, ua=1.0, ub=1.0):
    """``A`` [M, K] and ``B`` [K, N] (as the math sees them) hold integer multiples of the dyadic
    units ``ua`` / ``ub``, ``bias`` [N] of ``ua * ub``; asserts max_mn sum_k |a||b| + |bias| < 2^24
    counted in units of ``ua * ub`` and returns that bound."""
    global largest_bound
    a, b = A.detach().cpu().double() / ua, B.detach().cpu().double() / ub
    assert torch.equal(a, a.round()) and torch.equal(b, b.round()), "operands are not on their grid"
    s = a.abs() @ b.abs()
    if bias is not None:
        c = bias.detach().cpu().double() / (ua * ub)
        assert torch.equal(c, c.round()), "bias is not on the product grid"
        s = s + c.abs()
    bound = float(s.max()) if s.numel() else 0.0
    assert bound < TWO24, f"sum |a||b| + |bias| = {bound} is not below 2^24: fp32 sums may round"
    largest_bound = max(largest_bound, bound)
    return bound


def _fill_bits(t, poison):
    if isinstance(poison, float):
        t.fill_(poison)
    else:
        t.view(_INT_VIEW[t.dtype]).fill_(poison)


def embed(t, pad_rows, pad_cols, poison, pad_right=None):
    """A copy of ``t`` ([rows, cols] or [n]) inside a poisoned buffer with ``pad_rows`` rows
    above and below and ``pad_cols`` elements left (``pad_right``, default the same, right) of
    every row.  Returns ``(buf, view)``; ``poison``: a float value (NaN) or an int bit pattern."""
    pr = pad_cols if pad_right is None else pad_right
    if t.dim() == 1:
        buf = torch.empty(pad_cols + t.numel() + pr, dtype=t.dtype, device=t.device)
        view = buf[pad_cols:pad_cols + t.numel()]
    else:
        r, c = t.shape
        buf = torch.empty(r + 2 * pad_rows, pad_cols + c + pr, dtype=t.dtype, device=t.device)
        view = buf[pad_rows:pad_rows + r, pad_cols:pad_cols + c]
    _fill_bits(buf, poison)
    buf.poison_bits = int(buf.view(_INT_VIEW[t.dtype]).flatten()[0].item())
    view.copy_(t)
    return buf, view


def guards_intact(buf, view):
    """Everything of ``buf`` outside ``view`` still holds the poison, bit for bit."""
    iv = _INT_VIEW[buf.dtype]
    b = buf.clone()
    inner = b.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset())
    pz = torch.full((1,), buf.poison_bits, dtype=iv, device=b.device).view(b.dtype)
    inner.copy_(pz.reshape([1] * view.dim()).expand(view.shape))
    return bool((b.view(iv) == buf.poison_bits).all())


def same(got, want):
    """torch.equal plus dtype and shape: every value identical (a NaN never is; +-0 compare equal,
    the sign of a zero product depends on how act' is associated)."""
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want.cpu())


# ---- float64 oracles (CPU) -------------------------------------------------------------------
def d(t):
    return t.detach().cpu().double()


def act_f64(z, act):
    return torch.relu(z) if act == "relu" else torch.tanh(z) if act == "tanh" else z


def dact_f64(a, act):
    """act' through the activation's OUTPUT a: relu 0 / 1, tanh 1 - a^2."""
    return (a > 0).double() if act == "relu" else 1 - a * a if act == "tanh" else torch.ones_like(a)


def gemm(A, B):
    return d(A) @ d(B)


def preact(x, W, b):
    z = d(x) @ d(W).t()
    return z if b is None else z + d(b)


def fwd(x, W, b, act):
    return act_f64(preact(x, W, b), act)


def dgrad(dz, W, a_prev, act):
    return (d(dz) @ d(W)) * dact_f64(d(a_prev), act)


def wgrad(dz, x):
    return d(dz).t() @ d(x), d(dz).sum(0)


def slab_sum(ws):
    """ws [S, ...]: the sum over the S partial slabs."""
    return d(ws).sum(0)


def f32(t64):
    """float64 -> fp32, asserting nothing is lost (true under the 2^24 precondition)."""
    out = t64.float()
    assert torch.equal(out.double(), t64), "the oracle is not representable in fp32"
    return out


def bf16_rne(t64):
    """The round-to-nearest-even bf16 cast of an fp32-exact float64 oracle."""
    return f32(t64).to(torch.bfloat16)


def bf16_trunc(t64):
    """The truncating cast (negative control: what a kernel that drops the low 16 bits gives)."""
    bits = f32(t64).view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def tanh_grid(shape, seed):
    """tanh outputs on the grid k / 128, |k| <= 128 (bf16-exact): with |dZ . W| <= 1000 the
    product acc (1 - a^2) = acc (16384 - k^2) / 16384 is an integer below 2^24 over 2^14."""
    return ints(shape, -128, 128, seed, scale=2.0 ** -7)


def bf16_ulp_apart(got, want):
    """|got - want| in units of want's bf16 spacing (2^(e - 7)), elementwise, as float64."""
    w = want.double()
    e = torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126)))
    return (got.double() - w).abs() / torch.pow(2.0, e - 7)


def f32_ulp_apart(got, want):
    w = want.double()
    e = torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126)))
    return (got.double() - w).abs() / torch.pow(2.0, e - 23)
