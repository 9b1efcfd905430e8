"""The one-launch tiny-MLP step (csrc/kernels/tiny_mlp.hip) and its host twin
(csrc/host/tiny_host.cpp) against a float64 autograd oracle written here in plain PyTorch.

Every test drives ``ops.tiny_step`` the way the engine does (an Arena built from the layer
shapes, gradients read back from ``arena.grad``): ``HostOps`` on the CPU, ``HipOps`` on the GPU
(those parameters carry the ``gpu`` mark).  Kernel paths, and the test ids that reach them:

* ``tiny_mlp_kernel<ACT_RELU, LOSS_MSE, 1>`` (the 2-3-1 specialisation): ``fix231-*``; with four
  blocks, the slab combine and a ragged last wave in ``fix231-1000rows-4blocks-ragged``.
* ``tiny_mlp_kernel<ACT_RELU, LOSS_MSE, 0>``: ``relu_mse-*``; the grid-stride loop (256 blocks
  x 256 rows, then 300 more rows) in ``relu_mse-6x16x9x2-65836rows-gridstride``; a second block
  holding one row in ``relu_mse-16x16x16x16x16-257rows``; multi-output MSE, four layers and three
  blocks in ``relu_mse-5x9x16x4x2-700rows-3blocks``.
* ``tiny_mlp_kernel<ACT_TANH, LOSS_MSE, 0>``: ``tanh_mse-*`` (``tanh_mse-2x3x1-16rows`` is the
  reference widths on the generic kernel).
* ``tiny_mlp_kernel<ACT_RELU, LOSS_XENT, 0>``: ``relu_xent-*`` (three waves; a single layer).
* ``tiny_mlp_kernel<ACT_TANH, LOSS_XENT, 0>``: ``tanh_xent-7x16x5x3-300rows-2blocks`` (two
  blocks, the multi-block slab combine through ``splitk_reduce`` with M = 1, last wave 44 rows).

Two comparisons.  *Exact*: integer-valued inputs on which every fp32 operation is exact, so the
result must equal the oracle rounded to fp32 bit for bit whatever the summation order (asserted
precondition, from the oracle: every sum of absolute terms / inv_count and the loss sum stay
below 2^24).  *Tolerance*: per gradient tensor, ``max_elem |g - g64| / (2^-24 A)`` with
``A = sum_rows |delta| |a|`` from the oracle, against ``max(64, 8 x`` the same metric of a plain
fp32 PyTorch evaluation of the oracle's formula ``)``; one lost row costs about 2^24 / rows.

Measured metrics (largest over the gradient tensors of the case; fp32 PyTorch reference -> limit;
host twin; MI355X kernel; each tensor is held to its own limit).  The five-layer 16-wide
cross-entropy case is ill-conditioned beyond what A sees (cancellation in the back-propagated
deltas), for the fp32 reference too; the kernel's fast exp is a few ulp wider than libm's there:

    case                                   fp32 ref  limit   host    gpu
    tanh_xent-7x16x5x3-300rows-2blocks          5.20    64.0    5.20    1.07
    relu_mse-5x9x16x4x2-700rows-3blocks        13.52   108.2   11.81    8.14
    relu_xent-16x16x16x16x16-130rows-3waves   296.32  2370.6  143.90 1771.52
    tanh_mse-3x16x1-257rows                     4.20    64.0    4.01    0.54
    relu_xent-11x6-65rows-1layer                1.60    64.0    2.72    0.97
    tanh_mse-2x3x1-16rows                       1.10    64.0    1.36    0.77
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24

BACKENDS = [pytest.param("host", id="host"),
            pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def _ops(backend):
    if backend == "hip":
        from nnmpi_amd.ops.hip_ops import HipOps
        return HipOps("cuda"), torch.device("cuda")
    from nnmpi_amd.ops.host_ops import HostOps
    return HostOps("cpu"), torch.device("cpu")


def _f32(v: float) -> float:
    """The value a float argument has once the binding has narrowed it to fp32."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
class Case:
    def __init__(self, widths, act, loss, rows, Ws, bs, X, y, labels, inv_count):
        self.widths, self.act, self.loss, self.rows = tuple(widths), act, loss, rows
        self.Ws, self.bs, self.X, self.y, self.labels = Ws, bs, X, y, labels
        self.inv_count = _f32(inv_count)

    def replace(self, **kw):
        c = Case(self.widths, self.act, self.loss, self.rows, self.Ws, self.bs, self.X, self.y,
                 self.labels, self.inv_count)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


def _labels(g, rows, out):
    """Random labels in which 0 and out - 1 both appear."""
    lab = torch.randint(0, out, (rows,), generator=g, dtype=torch.int64)
    lab[0] = 0
    lab[rows - 1] = out - 1
    return lab


@functools.lru_cache(maxsize=None)
def exact_case(widths, rows, seed):
    """MSE + ReLU inputs on which fp32 arithmetic is exact: X in {-1, 0, 1}, two non-zeros of
    +-1 per weight row, biases in {-1, 0, 1}, targets in {-3..3}, inv_count = 2^-10."""
    g = torch.Generator().manual_seed(seed)
    Ws, bs = [], []
    for l in range(len(widths) - 1):
        out_f, in_f = widths[l + 1], widths[l]
        W = torch.zeros(out_f, in_f)
        for o in range(out_f):
            cols = torch.randperm(in_f, generator=g)[:2]
            W[o, cols] = torch.randint(0, 2, (len(cols),), generator=g).float() * 2 - 1
        Ws.append(W)
        bs.append(torch.randint(-1, 2, (out_f,), generator=g).float())
    X = torch.randint(-1, 2, (rows, widths[0]), generator=g).float()
    y = torch.randint(-3, 4, (rows, widths[-1]), generator=g).float()
    return Case(widths, "relu", "mse", rows, Ws, bs, X, y, None, 2.0 ** -10)


@functools.lru_cache(maxsize=None)
def random_case(widths, act, loss, rows, seed, last_scale=1.0):
    """Normal inputs: weights scaled 1 / sqrt(fan_in), biases 0.3 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    Ws = [torch.randn(widths[l + 1], widths[l], generator=g) / math.sqrt(widths[l])
          for l in range(len(widths) - 1)]
    Ws[-1] = Ws[-1] * last_scale
    bs = [0.3 * torch.randn(widths[l + 1], generator=g) for l in range(len(widths) - 1)]
    X = torch.randn(rows, widths[0], generator=g)
    out = widths[-1]
    y = torch.randn(rows, out, generator=g) if loss == "mse" else None
    labels = _labels(g, rows, out) if loss == "xent" else None
    inv = 1.0 / rows if loss == "xent" else 1.0 / (rows * out)
    return Case(widths, act, loss, rows, Ws, bs, X, y, labels, inv)


# ------------------------------------------------------------------------------------------
# oracle: plain PyTorch autograd, float64 (dtype=float32: the reference evaluation whose own
# error sets the tolerance)
# ------------------------------------------------------------------------------------------
class Result:
    """loss_sum; gW / gb per layer; with an oracle also A_W / A_b (the same sums with absolute
    terms), dlast (d loss / d logits per row) and min_hidden_z."""


def oracle(c: Case, dtype=torch.float64) -> Result:
    act = torch.relu if c.act == "relu" else torch.tanh
    L = len(c.widths) - 1
    Ws = [W.detach().to(dtype).clone().requires_grad_() for W in c.Ws]
    bs = [b.detach().to(dtype).clone().requires_grad_() for b in c.bs]
    a, ins, zs = c.X.to(dtype), [], []
    for l in range(L):
        ins.append(a)
        z = F.linear(a, Ws[l], bs[l])
        z.retain_grad()
        zs.append(z)
        a = act(z) if l < L - 1 else z
    if c.loss == "mse":
        total = ((a - c.y.to(dtype)) ** 2).sum()
    else:
        total = F.cross_entropy(a, c.labels, reduction="sum")
    (c.inv_count * total).backward()
    r = Result()
    r.loss_sum = total.detach()
    r.gW = [W.grad for W in Ws]
    r.gb = [b.grad for b in bs]
    r.A_W = [zs[l].grad.abs().t() @ ins[l].detach().abs() for l in range(L)]
    r.A_b = [zs[l].grad.abs().sum(0) for l in range(L)]
    r.dlast = zs[-1].grad
    r.logits = zs[-1].detach()
    r.min_hidden_z = min([float(z.detach().abs().min()) for z in zs[:-1]] or [math.inf])
    return r


def manual_f64(c: Case, swap_act_layers=False) -> Result:
    """The same step by hand in float64 (no autograd): equal to the oracle as it stands, and the
    vehicle of the negative controls (``swap_act_layers``: act' of hidden layer 1 taken from
    hidden layer 2 and vice versa, which needs equal hidden widths)."""
    act = torch.relu if c.act == "relu" else torch.tanh
    L = len(c.widths) - 1
    Ws = [W.double() for W in c.Ws]
    a = [c.X.double()]
    for l in range(L):
        z = a[l] @ Ws[l].t() + c.bs[l].double()
        a.append(act(z) if l < L - 1 else z)
    z = a[L]
    r = Result()
    if c.loss == "mse":
        d = z - c.y.double()
        r.loss_sum = (d * d).sum()
        delta = 2.0 * d * c.inv_count
    else:
        lse = torch.logsumexp(z, 1)
        r.loss_sum = (lse - z.gather(1, c.labels.view(-1, 1)).squeeze(1)).sum()
        delta = (torch.softmax(z, 1) - F.one_hot(c.labels, z.shape[1]).double()) * c.inv_count
    r.gW, r.gb = [None] * L, [None] * L
    for l in reversed(range(L)):
        r.gW[l] = delta.t() @ a[l]
        r.gb[l] = delta.sum(0)
        if l > 0:
            src = a[{1: 2, 2: 1}[l]] if swap_act_layers else a[l]
            dact = (src > 0).double() if c.act == "relu" else 1.0 - src * src
            delta = (delta @ Ws[l]) * dact
    return r


@functools.lru_cache(maxsize=None)
def _oracle_of(c: Case) -> Result:
    return oracle(c)


# ------------------------------------------------------------------------------------------
# comparisons: each returns the list of complaints (empty: accepted)
# ------------------------------------------------------------------------------------------
def exact_precondition(o: Result, inv_count: float):
    """A condition on the INPUTS: every partial sum any summation order can form is an integer
    multiple of the unit below 2^24 units, so fp32 represents it exactly."""
    worst = max(float(t.max()) for t in o.A_W + o.A_b) / inv_count
    assert worst < 2 ** 24, f"max(A) / inv_count = {worst:.4g} is not below 2^24"
    assert float(o.loss_sum) < 2 ** 24, f"loss sum {float(o.loss_sum):.4g} is not below 2^24"
    return worst


def compare_exact(got: Result, o: Result, loss_scale=1.0):
    bad = []
    for name, gs, ws in (("gW", got.gW, o.gW), ("gb", got.gb, o.gb)):
        for l, (g, w) in enumerate(zip(gs, ws)):
            g, w = g.detach().cpu().float(), w.float()
            if g.shape != w.shape or not torch.equal(g, w):
                n = int((g != w).sum()) if g.shape == w.shape else -1
                bad.append(f"{name}[{l}]: {n} elements differ from the oracle's fp32 value")
    want = float((o.loss_sum * loss_scale).float())
    if float(got.loss) != want:
        bad.append(f"loss {float(got.loss)!r} != {want!r}")
    return bad


def grad_metric(got: Result, o: Result):
    """Per gradient tensor: max_elem |g - g64| / (2^-24 A); an element whose A is 0 has an exactly
    zero gradient, so any non-zero value there counts as infinite."""
    out = {}
    for name, gs, ws, As in (("gW", got.gW, o.gW, o.A_W), ("gb", got.gb, o.gb, o.A_b)):
        for l, (g, w, A) in enumerate(zip(gs, ws, As)):
            err = (g.detach().cpu().double() - w).abs()
            m = torch.where(A > 0, err / (U24 * A).clamp_min(1e-300),
                            torch.where(err > 0, torch.full_like(err, math.inf),
                                        torch.zeros_like(err)))
            m = torch.where(torch.isnan(m), torch.full_like(m, math.inf), m)
            out[f"{name}[{l}]"] = float(m.max())
    return out


@functools.lru_cache(maxsize=None)
def tolerance_limits(c: Case):
    """max(64, 8 x the metric of the fp32 PyTorch evaluation), per gradient tensor; the factor 8
    covers the different summation trees (sequential rows in the host twin; butterfly, per-wave
    slots, four slots and block slabs on the GPU; blocked in PyTorch)."""
    ref = grad_metric(oracle(c, torch.float32), _oracle_of(c))
    return ref, {k: max(64.0, 8.0 * v) for k, v in ref.items()}


def compare_tolerance(got: Result, c: Case, loss_scale=1.0, report=None):
    o = _oracle_of(c)
    ref, limits = tolerance_limits(c)
    m = grad_metric(got, o)
    if report is not None:
        k = max(m, key=lambda t: m[t] / limits[t])
        print(f"\nTINY_METRIC {report}: worst {k} fp32-ref {ref[k]:.2f} limit {limits[k]:.1f} "
              f"got {m[k]:.2f}; max fp32-ref {max(ref.values()):.2f} max got {max(m.values()):.2f}")
    bad = [f"{k}: metric {m[k]:.1f} > limit {limits[k]:.1f} (fp32 reference {ref[k]:.2f})"
           for k in m if not m[k] <= limits[k]]
    want = float(o.loss_sum) * loss_scale
    rel = abs(float(got.loss) - want) / abs(want)
    if not rel <= c.rows * U24:
        bad.append(f"loss {float(got.loss)!r} vs {want!r}: relative error {rel:.3g} > rows 2^-24")
    return bad


# ------------------------------------------------------------------------------------------
# driver: the same function for both op sets
# ------------------------------------------------------------------------------------------
def make_arena(c: Case, dev, activation=None):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.models.mlp import MLPSpec
    spec = MLPSpec(c.widths, activation or c.act, c.loss)
    arena = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev)
    for l in range(spec.n_layers):
        arena.weight(l).copy_(c.Ws[l])
        arena.bias(l).copy_(c.bs[l])
    return spec, arena


def slot_mask(arena):
    m = torch.zeros(arena.numel, dtype=torch.bool)
    for s in arena.slots:
        m[s.offset:s.offset + s.numel] = True
    return m


def run_step(backend, c: Case, loss_scale=1.0, sgd_hp=None, first=True, momentum=None,
             rows=None, activation=None):
    """One ``ops.tiny_step``: gradients prefilled with 7.0, workspace with NaN.  Returns the
    Result (gradient views, loss) and the arena.  ``sgd_hp``: the in-kernel optimizer update."""
    ops, dev = _ops(backend)
    spec, arena = make_arena(c, dev, activation)
    arena.grad.fill_(7.0)
    if momentum is not None:
        arena.momentum.copy_(momentum)
    n = c.rows if rows is None else len(rows)
    sel = slice(None) if rows is None else rows
    X = c.X[sel].contiguous().to(dev)
    y = c.y[sel].contiguous().to(dev) if c.y is not None else None
    labels = c.labels[sel].contiguous().to(dev) if c.labels is not None else None
    ws = torch.full((ops.tiny_workspace_bytes(n, arena.numel) // 4 + 16,), float("nan"), device=dev)
    loss_out = torch.full((4,), float("nan"), device=dev)
    sgd = None
    if sgd_hp is not None:
        hp = torch.tensor(list(sgd_hp) + [0.0, 0.0, 0.0], device=dev)
        sgd = ops.sgd_fusion(arena, hp, False, first)
    ops.tiny_step(spec, arena, X, y, labels, c.inv_count, loss_out, ws, sgd=sgd,
                  loss_scale=loss_scale)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    r = Result()
    r.gW = [arena.grad_weight(l) for l in range(spec.n_layers)]
    r.gb = [arena.grad_bias(l) for l in range(spec.n_layers)]
    r.loss = loss_out[0].cpu()
    r.loss_tail = loss_out[1:].cpu()
    return r, arena


def check_arena_written(arena):
    """Every 7.0 sentinel of the model's arena region (here: the whole arena) was overwritten --
    the alignment gaps between the tensors with zeros -- and nothing of the NaN workspace leaked."""
    g = arena.grad.cpu()
    assert torch.isfinite(g).all(), "non-finite gradient (NaN workspace leaked?)"
    assert not (g == 7.0).any(), "a 7.0 sentinel survived inside the model's arena region"
    assert torch.count_nonzero(g[~slot_mask(arena)]) == 0, "alignment gaps must be written as 0"


# ------------------------------------------------------------------------------------------
# exact cases
# ------------------------------------------------------------------------------------------
EXACT = [
    pytest.param((6, 16, 9, 2), 65836, 0, id="relu_mse-6x16x9x2-65836rows-gridstride"),
    pytest.param((2, 3, 1), 1000, 0, id="fix231-1000rows-4blocks-ragged"),
    pytest.param((2, 3, 1), 1, 0, id="fix231-1row"),
    pytest.param((2, 3, 1), 16, 0, id="fix231-16rows"),
    pytest.param((16, 16, 16, 16, 16), 257, 0, id="relu_mse-16x16x16x16x16-257rows"),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("widths,rows,seed", EXACT)
def test_exact_inputs_equal_the_oracle_bit_for_bit(widths, rows, seed, backend):
    """MSE + ReLU on inputs where all fp32 arithmetic is exact: any dropped, duplicated or
    mis-masked row changes bits.  (relu'(0) = 0 in torch and in the kernels, so exact zeros in
    the pre-activations are fine.)"""
    c = exact_case(widths, rows, seed)
    o = _oracle_of(c)
    worst = exact_precondition(o, c.inv_count)
    got, arena = run_step(backend, c, loss_scale=1.0)
    print(f"\nTINY_EXACT {widths} {rows} rows: max(A)/inv_count {worst:.4g}, loss sum "
          f"{float(o.loss_sum):.4g} (< 2^24 = {2 ** 24})")
    assert compare_exact(got, o) == []
    g = arena.grad.cpu()
    assert torch.count_nonzero(g[~slot_mask(arena)]) == 0, "alignment gaps must be written as 0"
    assert torch.isnan(got.loss_tail).all(), "only loss_out[0] is the kernel's to write"


# ------------------------------------------------------------------------------------------
# tolerance cases
# ------------------------------------------------------------------------------------------
TOLERANCE = [
    pytest.param((7, 16, 5, 3), "tanh", "xent", 300, 0, id="tanh_xent-7x16x5x3-300rows-2blocks"),
    pytest.param((5, 9, 16, 4, 2), "relu", "mse", 700, 0, id="relu_mse-5x9x16x4x2-700rows-3blocks"),
    pytest.param((16, 16, 16, 16, 16), "relu", "xent", 130, 0,
                 id="relu_xent-16x16x16x16x16-130rows-3waves"),
    pytest.param((3, 16, 1), "tanh", "mse", 257, 0, id="tanh_mse-3x16x1-257rows"),
    pytest.param((11, 6), "relu", "xent", 65, 0, id="relu_xent-11x6-65rows-1layer"),
    pytest.param((2, 3, 1), "tanh", "mse", 16, 0, id="tanh_mse-2x3x1-16rows"),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("widths,act,loss,rows,seed", TOLERANCE)
def test_random_inputs_within_the_fp32_reference_tolerance(widths, act, loss, rows, seed, backend,
                                                           request):
    c = random_case(widths, act, loss, rows, seed)
    o = _oracle_of(c)
    # conditions on the inputs: no ReLU on its kink, both extreme labels present
    assert o.min_hidden_z > 1e-5, f"a hidden pre-activation sits at {o.min_hidden_z:.3g}: other seed"
    if loss == "xent":
        assert 0 in c.labels and widths[-1] - 1 in c.labels
    got, arena = run_step(backend, c, loss_scale=1.0)
    check_arena_written(arena)
    assert compare_tolerance(got, c, report=request.node.name) == []
    # loss_scale=None: the mean over these rows (and outputs, for MSE)
    mean, _ = run_step(backend, c, loss_scale=None)
    want = float(o.loss_sum) / (rows if loss == "xent" else rows * widths[-1])
    assert abs(float(mean.loss) - want) <= rows * U24 * abs(want)
    # an explicit loss_scale: exactly sum * loss_scale (a power of two: no rounding)
    eighth, _ = run_step(backend, c, loss_scale=0.125)
    assert float(eighth.loss) == float(got.loss) * 0.125


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("widths,rows", [pytest.param((11, 6), 65, id="relu_xent-11x6-65rows"),
                                         pytest.param((16, 16, 16, 16, 16), 130,
                                                      id="relu_xent-16x16x16x16x16-130rows")])
def test_cross_entropy_at_large_logits(widths, rows, backend):
    """Last layer's weights x 40, logits beyond +-60: everything stays finite, and each row's
    d loss / d logits sums to 0 within out 2^-23 inv_count -- read from the last layer's bias
    gradient of one-row steps (one row: the bias gradient IS that row's delta).  A softmax that
    does not subtract the row maximum overflows here; one normalised through a rounded
    log-sum-exp, exp(z - lse), misses the sum by |lse| 2^-24."""
    c = random_case(widths, "relu", "xent", rows, 0, 40.0)
    o = _oracle_of(c)
    assert float(o.logits.max()) > 60 and float(o.logits.min()) < -60
    got, arena = run_step(backend, c, loss_scale=1.0)
    check_arena_written(arena)
    assert math.isfinite(float(got.loss))
    assert abs(float(got.loss) - float(o.loss_sum)) <= rows * U24 * float(o.loss_sum)
    out = widths[-1]
    worst = 0.0
    for r in range(rows):
        one, _ = run_step(backend, c, rows=[r])
        gb = one.gb[-1].cpu().double()
        assert torch.isfinite(gb).all() and math.isfinite(float(one.loss))
        worst = max(worst, abs(float(gb.sum())) / (out * 2.0 ** -23 * c.inv_count))
    print(f"\nTINY_ROWSUM {backend}: max |sum_o delta_o| / (out 2^-23 inv_count) = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------
# in-kernel SGD
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_in_kernel_sgd(first, backend):
    """The optimizer update inside the step (7-16-5-3 tanh / cross-entropy, 200 rows: one block)
    against torch.optim.SGD in float64 on the oracle gradient, and bitwise against the un-fused
    step followed by the separate optimizer pass.  lr = 1: the momentum buffer takes the
    gradient's error with coefficient 1, the master weights with coefficient lr, so lr times the
    gradient tolerance bounds both only for lr >= 1."""
    lr, mom, damp, wd = 1.0, 0.9, 0.0, 1e-2
    c = random_case((7, 16, 5, 3), "tanh", "xent", 200, 1)
    o = _oracle_of(c)
    ops, dev = _ops(backend)
    assert ops.tiny_can_fuse_sgd(200)
    _, probe = make_arena(c, "cpu")
    mask = slot_mask(probe)
    g = torch.Generator().manual_seed(5)
    m0 = torch.where(mask, 0.1 * torch.randn(probe.numel, generator=g), torch.zeros(probe.numel))
    hp = [lr, mom, damp, wd, 1.0]
    _, fused = run_step(backend, c, sgd_hp=hp, first=first, momentum=m0)
    # un-fused: the same step, then the optimizer pass of the same op set's native library
    _, plain = run_step(backend, c, momentum=m0)
    hpt = torch.tensor(hp + [0.0, 0.0, 0.0], device=dev)
    if backend == "hip":
        ops.sgd(plain, hpt, False, first, zero_grad=False)
        torch.cuda.synchronize()
    else:
        ops.lib.sgd_momentum_host(plain.master.data_ptr(), plain.grad.data_ptr(),
                                  plain.momentum.data_ptr(), plain.numel, hpt.data_ptr(), 0,
                                  int(first), 0)
    assert torch.equal(fused.master, plain.master)
    assert torch.equal(fused.momentum, plain.momentum)
    # float64 torch.optim.SGD on the oracle gradient, in the arena's layout
    g64, A = torch.zeros(probe.numel, dtype=torch.float64), torch.zeros(probe.numel, dtype=torch.float64)
    lim = torch.zeros(probe.numel, dtype=torch.float64)
    _, limits = tolerance_limits(c)
    for l in range(len(c.widths) - 1):
        for kind, gs, As, view in (("gW", o.gW, o.A_W, probe.weight), ("gb", o.gb, o.A_b, probe.bias)):
            view(l, g64).copy_(gs[l])
            view(l, A).copy_(As[l])
            view(l, lim).fill_(limits[f"{kind}[{l}]"])
    p = torch.nn.Parameter(probe.master.double())
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, dampening=damp, weight_decay=wd)
    if not first:
        opt.state[p]["momentum_buffer"] = m0.double()
    p.grad = g64
    opt.step()
    tol_g = lim * U24 * A
    for name, got, want in (("master", fused.master, p.detach()),
                            ("momentum", fused.momentum, opt.state[p]["momentum_buffer"])):
        err = (got.cpu().double() - want).abs()
        tol = lr * tol_g + 2.0 ** -23 * want.abs()
        assert (err <= tol).all(), f"{name}: max err/tol {float((err / tol.clamp_min(1e-300)).max()):.2f}"


@pytest.mark.gpu
def test_sgd_fusion_needs_the_single_block_form():
    """257 rows are two blocks: the launcher refuses the in-kernel update (before any launch)."""
    ops, _ = _ops("hip")
    assert ops.tiny_can_fuse_sgd(256)
    assert not ops.tiny_can_fuse_sgd(257)
    c = random_case((7, 16, 5, 3), "tanh", "xent", 257, 0)
    with pytest.raises(RuntimeError, match="tiny_mlp_step"):
        run_step("hip", c, sgd_hp=[0.1, 0.9, 0.0, 0.0, 1.0])


def test_optimizer_fusion_is_the_op_sets_tuple():
    """Sgd.fusion (engine/optimizer.py), the only source of the fused-update operands the
    engine and the bucket pipeline use: entry for entry ops.sgd_fusion over the object's own
    arena / hyper-parameters / nesterov flag; at an offset of 64 elements the three fp32 pointers
    (gradient, master, momentum) advance by 4 * 64 bytes, the absent shadow stays 0 and the
    hyper-parameter pointer and the flags stay."""
    from nnmpi_amd.engine.optimizer import adam_hparams, make_optimizer, sgd_hparams
    ops, dev = _ops("host")
    _, arena = make_arena(random_case((2, 3, 1), "relu", "mse", 16, 0), dev)
    assert arena.numel > 64
    hp = sgd_hparams(0.1, 0.9, 0.0, 0.0, dev)
    for nesterov in (False, True):
        opt = make_optimizer("sgd", ops, arena, hp, nesterov)
        for first in (True, False):
            base = ops.sgd_fusion(arena, hp, nesterov, first)
            assert opt.fusion(first) == base
            assert base == (arena.grad.data_ptr(), arena.master.data_ptr(),
                            arena.momentum.data_ptr(), 0, hp.data_ptr(), int(nesterov), int(first))
            moved = opt.fusion(first, offset=64)
            assert moved == ops.sgd_fusion(arena, hp, nesterov, first, 64)
            assert [m - b for m, b in zip(moved, base)] == [4 * 64] * 3 + [0] * 4
    adam = make_optimizer("adam", ops, arena, adam_hparams(0.1, 0.9, 0.999, 1e-8, 0.0, dev))
    assert not adam.fusable
    with pytest.raises(RuntimeError, match="fused"):
        adam.fusion(True)


# ------------------------------------------------------------------------------------------
# activation code 0 ("none")
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_activation_none_is_refused_with_hidden_layers(backend):
    """Neither twin has an identity hidden layer to run: both launchers refuse the description
    (the GPU one used to run ReLU silently).  A single-layer model has no hidden activation and
    keeps working whatever the code."""
    c = random_case((2, 3, 1), "tanh", "mse", 16, 0)
    with pytest.raises(RuntimeError, match="tiny_mlp_step"):
        run_step(backend, c, activation="none")
    one = random_case((11, 6), "relu", "xent", 65, 0)
    got, arena = run_step(backend, one, activation="none")
    check_arena_written(arena)
    assert compare_tolerance(got, one) == []


# ------------------------------------------------------------------------------------------
# negative controls (CPU only, no kernel): the comparisons above reject wrong computations
# ------------------------------------------------------------------------------------------
def _as_got(r: Result, loss_scale=1.0) -> Result:
    g = Result()
    g.gW = [t.float() for t in r.gW]
    g.gb = [t.float() for t in r.gb]
    g.loss = (r.loss_sum * loss_scale).float()
    return g


def _drop_last_row(c: Case) -> Case:
    return c.replace(X=c.X[:-1], y=None if c.y is None else c.y[:-1],
                     labels=None if c.labels is None else c.labels[:-1])


def _swap_two_labels(c: Case) -> Case:
    lab = c.labels.clone()
    j = int((lab != lab[0]).nonzero()[0])
    lab[0], lab[j] = c.labels[j], c.labels[0]
    return c.replace(labels=lab)


WRONG = {
    "last_row_dropped": lambda c: manual_f64(_drop_last_row(c)),
    "act_derivative_from_the_wrong_layer": lambda c: manual_f64(c, swap_act_layers=True),
    "two_labels_swapped": lambda c: manual_f64(_swap_two_labels(c)),
    "inv_count_off_by_rows_over_rows_plus_1": lambda c: manual_f64(
        c.replace(inv_count=c.inv_count * c.rows / (c.rows + 1))),
}


def test_the_comparisons_accept_a_correct_computation():
    ce = exact_case((5, 8, 8, 3), 300, 0)
    exact_precondition(_oracle_of(ce), ce.inv_count)
    assert compare_exact(_as_got(manual_f64(ce)), _oracle_of(ce)) == []
    for c in (ce, random_case((5, 8, 8, 3), "tanh", "xent", 300, 0)):
        assert compare_tolerance(_as_got(manual_f64(c)), c) == []


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_the_comparisons_reject_a_wrong_computation(wrong):
    """Each deliberately wrong float64 computation is rejected by the exact comparison (on the
    exact inputs; the label swap, which needs labels, on the cross-entropy inputs) and by the
    tolerance comparison."""
    ce = exact_case((5, 8, 8, 3), 300, 0)
    cx = random_case((5, 8, 8, 3), "tanh", "xent", 300, 0)
    cm = random_case((5, 8, 8, 3), "relu", "mse", 300, 0)
    if wrong == "two_labels_swapped":
        bad = _as_got(WRONG[wrong](cx))
        assert compare_exact(bad, _oracle_of(cx)) != []
        assert compare_tolerance(bad, cx) != []
        return
    exact_precondition(_oracle_of(ce), ce.inv_count)
    assert compare_exact(_as_got(WRONG[wrong](ce)), _oracle_of(ce)) != []
    for c in (cx, cm):
        assert compare_tolerance(_as_got(WRONG[wrong](c)), c) != []
