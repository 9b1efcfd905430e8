"""head_eval (csrc/kernels/head_eval.hip), the forward-only output layer, against a float64 oracle.

Exact-integer idiom of tests/_exact.py: activations, weights and bias are small integers (or
dyadic multiples) with sum |a||w| + |b| < 2^24, so every logit is exact in fp32 in any summation
order, and logits, predictions, ``correct``, the MSE ``loss_sum`` and ``abs_err_sum`` must equal
the oracle EXACTLY.  Inputs sit in NaN-poisoned buffers, outputs in sentinel buffers whose guards
are compared bit for bit.

Dispatch boundaries of the kernel covered here (one case on each side):
  8-wide forms by in / 8 chunks: <= 64 (16 waves x 2 rows), <= 128 (8 x 4), <= 256 (4 x 2),
  <= 1024 (4 x 1)            -> in = 512 | 520, 1024 | 1032, 2048 | 2056, 8192 | 8200 (refused)
  scalar forms (fp32, in % 8 != 0 or unaligned rows) by in: <= 64 (8 x 4), <= 512 (8 x 2),
  <= 8192 (4 x 1)            -> in = 64 | 65, 512 | 513
  output tile: min(16, out, 16384 / in) -> out = 16 | 17; in = 1024 | 1032 (16 | 15 per tile)
  matrix-core form (bf16, in 512 / 1024, 2 <= out <= 16, 16-byte aligned W; 16 rows per
  block-iteration)           -> its own cases, and one step outside each of its conditions
  grid: 256 blocks           -> rows above 256 x rows-per-block of every form

Cross-entropy ``loss_sum`` is the one inexact quantity (device exp / log); errors measured on
the MI355X are recorded in test_xent_loss_vs_training_head's docstring.
"""
import pytest
import torch

import _exact as ex

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRED_SENTINEL = 0x5A5A5A5A
BIG_LABEL = 2 ** 32 + 3      # must not alias to class 3


def _ops():
    from nnmpi_amd.ops.hip_ops import HipOps
    return HipOps(torch.device(DEV))


class Case:
    """Integer operands on the device inside poisoned buffers, and their float64 logits."""

    def __init__(self, rows, in_f, out, bf16, seed, unaligned=False, w_scale=1.0, a_hi=3, w_pad=5):
        dt = torch.bfloat16 if bf16 else torch.float32
        self.rows, self.in_f, self.out, self.bf16 = rows, in_f, out, bf16
        self.a = ex.ints((rows, in_f), -a_hi, a_hi, seed, dtype=dt)
        self.W = ex.ints((out, in_f), -2, 2, seed + 1, scale=w_scale, dtype=torch.float32)
        self.b = ex.ints(out, -5, 5, seed + 2, scale=w_scale, dtype=torch.float32)
        self.w_scale = w_scale
        self.pad = 3 if unaligned else 8
        self.w_pad = w_pad            # elements before W in its buffer: 5 -> W off the 16-byte grid
        self.upload()

    def upload(self):
        """(Re)build the device buffers and the oracle from self.a / W / b."""
        if self.rows:
            ex.assert_exact_ok(torch.nan_to_num(self.a.float(), 0.0, 0.0, 0.0), self.W.t(), self.b,
                               ub=self.w_scale)
        self.z = ex.preact(self.a, self.W, self.b)            # float64 [rows, out]
        self.abuf, self.av = ex.embed(self.a.to(DEV), 1, self.pad, ex.NAN)
        self.wbuf, wv = ex.embed(self.W.reshape(-1).to(DEV), 0, self.w_pad, ex.NAN)
        self.wv = wv.view(self.out, self.in_f)
        self.bbuf, self.bv = ex.embed(self.b.to(DEV), 0, 3, ex.NAN)

    def outputs(self):
        rows, out = self.rows, self.out
        lbuf, lv = ex.embed(torch.zeros(rows, out, dtype=torch.float32, device=DEV), 1, 3,
                            ex.SENTINEL_F32)
        pbuf = torch.full((rows + 8,), PRED_SENTINEL, dtype=torch.int32, device=DEV)
        return lbuf, lv, pbuf, pbuf[4:4 + rows]

    def form(self, ops):
        """The kernel form this case runs: 0 scalar VALU, 1 16-byte VALU, 2 matrix cores."""
        return ops.lib.head_eval_form(self.av.data_ptr(), int(self.bf16), self.av.stride(0), self.in_f,
                                      self.out, self.wv.data_ptr())

    def ws(self, ops):
        n = ops.head_eval_workspace_bytes(self.rows, self.in_f, self.out) // 4 + 16
        return torch.full((n,), ex.NAN, dtype=torch.float32, device=DEV)


def pred_guards_ok(pbuf, rows):
    g = torch.cat([pbuf[:4], pbuf[4 + rows:]]).cpu()
    return bool((g == PRED_SENTINEL).all())


def xent_oracle(z, labels):
    """(per-row loss, per-row lse) in float64; a label outside [0, out) contributes a zero logit."""
    out = z.shape[1]
    lab = labels.cpu().view(-1)
    ok = (lab >= 0) & (lab < out)
    zl = z.gather(1, lab.clamp(0, out - 1).view(-1, 1)).squeeze(1)
    zl = torch.where(ok, zl, torch.zeros_like(zl))
    lse = torch.logsumexp(z, dim=1)
    return lse - zl, lse


def xent_tol(z, labels):
    """Bound on |device loss_sum - oracle| from the number formats: per row, lse = m + log(s) and
    lse - z_label are one fp32 rounding each (2^-24 of their magnitudes; 2^-22 allows the online
    rescale's extra roundings), log(s) with s in [1, out] carries the fast exp / log routines'
    few-ulp errors (each term's exp error is |x| 2^-24 of a term <= 1/e: (out + 16) 2^-24
    in all).  The double-precision sum over rows adds nothing visible."""
    per, lse = xent_oracle(z, labels)
    return float((2.0 ** -22 * (lse.abs() + per.abs()) + (z.shape[1] + 16) * 2.0 ** -24).sum())


def check_case(c, loss, seed, form):
    """One call with every output; everything exact but the cross-entropy loss_sum."""
    ops = _ops()
    assert c.form(ops) == form, "the case does not reach the kernel form it is meant for"
    rows, out = c.rows, c.out
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.full((4,), ex.NAN, dtype=torch.float64, device=DEV)   # stale slots
    want_pred = torch.argmax(c.z, dim=1)
    y = labels = None
    if loss == "mse":
        # integer targets near the logits: per-row sum (z - y)^2 < 2^24, exact in fp32
        y64 = c.z + ex.ints((rows, out), -3, 3, seed + 7, scale=c.w_scale, dtype=torch.float64)
        assert float(((c.z - y64) ** 2).sum(1).max()) / c.w_scale ** 2 < ex.TWO24
        ybuf, yflat = ex.embed(ex.f32(y64).reshape(-1).to(DEV), 0, 3, ex.NAN)
        y = yflat.view(rows, out)
    elif loss == "xent":
        g = torch.Generator().manual_seed(seed + 9)
        labels = torch.where(torch.rand(rows, generator=g) < 0.5, want_pred,
                             torch.randint(0, out, (rows,), generator=g)).to(DEV)
    ops.head_eval(c.av, c.wv, c.bv, y, labels, loss, logits_out=lv, pred_out=pv, metrics=metrics,
                  ws=c.ws(ops))
    torch.cuda.synchronize()
    assert ex.same(lv, ex.f32(c.z)), "logits are not the float64 oracle"
    assert ex.guards_intact(lbuf, lv) and pred_guards_ok(pbuf, rows)
    assert ex.guards_intact(c.abuf, c.av) and ex.guards_intact(c.wbuf, c.wv.reshape(-1))
    assert torch.equal(pv.cpu().long(), want_pred), "predictions differ from torch.argmax"
    m = metrics.cpu()
    assert m[3].item() == rows
    if loss == "mse":
        d = c.z - y64
        assert m[0].item() == float((d * d).sum()) and m[2].item() == float(d.abs().sum())
        assert m[1].item() == 0.0
    elif loss == "xent":
        per, _ = xent_oracle(c.z, labels)
        assert m[1].item() == float((want_pred == labels.cpu()).sum())
        assert m[2].item() == 0.0
        err, tol = abs(m[0].item() - float(per.sum())), xent_tol(c.z, labels)
        print(f"xent loss_sum error {err:.3e} (bound {tol:.3e}, sum {float(per.sum()):.6e})")
        assert err <= tol
    else:
        assert m[:3].tolist() == [0.0, 0.0, 0.0]


# (rows, in, out, bf16, loss, unaligned)
CASES = [
    # bf16, 8-wide forms
    (1, 8, 1, True, "mse", False),
    (15, 24, 3, True, "xent", False),
    (15, 24, 37, True, "xent", False),
    (16, 512, 10, True, "xent", False),
    (17, 520, 16, True, "mse", False),
    (33, 1024, 17, True, "xent", False),
    (777, 1032, 10, True, "xent", False),
    (16, 2048, 37, True, "mse", False),
    (777, 2056, 37, True, "xent", False),
    (33, 8192, 100, True, "mse", False),
    (5000, 8, 100, True, "xent", False),
    # above a full grid of each 8-wide form (256 blocks x 32 / 32 / 8 / 4 rows)
    (8209, 8, 17, True, "xent", False),
    (8209, 1024, 10, True, "xent", False),
    (2065, 2048, 3, True, "mse", False),
    (1029, 8192, 17, True, "xent", False),
    # fp32: the 8-wide forms on aligned rows
    (16, 16, 16, False, "mse", False),
    (777, 512, 10, False, "xent", False),
    # fp32: the scalar forms (in % 8 != 0, or rows that are not 16-byte aligned)
    (17, 2, 1, False, "mse", False),
    (33, 3, 1, False, "mse", False),
    (15, 7, 10, False, "xent", False),
    (16, 16, 3, False, "xent", True),
    (33, 64, 17, False, "xent", True),
    (33, 65, 3, False, "mse", False),
    (17, 512, 10, False, "xent", True),
    (15, 513, 37, False, "mse", False),
    (8209, 3, 1, False, "mse", False),
    (4113, 100, 10, False, "xent", False),
    (1029, 520, 17, False, "xent", True),
]


@pytest.mark.parametrize("rows,in_f,out,bf16,loss,unaligned", CASES)
def test_exact(rows, in_f, out, bf16, loss, unaligned):
    seed = rows * 7 + in_f * 3 + out
    vec = in_f % 8 == 0 and not unaligned
    check_case(Case(rows, in_f, out, bf16, seed, unaligned=unaligned), loss, seed, 1 if vec else 0)


# the matrix-core form: bf16 rows of 512 / 1,024 features, 2 <= out <= 16, W on the 16-byte grid;
# 16-row groups (partial last group: 1, 15, 17 rows), above its full grid (256 blocks x 16 rows)
MFMA_CASES = [(1, 512, 2, "xent"), (15, 1024, 10, "xent"), (16, 512, 10, "mse"),
              (17, 1024, 16, "mse"), (33, 512, 13, "xent"), (777, 1024, 10, "xent"),
              (5000, 512, 3, "mse"), (8209, 1024, 10, "xent"), (4113, 512, 16, "xent")]


@pytest.mark.parametrize("rows,in_f,out,loss", MFMA_CASES)
def test_exact_mfma_form(rows, in_f, out, loss):
    seed = rows * 5 + in_f + out
    check_case(Case(rows, in_f, out, True, seed, w_pad=4), loss, seed, 2)


def test_mfma_form_boundaries():
    """One step outside each condition of the matrix-core form runs a VALU form instead."""
    ops = _ops()
    assert Case(16, 512, 16, True, 1, w_pad=4).form(ops) == 2
    assert Case(16, 512, 17, True, 1, w_pad=4).form(ops) == 1      # out > 16
    assert Case(16, 512, 1, True, 1, w_pad=4).form(ops) == 1       # out == 1
    assert Case(16, 520, 10, True, 1, w_pad=4).form(ops) == 1      # another width
    assert Case(16, 512, 10, True, 1, w_pad=5).form(ops) == 1      # W off the 16-byte grid
    assert Case(16, 512, 10, False, 1, w_pad=4).form(ops) == 1     # fp32 rows


def _mfma_tie_case():
    """All-ones rows against random {-1, 0, 1} weights, outputs 3 and 13 (different lanes of the
    logit tile) both 2 x 512: the row maximum twice.  Row 7 has a NaN activation, row 33 a +inf
    against a weight column [1, 0, 1, 0, ...]: logits [inf, nan, inf, nan, ...]."""
    rows, in_f, out = 40, 512, 14
    c = Case(rows, in_f, out, True, 71, w_pad=4, a_hi=1)
    c.a = torch.ones(rows, in_f, dtype=torch.bfloat16)
    c.W = c.W.clamp(-1, 1)
    c.W[3] = 2.0
    c.W[13] = 2.0
    c.W[:, 9] = (torch.arange(out) % 2 == 0).float()
    c.W[3, 9] = c.W[13, 9] = 1.0
    c.b.zero_()
    return c


def test_mfma_form_ties_nan_labels():
    """The matrix-core form's argmax merge: equal maxima across lanes (3, 13) and inside one
    lane's four outputs (4, 5) -> the lowest index; a NaN beats every number, the first NaN
    wins; out-of-range labels count as wrong rows."""
    c = _mfma_tie_case()
    rows, out = c.rows, c.out
    c.a[7, 5] = float("nan")
    c.a[33, 9] = float("inf")
    c.upload()
    want = torch.argmax(c.z, 1)
    assert want[0].item() == 3 and want[7].item() == 0 and want[33].item() == 1
    assert torch.equal(c.z[0, 3], c.z[0, 13])
    labels = want.clone()
    labels[10:14] = torch.tensor([-1, out, BIG_LABEL, 13])
    labels = labels.to(DEV)
    ops = _ops()
    assert c.form(ops) == 2
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", logits_out=lv, pred_out=pv,
                  metrics=metrics, ws=c.ws(ops))
    torch.cuda.synchronize()
    assert torch.equal(pv.cpu().long(), want)
    got = lv.cpu().double()
    fin = c.z.isfinite().all(1)
    assert int(fin.sum()) == rows - 2 and torch.equal(got[fin], c.z[fin])
    assert bool(got[7].isnan().all()) and torch.equal(got[33].isnan(), c.z[33].isnan())
    assert torch.equal(got[33][::2], c.z[33][::2])
    m = metrics.cpu()
    assert m[0].isnan().item() and m[1].item() == float(rows - 4) and m[3].item() == rows
    assert ex.guards_intact(lbuf, lv) and pred_guards_ok(pbuf, rows)
    assert ex.guards_intact(c.wbuf, c.wv.reshape(-1)) and ex.guards_intact(c.abuf, c.av)
    # a tie inside one lane's outputs: 4 and 5 become the (equal) maxima
    c = _mfma_tie_case()
    c.W[3] = -1.0
    c.W[13] = -1.0
    c.W[4] = 1.0
    c.W[5] = 1.0
    c.upload()
    want = torch.argmax(c.z, 1)
    assert want.tolist() == [4] * rows and torch.equal(c.z[:, 4], c.z[:, 5])
    _, _, pbuf, pv = c.outputs()
    ops.head_eval(c.av, c.wv, c.bv, pred_out=pv)
    torch.cuda.synchronize()
    assert torch.equal(pv.cpu().long(), want) and pred_guards_ok(pbuf, rows)


@pytest.mark.parametrize("hit36", [False, True])
def test_ties_and_labels(hit36):
    """Equal maxima in different tiles (outputs 3 and 19 of 37): the first wins.  Labels on the
    last output of the partial tile (36), and outside [0, out): those rows count as wrong."""
    rows, in_f, out = 40, 8, 37
    c = Case(rows, in_f, out, False, 5)
    c.a = c.a.abs().clamp_min(1.0)
    c.W = c.W.clamp(-1, 1)
    c.W[3] = 2.0
    c.W[19] = 2.0
    if hit36:
        c.W[36] = 3.0
    c.b.zero_()
    c.upload()
    want = 36 if hit36 else 3
    assert torch.equal(torch.argmax(c.z, 1), torch.full((rows,), want))
    assert torch.equal(c.z[:, 3], c.z[:, 19])
    labels = torch.full((rows,), 36, dtype=torch.int64)
    labels[10:20] = 3
    labels[20:25] = -1
    labels[25:30] = out
    labels[30:35] = BIG_LABEL
    labels[35:] = 19
    labels = labels.to(DEV)
    ops = _ops()
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", logits_out=lv, pred_out=pv,
                  metrics=metrics, ws=c.ws(ops))
    torch.cuda.synchronize()
    assert torch.equal(pv.cpu().long(), torch.full((rows,), want))
    assert ex.same(lv, ex.f32(c.z))
    assert ex.guards_intact(c.wbuf, c.wv.reshape(-1)) and ex.guards_intact(c.abuf, c.av)
    assert ex.guards_intact(lbuf, lv) and pred_guards_ok(pbuf, rows)
    per, _ = xent_oracle(c.z, labels)
    m = metrics.cpu()
    assert m[1].item() == float((labels.cpu() == want).sum())
    assert abs(m[0].item() - float(per.sum())) <= xent_tol(c.z, labels)


def test_nan_activation():
    """One NaN activation: that row's prediction is torch.argmax of the float64 logits, loss_sum
    is NaN, every other row stays exact.  A +inf activation against weights [1, 0, 1, 0, ...]
    gives logits [inf, nan, inf, nan, ...]: the first NaN (index 1) wins."""
    rows, in_f, out = 33, 24, 37
    c = Case(rows, in_f, out, True, 11)
    c.W[:, 9] = (torch.arange(out) % 2 == 0).float()
    c.a[7, 5] = float("nan")
    c.a[20, 9] = float("inf")
    c.upload()
    want = torch.argmax(c.z, 1)
    assert want[7].item() == 0 and want[20].item() == 1
    ops = _ops()
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.zeros(4, dtype=torch.float64, device=DEV)
    labels = want.to(DEV)
    ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", logits_out=lv, pred_out=pv,
                  metrics=metrics, ws=c.ws(ops))
    torch.cuda.synchronize()
    assert torch.equal(pv.cpu().long(), want)
    got = lv.cpu().double()
    fin = torch.ones(rows, dtype=torch.bool)
    fin[7] = fin[20] = False
    assert torch.equal(got[fin], c.z[fin])
    assert bool(got[7].isnan().all())
    assert torch.equal(got[20].isnan(), c.z[20].isnan()) and torch.equal(got[20][::2], c.z[20][::2])
    m = metrics.cpu()
    assert m[0].isnan().item() and m[1].item() == float(rows) and m[3].item() == rows
    assert ex.guards_intact(lbuf, lv) and pred_guards_ok(pbuf, rows)


@pytest.mark.parametrize("in_f,out,w_pad", [(520, 17, 5), (512, 10, 4)])
@pytest.mark.parametrize("loss", ["mse", "xent"])
def test_accumulate(loss, in_f, out, w_pad):
    """Two calls over the halves of a batch == one call over the whole; accumulate = 0 overwrites
    stale slots; rows == 0 zeroes them (and leaves them alone under accumulate)."""
    rows = 777
    c = Case(rows, in_f, out, True, 21, w_pad=w_pad)
    ops = _ops()
    assert c.form(ops) == (2 if w_pad == 4 else 1)
    ws = c.ws(ops)
    if loss == "mse":
        y = ex.f32(c.z + ex.ints((rows, out), -3, 3, 3, dtype=torch.float64)).to(DEV)
        labels = None
    else:
        y = None
        labels = torch.argmax(c.z, 1).to(DEV)
        labels[::3] = 0
    whole = torch.full((4,), ex.NAN, dtype=torch.float64, device=DEV)
    ops.head_eval(c.av, c.wv, c.bv, y, labels, loss, metrics=whole, ws=ws)
    parts = torch.full((4,), 123.0, dtype=torch.float64, device=DEV)
    h = 400
    sl = lambda t, a, b: None if t is None else t[a:b]   # noqa: E731
    ops.head_eval(c.av[:h], c.wv, c.bv, sl(y, 0, h), sl(labels, 0, h), loss, metrics=parts, ws=ws)
    ops.head_eval(c.av[h:], c.wv, c.bv, sl(y, h, rows), sl(labels, h, rows), loss, metrics=parts,
                  accumulate=True, ws=ws)
    torch.cuda.synchronize()
    w, p = whole.cpu(), parts.cpu()
    assert p[3].item() == rows and w[3].item() == rows
    assert p[1].item() == w[1].item() and p[2].item() == w[2].item()
    if loss == "mse":
        assert p[0].item() == w[0].item()        # integers: exact in any grouping
    else:
        assert abs(p[0].item() - w[0].item()) <= 2.0 ** -40 * abs(w[0].item())   # double regrouping
    # rows == 0
    empty = c.av[:0]
    ops.head_eval(empty, c.wv, c.bv, sl(y, 0, 0), sl(labels, 0, 0), loss, metrics=parts,
                  accumulate=True, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(parts.cpu(), p)
    ops.head_eval(empty, c.wv, c.bv, sl(y, 0, 0), sl(labels, 0, 0), loss, metrics=parts, ws=ws)
    torch.cuda.synchronize()
    assert parts.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]


def test_no_targets():
    """loss = -1: logits and predictions only; the (poisoned) target pointers are never read."""
    from nnmpi_amd import native
    rows, in_f, out = 33, 1024, 17
    c = Case(rows, in_f, out, True, 31)
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.full((4,), 5.0, dtype=torch.float64, device=DEV)
    y = torch.full((4,), ex.NAN, dtype=torch.float32, device=DEV)        # far too small: unread
    labels = torch.full((2,), 2 ** 40, dtype=torch.int64, device=DEV)
    ops = _ops()
    ws = c.ws(ops)
    ops.lib.head_eval(c.av.data_ptr(), 1, c.av.stride(0), rows, in_f, c.wv.data_ptr(),
                      c.bv.data_ptr(), out, y.data_ptr(), labels.data_ptr(), -1, lv.data_ptr(),
                      lv.stride(0), pv.data_ptr(), metrics.data_ptr(), 0, ws.data_ptr(),
                      native.stream_handle())
    torch.cuda.synchronize()
    assert ex.same(lv, ex.f32(c.z)) and torch.equal(pv.cpu().long(), torch.argmax(c.z, 1))
    assert metrics.cpu().tolist() == [0.0, 0.0, 0.0, float(rows)]
    assert ex.guards_intact(lbuf, lv) and pred_guards_ok(pbuf, rows)
    # through the wrapper, outputs one at a time
    lbuf2, lv2, pbuf2, pv2 = c.outputs()
    ops.head_eval(c.av, c.wv, c.bv, logits_out=lv2)
    ops.head_eval(c.av, c.wv, c.bv, pred_out=pv2)
    torch.cuda.synchronize()
    assert ex.same(lv2, lv) and torch.equal(pv2, pv)


@pytest.mark.parametrize("in_f,out,w_pad", [(512, 10, 5), (24, 10, 5), (1024, 10, 5), (512, 10, 4),
                                            (1024, 10, 4)])
def test_xent_loss_vs_training_head(in_f, out, w_pad):
    """Cross-entropy loss_sum against the float64 oracle, next to the error of the training head
    (ops.head, loss_scale = 1) on the same exact logits: eval error <= max(4 x head error,
    2^-22 x |sum|).  Weights on the 1/8 grid keep the logits exact and of order one, so exp / log
    matter.  Measured on the MI355X (eval error | training-head error | sum):
      in  512, VALU form:         9.862e-06 | 6.672e-05 | 4192.732
      in   24, VALU form:         4.148e-05 | 5.924e-05 | 2037.883
      in 1024, VALU form:         9.804e-06 | 2.635e-04 | 5768.506
      in  512, matrix-core form:  8.908e-06 | 6.672e-05 | 4192.732
      in 1024, matrix-core form:  9.566e-06 | 2.635e-04 | 5768.506
    """
    rows = 777
    c = Case(rows, in_f, out, True, 41, w_scale=2.0 ** -3, a_hi=1, w_pad=w_pad)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, out, (rows,), generator=g).to(DEV)
    per, _ = xent_oracle(c.z, labels)
    want = float(per.sum())
    ops = _ops()
    metrics = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", metrics=metrics, ws=c.ws(ops))
    a = c.av.contiguous()
    gW = torch.zeros(out, in_f, dtype=torch.float32, device=DEV)
    gb = torch.zeros(out, dtype=torch.float32, device=DEV)
    dl = torch.zeros(rows, out, dtype=torch.float32, device=DEV)
    loss_out = torch.zeros(4, dtype=torch.float32, device=DEV)
    ws = torch.zeros(ops.head_workspace_bytes(rows, in_f, out) // 4 + 64, dtype=torch.float32,
                     device=DEV)
    ops.head(a, c.wv.contiguous(), c.bv.contiguous(), None, labels, "xent", 0.0, "relu", None, gW,
             gb, dl, loss_out, 1.0, ws=ws)
    torch.cuda.synchronize()
    e_eval = abs(metrics[0].item() - want)
    e_head = abs(float(loss_out[0].item()) - want)
    print(f"in {in_f} form {c.form(ops)}: eval error {e_eval:.3e}, training-head error {e_head:.3e}, "
          f"sum {want:.6e}")
    assert e_eval <= max(4.0 * e_head, 2.0 ** -22 * abs(want))


@pytest.mark.parametrize("w_pad", [5, 4])
def test_deterministic(w_pad):
    rows, in_f, out = 5000, 1024, 10
    c = Case(rows, in_f, out, True, 51, w_scale=2.0 ** -3, a_hi=1, w_pad=w_pad)
    labels = torch.argmax(c.z, 1).to(DEV)
    labels[::2] = 1
    ops = _ops()
    got = []
    for _ in range(2):
        metrics = torch.full((4,), ex.NAN, dtype=torch.float64, device=DEV)
        ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", metrics=metrics, ws=c.ws(ops))
        torch.cuda.synchronize()
        got.append(metrics.cpu().view(torch.int64).tolist())
    assert got[0] == got[1]


def test_refusals():
    """Everything the kernel does not take is refused before a launch: the sentinel outputs and
    the metrics stay untouched."""
    from nnmpi_amd import native
    rows, in_f, out = 16, 24, 5
    c = Case(rows, in_f, out, True, 61)
    cf = Case(rows, in_f, out, False, 62)
    ops = _ops()
    lib = ops.lib
    lbuf, lv, pbuf, pv = c.outputs()
    metrics = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    ws = c.ws(ops)
    y = torch.zeros(rows, out, dtype=torch.float32, device=DEV)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    good = dict(a=c.av.data_ptr(), a_bf16=1, lda=c.av.stride(0), rows=rows, in_f=in_f,
                W=c.wv.data_ptr(), b=c.bv.data_ptr(), out=out, y=y.data_ptr(),
                labels=labels.data_ptr(), loss=1, logits=lv.data_ptr(), ldl=lv.stride(0),
                pred=pv.data_ptr(), metrics=metrics.data_ptr(), accumulate=0, ws=ws.data_ptr())

    def call(**over):
        k = dict(good, **over)
        lib.head_eval(k["a"], k["a_bf16"], k["lda"], k["rows"], k["in_f"], k["W"], k["b"], k["out"],
                      k["y"], k["labels"], k["loss"], k["logits"], k["ldl"], k["pred"],
                      k["metrics"], k["accumulate"], k["ws"], native.stream_handle())

    bad = [dict(a=0), dict(W=0), dict(b=0), dict(ldl=out - 1), dict(lda=in_f - 1), dict(rows=-1),
           dict(in_f=8200, lda=8200), dict(in_f=0), dict(out=0), dict(ws=0), dict(labels=0),
           dict(loss=0, y=0), dict(loss=7),
           dict(a=c.av.data_ptr() + 2),                       # bf16 rows off the 16-byte grid
           dict(lda=c.av.stride(0) + 4),                      # bf16 leading dimension % 8 != 0
           dict(in_f=12, lda=c.av.stride(0))]                 # bf16 rows need in % 8 == 0
    for over in bad:
        with pytest.raises(RuntimeError, match="head_eval"):
            call(**over)
    # the Python wrapper checks the workspace size on the host
    with pytest.raises(ValueError, match="workspace"):
        ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", metrics=metrics,
                      ws=torch.zeros(1, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="workspace"):
        ops.head_eval(c.av, c.wv, c.bv, None, labels, "xent", metrics=metrics, ws=None)
    torch.cuda.synchronize()
    assert ex.guards_intact(lbuf, lv) and bool((lv == 0).all()) and pred_guards_ok(pbuf, rows)
    assert bool((pv.cpu() == PRED_SENTINEL).all())
    assert metrics.cpu().tolist() == [7.0] * 4
    # fp32 rows of the same shapes are taken (scalar form) -- the refusals above are bf16's
    lbuf2, lv2, _, _ = cf.outputs()
    ops.head_eval(cf.av[:, :12], cf.wv[:, :12].contiguous(), cf.bv, logits_out=lv2)
    torch.cuda.synchronize()
    assert ex.same(lv2, ex.f32(ex.preact(cf.a[:, :12], cf.W[:, :12], cf.b)))
    assert ex.guards_intact(lbuf2, lv2)
