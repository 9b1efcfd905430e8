"""Layer / RMS normalisation of hidden layers on the GPU (csrc/kernels/norm.hip, --norm): the two
kernels against float64 at the widths that reach every form, two rows that break a one-pass
variance, and the engine against float64 autograd."""
import copy

import pytest
import torch

import nnmpi_amd  # noqa: F401
from _exact import NAN, SENTINEL_BF16, SENTINEL_F32, bf16_ulp_apart, embed, guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
ROWS = (1, 67)     # ragged against the rows a wave holds (4 .. 256) and against a block
# chunks of 16 bytes per row C = H / 8 (bf16), H / 4 (fp32), H (fp32 scalar loads: H % 4 != 0):
# C <= 64 one chunk per lane on 2^k lanes, <= 128 two, <= 256 four (wave form); above, one block
# per row with 2 / 4 / 8 / 32 chunks per thread
WIDTHS = {torch.bfloat16: [8, 24, 512, 520, 2048, 2056, 8192],
          torch.float32: [3, 13, 250, 8, 24, 512, 520, 1024, 1028, 1030, 2048, 2056, 8190, 8192]}
CASES = [(dt, H) for dt, hs in WIDTHS.items() for H in hs]


def _act(n, act):
    return torch.relu(n) if act == "relu" else torch.tanh(n) if act == "tanh" else n


def _oracle(z, dn, norm, act, dtype):
    """(a, stats, dz) of the definitions in ``dtype`` by autograd; fp32: through
    torch.nn.functional.layer_norm."""
    z = z.to(dtype).requires_grad_()
    mu = z.mean(1, keepdim=True) if norm == "layer" else torch.zeros_like(z[:, :1])
    rstd = 1 / torch.sqrt(((z - mu) ** 2).mean(1, keepdim=True) + EPS)
    if dtype == torch.float32 and norm == "layer":
        n = torch.nn.functional.layer_norm(z, z.shape[1:], eps=EPS)
    else:
        n = (z - mu) * rstd
    (dz,) = torch.autograd.grad(n, z, dn.to(dtype))
    return _act(n, act).detach(), torch.cat([mu, rstd], 1).detach(), dz


def _run(z, dn, norm, act):
    """norm_act + norm_bwd on operands embedded in poisoned buffers: (a, stats, dz), guards
    checked bit for bit."""
    from nnmpi_amd.ops.hip_ops import HipOps
    ops, rows = HipOps(DEV), z.shape[0]
    sent = SENTINEL_BF16 if z.dtype == torch.bfloat16 else SENTINEL_F32
    zb, zv = embed(z.to(DEV), 1, 8, NAN)
    ab, av = embed(torch.zeros_like(zv), 1, 8, sent)
    gb, gv = embed(dn.to(DEV), 1, 8, sent)
    sb, sv = embed(torch.zeros(rows, 2, device=DEV), 1, 0, SENTINEL_F32)
    ops.norm_act(zv, norm, act, av, sv)
    ops.norm_bwd(gv, zv, sv, norm)
    torch.cuda.synchronize()
    for buf, view in ((ab, av), (gb, gv), (sb, sv)):
        assert guards_intact(buf, view)
    assert torch.equal(zv.cpu(), z), "the saved pre-activations were written"
    return av.cpu(), sv.cpu(), gv.cpu()


def _inputs(rows, H, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return ((1.5 * torch.randn(rows, H, generator=g) + 0.3).to(dtype),
            torch.randn(rows, H, generator=g).to(dtype))


@pytest.mark.parametrize("dtype,H", CASES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_norm_kernels_vs_float64(norm, act, dtype, H):
    """bf16 outputs: within 1 bf16 ulp of the rounded float64 result and at most 1e-3 of the
    elements not bit-identical to it (fp32 torch on the CPU reaches at most 7.3e-5 here).  fp32
    outputs and the statistics: at most 4x the error fp32 torch has against float64 on the same
    inputs, per case.  Seen on an MI355X (every figure is printed): reference errors 2.1e-8 ..
    6.5e-7 (a), 1.1e-8 .. 1.2e-6 (dz), 1.6e-9 .. 3.0e-7 (stats); the kernels' largest errors
    4.2e-7 / 9.1e-7 / 1.8e-7, at worst 1.98x / 1.02x / 1.0003x their case's reference error;
    bf16: at most 1 ulp, share at most 2.9e-5."""
    for rows in ROWS:
        z, dn = _inputs(rows, H, dtype, 1000 * H + rows)
        want = _oracle(z, dn, norm, act, torch.float64)
        got = _run(z, dn, norm, act)
        ref = _oracle(z, dn, norm, act, torch.float32)
        for name, g, w, r in zip(("a", "stats", "dz"), got, want, ref):
            err, allowed = float((g.double() - w).abs().max()), 4 * float((r.double() - w).abs().max())
            if dtype == torch.bfloat16 and name != "stats":
                w16 = w.to(torch.bfloat16)
                ulps = float(bf16_ulp_apart(g, w16).max())
                share = float((g.view(torch.int16) != w16.view(torch.int16)).double().mean())
                print(f"{norm} {act} bf16 H={H} rows={rows} {name}: {ulps} ulp, share {share:.2e}")
                assert ulps <= 1 and share <= 1e-3, (name, rows, ulps, share)
            else:
                print(f"{norm} {act} H={H} rows={rows} {name}: err {err:.3e} allowed {allowed:.3e}")
                assert err <= allowed, (name, rows, err, allowed)


@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_offset_and_constant_rows(norm):
    """fp32, H = 512.  Row 1000 + randn: fp32 torch is 6.6e-5 from float64, E[z^2] - E[z]^2 is
    0.59 away: below 1e-3.  Constant row: the layer norm gives act(0) exactly, rstd = 1/sqrt(eps)
    (rms: x = c / sqrt(c^2 + eps)), and dz is finite and the float64 result -- to the same 1e-3:
    rstd (316) times the error of the 512-term mean of dn (about 9 * 2^-24) is 2e-4."""
    g = torch.Generator().manual_seed(7)
    z = torch.cat([1000 + torch.randn(1, 512, generator=g), torch.full((1, 512), 3.25)])
    dn = torch.randn(2, 512, generator=g)
    want = _oracle(z, dn, norm, "none", torch.float64)
    got = _run(z, dn, norm, "none")
    for name, gt, w in zip(("a", "stats", "dz"), got, want):
        err = (gt.double() - w).abs().amax(1)
        print(f"{norm} {name}: offset row {float(err[0]):.3e}, constant row {float(err[1]):.3e}")
        assert torch.isfinite(gt).all() and float(err.max()) < 1e-3, (name, err)
    if norm == "layer":
        assert torch.equal(got[0][1], torch.zeros(512)) and float(got[1][1, 0]) == 3.25


def _engine(widths, act, loss, norm, dtype, **kw):
    from nnmpi_amd.engine.arena import Arena
    from nnmpi_amd.engine.engine import MLPEngine
    from nnmpi_amd.models.mlp import MLPSpec, reference_init
    from nnmpi_amd.ops.hip_ops import HipOps
    from nnmpi_amd.parallel.sync import NoSync
    spec = MLPSpec(tuple(widths), act, loss, norm)
    ar = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], DEV,
               shadow_dtype=torch.bfloat16 if dtype == torch.bfloat16 else None)
    model = reference_init(widths, act, seed=1, norm=norm)
    init = copy.deepcopy(model)
    ar.bind_model(model)
    eng = MLPEngine(spec, ar, HipOps(DEV), NoSync(ar), device=DEV, dtype=dtype, rows_capacity=67,
                    **kw)
    return ar, eng, init


def _steps(ar, eng, X, Y, labels, n=3):
    per = eng.spec.widths[-1] if eng.loss_kind == "mse" else 1
    eng.load_batch(X.to(DEV, eng.dtype), None if Y is None else Y.to(DEV),
                   None if labels is None else labels.to(DEV))
    eng.set_scales(1.0 / (67 * per), 1.0 / (67 * per), 1.0)
    losses = []
    for _ in range(n):
        eng.step()
        losses.append(eng.loss())
    return losses, ar.flat_params_forward_order().cpu()


@pytest.mark.parametrize("widths,act,loss", [([16, 24, 24, 3], "relu", "xent"), ([8, 16, 1], "tanh", "mse")])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_fp32_engine_vs_float64_autograd(norm, widths, act, loss):
    """Three SGD-momentum steps of the fp32 engine against a float64 Sequential(Linear, norm, act,
    ...) under torch.optim.SGD from the same parameters: losses rel 1e-4, parameters atol 1e-5 /
    rtol 1e-4 (test_engine_gpu.py's fp32 engine-vs-PyTorch bounds); predict() on the training
    rows likewise; the sequential schedule; a graph-replayed run bitwise equal to the eager one."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(67, widths[0], generator=g)
    Y = torch.randn(67, widths[-1], generator=g) if loss == "mse" else None
    labels = torch.randint(0, widths[-1], (67,), generator=g) if loss == "xent" else None
    kw = dict(lr=0.05, momentum=0.9)
    ar, eng, init = _engine(widths, act, loss, norm, torch.float32, use_graph=False, **kw)
    losses, params = _steps(ar, eng, X, Y, labels)
    assert eng.schedule_name() == "sequential"
    lins = [copy.deepcopy(m).double() for m in init.linears()]
    mods = []
    cls = torch.nn.LayerNorm if norm == "layer" else torch.nn.RMSNorm
    for lin in lins[:-1]:
        mods += [lin, cls(lin.out_features, eps=EPS, elementwise_affine=False),
                 torch.nn.ReLU() if act == "relu" else torch.nn.Tanh()]
    ref = torch.nn.Sequential(*mods, lins[-1])
    opt = torch.optim.SGD(ref.parameters(), **kw)
    want = []
    for _ in range(3):
        opt.zero_grad()
        out = ref(X.double())
        lv = (torch.nn.functional.cross_entropy(out, labels) if loss == "xent" else
              torch.nn.functional.mse_loss(out, Y.double()))
        lv.backward()
        want.append(float(lv.detach()))
        opt.step()
    flat = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    assert losses == pytest.approx(want, rel=1e-4)
    assert torch.allclose(params.double(), flat, atol=1e-5, rtol=1e-4)
    assert torch.allclose(eng.predict(X.to(DEV)).cpu().double(), ref(X.double()).detach(),
                          atol=1e-5, rtol=1e-4)
    ar2, eng2, _ = _engine(widths, act, loss, norm, torch.float32, use_graph=True, **kw)
    losses2, params2 = _steps(ar2, eng2, X, Y, labels)
    assert eng2.use_graph and eng2._graphs and losses2 == losses and torch.equal(params2, params)


def test_bf16_engine_deterministic_and_composes():
    """512,512,512,1 in bf16, 67 rows, --norm layer with Adam and --clip_grad_norm 1: two runs of
    three steps are bitwise equal, and so is the run without graphs."""
    g = torch.Generator().manual_seed(5)
    X, Y = torch.randn(67, 512, generator=g), torch.randn(67, 1, generator=g)
    runs = []
    for graph in (True, True, False):
        ar, eng, _ = _engine([512, 512, 512, 1], "relu", "mse", "layer", torch.bfloat16, lr=1e-3,
                             momentum=0.0, optimizer="adam", clip_grad_norm=1.0, use_graph=graph)
        runs.append(_steps(ar, eng, X, Y, None))
        assert eng.schedule_name() == "sequential"
    assert all(l == l for l in runs[0][0])
    for losses, params in runs[1:]:
        assert losses == runs[0][0] and torch.equal(params, runs[0][1])
