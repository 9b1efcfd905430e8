"""The bf16 / fp32 GEMM family and the slab reducer against an exact float64 oracle.

Every operand is a small integer (or a dyadic multiple of one) with sum |a||b| + |bias| < 2^24
(tests/_exact.py: ``assert_exact_ok``, called by every test on its own inputs), so every product
and partial sum is exact in fp32 whatever the tile, main loop, epilogue form or split count: an
fp32 result must equal the float64 matmul and a bf16 result its round-to-nearest-even cast, in
every element (``torch.equal``; a NaN never compares equal).  Outputs live inside sentinel-filled
buffers whose guards are compared bit for bit afterwards; inputs, in at least one case per
launcher, inside NaN-filled ones, so a read past an M, N or K tail that the predicate should
have zeroed turns the result into NaN.

The one inexact case is the tanh forward: the pre-activations are still exact (W and the bias on
a 2^-6 grid, |z| up to about 4), tanhf is not.  bf16: every output within 1 bf16 ulp of
bf16(tanh_f64(z)) and at most 1e-3 of them not identical (a few-ulp fp32 tanhf error is 2^-22
relative against a bf16 spacing of 2^-8: a rounding-boundary crossing is a ~1e-4 event; the cap
is that with a 10x margin).  Shares of non-identical outputs on the (200, 136, 72) case: fp32
torch.tanh on the CPU 0 (tests/test_exact_cpu.py), the GPU kernels 0 as well, on every tile and
main loop (printed by test_linear_fwd_bf16 as "TANH_SHARE").  fp32 mode: within 1 fp32 ulp of fp32(tanh_f64(z)) --
the device tanhf is not correctly rounded, so bit equality with the float64 value is not
something the kernel promises, while its argument z is exact.

Paths no test here reaches: forward variants 3, 4, 7 and 9 (not in the issue's list), the
deep-ring variants 19-24, wide_pair and cu_mask_stream (experiments build only), and operands of
2 GiB or more (refused on the host; only the refusal is tested).  The 256 x 256 weight gradient's
set_pp_prefetch 1 / 2 branch IS reached (test_fused_sgd, forms epi256-pf1 / epi256-pf2).
"""
import contextlib

import pytest
import torch

import _exact as ex

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    from nnmpi_amd import native
    return native.lib()


def _ops():
    from nnmpi_amd.ops.hip_ops import HipOps
    return HipOps()


def _s():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _knobs(tile=0, impl=2, fwd_variant=-1, splits=0, group=-1, group_async=-1, sgd_epilogue=-1,
           pp_prefetch=-1):
    """Set the kernel-selection knobs (each call must report that it took effect) and put every
    one back to its default afterwards."""
    lib = _lib()
    try:
        assert lib.set_gemm_tile(tile) and lib.set_gemm_impl(impl)
        assert lib.set_fwd_variant(fwd_variant) and lib.set_wgrad_splits(splits)
        assert lib.set_bwd_group(group) and lib.set_group_async(group_async)
        assert lib.set_sgd_epilogue(sgd_epilogue) and lib.set_pp_prefetch(pp_prefetch)
        assert lib.get_gemm_impl() == impl
        yield lib
    finally:
        lib.set_gemm_tile(0)
        lib.set_gemm_impl(-1)
        lib.set_fwd_variant(-1)
        lib.set_wgrad_splits(0)
        lib.set_bwd_group(-1)
        lib.set_group_async(-1)
        lib.set_sgd_epilogue(-1)
        lib.set_pp_prefetch(-1)


# ---- operand placement ----------------------------------------------------------------------
def _put(t, nan):
    """An input on the device: dense, or (``nan``) inside a NaN-filled buffer -- two rows above
    and below, 8 elements left, 8+ right, so the view keeps a 16-byte aligned base and
    ld % 8 == 0 (what the loaders take) with ld > width."""
    t = t.to(DEV)
    if not nan:
        return t.contiguous()
    if t.dim() == 1:
        return ex.embed(t, 0, 4, ex.NAN)[1]
    return ex.embed(t, 2, 8, ex.NAN, pad_right=8 + (-t.shape[1]) % 8)[1]


def _out(shape, dtype, left=8, right=8, rows=2):
    """An output view full of NaN inside a sentinel-filled buffer: ``(buf, view)``."""
    sent = ex.SENTINEL_BF16 if dtype == BF16 else ex.SENTINEL_F32
    return ex.embed(torch.full(shape, ex.NAN, dtype=dtype, device=DEV), rows, left, sent,
                    pad_right=right)


def _out_dense(shape, dtype, left=8):
    """A dense [M, N] (or [n]) output carved out of a guarded 1-D buffer."""
    n = 1
    for s in shape:
        n *= s
    buf, v = _out((n,), dtype, left=left, right=8)
    return buf, v.view(shape)


def _guards(buf, view):
    return ex.guards_intact(buf, view.reshape(-1) if buf.dim() == 1 else view)


def _eq(got, want, what):
    torch.cuda.synchronize()
    g = got.detach().cpu()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    if not torch.equal(g, want):
        bad = (g != want) | torch.isnan(g)
        idx = bad.nonzero()[:4].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements differ, first at "
                             f"{idx}: got {g[bad][:4].tolist()}, want {want[bad][:4].tolist()}")


def _done(pair, want, what):
    buf, view = pair
    _eq(view, want, what)
    assert _guards(buf, view), f"{what}: the memory around the output was written"


def _lepi_ok(epi, N, C, ldc, aux=None, bias=None):
    """The device predicate gemm_tiles.h lepi_ok, mirrored: the row-contiguous LDS epilogue of
    the 128 x 128 DMA tile is taken, else the fragment epilogue."""
    if N % 8:
        return False
    if epi == "f32":
        return ldc % 4 == 0 and C.data_ptr() % 16 == 0
    if epi == "dact":
        return (ldc % 8 == 0 and C.data_ptr() % 16 == 0 and aux.stride(0) % 8 == 0 and
                aux.data_ptr() % 16 == 0)
    return ldc % 8 == 0 and C.data_ptr() % 16 == 0 and bias.data_ptr() % 16 == 0


# ---- cases (CPU operands and oracles, computed once per shape) --------------------------------
_cache = {}


def _fwd_case(rows, out_f, in_f, act, dtype=BF16):
    key = ("fwd", rows, out_f, in_f, act == "tanh", dtype)
    if key not in _cache:
        u = 2.0 ** -6 if act == "tanh" else 1.0
        x = ex.ints((rows, in_f), -4, 4, 101, dtype=dtype)
        W = ex.ints((out_f, in_f), -4, 4, 102, scale=u, dtype=dtype)
        b = ex.ints(out_f, -64, 64, 103, scale=u, dtype=F32)
        ex.assert_exact_ok(x, W.t(), b, ub=u)
        _cache[key] = (x, W, b, ex.preact(x, W, b))
    return _cache[key]


def _dgrad_case(rows, out_f, in_f, dtype=BF16):
    key = ("dgrad", rows, out_f, in_f, dtype)
    if key not in _cache:
        dz = ex.ints((rows, out_f), -2, 2, 111, dtype=dtype)
        W = ex.ints((out_f, in_f), -2, 2, 112, dtype=dtype)
        assert ex.assert_exact_ok(dz, W) <= 1000     # keeps acc (1 - a^2) exact (tanh_grid)
        grid = ex.tanh_grid((rows, in_f), 113).to(dtype)
        a = {"tanh": grid, "relu": torch.relu(ex.ints((rows, in_f), -3, 3, 114, dtype=dtype)),
             "none": ex.ints((rows, in_f), -3, 3, 115, dtype=dtype)}
        _cache[key] = (dz, W, a, {k: ex.dgrad(dz, W, a[k], k) for k in a})
    return _cache[key]


def _wgrad_case(rows, out_f, in_f, dtype=BF16):
    key = ("wgrad", rows, out_f, in_f, dtype)
    if key not in _cache:
        dz = ex.ints((rows, out_f), -4, 4, 121, dtype=dtype)
        x = ex.ints((rows, in_f), -4, 4, 122, dtype=dtype)
        ex.assert_exact_ok(dz.t(), x)
        ex.assert_exact_ok(dz.t(), torch.ones(rows, 1))
        _cache[key] = (dz, x) + ex.wgrad(dz, x)
    return _cache[key]


def _ws(ops, rows, out_f, in_f, dtype=BF16):
    """A NaN-filled workspace of exactly wgrad_workspace_bytes inside sentinel guards."""
    n = ops.wgrad_workspace_bytes(rows, out_f, in_f, dtype) // 4
    if n == 0:
        return None, None
    return _out((n,), F32)


# =============================================================================================
# plain GEMM
# =============================================================================================
@pytest.mark.parametrize("tile", [64, 128, 256])
@pytest.mark.parametrize("la,lb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(40, 24, 8), (72, 136, 200), (264, 136, 72), (130, 260, 520)])
def test_plain_gemm(M, N, K, la, lb, tile):
    """gemm_bf16 (64 x 64 tiles) and gemm_bf16_tile at 128 / 256 in the four layout pairs.  The
    first shape is dense; the others read A and B out of NaN-filled buffers and write a strided
    C -- (72, 136, 200) one that keeps the LDS epilogue (aligned, ldc % 4 == 0), the last two one
    that does not (C 8 bytes off a 16-byte boundary, ldc % 4 == 2)."""
    lib = _lib()
    key = ("gemm", M, N, K)
    if key not in _cache:
        A, B = ex.ints((M, K), -4, 4, 1), ex.ints((K, N), -4, 4, 2)
        ex.assert_exact_ok(A, B)
        _cache[key] = (A, B, ex.f32(ex.gemm(A, B)))
    A, B, want = _cache[key]
    strided = K != 8
    # storage: KMAJ A = [M][K]; XMAJ A = [K][M]; KMAJ B = [N][K]; XMAJ B = [K][N]
    As = _put(A if la == 0 else A.t().contiguous(), strided)
    Bs = _put(B.t().contiguous() if lb == 0 else B, strided)
    if not strided:
        C = _out_dense((M, N), F32)
    elif K == 200:
        C = _out((M, N), F32, left=8, right=8)
    else:
        C = _out((M, N), F32, left=2, right=4)
    ldc = C[1].stride(0)
    assert _lepi_ok("f32", N, C[1], ldc) == (K in (8, 200) and N % 8 == 0)
    if tile == 64:
        lib.gemm_bf16(As.data_ptr(), As.stride(0), la, Bs.data_ptr(), Bs.stride(0), lb, M, N, K,
                      C[1].data_ptr(), ldc, _s())
    else:
        lib.gemm_bf16_tile(As.data_ptr(), As.stride(0), la, Bs.data_ptr(), Bs.stride(0), lb, M, N, K,
                           C[1].data_ptr(), ldc, tile, _s())
    _done(C, want, f"C {M}x{N}x{K} la{la} lb{lb} tile {tile}")


# =============================================================================================
# forward, dgrad, weight gradient (bf16)
# =============================================================================================
PATHS = {"tile64": (0, 2), "tile64-regstaged": (0, 1), "tile128": (128, 2),
         "tile128-regstaged": (128, 1), "tile256": (256, 2)}
LAYER_SHAPES = [(200, 136, 72), (40, 24, 8)]     # rows, out, in: all ragged; forward K = 8


def _check_fwd(pair, z, act, dtype, what):
    if act != "tanh":
        want = ex.act_f64(z, act)
        _done(pair, ex.bf16_rne(want) if dtype == BF16 else ex.f32(want), what)
        return None
    torch.cuda.synchronize()
    buf, view = pair
    got = view.detach().cpu()
    assert _guards(buf, view), f"{what}: the memory around the output was written"
    want = torch.tanh(z).to(dtype)
    if dtype == F32:
        worst = float(ex.f32_ulp_apart(got, want).max())
        assert worst <= 1.0, f"{what}: {worst} fp32 ulp from fp32(tanh_f64(z))"
        return None
    worst = float(ex.bf16_ulp_apart(got, want).max())
    share = float((got != want).double().mean())
    print(f"\nTANH_SHARE {what}: {share:.2e} of the outputs not identical, worst {worst} bf16 ulp")
    assert worst <= 1.0, f"{what}: {worst} bf16 ulp from bf16(tanh_f64(z))"
    assert share <= 1e-3, f"{what}: {share} of the outputs differ from bf16(tanh_f64(z))"
    return share


@pytest.mark.parametrize("nan_inputs", [False, True], ids=["dense", "nan-embedded"])
@pytest.mark.parametrize("rows,out_f,in_f", LAYER_SHAPES)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_linear_fwd_bf16(path, rows, out_f, in_f, nan_inputs):
    tile, impl = PATHS[path]
    ops = _ops()
    with _knobs(tile=tile, impl=impl):
        for act in ("none", "relu", "tanh"):
            x, W, b, z = _fwd_case(rows, out_f, in_f, act)
            out = _out((rows, out_f), BF16)
            ops.linear_act(_put(x, nan_inputs), _put(W, nan_inputs), _put(b, nan_inputs), act, out[1])
            _check_fwd(out, z, act, BF16, f"fwd {path} {act} {rows}x{out_f}x{in_f}")


@pytest.mark.parametrize("nan_inputs", [False, True], ids=["dense", "nan-embedded"])
@pytest.mark.parametrize("rows,out_f,in_f", LAYER_SHAPES)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_linear_dgrad_bf16(path, rows, out_f, in_f, nan_inputs):
    tile, impl = PATHS[path]
    ops = _ops()
    dz, W, a, want = _dgrad_case(rows, out_f, in_f)
    with _knobs(tile=tile, impl=impl):
        for act in ("relu", "tanh", "none"):
            out = _out((rows, in_f), BF16)
            ops.linear_dgrad(_put(dz, nan_inputs), _put(W, nan_inputs), _put(a[act], nan_inputs),
                             act, out[1])
            _done(out, ex.bf16_rne(want[act]), f"dgrad {path} {act} {rows}x{out_f}x{in_f}")


@pytest.mark.parametrize("nan_inputs", [False, True], ids=["dense", "nan-embedded"])
@pytest.mark.parametrize("rows,out_f,in_f", LAYER_SHAPES)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_linear_wgrad_bf16_unsplit(path, rows, out_f, in_f, nan_inputs):
    tile, impl = PATHS[path]
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
    with _knobs(tile=tile, impl=impl) as lib:
        assert lib.wgrad_splits(out_f, in_f, rows) == 1
        gW, gb = _out_dense((out_f, in_f), F32), _out_dense((out_f,), F32)
        ops.linear_wgrad(_put(dz, nan_inputs), _put(x, nan_inputs), gW[1], gb[1])
        _done(gW, ex.f32(wW), f"dW {path}")
        _done(gb, ex.f32(wb), f"db {path}")


@pytest.mark.parametrize("variant", [1, 2, 5, 6, 8, 10, 11, 12, 13])
def test_forward_variants_on_the_128_tile(variant):
    rows, out_f, in_f = 200, 136, 72
    ops = _ops()
    x, W, b, z = _fwd_case(rows, out_f, in_f, "relu")
    with _knobs(tile=128, fwd_variant=variant):
        out = _out((rows, out_f), BF16)
        ops.linear_act(_put(x, True), _put(W, True), _put(b, True), "relu", out[1])
        _done(out, ex.bf16_rne(torch.relu(z)), f"fwd variant {variant}")


# ---- the fragment-epilogue fallback (lepi_ok false), one case per way of failing it ------------
@pytest.mark.parametrize("case", ["aligned", "n%8==4", "ldc%8==4", "C+8B", "bias+4B"])
def test_fwd_epilogue_forms(case):
    rows, out_f, in_f = 200, (132 if case == "n%8==4" else 136), 72
    ops = _ops()
    x, W, b, z = _fwd_case(rows, out_f, in_f, "relu")
    out = {"ldc%8==4": _out((rows, out_f), BF16, left=8, right=4),
           "C+8B": _out((rows, out_f), BF16, left=4, right=4)}.get(case) or _out((rows, out_f), BF16)
    bias = ex.embed(b.to(DEV), 0, 1 if case == "bias+4B" else 4, ex.NAN)[1]
    assert _lepi_ok("bias", out_f, out[1], out[1].stride(0), bias=bias) == (case == "aligned")
    if case == "ldc%8==4":
        assert out[1].data_ptr() % 16 == 0 and out[1].stride(0) % 8 == 4
    if case == "C+8B":
        assert out[1].data_ptr() % 16 == 8 and out[1].stride(0) % 8 == 0
    if case == "bias+4B":
        assert bias.data_ptr() % 16 == 4
    with _knobs(tile=128):
        ops.linear_act(_put(x, True), _put(W, True), bias, "relu", out[1])
        _done(out, ex.bf16_rne(torch.relu(z)), f"fwd {case}")


@pytest.mark.parametrize("case", ["aligned", "ldc%8==4", "C+8B", "ldaux%8==4", "aux+8B"])
def test_dgrad_epilogue_forms(case):
    rows, out_f, in_f = 200, 136, 72
    ops = _ops()
    dz, W, a, want = _dgrad_case(rows, out_f, in_f)
    out = {"ldc%8==4": _out((rows, in_f), BF16, left=8, right=4),
           "C+8B": _out((rows, in_f), BF16, left=4, right=4)}.get(case) or _out((rows, in_f), BF16)
    pads = {"ldaux%8==4": (8, 4), "aux+8B": (4, 4)}.get(case, (8, 8))
    aux = ex.embed(a["tanh"].to(DEV), 2, pads[0], ex.NAN, pad_right=pads[1])[1]
    assert _lepi_ok("dact", in_f, out[1], out[1].stride(0), aux=aux) == (case == "aligned")
    if case == "ldaux%8==4":
        assert aux.data_ptr() % 16 == 0 and aux.stride(0) % 8 == 4
    if case == "aux+8B":
        assert aux.data_ptr() % 16 == 8 and aux.stride(0) % 8 == 0
    with _knobs(tile=128):
        ops.linear_dgrad(_put(dz, True), _put(W, True), aux, "tanh", out[1])
        _done(out, ex.bf16_rne(want["tanh"]), f"dgrad {case}")


@pytest.mark.parametrize("case", ["aligned", "C+8B"])
def test_wgrad_epilogue_forms(case):
    """(dW is dense, ld = in % 8 == 0: a pointer 8 bytes off is the launcher's one way out of the
    LDS epilogue besides the bf16 payload, test_wgrad_bf16_payload.)"""
    rows, out_f, in_f = 200, 136, 72
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
    gW = _out_dense((out_f, in_f), F32, left=2 if case == "C+8B" else 8)
    gb = _out_dense((out_f,), F32)
    assert _lepi_ok("f32", in_f, gW[1], in_f) == (case == "aligned")
    with _knobs(tile=128) as lib:
        assert lib.wgrad_splits(out_f, in_f, rows) == 1
        ops.linear_wgrad(_put(dz, True), _put(x, True), gW[1], gb[1])
        _done(gW, ex.f32(wW), f"dW {case}")
        _done(gb, ex.f32(wb), f"db {case}")


# =============================================================================================
# split-K weight gradient
# =============================================================================================
@pytest.mark.parametrize("form,cap", [("dense", 0), ("colslice", 0), ("dense", 1), ("dense", 2)])
@pytest.mark.parametrize("rows,want_req,want_run", [(520, 2, 2), (1100, 4, 4), (2050, 8, 7)])
@pytest.mark.parametrize("out_f,in_f", [(128, 128), (136, 200)])
def test_wgrad_splitk(out_f, in_f, rows, want_req, want_run, form, cap):
    """rows = 520: two splits, a tail in the last; 1100: four, the last one short; 2050: eight
    requested, seven launched (33 k-steps in fives), a 2-row tail, the workspace sized for eight.
    ``cap``: set_wgrad_splits.  ``colslice``: dZ is full[:, 256 : 256 + out] of a wider matrix
    (lddz > out, offset base), the rest of which -- like the surroundings of x -- is NaN."""
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
    req = min(want_req, cap) if cap else want_req
    with _knobs(splits=cap) as lib:
        assert lib.wgrad_splits(out_f, in_f, rows) == req
        ksteps = (rows + 63) // 64
        kps = (ksteps + req - 1) // req
        assert (ksteps + kps - 1) // kps == (want_run if not cap else req)
        if form == "colslice":
            full = torch.full((rows, 256 + out_f + 64), ex.NAN, dtype=BF16, device=DEV)
            dzv = full[:, 256:256 + out_f]
            dzv.copy_(dz)
            xv = _put(x, True)
        else:
            dzv, xv = _put(dz, False), _put(x, False)
        gW, gb = _out_dense((out_f, in_f), F32), _out_dense((out_f,), F32)
        wsb, ws = _ws(ops, rows, out_f, in_f)
        assert (ws is None) == (req == 1)
        ops.linear_wgrad(dzv, xv, gW[1], gb[1], ws=ws)
        _done(gW, ex.f32(wW), "dW")
        _done(gb, ex.f32(wb), "db")
        if ws is not None:
            assert ex.guards_intact(wsb, ws), "written beyond wgrad_workspace_bytes"


# =============================================================================================
# the slab reducer directly
# =============================================================================================
@pytest.mark.parametrize("M,N", [(1, 4), (5, 64), (130, 516)])
@pytest.mark.parametrize("S", [1, 2, 7, 8, 9, 16, 17, 33, 64, 65, 100])
def test_splitk_reduce(S, M, N):
    """Every slab_ws form (1, 2, 4, 8, 16 virtual waves and, beyond 64 partials, the deep one):
    integer slabs a few elements apart with NaN between them, ldo > N, bias partials, and 700
    loss partials (not a multiple of the block's 512 threads)."""
    lib = _lib()
    stride, bstride, nlp = M * N + 4, M + 3, 700
    ws = torch.full((S, stride), ex.NAN)
    ws[:, :M * N] = ex.ints((S, M * N), -1000, 1000, 200 + S, dtype=F32)
    bws = torch.full((S, bstride), ex.NAN)
    bws[:, :M] = ex.ints((S, M), -1000, 1000, 300 + S, dtype=F32)
    lp = ex.ints(nlp, -1000, 1000, 400 + S, dtype=F32)
    assert max(float(ws[:, :M * N].abs().sum(0).max()), float(bws[:, :M].abs().sum(0).max()),
               float(lp.abs().sum())) < ex.TWO24
    out, bout, lout = _out((M, N), F32, left=8, right=8), _out((M,), F32), _out((1,), F32)
    assert out[1].stride(0) > N
    wsd, bwsd, lpd = ws.to(DEV), bws.to(DEV), lp.to(DEV)
    lib.splitk_reduce(wsd.data_ptr(), S, stride, M, N, out[1].data_ptr(), out[1].stride(0),
                      bwsd.data_ptr(), bstride, bout[1].data_ptr(), lpd.data_ptr(), nlp, 0.5,
                      lout[1].data_ptr(), _s())
    _done(out, ex.f32(ex.slab_sum(ws[:, :M * N].reshape(S, M, N))), f"slab sum S={S}")
    _done(bout, ex.f32(ex.slab_sum(bws[:, :M])), f"bias slab sum S={S}")
    _done(lout, ex.f32(0.5 * ex.d(lp).sum().reshape(1)), "loss")


# =============================================================================================
# grouped backward
# =============================================================================================
GROUP_LAYERS = {"A": (200, 136, "tanh"), "B": (128, 128, "relu")}      # out, in, act of dgrad


def _group_job(ops, name, rows, dgrad, wgrad):
    out_f, in_f, act = GROUP_LAYERS[name]
    job = {"checks": []}
    dg = wg = None
    if dgrad:
        dz, W, a, want = _dgrad_case(rows, out_f, in_f)
        o = _out((rows, in_f), BF16)
        dg = (_put(dz, True), _put(W, True), _put(a[act], True), act, o[1])
        job["checks"].append((o, ex.bf16_rne(want[act]), f"dX {name}"))
    if wgrad:
        dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
        gW, gb = _out_dense((out_f, in_f), F32), _out_dense((out_f,), F32)
        wsb, ws = _ws(ops, rows, out_f, in_f)
        wg = (_put(dz, True), _put(x, True), gW[1], gb[1], ws)
        job["checks"] += [(gW, ex.f32(wW), f"dW {name}"), (gb, ex.f32(wb), f"db {name}")]
        job["ws"] = (wsb, ws)
    job["dg"], job["wg"] = dg, wg
    return job


@pytest.mark.parametrize("mode", ["grouped-async0", "grouped-async1", "grouped-async2", "fallback"])
@pytest.mark.parametrize("rows", [16, 72, 520])
@pytest.mark.parametrize("what", ["dgrad", "wgrad", "both", "chain"])
def test_bwd_group(what, rows, mode):
    """ops.bwd_group + slab_reduce: a dgrad, a weight gradient, both, and a chain (layer A's
    launch returns its pending combine, layer B's launch carries it, a final slab_reduce finishes
    B's); rows = 520 splits the weight gradients in two, 16 and 72 leave nothing pending.  The
    separate-launch branch (set_bwd_group(0)) must give the same oracle result."""
    ops = _ops()
    grouped = mode != "fallback"
    with _knobs(group=1 if grouped else 0, group_async=int(mode[-1]) if grouped else -1) as lib:
        for out_f, in_f, _ in GROUP_LAYERS.values():
            assert ops.bwd_group_supported(rows, out_f, in_f) == grouped
            assert lib.wgrad_splits(out_f, in_f, rows) == (2 if rows == 520 else 1)
        jobs = [_group_job(ops, "A", rows, what != "wgrad", what != "dgrad")]
        if what == "chain":
            jobs.append(_group_job(ops, "B", rows, True, True))
        pending = None
        for job in jobs:
            pending = ops.bwd_group(job["dg"], job["wg"], None, pending)
            assert pending.S == (2 if rows == 520 and job["wg"] is not None else 0)
        ops.slab_reduce(pending if pending.pending() else None)
        for job in jobs:
            for pair, want, name in job["checks"]:
                _done(pair, want, f"{name} {what} rows {rows} {mode}")
            if job.get("ws", (None, None))[1] is not None:
                assert ex.guards_intact(*job["ws"]), "written beyond wgrad_workspace_bytes"


# =============================================================================================
# bf16 payload epilogue
# =============================================================================================
@pytest.mark.parametrize("tile", [0, 128, 256])
def test_wgrad_bf16_payload(tile):
    rows, out_f, in_f = 200, 136, 72
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
    assert float(wW.abs().max()) > 256      # the payload really rounds
    with _knobs(tile=tile):
        assert ops.wgrad_can_write_bf16(rows, out_f, in_f)
        gW16, gb16 = _out_dense((out_f, in_f), BF16), _out_dense((out_f,), BF16)
        ops.linear_wgrad(_put(dz, True), _put(x, True), None, None, out_bf16=(gW16[1], gb16[1]))
        _done(gW16, ex.bf16_rne(wW), f"gW16 tile {tile}")
        _done(gb16, ex.bf16_rne(wb), f"gb16 tile {tile}")


# =============================================================================================
# fused updates
# =============================================================================================
def _arena_pair(shapes, seed):
    """Two arenas with the same random master / momentum / shadow everywhere (padding included)
    and zero gradients."""
    from nnmpi_amd.engine.arena import Arena
    a1, a2 = (Arena(shapes, DEV, shadow_dtype=BF16) for _ in range(2))
    g = torch.Generator(device=DEV).manual_seed(seed)
    a1.master.copy_(torch.randn(a1.numel, generator=g, device=DEV))
    a1.momentum.copy_(torch.randn(a1.numel, generator=g, device=DEV))
    a1.shadow.copy_(torch.randn(a1.numel, generator=g, device=DEV))
    for name in ("master", "momentum", "shadow"):
        getattr(a2, name).copy_(getattr(a1, name))
    return a1, a2


def _arenas_equal(a1, a2, what):
    torch.cuda.synchronize()
    for name in ("master", "momentum", "shadow", "grad"):
        t1, t2 = getattr(a1, name), getattr(a2, name)
        if not torch.equal(t1, t2):
            bad = (t1 != t2).nonzero().flatten()
            raise AssertionError(f"{what}: arena.{name} differs in {bad.numel()} of {t1.numel()} "
                                 f"elements, first at {bad[:4].tolist()}")


FUSED_FORMS = {   # tile, set_wgrad_splits, set_sgd_epilogue, set_pp_prefetch
    "splitk": (0, 0, -1, -1), "epi64": (64, 1, -1, -1), "epi128": (128, 1, -1, -1),
    "epi256-s0": (256, 1, 0, 0), "epi256-s1": (256, 1, 1, 0), "epi256-s2": (256, 1, 2, 0),
    "epi256-pf1": (256, 1, 0, 1), "epi256-pf2": (256, 1, 0, 2)}


@pytest.mark.parametrize("opt", ["first", "later", "nesterov-wd"])
@pytest.mark.parametrize("form", sorted(FUSED_FORMS))
def test_fused_sgd(form, opt):
    """The weight gradient that applies SGD-momentum itself -- in its split-K combine, in the
    un-split epilogue of the 64 / 128 tiles, and in the 256 x 256 tile's three epilogue forms and
    two operand-prefetch forms -- against the float64-oracle gradient written into a second arena
    and updated by the separate ops.sgd pass: master, momentum and shadow equal everywhere, the
    gradient arena untouched, nothing outside the layer's weight and bias changed."""
    rows, out_f, in_f = 520, 136, 200
    tile, cap, serial, pf = FUSED_FORMS[form]
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f)
    a1, a2 = _arena_pair([(out_f, in_f), (8, out_f)], 7)
    nesterov, first = opt == "nesterov-wd", opt == "first"
    hp = torch.tensor([0.01, 0.9, 0.0, 1e-2 if nesterov else 0.0, 0.5, 0, 0, 0], device=DEV)
    with _knobs(tile=tile, splits=cap, sgd_epilogue=serial, pp_prefetch=pf) as lib:
        assert lib.wgrad_splits(out_f, in_f, rows) == (2 if form == "splitk" else 1)
        assert ops.wgrad_can_fuse_sgd(rows, out_f, in_f, BF16, epilogue=form != "splitk")
        wsb, ws = _ws(ops, rows, out_f, in_f)
        ops.linear_wgrad(_put(dz, True), _put(x, True), a1.grad_weight(0), a1.grad_bias(0), ws=ws,
                         sgd=ops.sgd_fusion(a1, hp, nesterov, first))
        torch.cuda.synchronize()
    a2.grad_weight(0).copy_(ex.f32(wW))
    a2.grad_bias(0).copy_(ex.f32(wb))
    for kind in ("weight", "bias"):
        slot = a2.by_name[f"layers.0.{kind}"]
        ops.sgd(a2, hp, nesterov, first, offset=slot.offset, numel=slot.numel)
    _arenas_equal(a1, a2, f"fused {form} {opt}")
    assert torch.count_nonzero(a1.grad) == 0
    if ws is not None:
        assert ex.guards_intact(wsb, ws)


# =============================================================================================
# deferred update
# =============================================================================================
def test_wgrad_deferred_update():
    """linear_wgrad_defer at the smallest square shape wgrad_defer_ok accepts (4096 x 4096, 72
    rows; about half a GB of arenas): the bf16 payload of the layer being differentiated against
    the oracle; the OTHER layer's weights bit-equal to ops.sgd(..., grad_bf16=g16) on a copy; the
    differentiated layer's own parameters, every bias and all padding untouched."""
    rows, H = 72, 4096
    ops = _ops()
    assert ops.wgrad_defer_ok(rows, H, H)
    dz, x, wW, wb = _wgrad_case(rows, H, H)
    a1, a2 = _arena_pair([(H, H), (H, H)], 9)
    gen = torch.Generator(device=DEV).manual_seed(10)
    g16 = torch.randn(a1.numel, generator=gen, device=DEV).to(BF16)
    other = a1.by_name["layers.2.weight"]
    mine_w, mine_b = a1.by_name["layers.0.weight"], a1.by_name["layers.0.bias"]
    sent = torch.tensor([ex.SENTINEL_BF16], dtype=torch.int16, device=DEV).view(BF16)
    a1.weight(0, g16).copy_(sent.expand(H, H))
    a1.bias(0, g16).copy_(sent.expand(H))
    g16_before = g16.clone()
    hp = torch.tensor([0.01, 0.9, 0.0, 1e-2, 0.5, 0, 0, 0], device=DEV)
    ops.linear_wgrad_defer(_put(dz, True), _put(x, True), a1.weight(0, g16), a1.bias(0, g16), a1,
                           other.offset, g16, ops.sgd_fusion(a1, hp, False, False, other.offset))
    torch.cuda.synchronize()
    _eq(a1.weight(0, g16), ex.bf16_rne(wW), "payload gW16")
    _eq(a1.bias(0, g16), ex.bf16_rne(wb), "payload gb16")
    keep = torch.ones(a1.numel, dtype=torch.bool, device=DEV)
    for slot in (mine_w, mine_b):
        keep[slot.offset:slot.offset + slot.numel] = False
    assert torch.equal(g16.view(torch.int16)[keep], g16_before.view(torch.int16)[keep])
    ops.sgd(a2, hp, False, False, offset=other.offset, numel=other.numel, grad_bf16=g16_before)
    _arenas_equal(a1, a2, "deferred update")
    assert torch.count_nonzero(a1.grad) == 0
    _cache.pop(("wgrad", rows, H, H, BF16))      # (128 MB of float64 oracle)


# =============================================================================================
# fp32 mode
# =============================================================================================
F32_SHAPES = [(70, 36, 9), (200, 136, 72)]


@pytest.mark.parametrize("rows,out_f,in_f", F32_SHAPES)
def test_linear_fwd_dgrad_f32(rows, out_f, in_f):
    """linear_fwd_f32 / linear_dgrad_f32 (v_mfma_f32_16x16x4_f32: a k-ordered fma chain), same
    oracle, every element equal; tanh forward within 1 fp32 ulp (module docstring)."""
    ops = _ops()
    for act in ("none", "relu", "tanh"):
        x, W, b, z = _fwd_case(rows, out_f, in_f, act, dtype=F32)
        out = _out((rows, out_f), F32, left=3, right=2)
        ops.linear_act(_put(x, True), _put(W, True), _put(b, True), act, out[1])
        _check_fwd(out, z, act, F32, f"fwd f32 {act}")
    dz, W, a, want = _dgrad_case(rows, out_f, in_f, dtype=F32)
    for act in ("relu", "tanh", "none"):
        out = _out((rows, in_f), F32, left=3, right=2)
        ops.linear_dgrad(_put(dz, True), _put(W, True), _put(a[act], True), act, out[1])
        _done(out, ex.f32(want[act]), f"dgrad f32 {act}")


@pytest.mark.parametrize("rows,out_f,in_f,splits", [(20, 36, 9, 1), (200, 136, 72, 4),
                                                     (9 * 32 + 5, 136, 72, 8)])
def test_linear_wgrad_f32(rows, out_f, in_f, splits):
    """Un-split with N % 4 != 0 (20 rows: one k-step); four splits; and 293 rows, whose ten
    32-deep k-steps go to eight splits in twos: the last three own none and must still deposit
    zeros in their slabs (the workspace starts as NaN)."""
    ops = _ops()
    dz, x, wW, wb = _wgrad_case(rows, out_f, in_f, dtype=F32)
    nbytes = ops.wgrad_workspace_bytes(rows, out_f, in_f, F32)
    assert nbytes == (0 if splits == 1 else splits * (out_f * in_f + out_f) * 4)
    gW, gb = _out_dense((out_f, in_f), F32), _out_dense((out_f,), F32)
    wsb, ws = _ws(ops, rows, out_f, in_f, F32)
    ops.linear_wgrad(_put(dz, True), _put(x, True), gW[1], gb[1], ws=ws)
    _done(gW, ex.f32(wW), "dW f32")
    _done(gb, ex.f32(wb), "db f32")
    if ws is not None:
        assert ex.guards_intact(wsb, ws)


def test_linear_wgrad_f32_refuses_split_with_n_not_multiple_of_4_before_launching():
    rows, out_f, in_f = 70, 36, 9
    ops = _ops()
    dz, x, _, _ = _wgrad_case(rows, out_f, in_f, dtype=F32)
    assert ops.wgrad_workspace_bytes(rows, out_f, in_f, F32) > 0
    gW, gb = _out_dense((out_f, in_f), F32), _out_dense((out_f,), F32)
    wsb, ws = _ws(ops, rows, out_f, in_f, F32)
    with pytest.raises(RuntimeError, match="linear_wgrad_f32: invalid argument"):
        ops.linear_wgrad(_put(dz, False), _put(x, False), gW[1], gb[1], ws=ws)
    torch.cuda.synchronize()
    for t in (ws, gW[1], gb[1]):
        assert torch.isnan(t).all(), "a kernel ran before the refusal"


# =============================================================================================
# operands the bf16 launchers do not take: refused on the host, nothing launched
# =============================================================================================
KMAJ_A = ("fwd", "dgrad", "gemm", "gemm_tile", "bwd_group")      # operand A is k-major
REFUSALS = [(l, b) for l in KMAJ_A + ("wgrad", "wgrad_out16", "wgrad_defer")
            for b in ("ld%8", "base+8B", "K%8", "2GiB")
            if b != "K%8" or l in KMAJ_A]      # (a weight gradient's K is the row count: free)


@pytest.mark.parametrize("launcher,bad", REFUSALS)
def test_bf16_launchers_refuse_unsupported_operands(launcher, bad):
    """ld % 8 != 0, a base 8 bytes off a 16-byte boundary, K % 8 != 0 on a k-major operand and an
    operand extent beyond the 2 GiB buffer range (docs/ARCHITECTURE.md §5): hipErrorInvalidValue
    before anything is launched -- the outputs keep their NaN."""
    lib, s = _lib(), _s()
    M = N = K = 4096 if launcher == "wgrad_defer" else 64
    A = torch.zeros(80 * 80 + 8, dtype=BF16, device=DEV)
    B = torch.zeros(80 * 80 + 8, dtype=BF16, device=DEV)
    out = torch.full((64 * 64,), ex.NAN, device=DEV)
    aux = torch.zeros(64 * 64, dtype=BF16, device=DEV)
    a_ptr, lda, k = A.data_ptr(), (4096 if launcher == "wgrad_defer" else 64), K
    if bad == "ld%8":
        lda += 4
    elif bad == "base+8B":
        a_ptr += 8
    elif bad == "K%8":
        k = K - 4
    else:
        lda = 1 << 30
    b_ptr, ldb, o = B.data_ptr(), lda if bad == "2GiB" else N, out.data_ptr()
    hp = torch.zeros(8, device=DEV)
    sg = (o, o, o, 0, hp.data_ptr(), 0, 0)
    calls = {
        "fwd": lambda: lib.linear_fwd_bf16(a_ptr, lda, b_ptr, K, 0, o, N, M, N, k, 0, s),
        "dgrad": lambda: lib.linear_dgrad_bf16(a_ptr, lda, b_ptr, N, aux.data_ptr(), N, o, N, M, N, k,
                                               0, s),
        "wgrad": lambda: lib.linear_wgrad_bf16(a_ptr, lda, b_ptr, ldb, o, o, M, N, k, 0, s),
        "wgrad_out16": lambda: lib.linear_wgrad_bf16_out16(a_ptr, lda, b_ptr, ldb, o, o, M, N, k, s),
        "wgrad_defer": lambda: lib.linear_wgrad_bf16_out16_defer(a_ptr, lda, b_ptr, ldb, o, o, M, N,
                                                                 72, sg, o, s),
        "gemm": lambda: lib.gemm_bf16(a_ptr, lda, 0, b_ptr, K, 0, M, N, k, o, N, s),
        "gemm_tile": lambda: lib.gemm_bf16_tile(a_ptr, lda, 0, b_ptr, K, 0, M, N, k, o, N, 128, s),
        "bwd_group": lambda: lib.bwd_group((a_ptr, lda, b_ptr, N, aux.data_ptr(), N, o, N, M, N, k, 0),
                                           None, None, None, s),
    }
    name = {"fwd": "linear_fwd_bf16", "dgrad": "linear_dgrad_bf16", "wgrad": "linear_wgrad_bf16",
            "wgrad_out16": "linear_wgrad_bf16_out16", "wgrad_defer": "linear_wgrad_bf16_out16_defer",
            "gemm": "gemm_bf16", "gemm_tile": "gemm_bf16_tile", "bwd_group": "bwd_group"}[launcher]
    if launcher == "wgrad_defer":
        assert lib.wgrad_defer_ok(M, N, 72)
    with pytest.raises(RuntimeError, match=f"{name}: invalid argument"):
        calls[launcher]()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a kernel ran before the refusal"


def test_register_staged_loop_refuses_an_x_major_tail_chunk():
    """An x-major operand with X % 8 != 0: the DMA loop's range check clips the chunk across the
    end of X (test_plain_gemm, M = 130 / N = 260), the register-staged loop's plain 16-byte load
    would run past the storage, so there it is refused."""
    A = torch.zeros(64 * 64, dtype=BF16, device=DEV)
    out = torch.full((64 * 64,), ex.NAN, device=DEV)
    with _knobs(impl=1) as lib:
        with pytest.raises(RuntimeError, match="gemm_bf16: invalid argument"):
            lib.gemm_bf16(A.data_ptr(), 64, 1, A.data_ptr(), 64, 0, 60, 64, 64, out.data_ptr(), 64, _s())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a kernel ran before the refusal"


def test_largest_exactness_bound_reached():
    """(runs last in this file) the largest sum |a||b| + |bias| any test above relied on."""
    print(f"\nEXACT_BOUND largest sum |a||b| + |bias| checked: {ex.largest_bound:.0f} (2^24 = 16777216)")
    assert ex.largest_bound < ex.TWO24
