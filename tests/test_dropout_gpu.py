"""--dropout on the GPU (dropout.hip): kernels against TorchOps bit for bit, refusals, the engine
against float64 autograd with the reference mask, graph replay, evaluation, checkpoints."""
import pytest
import torch

import nnmpi_amd  # noqa: F401
from _exact import (NAN, SENTINEL_BF16, SENTINEL_F32, bf16_ulp_apart, embed, f32_ulp_apart,
                    guards_intact)
from nnmpi_amd.ops.torch_ops import TorchOps, dropout_consts, dropout_keep, dropout_state
from test_dropout_cpu import make_engine, reference_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# (rows, H, dtype, pad right of a row; 8 left): 16-byte chunks of 8 bf16 / 4 fp32
SHAPES = [(1, 8, BF16, 8),        # one chunk
          (3, 24, BF16, 8),       # partial last wave
          (5, 520, BF16, 0),      # row stride 528
          (2, 8192, BF16, 8),     # widest row accepted, two blocks
          (4, 12, F32, 8),        # vector form
          (3, 1028, F32, 8),      # vector form
          (7, 3, F32, 8),         # scalar form, call groups straddling rows
          (5, 13, F32, 8)]        # scalar form
WHERE = [(0, 0, 0), (5, 2, 3)]    # (pass, layer, rank)
SEED = 0x1234567887654321


def _hip():
    from nnmpi_amd.ops.hip_ops import HipOps
    return HipOps(DEV)


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("where", WHERE, ids=str)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,H,dtype,right", SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_kernels_vs_torch_ops(rows, H, dtype, right, p, where, acts=("relu", "none", "tanh")):
    """Operands inside poisoned buffers.  Forward, backward under relu / none: the bits of TorchOps.
    tanh: zeros exactly where the reference has them, the rest within 1 ulp of float64."""
    step, layer, rank = where
    g = torch.Generator().manual_seed(1000 * H + rows)
    a = (0.9 * torch.tanh(torch.randn(rows, H, generator=g))).to(dtype)    # (1 - a^2 is never 0)
    dd = torch.randn(rows, H, generator=g).to(dtype)
    state, ref = dropout_state(SEED, step, DEV), TorchOps("cpu")
    sent = SENTINEL_BF16 if dtype == BF16 else SENTINEL_F32
    want_d = torch.empty_like(a)
    ref.dropout(a, want_d, state.cpu(), p, layer, rank)
    for act in acts:
        want = dd.clone()
        ref.dropout_bwd(want, a, state.cpu(), p, act, layer, rank)
        ab, av = embed(a.to(DEV), 1, 8, NAN, right)
        db, dv = embed(torch.zeros_like(av), 1, 8, sent, right)
        gb, gv = embed(dd.to(DEV), 1, 8, sent, right)
        _hip().dropout(av, dv, state, p, layer, rank)
        _hip().dropout_bwd(gv, av, state, p, act, layer, rank)
        got_d, got = dv.cpu(), gv.cpu()
        assert guards_intact(db, dv) and guards_intact(gb, gv) and torch.equal(_bits(av), _bits(a))
        assert torch.equal(_bits(got_d), _bits(want_d)), act
        if act != "tanh":
            assert torch.equal(_bits(got), _bits(want)), act
            continue
        keep = dropout_keep(state, p, layer, rank, rows, H)
        exact = dd.double() * dropout_consts(p)[1] * (1 - a.double() ** 2)
        assert torch.equal(got == 0, ~keep) and torch.equal(want == 0, ~keep)
        apart = (bf16_ulp_apart if dtype == BF16 else f32_ulp_apart)(got[keep], exact[keep])
        assert float(apart.max()) <= 1, float(apart.max())


def test_second_trip_of_the_grid_loop():
    """1025 x 8192 fp32: 2,099,200 chunks, 2,048 more than one trip of the full grid holds."""
    test_kernels_vs_torch_ops(1025, 8192, F32, 0, 0.5, WHERE[1], acts=("relu",))


def test_forms_draw_one_mask_and_refusals():
    """4 x 12 fp32 on 16-byte accesses and, one element further, on scalar ones: the same bits.
    bf16 H % 8 != 0, H > 8192 and an output overlapping the input raise before a launch."""
    ops, state, out = _hip(), dropout_state(SEED, 1, DEV), []
    a = torch.randn(4, 12, generator=torch.Generator().manual_seed(0))
    for off in (0, 1):
        buf = torch.zeros(2, 4 * 12 + 4, device=DEV)
        av, dv = (b[off:off + 48].view(4, 12) for b in buf)
        av.copy_(a)
        ops.dropout(av, dv, state, 0.5, 1, 0)
        out.append(dv.cpu())
    assert torch.equal(_bits(out[0]), _bits(out[1])) and 0 < int((out[0] == 0).sum()) < 48
    for rows, H, dtype in ((2, 12, BF16), (1, 8200, BF16), (1, 8196, F32)):
        a = torch.zeros(rows, H, dtype=dtype, device=DEV)
        with pytest.raises(RuntimeError):
            ops.dropout(a, torch.ones_like(a), state, 0.5, 0, 0)
    a = torch.zeros(4, 16, device=DEV)
    for d in (a, a[1:3]):      # the same matrix, a part of it
        with pytest.raises(RuntimeError):
            ops.dropout(a[:d.shape[0]], d, state, 0.5, 0, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("widths,dtype,norm", [((16, 64, 64, 1), BF16, "none"),
                                               ((16, 64, 64, 1), BF16, "layer"),
                                               ((2, 3, 1), F32, "none")], ids=str)
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_engine_step_vs_float64_autograd(act, widths, dtype, norm):
    """One step at p = 0.5 against float64 autograd with the reference masks.  fp32: the bounds
    of test_norm_gpu.py's fp32 engine (29 rows: from 33 on the fp32 weight gradient splits K and
    refuses input widths that are no multiple of 4).  bf16: a gradient passes at most 13
    roundings to bf16 of 2^-9 each (weight shadows, z / a, three per layer on the way back; the
    mask's factor 2 is exact): loss and every layer's update (weight and bias together: the
    one-element output bias is a sum over rows that cancels, 0.12 off alone) within 2^-5 in
    relative norm.  relu is not continuous: a pre-activation within 3 * 2^-9 of 0 in units of
    its row's spread may take the other branch, 0.8 * 3 * 2^-9 = 0.47 % of standard-normal
    values, and a flipped gate moves that unit's whole term: sqrt(0.0047) = 0.068 more for relu
    (printed: with the layer norm, whose z is stored in bf16 before the gate, relu is 0.07 off)."""
    ar, eng, init, X, Y = make_engine(widths, act, norm, 0.5, _hip(), dtype,
                                      29 if dtype == F32 else 67, use_graph=False)
    before = ar.flat_params_forward_order().cpu().double()
    eng.step()
    loss, after = eng.loss(), ar.flat_params_forward_order().cpu().double()
    want_loss, want = reference_step(init, X.float(), Y, act, norm, 0.5)
    assert eng.schedule_name() == "sequential" and eng.dropout_step == 1
    sizes = [lin.weight.numel() + lin.bias.numel() for lin in init.linears()]
    rel = [float((g - w).norm() / w.norm())
           for g, w in zip((after - before).split(sizes), (want - before).split(sizes))]
    print(f"{act} {norm} {dtype}: loss {loss:.8f} / {want_loss:.8f}, parameters off by "
          f"{float((after - want).abs().max()):.3e}, updates off by", rel)
    if dtype == F32:
        assert loss == pytest.approx(want_loss, rel=1e-4)
        assert torch.allclose(after, want, atol=1e-5, rtol=1e-4)
    else:
        bound = 2.0 ** -5 + ((0.8 * 3 * 2.0 ** -9) ** 0.5 if act == "relu" else 0.0)
        assert loss == pytest.approx(want_loss, rel=2.0 ** -5) and max(rel) <= bound


def test_graph_replay_equals_eager_and_evaluation_ignores_dropout():
    """Four steps (one eager, three replays of one graph: the pass is read on the device) equal
    four eager steps bitwise; evaluate_metrics equals a p = 0 engine bitwise, counts no pass."""
    runs, model = [], ((16, 64, 64, 1), "relu", "layer")
    for graph in (True, False):
        ar, eng, _, X, Y = make_engine(*model, 0.5, _hip(), BF16, 67, use_graph=graph)
        if graph:
            plain, Xd, Yd = make_engine(*model, 0.0, _hip(), BF16, 67)[1], X.to(DEV), Y.to(DEV)
            assert eng.evaluate_metrics(Xd, Yd) == plain.evaluate_metrics(Xd, Yd)
            assert eng.dropout_step == 0
            eng.load_batch(Xd, Yd)
        losses = [(eng.step(), eng.loss())[1] for _ in range(4)]
        runs.append((losses, ar.flat_params_forward_order().cpu()))
        assert eng.dropout_step == 4 and bool(eng._graphs) == graph
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


def test_checkpoint_resume_is_bitwise(tmp_path):
    from nnmpi_amd.engine.trainer import run_worker
    from nnmpi_amd.utils.config import TrainConfig
    ck = str(tmp_path / "model.pt")
    cfg = TrainConfig(device="cuda", widths=[16, 64, 64, 1], n_samples=256, dtype="bf16",
                      print_rank="none", dropout=0.5, seed=7, nepochs=5)
    full = run_worker(cfg)
    run_worker(cfg.replace(nepochs=3, checkpoint=ck))
    res = run_worker(cfg.replace(resume=ck))
    assert res.losses == full.losses[3:] and torch.equal(res.final_params, full.final_params)
    st = torch.load(ck + ".train", weights_only=True)
    assert st["dropout_step"] == 3 and st["dropout_seed"] == 7
