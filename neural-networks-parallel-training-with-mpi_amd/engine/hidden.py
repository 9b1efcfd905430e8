"""What a hidden layer is besides a GEMM: the row-wise ``--norm`` (norm.hip) and ``--dropout``
(dropout.hip) between layer i's GEMM and whatever reads its activations.  :class:`HiddenChain`
owns their buffers, the mask generator's state and the order of the two backward passes; the
engine's sequential body (the only one that takes them) calls ``forward`` per layer, ``backward``
on every dZ right after it was produced and ``tick`` once per pass.  With neither option it
allocates nothing and launches nothing."""
import torch

from ..ops.torch_ops import dropout_state


class HiddenChain:
    def __init__(self, spec, ops, rows_capacity: int, dtype, device, seed: int = 0, rank: int = 0):
        self.ops, self.act = ops, spec.activation
        self.norm = None if spec.norm == "none" else spec.norm
        self.p_drop = float(spec.dropout)
        self.seed, self.rank = int(seed) & (2 ** 64 - 1), int(rank)
        nh, w, R = spec.n_layers - 1, spec.widths, rows_capacity
        if not 0.0 <= self.p_drop < 1.0:     # (also NaN)
            raise ValueError(f"dropout must be in [0, 1), got {spec.dropout!r}")
        if self.p_drop and (nh > 256 or not 0 <= self.rank < 2 ** 24):
            raise ValueError("dropout: at most 256 hidden layers and ranks below 2^24")
        self.active = self.norm is not None or self.p_drop != 0.0
        # what the head / linear_dgrad epilogues apply: under dropout they see the dropped
        # activations, and dropout_bwd applies act' through the undropped ones
        self.epilogue_act = "none" if self.p_drop else self.act
        # with a norm: every hidden layer's pre-activations (the backward recomputes the
        # normalised row from them) and per-row (mu, rstd) -- allocated once, like the engine's
        n = nh if self.norm is not None else 0
        self.zpre = [torch.zeros(R, w[i + 1], dtype=dtype, device=device) for i in range(n)]
        self.nstats = [torch.zeros(R, 2, dtype=torch.float32, device=device) for i in range(n)]
        # with dropout: every hidden layer's dropped activations (the engine's acts keep the
        # undropped ones) and the generator's device state (seed lo, seed hi, pass, unused)
        self.drop = [torch.zeros(R, w[i + 1], dtype=dtype, device=device)
                     for i in range(nh if self.p_drop else 0)]
        self.dstate = dropout_state(self.seed, 0, device) if self.p_drop else None

    def forward(self, i: int, h, W, b, out, rows: int, train: bool):
        """Layer i: ``out`` = act(norm(h W^T + b)).  Returns what the next reader gets: ``out``,
        or with ``train`` under dropout its dropped copy (the forward-only paths run without
        dropout and do not advance the pass number)."""
        if self.norm is None:
            self.ops.linear_act(h, W, b, self.act, out)
        else:
            z = self.zpre[i][:rows]
            self.ops.linear_act(h, W, b, "none", z)
            self.ops.norm_act(z, self.norm, self.act, out, self.nstats[i][:rows])
        if not (train and self.p_drop):
            return out
        d = self.drop[i][:rows]
        self.ops.dropout(out, d, self.dstate, self.p_drop, i, self.rank)
        return d

    def reads(self, i: int, acts, rows: int):
        """Layer i as layer i + 1, the head and the next weight gradient read it in training."""
        return (self.drop or acts)[i][:rows]

    def backward(self, i: int, dz, acts, rows: int):
        """In place on ``dz`` = dZ_i, right after the head / linear_dgrad left dL/d(``reads``) in
        it and before anything reads it: dropout_bwd (the forward's mask, scale, act' through the
        undropped acts[i]), THEN norm_bwd -> dL/dz_i.  ``i < 0`` (the input): nothing."""
        if i >= 0 and self.p_drop:
            self.ops.dropout_bwd(dz, acts[i][:rows], self.dstate, self.p_drop, self.act, i,
                                 self.rank)
        if i >= 0 and self.norm is not None:
            self.ops.norm_bwd(dz, self.zpre[i][:rows], self.nstats[i][:rows], self.norm)

    def tick(self):
        """The last dropout launch of every training pass: the next one draws another mask."""
        if self.p_drop:
            self.ops.dropout_tick(self.dstate)

    # the generator's pass number and seed, on the current stream (the engine makes its own so)
    def get_step(self) -> int:
        return int(self.dstate[2].item()) if self.p_drop else 0     # (synchronises the stream)

    def set_step(self, n: int):
        if self.p_drop:
            self.dstate[2:3].fill_(int(n))

    def set_seed(self, seed: int):
        self.seed = int(seed) & (2 ** 64 - 1)
        if self.p_drop:
            self.dstate[:2].copy_(dropout_state(self.seed, 0, "cpu")[:2])
