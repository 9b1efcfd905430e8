"""Use a trained model: ``Predictor`` turns a reference-format ``state_dict`` (a checkpoint file
or a dict in memory) into outputs, loss and accuracy / mean absolute error.

It wraps a single-rank :class:`~nnmpi_amd.engine.engine.MLPEngine` (``NoSync``): the hidden
layers run the engine's forward GEMMs and the output layer the forward-only head
(``csrc/kernels/head_eval.hip`` on the GPU, ``TorchOps.head_eval`` on the CPU) -- no gradient is
computed anywhere.  The layer widths come from the weight shapes; the activation and the loss are
not part of a ``state_dict`` and are given by the caller.
"""
from __future__ import annotations

import torch


def _widths_of(sd: dict) -> list:
    """Layer widths from the ``layers.{2i}.weight`` / ``.bias`` shapes; ValueError naming the key
    that is missing or has the wrong shape."""
    n = 0
    while f"layers.{2 * n}.weight" in sd or f"layers.{2 * n}.bias" in sd:
        n += 1
    if n == 0:
        raise ValueError("state_dict has no 'layers.0.weight': not a reference-format MLP")
    extra = sorted(k for k in sd if k not in {f"layers.{2 * i}.{p}" for i in range(n)
                                              for p in ("weight", "bias")})
    if extra:
        raise ValueError(f"state_dict has unexpected keys: {extra}")
    widths = []
    for i in range(n):
        wk, bk = f"layers.{2 * i}.weight", f"layers.{2 * i}.bias"
        for k in (wk, bk):
            if k not in sd:
                raise ValueError(f"state_dict is missing {k!r}")
        W, b = sd[wk], sd[bk]
        if W.dim() != 2 or (widths and W.shape[1] != widths[-1]):
            raise ValueError(f"{wk!r} has shape {tuple(W.shape)}, expected [out, "
                             f"{widths[-1] if widths else 'in'}]")
        if b.dim() != 1 or b.shape[0] != W.shape[0]:
            raise ValueError(f"{bk!r} has shape {tuple(b.shape)}, expected [{W.shape[0]}]")
        if not widths:
            widths.append(int(W.shape[1]))
        widths.append(int(W.shape[0]))
    return widths


class Predictor:
    """Outputs and metrics of a trained MLP.

    ``predict(X, classes=False)``: fp32 outputs ``[n, out]`` (logits for a cross-entropy model),
    or the int64 argmax ``[n]``.  ``evaluate(X, y)``: ``{"loss", "rows"}`` plus ``"accuracy"``
    (cross-entropy; ``y`` are int64 labels) or ``"mae"`` (MSE; ``y`` are the targets).  Inputs
    may live on any device; rows are processed ``batch_rows`` at a time."""

    def __init__(self, engine):
        self.engine = engine

    @classmethod
    def from_state_dict(cls, sd: dict, activation: str = "relu", loss: str = "mse",
                        dtype: str = "fp32", device: str = "auto", batch_rows: int = 4096):
        from .engine.arena import Arena
        from .engine.engine import MLPEngine
        from .engine.trainer import cpu_ops
        from .models.mlp import MLPSpec
        from .parallel.sync import NoSync
        from .utils.config import resolve_device
        if activation not in ("relu", "tanh") or loss not in ("mse", "xent"):
            raise ValueError(f"activation relu | tanh and loss mse | xent, got {activation!r}, {loss!r}")
        if dtype not in ("fp32", "bf16"):
            raise ValueError(f"dtype fp32 | bf16, got {dtype!r}")
        widths = _widths_of(sd)
        dev = torch.device(resolve_device(device) if device == "auto" else device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        tdtype = torch.bfloat16 if dtype == "bf16" else torch.float32
        spec = MLPSpec(tuple(widths), activation, loss)
        arena = Arena([spec.layer_shape(i) for i in range(spec.n_layers)], dev,
                      shadow_dtype=torch.bfloat16 if tdtype == torch.bfloat16 else None)
        arena.load_state_dict({k: v.detach().to(torch.float32) for k, v in sd.items()})
        arena.sync_shadow()
        if dev.type == "cuda":
            from .ops.hip_ops import HipOps
            ops = HipOps(dev)
        else:
            ops = cpu_ops(dev)
        eng = MLPEngine(spec, arena, ops, NoSync(arena), device=dev, dtype=tdtype,
                        rows_capacity=max(1, int(batch_rows)), lr=0.0, momentum=0.0,
                        use_graph=False)
        return cls(eng)

    @classmethod
    def from_checkpoint(cls, path: str, activation: str = "relu", loss: str = "mse",
                        dtype: str = "fp32", device: str = "auto", batch_rows: int = 4096):
        from .utils.checkpoint import load_state_dict
        return cls.from_state_dict(load_state_dict(path), activation=activation, loss=loss,
                                   dtype=dtype, device=device, batch_rows=batch_rows)

    @property
    def widths(self):
        return list(self.engine.spec.widths)

    def _x(self, X: torch.Tensor) -> torch.Tensor:
        eng = self.engine
        if X.dim() != 2 or X.shape[1] != eng.spec.widths[0]:
            raise ValueError(f"inputs must be [n, {eng.spec.widths[0]}], got {tuple(X.shape)}")
        return X.to(device=eng.device, dtype=eng.dtype)

    def predict(self, X: torch.Tensor, classes: bool = False) -> torch.Tensor:
        return self.engine.predict(self._x(X), classes=classes)

    def evaluate(self, X: torch.Tensor, y: torch.Tensor) -> dict:
        eng = self.engine
        out_f, n = eng.spec.widths[-1], X.shape[0]
        if y.shape[0] != n:
            raise ValueError(f"{n} input rows but {y.shape[0]} targets")
        if eng.loss_kind == "xent":
            m = eng.evaluate_metrics(self._x(X), labels=y.to(device=eng.device, dtype=torch.int64))
            rows = max(m["rows"], 1)
            return {"loss": m["loss_sum"] / rows, "accuracy": m["correct"] / rows, "rows": m["rows"]}
        Y = y.to(device=eng.device, dtype=torch.float32).reshape(n, out_f)
        m = eng.evaluate_metrics(self._x(X), Y=Y)
        cnt = max(m["rows"] * out_f, 1)
        return {"loss": m["loss_sum"] / cnt, "mae": m["abs_err_sum"] / cnt, "rows": m["rows"]}

