"""Shared by tests/test_train_head_host.py and tests/test_gpu_train_head.py: the cases of the HIP classifier head, its float64
reference in numpy, the same formulas on torch's CPU operators (the fp32 run is the error yardstick), and the bound.

The head: x [B, HW, C] -> pooled = mean over HW -> logits = pooled . W^T + b -> probs = softmax -> loss = mean of -log_softmax[target];
backward from an upstream gradient g of the loss.  Inputs are float32 values throughout (bf16 cases: float32 values that bf16
represents exactly), held in float64 for the reference, so every implementation starts from the same numbers.
"""

from __future__ import annotations

import functools
import itertools
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 10.0          # the project's margin over the fp32 reference's own error
LOGIT_GAP = 1e-2       # every row's two largest logits differ by at least this: the arg-max is not a rounding question
BS, HWS, CS, KS, DTYPES = (1, 3, 64, 257), (1, 49, 50), (8, 520, 512, 2048), (2, 3, 16), ("fp32", "bf16")


class Case(NamedTuple):
    B: int
    HW: int
    C: int
    K: int
    dtype: str
    scale: float = 1.0              # multiplies W: 100 puts |logits| beyond 80
    one_class: Optional[int] = None   # every target is this class

    @property
    def id(self) -> str:
        tag = ("-big" if self.scale != 1.0 else "") + ("" if self.one_class is None else f"-only{self.one_class}")
        return f"B{self.B}-HW{self.HW}-C{self.C}-K{self.K}-{self.dtype}{tag}"


GRID = [Case(b, hw, c, k, dt) for b, hw, c in itertools.product(BS, HWS, CS) for k, dt in itertools.product(KS, DTYPES)]   # x is shared by neighbours
BIG_LOGITS = [Case(64, 49, 512, 3, dt, scale=100.0) for dt in DTYPES]
ONE_CLASS = [Case(3, 49, 512, 2, dt, one_class=1) for dt in DTYPES]
CASES = GRID + BIG_LOGITS + ONE_CLASS


def to_bf16_values(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    return torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=2)
def _activations(B: int, HW: int, C: int) -> np.ndarray:
    """Post-ReLU-looking activations ~ N(0.5, 1), float32 [B, HW, C]; one array per shape, shared by the K / dtype cases."""
    rng = np.random.default_rng(1000003 * B + 1009 * HW + C)
    x = rng.standard_normal((B, HW, C), dtype=np.float32)
    x += np.float32(0.5)
    x.setflags(write=False)
    return x


def _logits64(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (x.sum(axis=1, dtype=np.float64) / x.shape[1]) @ w.astype(np.float64).T + b.astype(np.float64)


def logit_gap(logits: np.ndarray) -> np.ndarray:
    """Per row: the largest logit minus the second largest."""
    top = np.sort(logits, axis=1)
    return top[:, -1] - top[:, -2]


def make(case: Case) -> Dict[str, np.ndarray]:
    """x float32 [B, HW, C] (bf16-representable for a bf16 case), w float32 [K, C], b float32 [K], t int64 [B].  Rows whose two
    largest float64 logits come closer than LOGIT_GAP are drawn again until none is left."""
    rng = np.random.default_rng(hash((case.B, case.HW, case.C, case.K, case.dtype == "bf16", case.scale)) % (2 ** 32))
    x = _activations(case.B, case.HW, case.C)
    if case.dtype == "bf16":
        x = to_bf16_values(x)
    w = (rng.standard_normal((case.K, case.C)) * (2.0 * case.scale / np.sqrt(case.C))).astype(np.float32)
    b = rng.standard_normal(case.K).astype(np.float32)
    for _ in range(100):
        close = np.nonzero(logit_gap(_logits64(x, w, b)) < LOGIT_GAP)[0]
        if close.size == 0:
            break
        if not x.flags.writeable:
            x = x.copy()
        fresh = rng.standard_normal((close.size, case.HW, case.C), dtype=np.float32) + np.float32(0.5)
        x[close] = to_bf16_values(fresh) if case.dtype == "bf16" else fresh
    else:
        raise AssertionError(f"{case.id}: rows with close logits remain")
    t = rng.integers(0, case.K, case.B).astype(np.int64) if case.one_class is None else np.full(case.B, case.one_class, dtype=np.int64)
    return {"x": x, "w": w, "b": b, "t": t}


def head_f64(x: np.ndarray, w: np.ndarray, b: np.ndarray, t: np.ndarray, g: float = 1.0) -> Dict[str, np.ndarray]:
    """The head and its gradients in float64 numpy.  dx is [B, 1, C]: the same row for every one of the HW positions."""
    B, HW, _ = x.shape
    w, b = w.astype(np.float64), b.astype(np.float64)
    pooled = x.sum(axis=1, dtype=np.float64) / HW
    logits = pooled @ w.T + b
    z = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    probs = e / s
    rows = np.arange(B)
    loss = float(np.mean(np.log(s[:, 0]) - z[rows, t]))
    onehot = np.zeros_like(probs)
    onehot[rows, t] = 1.0
    dlogits = (probs - onehot) * (g / B)
    return {"pooled": pooled, "logits": logits, "probs": probs, "loss": np.float64(loss), "dlogits": dlogits, "dw": dlogits.T @ pooled,
            "db": dlogits.sum(axis=0), "dx": ((dlogits @ w) / HW)[:, None, :]}


def head_torch(x: np.ndarray, w: np.ndarray, b: np.ndarray, t: np.ndarray, dtype: torch.dtype, g: float = 1.0) -> Dict[str, np.ndarray]:
    """The same formulas on torch's CPU operators in `dtype` (F.adaptive_avg_pool2d, F.linear, F.softmax, F.cross_entropy, autograd),
    returned as float64 arrays; dx is the full [B, HW, C]."""
    B, HW, C = x.shape
    xt = torch.tensor(x, dtype=dtype).permute(0, 2, 1).reshape(B, C, HW, 1).requires_grad_(True)   # NCHW with H = HW, W = 1
    wt, bt = torch.tensor(w, dtype=dtype, requires_grad=True), torch.tensor(b, dtype=dtype, requires_grad=True)
    pooled = torch.flatten(F.adaptive_avg_pool2d(xt, 1), 1)
    logits = F.linear(pooled, wt, bt)
    logits.retain_grad()
    probs = F.softmax(logits.detach().clone(), dim=1)
    loss = F.cross_entropy(logits, torch.from_numpy(t))
    loss.backward(torch.tensor(g, dtype=dtype))
    n = lambda v: v.detach().double().numpy()   # noqa: E731
    return {"pooled": n(pooled), "logits": n(logits), "probs": n(probs), "loss": n(loss), "dlogits": n(logits.grad), "dw": n(wt.grad), "db": n(bt.grad),
            "dx": n(xt.grad.reshape(B, C, HW).permute(0, 2, 1))}


NAMES = ("pooled", "logits", "probs", "loss", "dlogits", "dw", "db", "dx")


def err(a: np.ndarray, ref: np.ndarray) -> float:
    """Largest absolute difference (broadcasting ref); a NaN or infinity anywhere is infinite error."""
    d = np.abs(np.asarray(a, dtype=np.float64) - ref)
    return float("inf") if not np.all(np.isfinite(d)) else float(d.max()) if d.size else 0.0


def ulp(value: float, dtype: str) -> float:
    """The spacing of `dtype` ("fp32" / "bf16") at |value|."""
    f = float(np.spacing(np.float32(abs(value))))
    return f if dtype == "fp32" else f * 2.0 ** 16


def bound(ref: np.ndarray, fp32: np.ndarray, dtype: str = "fp32") -> float:
    """MARGIN x the error of torch's fp32 CPU head (`fp32`) against the float64 reference `ref` on the same inputs, floored at one
    ulp of the tensor's storage dtype at its largest reference magnitude."""
    return max(MARGIN * err(fp32, ref), ulp(float(np.abs(ref).max()), dtype))
