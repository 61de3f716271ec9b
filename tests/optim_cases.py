"""Shared by tests/test_train_optim_host.py and tests/test_gpu_train_optim.py: the float64 Adam reference, its deliberately wrong
variants, torch's fp32 CPU Adam as the error yardstick, and the bound.

Inputs are float32 values throughout (held in float64 for the reference), so every implementation starts from the same numbers.
The reference is plain numpy in float64: torch.optim.Adam's documented update with amsgrad=False, maximize=False.
"""

from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

LR, EPS, WEIGHT_DECAY, BETAS, STEPS = 1e-2, 1e-3, 0.1, (0.9, 0.999), 3   # every term of the update is visible at these values
MARGIN = 10.0   # the project's margin over the fp32 reference's own error

Hyper = Union[float, Callable[[int, int], float]]   # a constant, or f(step index from 0, parameter index)
MUTANTS = ("no_weight_decay", "decoupled_decay", "no_bias_correction", "eps_inside_sqrt", "betas_swapped", "shared_step_count")


def _at(h: Hyper, k: int, i: int) -> float:
    return float(h(k, i)) if callable(h) else float(h)


def adam_f64(params: Sequence[np.ndarray], grads: Sequence[Sequence[Optional[np.ndarray]]], lr: Hyper = LR, betas: Tuple[float, float] = BETAS,
             eps: float = EPS, weight_decay: Hyper = WEIGHT_DECAY, variant: str = "adam", state=None):
    """len(grads) Adam steps in float64.  params: one array per parameter; grads[k][i]: step k's gradient of parameter i, or None
    (that parameter is skipped and keeps no state, its own step count does not advance).  state: (m, v, t) lists to continue from.
    Returns (p, m, v, t): lists per parameter; m, v are None and t is 0 for a parameter never stepped.
    variant: "adam", or one of MUTANTS -- the same code with one deliberate mistake."""
    assert variant == "adam" or variant in MUTANTS, variant
    b1, b2 = betas
    if variant == "betas_swapped":
        b1, b2 = b2, b1
    p = [np.asarray(x, dtype=np.float64).copy() for x in params]
    if state is None:
        m, v, t = [None] * len(p), [None] * len(p), [0] * len(p)
    else:
        m, v, t = ([None if a is None else np.asarray(a, dtype=np.float64).copy() for a in state[0]],
                   [None if a is None else np.asarray(a, dtype=np.float64).copy() for a in state[1]], list(state[2]))
    for k, step_grads in enumerate(grads):
        for i, g in enumerate(step_grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64)
            lr_i, wd_i = _at(lr, k, i), _at(weight_decay, k, i)
            if m[i] is None:
                m[i], v[i] = np.zeros_like(p[i]), np.zeros_like(p[i])
            t[i] += 1
            ti = k + 1 if variant == "shared_step_count" else t[i]   # (the mistake: one global counter for every parameter)
            if variant == "decoupled_decay":
                p[i] = p[i] * (1.0 - lr_i * wd_i)
            elif variant != "no_weight_decay":
                g = g + wd_i * p[i]
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** ti, 1.0 - b2 ** ti
            if variant == "no_bias_correction":
                bc1 = bc2 = 1.0
            if variant == "eps_inside_sqrt":
                denom = np.sqrt(v[i] / bc2 + eps)
            else:
                denom = np.sqrt(v[i]) / np.sqrt(bc2) + eps
            p[i] = p[i] - (lr_i / bc1) * m[i] / denom
    return p, m, v, t


def torch_adam(params: Sequence[np.ndarray], grads: Sequence[Sequence[Optional[np.ndarray]]], dtype: torch.dtype, lr: Hyper = LR,
               betas: Tuple[float, float] = BETAS, eps: float = EPS, weight_decay: Hyper = WEIGHT_DECAY):
    """The same steps on torch.optim.Adam on the CPU in `dtype` (one param group per parameter, so lr and weight_decay may differ
    per parameter and per step).  Returns (p, m, v, t) as adam_f64, as float64 arrays."""
    ps = [torch.nn.Parameter(torch.tensor(np.asarray(x), dtype=dtype)) for x in params]
    opt = torch.optim.Adam([{"params": [q], "lr": _at(lr, 0, i), "weight_decay": _at(weight_decay, 0, i)} for i, q in enumerate(ps)], betas=betas, eps=eps)
    for k, step_grads in enumerate(grads):
        for i, (q, g) in enumerate(zip(ps, step_grads)):
            opt.param_groups[i]["lr"], opt.param_groups[i]["weight_decay"] = _at(lr, k, i), _at(weight_decay, k, i)
            q.grad = None if g is None else torch.tensor(np.asarray(g), dtype=dtype)
        opt.step()
    p = [q.detach().double().numpy() for q in ps]
    m = [opt.state[q]["exp_avg"].double().numpy() if q in opt.state else None for q in ps]
    v = [opt.state[q]["exp_avg_sq"].double().numpy() if q in opt.state else None for q in ps]
    t = [int(opt.state[q]["step"]) if q in opt.state else 0 for q in ps]
    return p, m, v, t


def err(a: np.ndarray, ref: np.ndarray) -> float:
    """Largest absolute difference; a NaN or infinity anywhere (the comparisons here are over finite values) is infinite error."""
    d = np.abs(np.asarray(a, dtype=np.float64) - ref)
    return float("inf") if not np.all(np.isfinite(d)) else float(d.max()) if d.size else 0.0


def bound(ref: np.ndarray, fp32: np.ndarray) -> float:
    """MARGIN x the error of torch's fp32 CPU Adam (`fp32`) against the float64 reference `ref` on the same inputs, floored at one
    fp32 ulp of the tensor's largest reference magnitude."""
    floor = float(np.spacing(np.float32(np.abs(ref).max()))) if ref.size else 0.0
    return max(MARGIN * err(fp32, ref), floor)


def mixed_scale(rng: np.random.Generator, shape) -> np.ndarray:
    """Gradients of mixed scale: normal values times 10^u, u uniform in [-3, 1], rounded to float32."""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 1.0, shape)).astype(np.float32)


def make_problem(sizes: Sequence[int], steps: int = STEPS, seed: int = 0) -> Tuple[List[np.ndarray], List[List[np.ndarray]]]:
    """float32 parameters ~ N(0, 1) of the given element counts and `steps` sets of mixed-scale gradients."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = [[mixed_scale(rng, n) for n in sizes] for _ in range(steps)]
    return params, grads
