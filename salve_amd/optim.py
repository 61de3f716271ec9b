"""HipAdam: torch.optim.Adam's update for every parameter in ONE HIP launch (salve_amd/csrc/optim_train.hip: salve_adam_step),
which also leaves behind the bf16 copy of each convolution weight that the bf16 training convolutions read (opt-in:
`training.get_optimizer(args, model, optim="hip")`, `python -m salve_amd.train --optim hip`; torch.optim.Adam stays the default).

HipAdam subclasses torch.optim.Adam and replaces `step` only, so `param_groups`, `state`, `state_dict()` and
`load_state_dict()` are torch's own: the same group keys and defaults for the installed torch, `state[p]` = {"step": a float32
CPU scalar tensor, "exp_avg", "exp_avg_sq"}, no state for a parameter that never received a gradient.  A state dict moves between
HipAdam and torch.optim.Adam in either direction, and a checkpoint's "optimizer" entry keeps torch's format.

Each `step()` describes THIS step: the parameters whose `.grad` is set, their gradient pointers (zero_grad() frees them every
iteration) and, per parameter, the scalars of its own step count and its group's lr / betas / eps / weight_decay, computed in
double and rounded to float32 once.  The table and the chunk map are written into one pinned host buffer and copied to the
device asynchronously on the current stream, followed by the launch: no device synchronisation (torch's caching allocators keep
both buffers alive until the stream has passed them).

What it does not do: amsgrad, maximize, capturable, differentiable, decoupled weight decay (AdamW), sparse gradients, CPU /
non-contiguous / non-float32 parameters or gradients (all raise), parameters on more than one device.

bf16 shadows (`bf16_shadow=True`): every 4-D parameter (a convolution weight) that is stepped gets a bf16 tensor of its shape,
filled by the kernel with the new value rounded as `p.to(torch.bfloat16)` rounds.  `current_shadow(p)` hands it out only while
it is provably current: the step records the parameter's `data_ptr()` and `_version` (the HIP step writes through raw pointers
and bumps no version; every torch in-place write -- load_state_dict, copy_, mul_ -- does).  Anything else means: cast as before.
A write through `p.data` bumps no version and is not seen -- as it is not seen by autograd.  The step rewrites a copy in place:
each copy counts its steps, and the backward pass of a convolution that read one raises if the optimiser has stepped since its
forward (the weights it saved are gone), where torch would raise for its version counter.  The shadows are no optimiser state:
they are not saved, the first step after a load rewrites them.
"""

from __future__ import annotations

import ctypes
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from salve_amd import _lib

CHUNK = _lib.ADAM_CHUNK   # elements per workgroup (include/salve_hip.h: SALVE_ADAM_CHUNK)
MAX_SEGMENT = 2 ** 62     # (element offsets are 64-bit on both sides)
OPTIMS = ("torch", "hip")
_SHADOW_ATTR = "_salve_bf16_shadow"
GENERATION_ATTR = "_salve_generation"   # on a shadow tensor: how many steps have written it


class Segment(NamedTuple):
    """One parameter tensor of one step: device addresses (shadow 0 = none), length, its group's hyperparameters and `t`, the
    parameter's own step count AFTER this step."""
    param: int
    grad: int
    exp_avg: int
    exp_avg_sq: int
    shadow: int
    n: int
    lr: float
    beta1: float
    beta2: float
    eps: float
    weight_decay: float
    t: int


def adam_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, t: int) -> Dict[str, np.float32]:
    """The per-segment scalars of salve_adam_segment_t, each computed in double and rounded to float32 once."""
    lr, beta1, beta2 = float(lr), float(beta1), float(beta2)
    return {
        "step_size": np.float32(lr / (1.0 - beta1 ** t)),
        "sqrt_bc2": np.float32(math.sqrt(1.0 - beta2 ** t)),
        "beta1": np.float32(beta1),
        "beta2": np.float32(beta2),
        "eps": np.float32(float(eps)),
        "weight_decay": np.float32(float(weight_decay)),
        "one_minus_beta1": np.float32(1.0 - beta1),
        "one_minus_beta2": np.float32(1.0 - beta2),
    }


def chunk_count(n: int) -> int:
    return (n + CHUNK - 1) // CHUNK


def build_chunk_map(lengths) -> np.ndarray:
    """The chunk map of segments of `lengths` elements, in their order: per segment ceil(n / CHUNK) ADAM_CHUNK_DTYPE records (segment
    index, element offset), offsets ascending; an empty segment gets no chunk.  (Shared with dist_train.FlatBucket.)"""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    counts = (n + (CHUNK - 1)) // CHUNK
    chunk_map = np.zeros(int(counts.sum()), dtype=_lib.ADAM_CHUNK_DTYPE)
    chunk_map["segment"] = np.repeat(np.arange(len(n), dtype=np.int32), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)   # index of each chunk's segment's first chunk
    chunk_map["offset"] = (np.arange(len(chunk_map), dtype=np.int64) - first) * CHUNK
    return chunk_map


def build_tables(segments: List[Segment]) -> Tuple[np.ndarray, np.ndarray]:
    """(table, chunk_map) of salve_adam_step for `segments`, in their order: one ADAM_SEGMENT_DTYPE record each, and per segment
    ceil(n / CHUNK) ADAM_CHUNK_DTYPE records (segment index, element offset), offsets ascending.  An empty segment gets a record
    and no chunk."""
    table = np.zeros(len(segments), dtype=_lib.ADAM_SEGMENT_DTYPE)
    scalars: Dict[tuple, tuple] = {}   # a model has a handful of distinct (hyperparameters, t): computed once each
    rows = []
    for i, s in enumerate(segments):
        if s.t < 1:
            raise ValueError(f"segment {i}: step count {s.t} (the count AFTER the step is at least 1)")
        if not 0 <= s.n < MAX_SEGMENT:
            raise ValueError(f"segment {i}: {s.n} elements")
        key = s[6:]
        if key not in scalars:
            scalars[key] = tuple(adam_scalars(*key).values())
        rows.append(scalars[key])
    for k, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "shadow_bf16", "n")):
        table[name] = [s[k] for s in segments]
    for k, name in enumerate(_lib.ADAM_SEGMENT_DTYPE.names[6:]):   # (adam_scalars returns them in the record's order)
        table[name] = [r[k] for r in rows]
    return table, build_chunk_map(table["n"])


def current_shadow(p: Tensor) -> Optional[Tensor]:
    """The bf16 copy HipAdam's last step wrote for parameter `p` if it is provably current (same storage address, same
    version counter as when it was written), else None: the caller casts."""
    rec = getattr(p, _SHADOW_ATTR, None)
    if rec is None:
        return None
    shadow, ptr, version = rec
    if p.data_ptr() != ptr or p._version != version or shadow.device != p.device or shadow.shape != p.shape:
        return None
    return shadow


def _refuse_options(group: dict) -> None:
    for key in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "foreach", "fused"):
        if group.get(key, False):   # (foreach / fused select among torch's own implementations: None and False are accepted)
            raise ValueError(f"HipAdam does not implement {key}=True")
    for key in ("lr", "eps", "weight_decay"):
        if isinstance(group[key], Tensor):
            raise ValueError(f"HipAdam takes {key} as a Python number, not a tensor (it is read on the host every step)")
    if not 0.0 <= group["betas"][0] < 1.0 or not 0.0 <= group["betas"][1] < 1.0:
        raise ValueError(f"HipAdam: betas must lie in [0, 1), got {group['betas']}")


class HipAdam(torch.optim.Adam):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) whose `step` is one salve_adam_step launch.  bf16_shadow: also
    keep a bf16 copy of every 4-D parameter (module docstring)."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 amsgrad: bool = False, *, foreach: Optional[bool] = None, maximize: bool = False, capturable: bool = False,
                 differentiable: bool = False, fused: Optional[bool] = None, decoupled_weight_decay: bool = False, bf16_shadow: bool = False):
        _refuse_options({"lr": lr, "eps": eps, "weight_decay": weight_decay, "betas": betas, "amsgrad": amsgrad, "foreach": foreach,
                         "maximize": maximize, "capturable": capturable, "differentiable": differentiable, "fused": fused,
                         "decoupled_weight_decay": decoupled_weight_decay})
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         capturable=capturable, differentiable=differentiable)
        for group in self.param_groups:
            _refuse_options(group)
        self.bf16_shadow = bool(bf16_shadow)
        self._shadows: Dict[int, Tensor] = {}   # id(parameter) -> its bf16 copy (not optimiser state: never saved)

    # ---- this step's description -------------------------------------------------------------------------------------------
    def _active(self) -> List[Tuple[dict, Tensor]]:
        """(group, parameter) for every parameter that has a gradient, in param_groups order (torch's order)."""
        return [(group, p) for group in self.param_groups for p in group["params"] if p.grad is not None]

    def _validate(self, active: List[Tuple[dict, Tensor]]) -> None:
        """Every refusal -- options, tensors, and the state a parameter already has (a loaded one) -- before any state is created
        or advanced and before anything is launched."""
        device = None
        for group, p in active:
            _refuse_options(group)
            g = p.grad
            if g.is_sparse:
                raise RuntimeError("HipAdam does not support sparse gradients")
            for name, t in (("parameter", p), ("gradient", g)):   # (what the tensor is before where it is)
                if t.dtype != torch.float32:
                    raise RuntimeError(f"HipAdam: a {name} is {t.dtype}; parameters and gradients must be float32 (fp32 master weights)")
                if not t.is_contiguous():
                    raise RuntimeError(f"HipAdam: a {name} of shape {tuple(t.shape)} is not contiguous")
                if t.device.type != "cuda":
                    raise RuntimeError(f"HipAdam: a {name} is on {t.device}; the optimiser runs on the HIP device only (no CPU fallback)")
            if g.shape != p.shape:
                raise RuntimeError(f"HipAdam: gradient of shape {tuple(g.shape)} for a parameter of shape {tuple(p.shape)}")
            if device is None:
                device = p.device
            if p.device != device or g.device != device:
                raise RuntimeError(f"HipAdam: parameters on {device} and {p.device}; one device per optimiser")
            st = self.state[p] if p in self.state else {}
            if len(st) == 0:
                continue
            if set(st) != {"step", "exp_avg", "exp_avg_sq"}:
                raise RuntimeError(f"HipAdam: a parameter's state has the keys {sorted(st)}, expected step, exp_avg, exp_avg_sq")
            if not isinstance(st["step"], Tensor) or st["step"].device.type != "cpu" or st["step"].numel() != 1:
                raise RuntimeError("HipAdam: state step must be a CPU scalar tensor, as torch.optim.Adam keeps it without capturable / fused "
                                   "(it is read on the host every step; a device tensor would force a synchronisation)")
            for name in ("exp_avg", "exp_avg_sq"):
                t = st[name]
                if t.device != p.device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                    raise RuntimeError(f"HipAdam: state {name} must be a contiguous float32 tensor of the parameter's shape on {p.device}, "
                                       f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def _segments(self, active: List[Tuple[dict, Tensor]]) -> Tuple[List[Segment], List[Tensor]]:
        """The step's segments in `active`'s order, creating torch's state for a parameter seen for the first time (and its bf16
        copy).  `t` is the parameter's own step count + 1; the counters themselves are not advanced here.  Also returns the
        parameters whose shadow the step will write."""
        segs, shadowed = [], []
        for group, p in active:
            st = self.state[p]
            if len(st) == 0:   # as torch.optim.Adam._init_group
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            shadow = 0
            if self.bf16_shadow and p.dim() == 4:
                sh = self._shadows.get(id(p))
                if sh is None or sh.shape != p.shape or sh.device != p.device:
                    sh = self._shadows[id(p)] = torch.empty(p.shape, dtype=torch.bfloat16, device=p.device)
                shadow = sh.data_ptr()
                shadowed.append(p)
            b1, b2 = group["betas"]
            segs.append(Segment(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), shadow, p.numel(), float(group["lr"]), float(b1),
                                float(b2), float(group["eps"]), float(group["weight_decay"]), int(st["step"].item()) + 1))
        return segs, shadowed

    def plan(self) -> Tuple[np.ndarray, np.ndarray]:
        """The (table, chunk_map) the next `step()` would upload, for the gradients present now.  (Creates missing state, as the
        step would; advances no step count and launches nothing.)"""
        return build_tables(self._segments(self._active())[0])

    # ---- the step ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active = self._active()
        self._validate(active)
        if not active:
            return loss
        lib = _lib.load()
        device = active[0][1].device
        segs, shadowed = self._segments(active)
        table, chunk_map = build_tables(segs)
        # one pinned buffer: [table | chunk map], copied asynchronously on the current stream, then the launch on the same stream
        tb, cb = table.nbytes, chunk_map.nbytes
        host = torch.empty(tb + cb, dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        view[:tb] = table.view(np.uint8)
        view[tb:] = chunk_map.view(np.uint8)
        with torch.cuda.device(device):
            dev = host.to(device, non_blocking=True)
            stream = torch.cuda.current_stream(device).cuda_stream
            st = lib.salve_adam_step(ctypes.c_void_p(dev.data_ptr()), len(table), ctypes.c_void_p(dev.data_ptr() + tb), len(chunk_map),
                                     ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(host.data_ptr() + tb), ctypes.c_void_p(stream))
        _lib.check(st, "salve_adam_step")
        torch._foreach_add_([self.state[p]["step"] for _, p in active], 1)
        for p in shadowed:   # current from here on, until torch writes the parameter
            sh = self._shadows[id(p)]
            setattr(sh, GENERATION_ATTR, getattr(sh, GENERATION_ATTR, 0) + 1)   # (a backward pass that saved the old contents refuses)
            setattr(p, _SHADOW_ATTR, (sh, p.data_ptr(), p._version))
        return loss
