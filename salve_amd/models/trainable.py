"""The early-fusion verifier as a TRAINABLE module: every convolution on the HIP fp32 entries, the rest in torch autograd.

Training stands behind the reference's scripts/train.py (fp32, no AMP, every released config).  A training step's FLOPs are
nearly all convolutions: their forward, backward-data and backward-weight run in salve_amd/csrc/conv_train_f32.hip
(salve_conv_f32_*).  torch autograd is the plumbing for what remains -- BatchNorm (batch statistics in train mode, running
statistics in eval mode), ReLU, residual adds, max-pool, average pool + fc and the loss.

Opt-in bf16 mixed precision (`set_train_precision("bf16")`): activations in bf16, every convolution on the HIP bf16 entries
(salve_amd/csrc/conv_train_bf16.hip, salve_conv_bf16_*) through `Conv2dBF16Function`, fp32 master weights, fp32 weight
gradients, BatchNorm in fp32 (upcast at its input), fp32 logits and loss.  bf16 needs no loss scaling.  fp32 stays the default.

Opt-in HIP BatchNorm (`set_train_norm("hip")`): every BatchNorm runs on salve_amd/csrc/norm_train.hip (salve_bn_*) through
`BatchNormHipFunction`, with the ReLU and the residual add that follow it fused in, forward and backward, in either precision;
in bf16 no cast remains around BatchNorm.  torch's BatchNorm stays the default.  On top of it `set_sync_norm(dist)` (`--sync-bn`)
takes the train-mode statistics over the rows of all data-parallel ranks: `SyncBatchNormHipFunction`, the same kernels behind split
entries with one all-gather between them, forward and backward.

With the opt-in HIP Adam (salve_amd/optim.py: HipAdam, `--optim hip`) the bf16 convolutions read the bf16 copy of a weight that
the optimiser's step wrote, instead of casting the fp32 master on every call, while that copy is provably current
(`optim.current_shadow`); otherwise they cast as before.  The same bits either way.

Opt-in HIP classifier head (`set_train_head("hip")`, `forward_loss` / `forward_packed_loss`): average pool, fc, softmax,
cross-entropy and the accuracy counts run on salve_amd/csrc/head_train.hip (salve_head_*) through `ClassifierHeadHipFunction`, one
fused forward and one fused backward, with the loss and the counts accumulated in a device record (salve_amd.evaluate.
DeviceClassMeter) so that an epoch never waits for the device between batches.  torch's head stays the default.

`TrainableEarlyFusionCEResnet` subclasses `EarlyFusionCEResnet`: the same parameters and buffers under the same names, so state
dicts move between the two with strict=True, and a checkpoint trained here loads into the inference model (fp16 or fp32 engine).
There is no CPU path: a CPU tensor raises (no F.conv2d fallback).
"""

from __future__ import annotations

import ctypes
from typing import List, Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from salve_amd import _lib
from salve_amd.models.early_fusion import EarlyFusionCEResnet, num_input_images
from salve_amd.optim import GENERATION_ATTR, current_shadow


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def _nhwc(x: Tensor, cp: int) -> Tensor:
    """[B, C, H, W] (any memory format) -> contiguous NHWC [B, H, W, cp], channels C..cp-1 zero."""
    b, c, h, w = x.shape
    if c == cp:
        return x.permute(0, 2, 3, 1).contiguous()
    out = torch.zeros((b, h, w, cp), dtype=x.dtype, device=x.device)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


def _pack_weight(w: Tensor, cp: int) -> Tensor:
    """torch [Cout, Cin, KH, KW] -> the kernel layout [Cout, KH, KW, cp] (input channels zero-padded to cp)."""
    return _nhwc(w, cp)


def _run(prefix: str, entry: str, desc: "_lib.ConvDesc", pass_: int, a: Tensor, b: Tensor, out: Tensor) -> None:
    """One `prefix`_`entry` call (salve_conv_f32 / salve_conv_bf16; forward / backward_data / backward_weight) on `prefix`'s workspace."""
    lib = _lib.load()
    fn = f"{prefix}_{entry}"
    nbytes = int(getattr(lib, prefix + "_workspace_bytes")(ctypes.byref(desc), pass_))
    if nbytes == 0:
        raise _lib.SalveHipError(f"{fn}: refused: {lib.salve_last_error().decode('utf-8', 'replace')}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    stream = torch.cuda.current_stream(a.device).cuda_stream
    st = getattr(lib, fn)(ctypes.byref(desc), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(stream))
    _lib.check(st, fn)


class _Conv2dFunction(torch.autograd.Function):
    """y = conv2d(x, weight, stride, padding) without bias on the HIP entries (forward / dgrad / wgrad): the one body of
    Conv2dF32Function and Conv2dBF16Function, which set `prefix` (the entries), `act` (the dtype of x, y, dx and of the weight as
    the kernels read it) and `why` (for the dtype refusal).  The weight is always the fp32 parameter and dW always fp32.

    x: CUDA [B, Cin, H, W] (channels_last memory is used as is; other layouts are copied); weight: torch layout [Cout, Cin, KH, KW].
    Returns channels_last [B, Cout, Ho, Wo].  Input channels that are not a multiple of 8 (the stem's 6 / 12 / 18) are zero-padded
    here; the stem's dgrad is never needed (the network input takes no gradient) and raises if asked.  dgrad is skipped when x
    needs no gradient.  shadow: None, or the weight already in `act` (same shape), used instead of casting it."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, stride: int, padding: int, packed: bool = False, shadow: Optional[Tensor] = None) -> Tensor:
        cls = ctx._forward_cls   # the class `apply` was called on
        who = cls.__name__
        for name, t, dt in (("x", x, cls.act), ("weight", weight, torch.float32)):
            if t.device.type != "cuda":
                raise RuntimeError(f"{who}: {name} is on {t.device}; the training convolutions run on the HIP device only (no CPU fallback)")
            if t.dtype != dt:
                raise RuntimeError(f"{who}: {name} must be {dt} ({cls.why}), got {t.dtype}")
        b, cin, h, w = x.shape
        cout, cin_w, kh, kw = weight.shape
        if packed:   # x carries the weight's input channels zero-padded to a multiple of 8 already (forward_packed)
            if cin != _pad8(cin_w):
                raise RuntimeError(f"{who}: weight takes {cin_w} input channels, a packed x needs {_pad8(cin_w)}, got {cin}")
            cin = cin_w
        elif cin_w != cin:
            raise RuntimeError(f"{who}: weight takes {cin_w} input channels, x has {cin}")
        cp = _pad8(cin)
        ho, wo = (h + 2 * padding - kh) // stride + 1, (w + 2 * padding - kw) // stride + 1
        desc = _lib.ConvDesc(b, h, w, cp, ho, wo, cout, kh, kw, stride, padding)
        xn = _nhwc(x.detach(), cp)
        if shadow is not None and (shadow.dtype != cls.act or shadow.shape != weight.shape or shadow.device != weight.device):
            raise RuntimeError(f"{who}: the weight's {cls.act} copy must have its shape and device, got {shadow.dtype} {tuple(shadow.shape)} on {shadow.device}")
        # bf16: cast once per forward, unless the optimiser left a current copy behind (salve_amd.optim.current_shadow: the same bits);
        # the packed copy is saved for the backward pass (for a 1 x 1 kernel it is a view of `shadow`, which the next optimiser step
        # rewrites in place: backward checks the copy's step count)
        wk = _pack_weight(weight.detach().to(cls.act) if shadow is None else shadow, cp)
        y = torch.empty((b, cout, ho, wo), dtype=cls.act, device=x.device, memory_format=torch.channels_last)
        _run(cls.prefix, "forward", desc, _lib.CONV_FWD, xn, wk, y)
        ctx.save_for_backward(xn, wk)
        ctx.desc = (b, h, w, cp, ho, wo, cout, kh, kw, stride, padding)
        ctx.cin = cin
        ctx.shadow = shadow
        ctx.shadow_generation = None if shadow is None else getattr(shadow, GENERATION_ATTR, None)
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        cls = ctx._forward_cls
        if ctx.shadow is not None and getattr(ctx.shadow, GENERATION_ATTR, None) != ctx.shadow_generation:
            raise RuntimeError(f"{cls.__name__}: the optimiser has stepped since this forward pass and rewritten the weight copy it saved; "
                               "call backward before optimizer.step()")
        xn, wk = ctx.saved_tensors
        desc = _lib.ConvDesc(*ctx.desc)
        b, h, w, cp = ctx.desc[:4]
        gyn = gy.to(cls.act).permute(0, 2, 3, 1).contiguous()   # NHWC [B, Ho, Wo, Cout]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if cp != ctx.cin:
                raise RuntimeError(f"{cls.__name__}: no input gradient for the stem (its input channels are zero-padded)")
            dxn = torch.empty((b, h, w, cp), dtype=cls.act, device=gy.device)
            _run(cls.prefix, "backward_data", desc, _lib.CONV_DGRAD, gyn, wk, dxn)
            dx = dxn.permute(0, 3, 1, 2)   # channels_last view
        if ctx.needs_input_grad[1]:
            dwk = torch.empty(wk.shape, dtype=torch.float32, device=gy.device)   # (never accumulated in bf16)
            _run(cls.prefix, "backward_weight", desc, _lib.CONV_WGRAD, xn, gyn, dwk)
            dw = dwk[..., :ctx.cin].permute(0, 3, 1, 2).contiguous()
        return dx, dw, None, None, None, None


class Conv2dF32Function(_Conv2dFunction):
    """The convolution in fp32, the reference's precision: fp32 x, y, dx and weights on salve_conv_f32_*."""
    prefix, act, why = "salve_conv_f32", torch.float32, "training runs in the reference's fp32"


class Conv2dBF16Function(_Conv2dFunction):
    """The convolution in bf16 mixed precision: bf16 x, y and dx, a bf16 copy of the fp32 master weight, fp32 accumulation and fp32
    dW on salve_conv_bf16_*.  The copy is cast here, or is `shadow`: the one HipAdam's step wrote (`conv2d_bf16` passes it while
    it is current)."""
    prefix, act, why = "salve_conv_bf16", torch.bfloat16, "bf16 activations, fp32 master weights"


def conv2d_f32(x: Tensor, conv: nn.Conv2d, packed: bool = False) -> Tensor:
    assert conv.bias is None and conv.dilation == (1, 1) and conv.groups == 1
    return Conv2dF32Function.apply(x, conv.weight, conv.stride[0], conv.padding[0], packed)


def conv2d_bf16(x: Tensor, conv: nn.Conv2d, packed: bool = False) -> Tensor:
    assert conv.bias is None and conv.dilation == (1, 1) and conv.groups == 1
    return Conv2dBF16Function.apply(x, conv.weight, conv.stride[0], conv.padding[0], packed, current_shadow(conv.weight))


TRAIN_PRECISIONS = ("fp32", "bf16")
TRAIN_NORMS = ("torch", "hip")


def _run_bn(fn: str, desc: "_lib.BnDesc", pass_: int, ptrs, device) -> None:
    """One salve_bn_* call: `ptrs` are the entry's pointer arguments in order (tensors or None)."""
    lib = _lib.load()
    nbytes = int(lib.salve_bn_workspace_bytes(ctypes.byref(desc), pass_))
    if nbytes == 0:
        raise _lib.SalveHipError(f"{fn}: refused: {lib.salve_last_error().decode('utf-8', 'replace')}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    args = [ctypes.c_void_p(None if t is None else t.data_ptr()) for t in ptrs]
    st = getattr(lib, fn)(ctypes.byref(desc), *args, ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(stream))
    _lib.check(st, fn)


_BN_ENTRY = {torch.float32: "salve_bn_f32", torch.bfloat16: "salve_bn_bf16"}


class BatchNormHipFunction(torch.autograd.Function):
    """relu?(batch_norm(x) + residual?) on the HIP entries (salve_bn_*), forward and backward.

    x: fp32 or bf16 CUDA [B, C, H, W] (channels_last memory is used as is; other layouts are copied); residual: None or a tensor
    of x's shape and dtype; weight, bias, running_mean, running_var: the fp32 parameters and buffers of an nn.BatchNorm2d,
    num_batches_tracked its counter (or None); relu: fuse max(0, .); training: batch statistics (running statistics updated in
    place with `momentum`, or with the cumulative average 1 / num_batches_tracked when momentum is None, and the counter
    incremented, as torch does) or, when False, the running statistics -- forward only, the eval form has no backward pass.
    Returns channels_last [B, C, H, W] in x's dtype.  Backward: dx and the residual's gradient in x's dtype, fp32 dweight and
    dbias; the ReLU mask is taken from the saved output."""

    @staticmethod
    def forward(ctx, x: Tensor, residual: Optional[Tensor], weight: Tensor, bias: Tensor, running_mean: Optional[Tensor],
                running_var: Optional[Tensor], num_batches_tracked: Optional[Tensor], relu: bool, eps: float, momentum: Optional[float],
                training: bool) -> Tensor:
        if x.dtype not in _BN_ENTRY:
            raise RuntimeError(f"BatchNormHipFunction: x must be float32 or bfloat16, got {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError(f"BatchNormHipFunction: x is on {x.device}; the HIP BatchNorm runs on the HIP device only (no CPU fallback)")
        if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape or residual.device != x.device):
            raise RuntimeError(f"BatchNormHipFunction: residual must match x ({x.dtype}, {tuple(x.shape)}, {x.device}), got {residual.dtype}, "
                               f"{tuple(residual.shape)}, {residual.device}")
        for name, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if t is None:
                if name in ("weight", "bias") or not training:
                    raise RuntimeError(f"BatchNormHipFunction: {name} is required")
                continue
            if t.device != x.device:
                raise RuntimeError(f"BatchNormHipFunction: {name} is on {t.device}, x on {x.device} (no CPU fallback)")
            if t.dtype != torch.float32 or t.numel() != x.shape[1]:
                raise RuntimeError(f"BatchNormHipFunction: {name} must be float32 [{x.shape[1]}], got {t.dtype} {tuple(t.shape)}")
        b, c, h, w = x.shape
        factor = 0.0
        if training and running_mean is not None:
            if num_batches_tracked is not None:
                num_batches_tracked.add_(1)
            factor = momentum if momentum is not None else 1.0 / float(num_batches_tracked)
        flags = (_lib.BN_RELU if relu else 0) | (_lib.BN_ADD if residual is not None else 0) | (0 if training else _lib.BN_EVAL)
        desc = (b * h * w, c, flags, eps, factor)
        xn = _nhwc(x.detach(), c)
        rn = None if residual is None else _nhwc(residual.detach(), c)
        y = torch.empty((b, c, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        mean = invstd = None
        if training:
            mean = torch.empty(c, dtype=torch.float32, device=x.device)
            invstd = torch.empty(c, dtype=torch.float32, device=x.device)
        _run_bn(_BN_ENTRY[x.dtype] + "_forward", _lib.BnDesc(*desc), _lib.BN_FWD,
                (xn, rn, weight, bias, running_mean, running_var, y.permute(0, 2, 3, 1), mean, invstd), x.device)
        ctx.desc, ctx.relu, ctx.add, ctx.training = desc, relu, residual is not None, training
        if training:
            ctx.save_for_backward(xn, weight, mean, invstd, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        if not ctx.training:
            raise RuntimeError("BatchNormHipFunction: the eval form has no backward pass")
        xn, weight, mean, invstd, y = ctx.saved_tensors
        b, h, w, c = xn.shape
        gyn = gy.to(xn.dtype).permute(0, 2, 3, 1).contiguous()
        dxn = torch.empty_like(xn)
        dresn = torch.empty_like(xn) if ctx.add else None
        dgamma = torch.empty(c, dtype=torch.float32, device=xn.device)
        dbeta = torch.empty(c, dtype=torch.float32, device=xn.device)
        yn = None if y is None else y.permute(0, 2, 3, 1)
        _run_bn(_BN_ENTRY[xn.dtype] + "_backward", _lib.BnDesc(*ctx.desc), _lib.BN_BWD,
                (gyn, xn, yn, weight, mean, invstd, dxn, dresn, dgamma, dbeta), xn.device)
        dres = None if dresn is None else dresn.permute(0, 3, 1, 2)
        return dxn.permute(0, 3, 1, 2), dres, dgamma, dbeta, None, None, None, None, None, None, None


def _call_bn(fn: str, desc: "_lib.BnDesc", args, ws_pass: Optional[int], device) -> None:
    """One split salve_bn_* call: `args` are its arguments behind the descriptor in order (tensors, None or ctypes values); ws_pass:
    the workspace pass of an entry that takes one (the workspace then goes in front of the stream)."""
    lib = _lib.load()
    args = [a if isinstance(a, ctypes._SimpleCData) else ctypes.c_void_p(None if a is None else a.data_ptr()) for a in args]
    if ws_pass is not None:
        nbytes = int(lib.salve_bn_workspace_bytes(ctypes.byref(desc), ws_pass))
        if nbytes == 0:
            raise _lib.SalveHipError(f"{fn}: refused: {lib.salve_last_error().decode('utf-8', 'replace')}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        args += [ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(nbytes)]
    st = getattr(lib, fn)(ctypes.byref(desc), *args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    _lib.check(st, fn)


class SyncBatchNormHipFunction(torch.autograd.Function):
    """BatchNormHipFunction in train mode over the rows of ALL data-parallel ranks (opt-in: set_sync_norm, --sync-bn), on the split
    HIP entries: forward salve_bn_*_stats -> ONE all-gather of [2, C] -> salve_bn_combine -> salve_bn_*_apply, backward
    salve_bn_*_backward_reduce -> ONE all-gather of [2, C] -> salve_bn_*_backward_apply.  The gathers, not reductions, on purpose:
    every rank adds the same numbers in the same (rank) order, so mean, invstd and the running statistics are bit-identical on every
    rank whatever the backend's reduction order.

    The arguments of BatchNormHipFunction up to `momentum`, then group: what runs the all-gather -- `rank`, `world` and
    `_gather(t) -> [world, *t.shape]` on t's device, in rank order (a dist_train.DataParallel: its group, stream and tensor
    handling); batches: the batch rows of every rank, [world] (from the batch plan, no collective), of which this rank's must be
    x's.  Returns what BatchNormHipFunction returns.  Backward: dx and the residual's gradient over the whole batch's statistics;
    dweight and dbias are THIS rank's sums, which the gradient all-reduce adds like every other parameter gradient's."""

    @staticmethod
    def forward(ctx, x: Tensor, residual: Optional[Tensor], weight: Tensor, bias: Tensor, running_mean: Optional[Tensor],
                running_var: Optional[Tensor], num_batches_tracked: Optional[Tensor], relu: bool, eps: float, momentum: Optional[float],
                group, batches) -> Tensor:
        who = "SyncBatchNormHipFunction"
        if x.dtype not in _BN_ENTRY:
            raise RuntimeError(f"{who}: x must be float32 or bfloat16, got {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError(f"{who}: x is on {x.device}; the HIP BatchNorm runs on the HIP device only (no CPU fallback)")
        if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape or residual.device != x.device):
            raise RuntimeError(f"{who}: residual must match x ({x.dtype}, {tuple(x.shape)}, {x.device}), got {residual.dtype}, "
                               f"{tuple(residual.shape)}, {residual.device}")
        for name, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if t is None:
                if name in ("weight", "bias"):
                    raise RuntimeError(f"{who}: {name} is required")
                continue
            if t.device != x.device:
                raise RuntimeError(f"{who}: {name} is on {t.device}, x on {x.device} (no CPU fallback)")
            if t.dtype != torch.float32 or t.numel() != x.shape[1]:
                raise RuntimeError(f"{who}: {name} must be float32 [{x.shape[1]}], got {t.dtype} {tuple(t.shape)}")
        b, c, h, w = x.shape
        world, rank = int(group.world), int(group.rank)
        batches = [int(n) for n in batches]
        if len(batches) != world or batches[rank] != b or world > _lib.BN_MAX_WORLD:
            raise RuntimeError(f"{who}: rank {rank} of {world} (at most {_lib.BN_MAX_WORLD}) holds {b} batch rows, the batch plan says {batches}")
        factor = 0.0
        if running_mean is not None:
            if num_batches_tracked is not None:
                num_batches_tracked.add_(1)
            factor = momentum if momentum is not None else 1.0 / float(num_batches_tracked)
        flags = (_lib.BN_RELU if relu else 0) | (_lib.BN_ADD if residual is not None else 0)
        desc = (b * h * w, c, flags, eps, factor)
        rows = (ctypes.c_int64 * world)(*[n * h * w for n in batches])
        entry, dev = _BN_ENTRY[x.dtype], x.device
        xn = _nhwc(x.detach(), c)
        rn = None if residual is None else _nhwc(residual.detach(), c)
        y = torch.empty((b, c, h, w), dtype=x.dtype, device=dev, memory_format=torch.channels_last)
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        partial = torch.empty((2, c), dtype=torch.float32, device=dev)
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty(c, dtype=torch.float32, device=dev)
        _call_bn(entry + "_stats", _lib.BnDesc(*desc), (xn, partial), _lib.BN_STATS, dev)
        partials = group._gather(partial).contiguous()
        _call_bn("salve_bn_combine", _lib.BnDesc(*desc), (partials, ctypes.cast(rows, ctypes.c_void_p), ctypes.c_int32(world), running_mean,
                                                          running_var, mean, invstd), None, dev)
        _call_bn(entry + "_apply", _lib.BnDesc(*desc), (xn, rn, weight, bias, mean, invstd, y.permute(0, 2, 3, 1)), None, dev)
        ctx.desc, ctx.relu, ctx.add, ctx.group, ctx.total_rows = desc, relu, residual is not None, group, sum(rows)
        ctx.save_for_backward(xn, weight, mean, invstd, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        xn, weight, mean, invstd, y = ctx.saved_tensors
        b, h, w, c = xn.shape
        entry, dev = _BN_ENTRY[xn.dtype], xn.device
        gyn = gy.to(xn.dtype).permute(0, 2, 3, 1).contiguous()
        dxn = torch.empty_like(xn)
        dresn = torch.empty_like(xn) if ctx.add else None
        sums = torch.empty((2, c), dtype=torch.float32, device=dev)   # this rank's dbeta, dgamma
        yn = None if y is None else y.permute(0, 2, 3, 1)
        _call_bn(entry + "_backward_reduce", _lib.BnDesc(*ctx.desc), (gyn, xn, yn, mean, invstd, sums), _lib.BN_BWD_REDUCE, dev)
        every = ctx.group._gather(sums).contiguous()
        _call_bn(entry + "_backward_apply", _lib.BnDesc(*ctx.desc), (gyn, xn, yn, weight, mean, invstd, every, ctypes.c_int32(int(ctx.group.world)),
                                                                     ctypes.c_int64(int(ctx.total_rows)), dxn, dresn), None, dev)
        dres = None if dresn is None else dresn.permute(0, 3, 1, 2)
        return dxn.permute(0, 3, 1, 2), dres, sums[1], sums[0], None, None, None, None, None, None, None, None


class SyncNorm:
    """What batch_norm_hip needs to synchronise a train-mode BatchNorm: the group (SyncBatchNormHipFunction's) and the batch plan.
    batch_size: the rows of the WHOLE batch, split over the ranks as the feeds split it (train_feed.shard_bounds); None: every rank
    holds as many rows as this one -- the train feeds' contract (train_feed.check_shard)."""

    def __init__(self, group, batch_size: Optional[int] = None) -> None:
        self.group, self.batch_size = group, None if batch_size is None else int(batch_size)

    def batches(self, local: int) -> List[int]:
        world = int(self.group.world)
        if self.batch_size is None:
            return [int(local)] * world
        return [(r + 1) * self.batch_size // world - r * self.batch_size // world for r in range(world)]


def batch_norm_hip(bn: nn.BatchNorm2d, x: Tensor, residual: Optional[Tensor] = None, relu: bool = False, sync: Optional[SyncNorm] = None) -> Tensor:
    """relu?(bn(x) + residual?) on BatchNormHipFunction: batch statistics when the module is in train mode (or tracks none),
    running statistics otherwise.  sync: batch statistics are taken over the rows of all ranks (SyncBatchNormHipFunction); the
    running-statistics form is untouched."""
    training = bn.training or bn.running_mean is None
    tracked = bn.training and bn.track_running_stats
    if sync is not None and training:
        return SyncBatchNormHipFunction.apply(x, residual, bn.weight, bn.bias, bn.running_mean if tracked else None,
                                              bn.running_var if tracked else None, bn.num_batches_tracked if tracked else None,
                                              relu, bn.eps, bn.momentum, sync.group, sync.batches(x.shape[0]))
    return BatchNormHipFunction.apply(x, residual, bn.weight, bn.bias, bn.running_mean if (tracked or not training) else None,
                                      bn.running_var if (tracked or not training) else None, bn.num_batches_tracked if tracked else None,
                                      relu, bn.eps, bn.momentum, training)


TRAIN_HEADS = ("torch", "hip")
_HEAD_ENTRY = {torch.float32: "salve_head_f32", torch.bfloat16: "salve_head_bf16"}


def _run_head(fn: str, desc: "_lib.HeadDesc", pass_: int, ptrs, device) -> None:
    """One salve_head_* call: `ptrs` are the entry's pointer arguments in order (tensors or None)."""
    lib = _lib.load()
    nbytes = int(lib.salve_head_workspace_bytes(ctypes.byref(desc), pass_))
    if nbytes == 0:
        raise _lib.SalveHipError(f"{fn}: refused: {lib.salve_last_error().decode('utf-8', 'replace')}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    args = [ctypes.c_void_p(None if t is None else t.data_ptr()) for t in ptrs]
    st = getattr(lib, fn)(ctypes.byref(desc), *args, ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(stream))
    _lib.check(st, fn)


class ClassifierHeadHipFunction(torch.autograd.Function):
    """loss, probs, logits = the classifier head on the HIP entries (salve_head_*), forward and backward: average pool over H x W,
    fc, max-subtracted softmax, cross_entropy(logits, target) with its default mean reduction, and the per-class accuracy counts.

    x: the last block's output, fp32 or bf16 CUDA [B, C, H, W] (channels_last memory is used as is; other layouts are copied);
    weight [K, C], bias [K]: fc's fp32 parameters; target: int64 CUDA [B]; record: None or a DeviceClassMeter's record, updated in
    place on the stream (counts always; the loss sum only with accumulate_loss).  Returns (loss, probs, logits): loss a 0-dim fp32
    tensor with a gradient towards x, weight and bias; probs and logits [B, K] fp32, not differentiable.  Nothing here reads the
    device: a target outside [0, K) is counted in the record (DeviceClassMeter.read raises) and contributes nothing."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor, target: Tensor, record: Optional[Tensor], accumulate_loss: bool):
        if x.dtype not in _HEAD_ENTRY:
            raise RuntimeError(f"ClassifierHeadHipFunction: x must be float32 or bfloat16, got {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError(f"ClassifierHeadHipFunction: x is on {x.device}; the HIP head runs on the HIP device only (no CPU fallback)")
        if x.dim() != 4:
            raise RuntimeError(f"ClassifierHeadHipFunction: x must be [B, C, H, W], got {tuple(x.shape)}")
        b, c, h, w = x.shape
        k = weight.shape[0]
        for name, t, dt, shape in (("weight", weight, torch.float32, (k, c)), ("bias", bias, torch.float32, (k,)), ("target", target, torch.int64, (b,)),
                                   ("record", record, torch.int64, (_lib.HEAD_METER_DTYPE.itemsize // 8,))):
            if t is None and name == "record":
                continue
            if t.device != x.device:
                raise RuntimeError(f"ClassifierHeadHipFunction: {name} is on {t.device}, x on {x.device} (no CPU fallback)")
            if t.dtype != dt or tuple(t.shape) != shape:
                raise RuntimeError(f"ClassifierHeadHipFunction: {name} must be {dt} {list(shape)}, got {t.dtype} {list(t.shape)}")
        if record is not None and not record.is_contiguous():
            raise RuntimeError("ClassifierHeadHipFunction: the meter record must be contiguous")
        xn = _nhwc(x.detach(), c)
        weight, bias, target = weight.detach().contiguous(), bias.detach().contiguous(), target.contiguous()
        pooled = torch.empty((b, c), dtype=torch.float32, device=x.device)
        logits = torch.empty((b, k), dtype=torch.float32, device=x.device)
        probs = torch.empty((b, k), dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        desc = (b, h * w, c, k, _lib.HEAD_ACCUMULATE_LOSS if accumulate_loss else 0)
        _run_head(_HEAD_ENTRY[x.dtype] + "_forward", _lib.HeadDesc(*desc), _lib.HEAD_FWD,
                  (xn, weight, bias, target, pooled, logits, probs, loss, record), x.device)
        ctx.save_for_backward(pooled, probs, target, weight)
        ctx.desc, ctx.hw, ctx.act = desc, (h, w), x.dtype
        ctx.mark_non_differentiable(probs, logits)
        return loss, probs, logits

    @staticmethod
    def backward(ctx, g_loss: Tensor, g_probs, g_logits):
        pooled, probs, target, weight = ctx.saved_tensors
        b, _, c, k, _ = ctx.desc
        g = g_loss.detach().to(torch.float32).reshape(()).contiguous()
        dxn = torch.empty((b, ctx.hw[0], ctx.hw[1], c), dtype=ctx.act, device=pooled.device)
        dlogits = torch.empty((b, k), dtype=torch.float32, device=pooled.device)
        dw = torch.empty((k, c), dtype=torch.float32, device=pooled.device)
        db = torch.empty((k,), dtype=torch.float32, device=pooled.device)
        _run_head(_HEAD_ENTRY[ctx.act] + "_backward", _lib.HeadDesc(*ctx.desc), _lib.HEAD_BWD,
                  (pooled, probs, target, weight, g, dlogits, dw, db, dxn), pooled.device)
        return dxn.permute(0, 3, 1, 2), dw, db, None, None, None


def _conv(precision: str):
    """The convolution of a training precision, looked up at call time (tools/measure/bench_train.py swaps these functions)."""
    return conv2d_bf16 if precision == "bf16" else conv2d_f32


def _bn(bn: nn.BatchNorm2d, x: Tensor) -> Tensor:
    return bn(x)


def _bn_bf16(bn: nn.BatchNorm2d, x: Tensor) -> Tensor:
    """BatchNorm of a bf16 activation, upcast at its input: fp32 statistics, normalisation and parameters, the output rounded to
    bf16 once.  (Why not torch's mixed-type BatchNorm: DESIGN.md section 4.8.)"""
    return bn(x.float()).to(torch.bfloat16)


def _basic(blk, x: Tensor, conv, bn) -> Tensor:
    out = F.relu(bn(blk.bn1, conv(x, blk.conv1)))
    out = bn(blk.bn2, conv(out, blk.conv2))
    idt = x if blk.downsample is None else bn(blk.downsample[1], conv(x, blk.downsample[0]))
    return F.relu(out + idt)


def _bottleneck(blk, x: Tensor, conv, bn) -> Tensor:
    out = F.relu(bn(blk.bn1, conv(x, blk.conv1)))
    out = F.relu(bn(blk.bn2, conv(out, blk.conv2)))
    out = bn(blk.bn3, conv(out, blk.conv3))
    idt = x if blk.downsample is None else bn(blk.downsample[1], conv(x, blk.downsample[0]))
    return F.relu(out + idt)


def _basic_hip(blk, x: Tensor, conv, sync: Optional[SyncNorm] = None) -> Tensor:
    out = batch_norm_hip(blk.bn1, conv(x, blk.conv1), relu=True, sync=sync)
    idt = x if blk.downsample is None else batch_norm_hip(blk.downsample[1], conv(x, blk.downsample[0]), sync=sync)
    return batch_norm_hip(blk.bn2, conv(out, blk.conv2), residual=idt, relu=True, sync=sync)


def _bottleneck_hip(blk, x: Tensor, conv, sync: Optional[SyncNorm] = None) -> Tensor:
    out = batch_norm_hip(blk.bn1, conv(x, blk.conv1), relu=True, sync=sync)
    out = batch_norm_hip(blk.bn2, conv(out, blk.conv2), relu=True, sync=sync)
    idt = x if blk.downsample is None else batch_norm_hip(blk.downsample[1], conv(x, blk.downsample[0]), sync=sync)
    return batch_norm_hip(blk.bn3, conv(out, blk.conv3), residual=idt, relu=True, sync=sync)


class TrainableEarlyFusionCEResnet(EarlyFusionCEResnet):
    """EarlyFusionCEResnet whose forward is an autograd graph (salve/models/early_fusion.py:41-83 op for op): HIP fp32
    convolutions, torch BatchNorm2d / ReLU / max-pool / average pool / Linear.  Train mode: batch statistics, running statistics
    updated, gradients for every parameter.  Eval mode: running statistics -- the validation pass scripts/train.py:76-77 runs under
    torch.no_grad().  The inference engines (`compiled`, `forward_nhwc`) stay available through the parent class.

    `set_train_precision("bf16")` opts into mixed precision: the concatenated input is cast to bf16 once before the stem, the
    convolutions run on Conv2dBF16Function, BatchNorm upcasts its bf16 input to fp32 (fp32 weight, bias, running statistics and
    arithmetic; the output is rounded to bf16), ReLU / max-pool / residual adds run in bf16, and the average pool output is cast to fp32 before `fc`.
    Parameters and gradients stay fp32.  Train and eval mode alike.  Separate from the parent's inference `set_precision`.

    `set_train_norm("hip")` opts into the HIP BatchNorm: one fused operation per BatchNorm (bn + relu after the stem, conv1 and
    conv2, plain bn on the downsample branch, bn + add + relu at the end of a block), in fp32 and in bf16 (no casts around
    BatchNorm then).  Train mode uses batch statistics; eval mode under torch.no_grad() (the validation pass) the eval form; eval
    mode with gradients enabled runs the torch path, which has a backward pass.  The same parameters and buffers either way.
    `set_sync_norm(dist)` on top of it synchronises the train-mode statistics over the data-parallel ranks.

    `set_train_head("hip")` opts into the HIP classifier head for `forward_loss` / `forward_packed_loss`, which return (probs,
    loss): the last block's output goes through ClassifierHeadHipFunction (average pool, fc, softmax, cross-entropy and the
    accuracy counts in one forward and one backward, in fp32 and in bf16) instead of torch's avgpool / flatten / cast / fc /
    softmax / cross_entropy.  `forward` and `forward_packed`, which return logits, run torch's head in both settings."""

    _train_precision = "fp32"
    _train_norm = "torch"
    _train_head = "torch"
    _sync_norm: Optional[SyncNorm] = None

    def set_train_precision(self, precision: str) -> "TrainableEarlyFusionCEResnet":
        """"fp32" (the default, the reference's precision) or "bf16" (opt-in mixed precision).  Returns self."""
        if precision not in TRAIN_PRECISIONS:
            raise ValueError(f"training precision must be one of {TRAIN_PRECISIONS}, got {precision!r}")
        self._train_precision = precision
        return self

    @property
    def train_precision(self) -> str:
        return self._train_precision

    def set_train_norm(self, norm: str) -> "TrainableEarlyFusionCEResnet":
        """"torch" (the default: nn.BatchNorm2d, F.relu and the add as separate operations) or "hip" (opt-in: BatchNormHipFunction).
        Returns self."""
        if norm not in TRAIN_NORMS:
            raise ValueError(f"training norm must be one of {TRAIN_NORMS}, got {norm!r}")
        self._train_norm = norm
        return self

    @property
    def train_norm(self) -> str:
        return self._train_norm

    def set_sync_norm(self, dist, batch_size: Optional[int] = None) -> "TrainableEarlyFusionCEResnet":
        """Opt-in: every train-mode BatchNorm normalises over the rows of all data-parallel ranks (SyncBatchNormHipFunction: two
        all-gathers of [2, C] per BatchNorm and step, through `dist`, a dist_train.DataParallel).  Needs the HIP norm.  batch_size:
        SyncNorm's.  Eval mode is untouched: running statistics, no collective.  A `dist` that runs no collectives (None, or a world
        of one that is not forced) switches it off: the fused entries.  Returns self."""
        if dist is not None and self._train_norm != "hip":
            raise ValueError("BatchNorm statistics are synchronised by the HIP BatchNorm only: choose --norm hip (set_train_norm(\"hip\"))")
        self._sync_norm = SyncNorm(dist, batch_size) if dist is not None and getattr(dist, "active", True) else None
        return self

    @property
    def sync_norm(self) -> Optional[SyncNorm]:
        return self._sync_norm

    def set_train_head(self, head: str) -> "TrainableEarlyFusionCEResnet":
        """"torch" (the default: avgpool, fc, softmax and cross_entropy as separate torch operations) or "hip" (opt-in:
        ClassifierHeadHipFunction) for `forward_loss` / `forward_packed_loss`.  Returns self."""
        if head not in TRAIN_HEADS:
            raise ValueError(f"training head must be one of {TRAIN_HEADS}, got {head!r}")
        self._train_head = head
        return self

    @property
    def train_head(self) -> str:
        return self._train_head

    def forward(self, x1: Tensor, x2: Tensor, x3: Optional[Tensor] = None, x4: Optional[Tensor] = None, x5: Optional[Tensor] = None,
                x6: Optional[Tensor] = None) -> Tensor:
        return self._from_stem(self._cat(self._images(x1, x2, x3, x4, x5, x6)), packed=False)

    def _images(self, x1, x2, x3, x4, x5, x6):
        n = num_input_images(self.modalities)
        xs = [x1, x2, x3, x4, x5, x6][:n]
        if any(x is None for x in xs):
            raise RuntimeError(f"{n} input images are required for modalities {self.modalities}")
        if x1.device.type != "cuda":
            raise RuntimeError("TrainableEarlyFusionCEResnet runs on the HIP device only (no CPU fallback)")
        return xs

    def _cat(self, xs) -> Tensor:
        x = torch.cat(xs, dim=1)
        if self._train_precision == "bf16":
            x = x.to(torch.bfloat16)
        return x

    def forward_packed(self, x: Tensor) -> Tensor:
        """`forward` on the input as the stem convolution reads it: x [B, H, W, Cp], contiguous NHWC, Cp = the 3 * images channels
        in `forward`'s concatenation order zero-padded to a multiple of 8, in the training precision (float32 / bfloat16) -- what
        salve_bev_train_tiles writes (salve_amd.train_render).  The same graph as `forward` from the stem on, without its torch.cat,
        cast and padding copy: the same kernels on the same bytes, so logits and gradients are bit-identical."""
        return self._from_stem(self._packed(x), packed=True)

    def _packed(self, x: Tensor) -> Tensor:
        """forward_packed's input checked, as the NCHW view of its NHWC bytes (the stem uses them as they are)."""
        cp = _pad8(3 * num_input_images(self.modalities))
        want = torch.bfloat16 if self._train_precision == "bf16" else torch.float32
        if x.dim() != 4 or x.shape[3] != cp:
            raise RuntimeError(f"forward_packed takes [B, H, W, {cp}] for modalities {self.modalities}, got {tuple(x.shape)}")
        if x.dtype != want:
            raise RuntimeError(f"forward_packed: train precision {self._train_precision} takes {want}, got {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError("TrainableEarlyFusionCEResnet runs on the HIP device only (no CPU fallback)")
        if not x.is_contiguous():
            raise RuntimeError("forward_packed takes a contiguous NHWC tensor")
        return x.permute(0, 3, 1, 2)

    def forward_loss(self, x1: Tensor, x2: Tensor, x3: Optional[Tensor], x4: Optional[Tensor], x5: Optional[Tensor], x6: Optional[Tensor],
                     is_match: Tensor, meters=None, accumulate_loss: bool = False):
        """(softmax probabilities [B, K], cross-entropy loss) of a batch, as training.cross_entropy_forward forms them.  With head
        "torch": `forward`'s graph followed by softmax on a detached clone of the logits and F.cross_entropy(logits,
        is_match.squeeze()) -- the present results; `meters` must be None (the host meter is the caller's).  With head "hip": the
        trunk's output through ClassifierHeadHipFunction; meters: None or a salve_amd.evaluate.DeviceClassMeter, whose counts this
        batch is added to on the device (and, with accumulate_loss, its loss sum).  The caller chooses the gradient mode."""
        return self._loss(self._cat(self._images(x1, x2, x3, x4, x5, x6)), False, is_match, meters, accumulate_loss)

    def forward_packed_loss(self, x_packed: Tensor, is_match: Tensor, meters=None, accumulate_loss: bool = False):
        """`forward_loss` on `forward_packed`'s input: the same kernels on the same bytes, so the results are bit-identical."""
        return self._loss(self._packed(x_packed), True, is_match, meters, accumulate_loss)

    def _loss(self, x: Tensor, packed: bool, is_match: Tensor, meters, accumulate_loss: bool):
        if self._train_head == "hip":
            record = None
            if meters is not None:
                if meters.num_classes != self.fc.out_features:
                    raise RuntimeError(f"the meter counts {meters.num_classes} classes, the model has {self.fc.out_features}")
                record = meters.record
            loss, probs, _ = ClassifierHeadHipFunction.apply(self._features(x, packed), self.fc.weight, self.fc.bias, is_match.reshape(-1), record,
                                                             bool(accumulate_loss))
            return probs, loss
        if meters is not None:
            raise RuntimeError("a DeviceClassMeter is updated by the HIP head only: set_train_head(\"hip\")")
        logits = self._from_stem(x, packed)
        probs = F.softmax(logits.detach().clone(), dim=1)
        return probs, F.cross_entropy(logits, is_match.squeeze())

    def _from_stem(self, x: Tensor, packed: bool) -> Tensor:
        x = torch.flatten(self.resnet.avgpool(self._features(x, packed)), 1)
        if self._train_precision == "bf16":
            x = x.float()
        return self.fc(x)

    def _features(self, x: Tensor, packed: bool) -> Tensor:
        """The last block's output [B, C, H, W] in the training precision."""
        bf16 = self._train_precision == "bf16"
        conv, bn = _conv(self._train_precision), (_bn_bf16 if bf16 else _bn)
        r = self.resnet
        x = conv(x, self.conv1, True) if packed else conv(x, self.conv1)
        if self._train_norm == "hip" and (self.training or not torch.is_grad_enabled()):
            sync = self._sync_norm
            x = r.maxpool(batch_norm_hip(r.bn1, x, relu=True, sync=sync))
            block = _bottleneck_hip if r.block_kind == "bottleneck" else _basic_hip
            for layer in (r.layer1, r.layer2, r.layer3, r.layer4):
                for blk in layer:
                    x = block(blk, x, conv, sync)
        else:
            x = r.maxpool(F.relu(bn(r.bn1, x)))
            block = _bottleneck if r.block_kind == "bottleneck" else _basic
            for layer in (r.layer1, r.layer2, r.layer3, r.layer4):
                for blk in layer:
                    x = block(blk, x, conv, bn)
        return x
