"""Time one training step of the verifier (forward + backward + Adam) on the HIP training convolutions, split into HIP
convolution time and the rest (torch: BatchNorm, ReLU, pooling, fc, loss, Adam), and the same step with torch's own F.conv2d
beside it, in the same process and alternating (context only: the product never calls F.conv2d).  --precision fp32,bf16 times
the reference's fp32 step and the opt-in bf16 mixed-precision step (TrainableEarlyFusionCEResnet.set_train_precision) one after
the other in the same process; the torch step of a precision runs F.conv2d in that precision.  --norm torch,hip times the step
with torch's BatchNorm and with the opt-in fused HIP BatchNorm (TrainableEarlyFusionCEResnet.set_train_norm), alternating the two
step by step inside the same process; the event split then also reports the time inside the salve_bn_* calls.  --optim
torch,fused,hip times the step with torch.optim.Adam (the default), torch.optim.Adam(fused=True) and the opt-in HipAdam
(salve_amd/optim.py; with bf16 it also writes the convolution weights' bf16 copies), each on its own copy of the model (a
weight's bf16 copy belongs to the parameter, so the variants cannot share one), alternating step by step.  Without hip in the
list the model's weights are converted to channels_last as before; with it every variant keeps the contiguous weights that
training.get_model creates (HipAdam refuses non-contiguous parameters), so those lines are not comparable with earlier tables.
--head torch,hip times the step with torch's classifier head and with the opt-in fused HIP head
(TrainableEarlyFusionCEResnet.set_train_head), alternating step by step on the same model; with hip in the list every head's step
goes through `model.forward_loss` (for torch: today's graph plus the softmax of training.cross_entropy_forward).
--run-epoch N times whole `training.run_epoch` passes instead of bare steps -- a train pass and a val pass over N batches held on
the device in the stem's layout -- because the host synchronisations the HIP head removes live in run_epoch, not in the step:
per-batch wall time per head, alternating the heads pass by pass, each head on its own copy of the model, with the first --optim
and the first --norm.

    python tools/measure/bench_train.py [--configs 50:1,152:2] [--batches 64,256] [--steps 3] [--warmup 1] [--hw 224]
                                        [--precision fp32,bf16] [--norm torch,hip] [--optim torch,fused,hip] [--head torch,hip]
                                        [--run-epoch N]

Per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/measure/bench_train.py ...` on its own.
"""

from __future__ import annotations

import argparse
import copy
import sys
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from salve_amd.models import trainable  # noqa: E402
from salve_amd.optim import HipAdam  # noqa: E402

MODS = {1: ["floor_rgb_texture"], 2: ["ceiling_rgb_texture", "floor_rgb_texture"], 3: ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]}
_events = []
_hip_run = trainable._run
_hip_run_bn = trainable._run_bn
_hip_conv = {"fp32": trainable.conv2d_f32, "bf16": trainable.conv2d_bf16}
_conv_attr = {"fp32": "conv2d_f32", "bf16": "conv2d_bf16"}


def _timed_run(prefix, entry, desc, pass_, a, b, out):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    _hip_run(prefix, entry, desc, pass_, a, b, out)
    e.record()
    _events.append((f"{prefix}_{entry}", s, e))


def _timed_run_bn(fn, desc, pass_, ptrs, device):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    _hip_run_bn(fn, desc, pass_, ptrs, device)
    e.record()
    _events.append((fn, s, e))


def _torch_conv(x, conv):
    return F.conv2d(x, conv.weight.to(x.dtype), stride=conv.stride, padding=conv.padding)


def step(model, opt, xs, y, through_forward_loss: bool = False):
    opt.zero_grad(set_to_none=True)
    if through_forward_loss:
        loss = model.forward_loss(*(list(xs) + [None] * (6 - len(xs))), y)[1]
    else:
        loss = F.cross_entropy(model(*xs), y)
    loss.backward()
    opt.step()


class _DeviceBatches:
    """`n` batches for run_epoch, cycling over two distinct ones held on the device as 2-tuples (x_packed, is_match)."""

    def __init__(self, n, batch, hw, images, dtype, dev):
        cp = (3 * images + 7) // 8 * 8
        self.n = n
        self.items = [(torch.randn(batch, hw, hw, cp, device=dev).to(dtype), torch.randint(0, 2, (batch, 1), device=dev)) for _ in range(2)]

    def __len__(self):
        return self.n

    def __iter__(self):
        return (self.items[i % 2] for i in range(self.n))


def run_epoch_mode(a, heads, precs, norm, optim, dev) -> None:
    from salve_amd import training

    print(f"# {torch.cuda.get_device_name(dev)}; training.run_epoch over {a.run_epoch} device-resident batches, input {a.hw}x{a.hw}, norm {norm}, "
          f"optim {optim}; per-batch wall time, median of {a.steps} passes after {a.warmup} warm-up; heads alternate pass by pass")
    for cfg in a.configs.split(","):
        layers, nm = (int(v) for v in cfg.split(":"))
        for batch, prec in ((int(b), p) for b in a.batches.split(",") for p in precs):
            torch.manual_seed(0)
            args = SimpleNamespace(num_ce_classes=2, num_epochs=1000, base_lr=1e-4, lr_annealing_strategy="poly", poly_lr_power=0.9,
                                   print_every=10 ** 9)   # (the first iteration of a train pass logs: one loss read per pass, as in training)
            base = trainable.TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[nm])).to(dev)
            base.set_train_precision(prec).set_train_norm(norm)
            variants = []
            for hd in heads:
                m = copy.deepcopy(base).set_train_head(hd)
                variants.append((hd, m, HipAdam(m.parameters(), lr=1e-4, bf16_shadow=prec == "bf16") if optim == "hip" else
                                 torch.optim.Adam(m.parameters(), lr=1e-4, fused=True if optim == "fused" else None)))
            del base
            src = _DeviceBatches(a.run_epoch, batch, a.hw, 2 * nm, torch.bfloat16 if prec == "bf16" else torch.float32, dev)
            res = {(hd, split): [] for hd in heads for split in ("train", "val")}
            for i in range(a.warmup + a.steps):
                for hd, m, opt in variants:
                    for split in ("train", "val"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        with torch.set_grad_enabled(split == "train"):
                            training.run_epoch(args, 0, m, src, opt, split)
                        torch.cuda.synchronize()
                        if i >= a.warmup:
                            res[(hd, split)].append((time.perf_counter() - t0) / a.run_epoch)
            for split in ("train", "val"):
                med = {hd: sorted(res[(hd, split)])[len(res[(hd, split)]) // 2] for hd in heads}
                for hd in heads:
                    v = res[(hd, split)]
                    line = (f"resnet{layers} {6 * nm}ch batch {batch} {prec} run_epoch {split} head {hd}: {med[hd] * 1e3:.2f} ms per batch "
                            f"({batch / med[hd]:.0f} samples/s); its passes {min(v) * 1e3:.2f} .. {max(v) * 1e3:.2f} ms")
                    if hd != "torch" and "torch" in med:
                        line += f"; {med[hd] / med['torch']:.3f} x the torch head's time"
                    print(line, flush=True)
            del variants, src
            torch.cuda.empty_cache()


def timed(model, opt, xs, y, conv_impl, split: bool, prec: str = "fp32", through_forward_loss: bool = False):
    setattr(trainable, _conv_attr[prec], conv_impl)
    trainable._run = _timed_run if split else _hip_run
    trainable._run_bn = _timed_run_bn if split else _hip_run_bn
    _events.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step(model, opt, xs, y, through_forward_loss)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    conv = sum(s.elapsed_time(e) for fn, s, e in _events if fn.startswith("salve_conv_")) / 1e3 if split else 0.0
    per = {}
    for fn, s, e in _events:
        pass_ = fn.split("_", 3)[3] if fn.startswith("salve_conv_") else "bn"   # salve_conv_{f32,bf16}_<pass> | salve_bn_*
        per[pass_] = per.get(pass_, 0.0) + s.elapsed_time(e) / 1e3
    return dt, conv, per


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="50:1,152:2", help="layers:modalities, comma separated")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--no-torch", action="store_true", help="skip the F.conv2d comparison")
    ap.add_argument("--precision", default="fp32", help="training precisions, comma separated: fp32, bf16")
    ap.add_argument("--norm", default="torch", help="BatchNorm implementations, comma separated: torch, hip (alternated step by step)")
    ap.add_argument("--optim", default="torch", help="optimisers, comma separated: torch, fused (torch's fused=True), hip (alternated step by step)")
    ap.add_argument("--head", default="torch", help="classifier heads, comma separated: torch, hip (alternated step by step)")
    ap.add_argument("--run-epoch", type=int, default=0, metavar="N",
                    help="time whole training.run_epoch passes (train and val) over N device-resident batches instead of bare steps")
    a = ap.parse_args()
    heads = a.head.split(",")
    if not heads or any(h not in trainable.TRAIN_HEADS for h in heads):
        ap.error(f"--head takes a comma-separated list of {trainable.TRAIN_HEADS}")
    fl = heads != ["torch"]   # every head's step through model.forward_loss, so that the heads differ in the head only
    optims = a.optim.split(",")
    if not optims or any(o not in ("torch", "fused", "hip") for o in optims):
        ap.error("--optim takes a comma-separated list of torch, fused, hip")
    precs = a.precision.split(",")
    if not precs or any(p not in trainable.TRAIN_PRECISIONS for p in precs):
        ap.error(f"--precision takes a comma-separated list of {trainable.TRAIN_PRECISIONS}")
    norms = a.norm.split(",")
    if not norms or any(n not in trainable.TRAIN_NORMS for n in norms):
        ap.error(f"--norm takes a comma-separated list of {trainable.TRAIN_NORMS}")
    dev = torch.device("cuda:0")
    if a.run_epoch > 0:
        run_epoch_mode(a, heads, precs, norms[0], optims[0], dev)
        return
    fp32_step = {}
    print(f"# {torch.cuda.get_device_name(dev)}; {' / '.join(precs)} training step = forward + backward + Adam, input {a.hw}x{a.hw}, "
          f"median of {a.steps} after {a.warmup} warm-up; alternating HIP / torch-conv steps")
    for cfg in a.configs.split(","):
        layers, nm = (int(v) for v in cfg.split(":"))
        for batch, prec in ((int(b), p) for b in a.batches.split(",") for p in precs):
            torch.manual_seed(0)
            model = trainable.TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[nm])).to(dev).train()
            model.set_train_precision(prec)
            if "hip" not in optims:   # HipAdam takes contiguous parameters, as training.get_model creates them: with it in the list
                model = model.to(memory_format=torch.channels_last)   # every variant keeps them, so the variants differ in the optimiser only
            variants = []   # (optimiser name, its model, its optimiser)
            for o in optims:
                mo = model if o == optims[-1] else copy.deepcopy(model)
                variants.append((o, mo, HipAdam(mo.parameters(), lr=1e-4, bf16_shadow=prec == "bf16") if o == "hip" else
                                 torch.optim.Adam(mo.parameters(), lr=1e-4, fused=True if o == "fused" else None)))
            xs = [torch.randn(batch, 3, a.hw, a.hw, device=dev) for _ in range(2 * nm)]
            y = torch.randint(0, 2, (batch,), device=dev)
            impls = [("hip", _hip_conv[prec])] + ([] if a.no_torch else [("torch", _torch_conv)])
            nh = [(norm, hd) for norm in norms for hd in heads]   # (a head is a switch of the model, as the norm is)
            res = {(o, v, k): [] for o in optims for v in nh for k, _ in impls}
            split = {(o, v): [] for o in optims for v in nh}
            for i in range(a.warmup + a.steps):
                for o, model, opt in variants:
                    for v in nh:
                        model.set_train_norm(v[0]).set_train_head(v[1])
                        for name, impl in impls:
                            dt, _, _ = timed(model, opt, xs, y, impl, False, prec, fl)
                            if i >= a.warmup:
                                res[(o, v, name)].append(dt)
            for i in range(a.steps):   # separate steps with an event pair around every HIP convolution (and HIP BatchNorm) call
                for o, model, opt in variants:
                    for v in nh:
                        model.set_train_norm(v[0]).set_train_head(v[1])
                        split[(o, v)].append(timed(model, opt, xs, y, _hip_conv[prec], True, prec, fl))
            setattr(trainable, _conv_attr[prec], _hip_conv[prec])
            trainable._run = _hip_run
            trainable._run_bn = _hip_run_bn
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            for o, nv in ((o, v) for o in optims for v in nh):
                norm, hd = nv
                sp = sorted(split[(o, nv)], key=lambda t: t[0])[len(split[(o, nv)]) // 2]
                step_s = med[(o, nv, "hip")]
                tag = (("" if prec == "fp32" else f" {prec}") + ("" if norms == ["torch"] else f" norm {norm}") + ("" if optims == ["torch"] else f" optim {o}")
                       + ("" if heads == ["torch"] else f" head {hd}"))
                bn = sp[2].get("bn", 0.0)
                line = (f"resnet{layers} {6 * nm}ch batch {batch}{tag}: step {step_s * 1e3:.1f} ms ({batch / step_s:.0f} samples/s); "
                        f"HIP convolutions {sp[1] * 1e3:.1f} ms of a {sp[0] * 1e3:.1f} ms event-split step "
                        f"[fwd {sp[2].get('forward', 0) * 1e3:.1f}, dgrad {sp[2].get('backward_data', 0) * 1e3:.1f}, "
                        f"wgrad {sp[2].get('backward_weight', 0) * 1e3:.1f} ms], ")
                if norm == "hip":
                    line += f"HIP BatchNorm {bn * 1e3:.1f} ms, "
                line += f"torch + host {(sp[0] - sp[1] - bn) * 1e3:.1f} ms"
                if (o, nv, "torch") in med:
                    line += f"; same step with F.conv2d: {med[(o, nv, 'torch')] * 1e3:.1f} ms ({batch / med[(o, nv, 'torch')]:.0f} samples/s)"
                fp32_step[(layers, nm, batch, prec, nv, o)] = step_s
                if prec != "fp32" and (layers, nm, batch, "fp32", nv, o) in fp32_step:
                    line += f"; {step_s / fp32_step[(layers, nm, batch, 'fp32', nv, o)]:.2f} x the fp32 step's time"
                if norm != "torch" and (o, ("torch", hd), "hip") in med:
                    line += f"; {step_s / med[(o, ('torch', hd), 'hip')]:.2f} x the torch-norm step's time"
                if o != "torch" and ("torch", nv, "hip") in med:
                    line += f"; {step_s / med[('torch', nv, 'hip')]:.3f} x the torch.optim.Adam step's time"
                if hd != "torch" and (o, (norm, "torch"), "hip") in med:
                    line += f"; {step_s / med[(o, (norm, 'torch'), 'hip')]:.3f} x the torch-head step's time"
                if (o == "torch" and optims != ["torch"]) or (hd == "torch" and heads != ["torch"]):
                    v = res[(o, nv, "hip")]
                    line += f"; its steps {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f} ms"
                print(line, flush=True)
            del variants, model, opt, xs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
