"""The fp32 verifier engine against the fp16 one on the same weights, alternating in ONE process on one box (the ab_flags.py
pattern: box-to-box drift is larger than some of what is compared).  Trained-looking BatchNorm statistics and head (|logit| of
several units), tile-like fp32 input; the fp16 engine gets that input rounded to fp16 NHWC, as the product does.
usage: python tools/measure/bench_resnet_f32.py <layers> <batch> [rounds] [--precision {fp32,bf16x3}]
--precision bf16x3 puts the bf16x3 engine (the fp32 engine with its products on the bf16 matrix cores) in the fp32 engine's place.
ResNet-152 runs the two-surface (12-channel) modality set, every other depth one surface (6 channels); algorithmic FLOPs per
sample from SURVEY.md section 8d."""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from types import SimpleNamespace

import torch

from salve_amd import status, synthetic
from salve_amd.models.early_fusion import EarlyFusionCEResnet
from salve_amd.models.hip_resnet import nchw_to_input

GFLOP_PER_SAMPLE = {(50, 6): 8.410, (50, 12): 8.882, (152, 6): 23.259, (152, 12): 23.731}

dev = torch.device("cuda:0")
argv = sys.argv[1:]
PREC = "fp32"
if "--precision" in argv:
    i = argv.index("--precision")
    PREC = argv[i + 1]
    del argv[i:i + 2]
    if PREC not in ("fp32", "bf16x3"):
        raise SystemExit(f"--precision must be fp32 or bf16x3, got {PREC}")
layers, B = int(argv[0]), int(argv[1])
rounds = int(argv[2]) if len(argv) > 2 else 6
mods = ["ceiling_rgb_texture", "floor_rgb_texture"] if layers == 152 else ["floor_rgb_texture"]
torch.manual_seed(0)
model = EarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=mods)).eval()
synthetic.trained_looking_batchnorm(model)
synthetic.trained_looking_head(model, 30.0)
C = 3 * model.num_images
e16 = model.compiled(dev, precision="fp16")
e32 = model.compiled(dev, precision=PREC)
g = torch.Generator().manual_seed(1)
v = torch.randint(0, 256, (B, C, 224, 224), generator=g).float()
mean = torch.tensor([123.675, 116.28, 103.53] * (C // 3)).view(1, C, 1, 1)
std = torch.tensor([58.395, 57.12, 57.375] * (C // 3)).view(1, C, 1, 1)
x32 = ((v - mean) / std).to(dev)
del v
x16 = nchw_to_input([x32], e16.in_channels)
runs = {"fp16": lambda: e16.forward_nhwc(x16), PREC: lambda: e32.forward_nchw(x32)}
with torch.no_grad():
    out = {k: f().clone() for k, f in runs.items()}   # warm-up (and the logits compared below)
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    status.check(dev, "bench_resnet_f32 warm-up")
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / 3 * 1e3)
    status.check(dev, "bench_resnet_f32")
gf = GFLOP_PER_SAMPLE.get((layers, C))
for k, t in times.items():
    best = min(t)
    med = sorted(t)[len(t) // 2]
    tf = f"  {gf * B / (med * 1e-3) / 1e3:.1f} TFLOP/s algorithmic (median)" if gf else ""
    print(f"resnet{layers} {C}-ch B={B} {k}: " + " ".join(f"{x:.2f}" for x in t) +
          f"  | median {med:.2f} ms, min {best:.2f} ms, {B / (med * 1e-3):.0f} samples/s{tf}", flush=True)
d = (out[PREC] - out["fp16"]).abs().max().item()
print(f"resnet{layers} {C}-ch B={B}: max |logit| {out[PREC].abs().max().item():.3f}, max |logit {PREC} - logit fp16| {d:.3e}, "
      f"{PREC} / fp16 time {sorted(times[PREC])[rounds // 2] / sorted(times['fp16'])[rounds // 2]:.2f}", flush=True)
