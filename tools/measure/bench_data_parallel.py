"""Data-parallel training's two costs on one MI355X (profiles/r15_data_parallel.txt):

    python tools/measure/bench_data_parallel.py [--layers 152] [--batch 256] [--steps 10] [--repeats 5] [--skip-step] [--sync-bn]

1. Pack throughput: `FlatBucket.pack` over the gradient set of one real backward pass of the ResNet (the parameters that received
   a gradient), timed with device events over windows of 50 launches, --repeats windows per scale (1 / 2: a multiply; 1: the bit
   copy); bytes = 8 per element (one fp32 read, one fp32 write).  Beside it, in the same call, torch's own copy of a flat buffer
   of the same size.
2. Step overhead: the training step (zero_grad, forward with the loss, backward, Adam) with bf16 / --norm hip / --optim hip /
   --head hip on a fixed batch, without `dist` -- the step as it runs without the feature -- and with a forced RCCL world of one
   (pack at scale 1, the all-reduce of the flat buffer, the gradients re-pointed), in alternating windows of --steps steps, each
   ending in a device synchronise; medians and the spread between the windows.

3. --sync-bn (instead of 1 and 2; profiles/r17_sync_bn.txt): the same step in the forced RCCL world of one, without and with
   `set_sync_norm` -- the split BatchNorm entries in place of the fused ones (three more small launches per BatchNorm and pass) plus
   two all-gathers of [2, C] per BatchNorm and step, 310 collectives of one rank for ResNet-152 -- in the same alternating windows.

One GPU: nothing here measures scaling, nor what the collectives cost between several GPUs."""

from __future__ import annotations

import argparse
import os
import socket
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch  # noqa: E402

from salve_amd import training  # noqa: E402
from salve_amd.dist_train import DataParallel, FlatBucket  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per variant")
    ap.add_argument("--skip-step", action="store_true", help="pack throughput only")
    ap.add_argument("--sync-bn", action="store_true", help="the step in a forced world of one with and without synchronised BatchNorm, nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data_parallel.py measures on the HIP device; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    args = TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10 ** 9, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=a.layers, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="dp", num_epochs=1,
                          workers=0, batch_size=a.batch, data_root="", layout_data_root="", model_save_dirpath="")
    torch.manual_seed(0)
    model = training.get_model(args, "bf16", "hip", "hip").train()
    opt = training.get_optimizer(args, model, "hip")
    g = torch.Generator().manual_seed(1)
    x = torch.randn((a.batch, 224, 224, 8), generator=g)
    x[..., 6:] = 0
    x, y = x.to(dev).to(torch.bfloat16), torch.randint(0, 2, (a.batch, 1), generator=g).to(dev)

    def step(dist=None, rows=None):
        opt.zero_grad()
        _, loss = training.cross_entropy_forward_packed(model, "train", x[:rows], y[:rows])
        loss.backward()
        if dist is not None:
            dist.all_reduce_gradients(model.parameters())
        opt.step()

    if a.sync_bn:
        return sync_bn_step(a, model, step)

    # ---- 1. pack throughput over the real gradient set
    step(rows=2)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    bucket = FlatBucket(grads, dev)
    n = sum(bucket.lengths)
    print(f"ResNet-{a.layers}: {len(grads)} gradient tensors, {n} elements ({n * 4 / 1e6:.1f} MB), flat buffer {bucket.elems} elements")
    other = torch.empty_like(bucket.flat)

    def window(fn, reps=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3

    for name, fn in (("pack, scale 1/2", lambda: bucket.pack(0.5)), ("pack, scale 1 (bit copy)", lambda: bucket.pack(1.0)),
                     ("unpack, scale 1", lambda: bucket.unpack(1.0)), ("torch copy_ of the flat buffer", lambda: other.copy_(bucket.flat))):
        window(fn, 10)
        times = [window(fn) for _ in range(a.repeats)]
        rates = [8 * n / t / 1e9 for t in times]
        print(f"{name:32s} median {statistics.median(times) * 1e6:8.1f} us  {statistics.median(rates):7.0f} GB/s  "
              f"(windows: {min(rates):.0f} .. {max(rates):.0f} GB/s; {bucket._n_chunks} workgroups)")
    if a.skip_step:
        return

    # ---- 2. the step with and without a forced world of one
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dist = DataParallel.from_env("nccl", timeout_s=60, force=True)
    try:
        for d in (None, dist, None, dist):   # warm-up: code objects, the allocator, RCCL's first collective
            step(d)
        torch.cuda.synchronize()
        times = {"plain": [], "world of one": []}
        for _ in range(a.repeats):
            for name, d in (("plain", None), ("world of one", dist)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(d)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps)
        for name, t in times.items():
            print(f"step, {name:14s} batch {a.batch}: median {statistics.median(t) * 1e3:8.2f} ms  (windows of {a.steps} steps: "
                  f"{min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f} ms)")
        print(f"difference of the medians: {(statistics.median(times['world of one']) - statistics.median(times['plain'])) * 1e3:+.2f} ms")
    finally:
        dist.close()


def sync_bn_step(a, model, step) -> None:
    """3.: the step in a forced world of one, fused BatchNorm entries against the split entries with their collectives."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dist = DataParallel.from_env("nccl", timeout_s=60, force=True)
    variants = (("fused", None), ("sync-bn", dist))
    try:
        for _ in range(2):   # warm-up: code objects, the allocator, RCCL's first collectives
            for _, sync in variants:
                model.set_sync_norm(sync, batch_size=a.batch)
                step(dist)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(a.repeats):
            for name, sync in variants:
                model.set_sync_norm(sync, batch_size=a.batch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(dist)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps)
        norms = sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules())
        print(f"ResNet-{a.layers} bf16, HIP norm / optimiser / head, forced RCCL world of one; {norms} BatchNorms, {2 * norms} all-gathers per step with sync-bn")
        for name, t in times.items():
            print(f"step, {name:8s} batch {a.batch}: median {statistics.median(t) * 1e3:8.2f} ms  (windows of {a.steps} steps: "
                  f"{min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f} ms)")
        print(f"difference of the medians: {(statistics.median(times['sync-bn']) - statistics.median(times['fused'])) * 1e3:+.2f} ms")
    finally:
        model.set_sync_norm(None)
        dist.close()


if __name__ == "__main__":
    main()
