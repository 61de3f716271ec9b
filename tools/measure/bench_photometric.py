"""Time the photometric train-tile call (salve_bev_train_tiles_jitter: memset + grey-sum launch + tile launch) beside
the plain one (salve_bev_train_tiles) on the same inputs, on one MI355X, at the shipped shape: 501 x 501 images, 234 -> 224,
ceiling + floor (four images per example, 16 channels), batch 256, bf16.

    python tools/measure/bench_photometric.py [--batch 256] [--reps 30] [--rounds 5] [--precision {bf16,fp32}]

HIP events around each call; the two calls alternate call by call inside a round; a round reports the median of its `reps` calls, and
the rounds' minimum and maximum are the spread.  Also: the jitter call with every record's contrast disabled (no grey sum is taken: the
first launch returns at once), and with contrast alone (the sum and one blend, no hue).  The draws are `TrainTransform.draw_jitter`'s.
Per-kernel times: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/measure/bench_photometric.py`.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from salve_amd import status, train_feed  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402
from salve_amd.transforms import TrainTransform  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric.py measures on the MI355X: no device, no number")
    dev = torch.device("cuda:0")
    B, K = a.batch, 2
    ras = BevRasteriser(dev)                       # 501 x 501 BEV images, 234 -> 224
    H, W = ras.bev_hw
    gen = torch.Generator(device="cpu").manual_seed(0)
    # smooth-ish images with colour (pure noise would make every pixel take hue's slowest select; a render is mostly flat)
    base = torch.randint(0, 256, (2 * B * K, H // 8 + 1, W // 8 + 1, 3), generator=gen, dtype=torch.int32).to(dev)
    img = base.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
    bev = (img[..., 0] | (img[..., 1] << 8) | (img[..., 2] << 16)).contiguous()
    smp = np.repeat(np.arange(B), K)
    k = np.tile(np.arange(K), B)
    jobs_a = ras.upload_tile_jobs(np.arange(B * K), smp, 6 * k)
    jobs_b = ras.upload_tile_jobs(B * K + np.arange(B * K), smp, 6 * k + 3)
    tf = TrainTransform((ras.resize, ras.resize), (ras.crop, ras.crop), jitter_types=train_feed.JITTER_TYPES)
    import random

    random.seed(0)
    torch.manual_seed(0)
    aug = torch.from_numpy(train_feed.aug_table([tf.draw() for _ in range(B)]).view(np.uint8)).to(dev)
    draws = train_feed.jitter_draws(tf, B, 2 * K)
    table = lambda d: torch.from_numpy(train_feed.jitter_table(d).view(np.uint8)).to(dev)
    variants = {
        "plain salve_bev_train_tiles": None,
        "jitter, all four operations": table(draws),
        "jitter, contrast disabled (no grey sum)": table([(o, m & ~2, *f) for o, m, *f in draws]),
        "jitter, contrast alone": table([(o, 2, *f) for o, m, *f in draws]),
    }
    out = torch.empty((B, ras.crop, ras.crop, 16), dtype=torch.bfloat16 if a.precision == "bf16" else torch.float32, device=dev)

    def call(jit):
        ras.train_tiles(bev, bev, jobs_a, jobs_b, K, aug, B, out, jitter=jit)

    for jit in variants.values():   # warm-up: code objects, the workspace
        for _ in range(3):
            call(jit)
    torch.cuda.synchronize()
    status.check(dev, "warm-up")
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        times = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, jit in variants.items():   # alternating call by call
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(jit)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        for name in variants:
            rounds[name].append(statistics.median(times[name]))
    status.check(dev, "timed calls")
    print(f"# {torch.cuda.get_device_name(0)}; batch {B}, {2 * B * K} images of {H} x {W}, {ras.resize} -> {ras.crop}, 16 channels, {a.precision}; "
          f"HIP events around one call, median of {a.reps} alternating calls per round, {a.rounds} rounds")
    plain = statistics.median(rounds["plain salve_bev_train_tiles"])
    for name, r in rounds.items():
        print(f"{name}: {statistics.median(r):.3f} ms per batch (rounds {min(r):.3f} .. {max(r):.3f}); + {statistics.median(r) - plain:.3f} ms over the plain call")


if __name__ == "__main__":
    main()
