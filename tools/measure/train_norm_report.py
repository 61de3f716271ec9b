"""Per-kernel table of a training step from a `rocprofv3 --kernel-trace --stats --output-format csv` run of
tools/measure/bench_train.py, with the bytes every HIP BatchNorm kernel has to move (computed from the model's shapes) over its
kernel time beside the achievable HBM rate.

    python tools/measure/train_norm_report.py <..._kernel_stats.csv> --layers 152 --batch 256 --steps 5 [--top 30]

--steps: training steps of ONE precision in the trace (bench_train.py: warm-up + timed + event-split steps per norm).
"""

from __future__ import annotations

import argparse
import csv
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from salve_amd.models.resnet_factory import RESNET_SPECS  # noqa: E402

HBM_TBS = 6.3   # achievable HBM rate of the MI355X
RELU, ADD = 1, 2


def bn_layers(layers: int, hw: int = 224):
    """(C, H, flags) of every BatchNorm layer of the trunk, with multiplicity, as the model fuses them."""
    kind, blocks = RESNET_SPECS[layers]
    exp = 4 if kind == "bottleneck" else 1
    out, h, inpl = [(64, hw // 2, RELU)], hw // 4, 64
    for si, (planes, n) in enumerate(zip([64, 128, 256, 512], blocks)):
        for bi in range(n):
            s = 2 if (bi == 0 and si > 0) else 1
            if kind == "bottleneck":
                out += [(planes, h, RELU), (planes, h // s, RELU), (planes * 4, h // s, ADD | RELU)]
            else:
                out += [(planes, h // s, RELU), (planes, h // s, ADD | RELU)]
            if bi == 0 and (s != 1 or inpl != planes * exp):
                out.append((planes * exp, h // s, 0))
            inpl, h = planes * exp, h // s
    return out


def bn_bytes(layers: int, batch: int, esize: int):
    """Activation bytes per training step by kernel family (the per-channel vectors and partials are left out)."""
    b = {"bn_stats_kernel": 0, "bn_apply_kernel": 0, "bn_bwd_reduce_kernel": 0, "bn_bwd_dx_kernel": 0}
    for c, h, f in bn_layers(layers):
        e = batch * h * h * c * esize
        relu, add = bool(f & RELU), bool(f & ADD)
        b["bn_stats_kernel"] += e
        b["bn_apply_kernel"] += e * (2 + add)
        b["bn_bwd_reduce_kernel"] += e * (2 + relu)
        b["bn_bwd_dx_kernel"] += e * (3 + relu + add)
    return b


def short(name: str) -> str:
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return name.split("(")[0][:72] if not name.startswith("at::") else name[:72]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--layers", type=int, default=152)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--top", type=int, default=30)
    a = ap.parse_args()
    rows = {}
    with open(a.csv) as f:
        for r in csv.DictReader(f):
            k = short(r["Name"])
            calls, ns = rows.get(k, (0, 0))
            rows[k] = (calls + int(r["Calls"]), ns + int(r["TotalDurationNs"]))
    total = sum(ns for _, ns in rows.values())
    print("| kernel | calls per step | ms per step | share |\n|---|---:|---:|---:|")
    for k, (calls, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1])[:a.top]:
        print(f"| `{k}` | {calls / a.steps:g} | {ns / a.steps / 1e6:.2f} | {100 * ns / total:.1f} % |")
    print(f"| all kernels | | {total / a.steps / 1e6:.1f} | 100 % |\n")
    print("| BatchNorm kernel | dtype | GB per step | ms per step | TB/s | of 6.3 TB/s |\n|---|---|---:|---:|---:|---:|")
    for dt, esize in (("float", 4), ("unsigned short", 2)):
        for fam, nbytes in bn_bytes(a.layers, a.batch, esize).items():
            ns = sum(v[1] for k, v in rows.items() if k.startswith(f"{fam}<{dt}"))
            if ns:
                rate = nbytes / (ns / a.steps / 1e9) / 1e12
                print(f"| `{fam}` | {'fp32' if esize == 4 else 'bf16'} | {nbytes / 1e9:.2f} | {ns / a.steps / 1e6:.2f} | {rate:.2f} | {100 * rate / HBM_TBS:.0f} % |")


if __name__ == "__main__":
    main()
