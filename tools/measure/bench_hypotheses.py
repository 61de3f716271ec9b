"""GPU box: what generating the alignment hypotheses costs (salve_hypotheses_generate; results in profiles/r26_hypotheses.txt).
Nothing here is gated, and no required time is set.

  python tools/measure/bench_hypotheses.py [--out profiles/r26_hypotheses.txt]

HIP events around `iters` calls through the C ABI, the tables uploaded once and every shape warmed up first, `rounds` rounds each (the spread is
printed with the median): one floor of 64 synthetic panoramas (2 doors, 1 window, 1 opening each: 2016 pairs of 11 candidates) and 512 such
floors in one call (1 032 192 pairs, 11 354 112 candidate rows of 48 bytes); and ZInD 0000 floor_01 with MHNet's predictions
(tests/golden: 32 panoramas, 496 pairs, 4882 candidates, 2672 hypotheses) once through generate(), uploads, download and host assembly included
(a host clock around it, after a synchronise).
The reference's loop cannot run on this box (gtsam and shapely are not installed): NO speed-up over it is claimed."""
import argparse
import ctypes
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]


def events_ms(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def floor_of_64(hc, np, seed):
    rng = np.random.default_rng(seed)
    return hc.make_floor(f"{1000 + seed}", "floor_01", list(range(64)), [hc.random_wdos(rng, 2, 1, 1) for _ in range(64)],
                         gt_wdos=[[v for _, v in hc.random_wdos(rng, 1, 1, 0)] for _ in range(64)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--floors", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    for p in (ROOT, ROOT / "tests"):
        sys.path.insert(0, str(p))
    import numpy as np
    import torch

    from salve_amd import _lib, hypotheses
    from tests import hypotheses_cases as hc

    assert torch.cuda.is_available(), "bench_hypotheses.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# salve_hypotheses_generate on {torch.cuda.get_device_name(0)}: ms per call (HIP events), {args.iters} calls per round, {args.rounds} rounds: median [min .. max]")
    say("# the reference's per-pair Python loop cannot run here (no gtsam, no shapely): no speed-up over it is claimed")
    one = hc.floor_input(floor_of_64(hc, np, 0))
    shapes = [("1 floor of 64 panoramas", [one]), (f"{args.floors} floors of 64 panoramas", [hc.floor_input(floor_of_64(hc, np, k)) for k in range(args.floors)])]
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for label, floors in shapes:
        packed = hypotheses.pack(floors)
        t = [up(a) for a in (packed.wdo_xy, packed.wdo_type, packed.wdo_off, packed.gt_xy, packed.gt_off, packed.poses, packed.pairs)]
        rows = torch.empty(max(1, packed.n_rows) * _lib.HYP_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        out = torch.empty(len(packed.pairs) * _lib.HYP_PAIR_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.salve_hypotheses_generate(vp(t[0]), vp(t[1]), vp(t[2]), len(packed.wdo_type), vp(t[3]), vp(t[4]), len(packed.gt_xy), vp(t[5]),
                                                     len(packed.poses), vp(t[6]), len(packed.pairs), packed.max_capacity, 0.65, vp(rows), packed.n_rows, vp(out),
                                                     stream), "salve_hypotheses_generate")

        call()
        torch.cuda.synchronize()
        po = out.cpu().numpy().view(_lib.HYP_PAIR_OUT_DTYPE)
        assert int(po["n_kept"].min()) >= 0
        events_ms(torch, call, 2)   # warm-up
        ms = [events_ms(torch, call, args.iters) for _ in range(args.rounds)]
        med = statistics.median(ms)
        written = int(po["n_kept"].sum()) * _lib.HYP_ROW_DTYPE.itemsize + len(po) * _lib.HYP_PAIR_OUT_DTYPE.itemsize
        say(f"{label:28s} {len(packed.pairs):9d} pairs {packed.n_rows:10d} candidates {int(po['n_kept'].sum()):10d} kept {int(po['n_rejected'].sum()):9d} rejected   "
            f"{med:9.4f} [{min(ms):.4f} .. {max(ms):.4f}] ms   {1e3 * med / max(1, len(packed.pairs)):.4f} us per pair, {written / med / 1e6:.2f} GB/s written")
    # the fixture floor end to end
    with tempfile.TemporaryDirectory() as tmp:
        raw, root = hc.expand_fixture(ROOT / "tests" / "golden", tmp)
        t0 = time.perf_counter()
        floors = hypotheses.load_floors(raw, root, ["0000"])
        t_load = time.perf_counter() - t0
        hypotheses.generate(floors, dev)   # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            (h,) = hypotheses.generate(floors, dev)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        n = hypotheses.write_tree([h], Path(tmp) / "out")
        t_write = time.perf_counter() - t0
    say(f"ZInD 0000 floor_01 end to end: load_floors (host: 32 prediction files, layouts) {1e3 * t_load:.1f} ms; generate() with uploads, download and host "
        f"assembly {statistics.median(ts):.2f} [{min(ts):.2f} .. {max(ts):.2f}] ms (host clock) for {len(h)} hypotheses; write_tree (optional) {1e3 * t_write:.1f} ms for {n} files")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
