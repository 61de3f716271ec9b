"""GPU box: what axis alignment by vanishing angle costs (salve_pose_graph_axis_align; results in profiles/r27_axis_align.txt).
Nothing here is gated, and no required time is set.

  python tools/measure/bench_axis_align.py [--out profiles/r27_axis_align.txt]

HIP events around `iters` calls through the C ABI, the tables uploaded once and every shape warmed up first, `rounds` rounds each (the spread is
printed with the median): one floor of 64 panoramas and 2048 rows, 512 such floors in one call (1 048 576 rows), and one floor of 256
panoramas and 8192 rows.  The floors are tests/axis_align_cases.py's synthetic ones (rooms of 4 to 30 vertices, seven W/D/Os a panorama,
corrections on both sides of 15 degrees); the first shape's result is compared with the emulator before anything is timed.
The reference's per-measurement Python loop cannot run on this box (gtsam is not installed): NO speed-up over it is claimed."""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
TABLES = ("rows", "floor_start", "n_nodes", "row_wdo", "pano_base", "room_off", "room_xy", "wdo_off", "wdo_xy", "wdo_type", "vanishing_deg")


def events_ms(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def repeat_floor(np, case, times):
    """The one-floor case `times` times in one call: the row tables tiled, the panorama tables tiled with their offsets moved on."""
    N, P = len(case["rows"]), len(case["vanishing_deg"])
    tile_off = lambda off, total: np.concatenate([[0]] + [off[1:] + k * total for k in range(times)]).astype(np.int64)
    return {**case, "rows": np.tile(case["rows"], times), "row_wdo": np.tile(case["row_wdo"], times),
            "floor_start": (np.arange(times + 1) * N).astype(np.int32), "n_nodes": np.full(times, P, np.int32), "pano_base": (np.arange(times) * P).astype(np.int32),
            "room_off": tile_off(case["room_off"], len(case["room_xy"])), "room_xy": np.tile(case["room_xy"], (times, 1)),
            "wdo_off": tile_off(case["wdo_off"], len(case["wdo_type"])), "wdo_xy": np.tile(case["wdo_xy"], (times, 1, 1)),
            "wdo_type": np.tile(case["wdo_type"], times), "vanishing_deg": np.tile(case["vanishing_deg"], times)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--floors", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    from salve_amd import _lib
    from tests import axis_align_cases as ac

    assert torch.cuda.is_available(), "bench_axis_align.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def floor(n_panos, n_rows, seed):
        b = ac.Builder(f"{n_panos}-panoramas")
        ac.bulk_floor(b, n_panos, n_rows, seed)
        return b.build()

    say(f"# salve_pose_graph_axis_align on {torch.cuda.get_device_name(0)}: ms per call (HIP events), {args.iters} calls per round, {args.rounds} rounds: median [min .. max]")
    say("# the reference's per-measurement Python loop cannot run here (no gtsam): no speed-up over it is claimed")
    one = floor(64, 2048, 1)
    shapes = [("1 floor of 64 panoramas", one, True), (f"{args.floors} floors of 64 panoramas", repeat_floor(np, one, args.floors), False),
              ("1 floor of 256 panoramas", floor(256, 8192, 2), False)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for label, case, verify in shapes:
        N, F = len(case["rows"]), len(case["n_nodes"])
        t = {k: torch.from_numpy(np.ascontiguousarray(case[k]).reshape(-1).view(np.uint8).copy()).to(dev) for k in TABLES}
        p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
        out_rows = torch.empty(N * ac.ROW.itemsize, dtype=torch.uint8, device=dev)
        out_axis = torch.empty(N * ac.ROW_OUT.itemsize, dtype=torch.uint8, device=dev)
        out_floors = torch.empty(F * ac.FLOOR_OUT.itemsize, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.salve_pose_graph_axis_align(p["rows"], N, p["floor_start"], p["n_nodes"], F, p["row_wdo"], p["pano_base"], p["room_off"], p["room_xy"],
                                                       len(case["room_xy"]), p["wdo_off"], p["wdo_xy"], p["wdo_type"], len(case["wdo_type"]), p["vanishing_deg"],
                                                       len(case["vanishing_deg"]), ctypes.c_void_p(out_rows.data_ptr()), ctypes.c_void_p(out_axis.data_ptr()),
                                                       ctypes.c_void_p(out_floors.data_ptr()), None, stream), "salve_pose_graph_axis_align")

        call()
        torch.cuda.synchronize()
        fo = out_floors.cpu().numpy().view(ac.FLOOR_OUT)
        assert int(fo["n_malformed"].sum()) == 0 and int(fo["bad_extent"].sum()) == 0
        if verify:
            _, want_axis, want_floors, _, _, _ = ac.emulate(case)
            assert fo.tobytes() == want_floors.tobytes() and out_axis.cpu().numpy().view(ac.ROW_OUT)["status"].tolist() == want_axis["status"].tolist()
        events_ms(torch, call, 2)   # warm-up
        ms = [events_ms(torch, call, args.iters) for _ in range(args.rounds)]
        med = statistics.median(ms)
        moved = N * (2 * ac.ROW.itemsize + ac.WDO.itemsize + ac.ROW_OUT.itemsize)
        say(f"{label:28s} {N:9d} rows {int(fo['n_applied'].sum()):9d} applied {int(fo['n_too_large'].sum()):9d} too large   "
            f"{med:9.4f} [{min(ms):.4f} .. {max(ms):.4f}] ms   {1e3 * med / N:.4f} us per row, {moved / med / 1e6:.2f} GB/s of rows read and written")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
