"""GPU box: what the floor reconstruction report costs (salve_floor_align, salve_floor_iou; results in
profiles/r24_floor_report.txt).  Nothing here is gated.

  python tools/measure/bench_floor_report.py                  (a) the two calls alone, beside salve_pose_graph_solve on floors of the same size
  python tools/measure/bench_floor_report.py --differences    (b) the device's float64 outputs against the numpy emulator over the test cases

(a) HIP events around `iters` calls through the C ABI, tables uploaded once, the entries ALTERNATING round by round on one box: one floor of 64
    panoramas with 1000 alignment subsets and the reference's 501 x 501 raster; 512 such floors (512 000 subsets) in one call.
    salve_pose_graph_solve runs beside them on tools/measure/bench_pose_graph_sample.py's floors of 64 panoramas and 2048 rows.
    The reference's loop cannot run on this box (gtsam, gtsfm and cv2 are not installed): no speed-up over it is claimed.
(b) every case of tests/floor_report_cases.py and the 1210 floor: the largest absolute difference of a float64 output (degrees, coordinate
    units) -- the device's atan2 / sin / cos against numpy's.  tests/test_gpu_floor_report.py asserts four times this value."""
import argparse
import ctypes
import sys
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


def calls_alone(args):
    import numpy as np
    import torch

    from salve_amd import _lib, status
    from tests import floor_report_cases as fc
    from tests import pose_graph_cases as pc
    from tools.measure.bench_pose_graph_sample import floor_of_64

    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    mk = lambda nbytes: torch.empty(max(16, nbytes), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(0)
    print(f"# (a) ms per call (HIP events), {args.iters} calls per round, alternating: floor_align ({args.subsets} subsets per floor) | floor_iou (501 x 501) | "
          "pose_graph_solve (64 panoramas, 2048 rows per floor)")
    for label, n_floors in (("1 floor of 64", 1), ("512 floors of 64", 512)):
        case = fc.build_call(label, [fc.make_floor(rng, 64, n_hyps=args.subsets, p_est=0.9, metres=1.0) for _ in range(n_floors)], img=(501, 501),
                             off=(25.0, 25.0), ppm=10.0)
        t = {k: up(case[k]) for k in ("node_start", "truth", "est", "hyp_start", "masks", "gt_scale", "metres", "room_xy", "room_off")}
        F, N, H, V = n_floors, case["n_nodes"], len(case["masks"]), len(case["room_xy"])
        outs = [mk(H * fc.HYP_OUT.itemsize), mk(N * fc.NODE.itemsize), mk(N * 8), mk(N * 8), mk(F * fc.FLOOR_OUT.itemsize), mk(F * fc.IOU_OUT.itemsize)]
        ws_bytes = int(lib.salve_floor_iou_workspace_bytes(V, N))
        ws = mk(ws_bytes)
        floors = [floor_of_64(pc, np, k) for k in range(n_floors)]
        rows = np.concatenate([r for r, _ in floors])
        tg = {"rows": up(rows), "floor_start": up(np.concatenate([[0], np.cumsum([len(r) for r, _ in floors])]).astype(np.int32)),
              "n_nodes": up(np.array([n for _, n in floors], dtype=np.int32))}
        solve_outs = [mk(len(rows) * pc.ROW_OUT.itemsize), mk(F * 64 * pc.NODE_OUT.itemsize), mk(F * pc.FLOOR_OUT.itemsize)]

        def align():
            _lib.check(lib.salve_floor_align(vp(t["node_start"]), F, N, vp(t["truth"]), vp(t["est"]), vp(t["hyp_start"]), vp(t["masks"]), H, vp(t["gt_scale"]),
                                             vp(t["metres"]), vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]), vp(outs[4]), status.ptr(dev), stream),
                       "salve_floor_align")

        def iou():
            _lib.check(lib.salve_floor_iou(vp(t["room_xy"]), vp(t["room_off"]), V, vp(t["node_start"]), F, N, vp(outs[1]), vp(t["truth"]), vp(t["metres"]), 501,
                                           501, 25.0, 25.0, 10.0, vp(outs[5]), None, vp(ws), ws_bytes, status.ptr(dev), stream), "salve_floor_iou")

        def solve():
            _lib.check(lib.salve_pose_graph_solve(vp(tg["rows"]), len(rows), vp(tg["floor_start"]), vp(tg["n_nodes"]), F, 64, 0.5, 0.5, 0.01, 1, vp(solve_outs[0]),
                                                  vp(solve_outs[1]), vp(solve_outs[2]), None, 0, status.ptr(dev), stream), "salve_pose_graph_solve")

        for _ in range(2):
            align()
            iou()
            solve()
        status.check(dev, label)
        fo, io = outs[4].cpu().numpy().view(fc.FLOOR_OUT)[:F], outs[5].cpu().numpy().view(fc.IOU_OUT)[:F]
        ms = [(events_ms(torch, align, args.iters), events_ms(torch, iou, args.iters), events_ms(torch, solve, args.iters)) for _ in range(args.rounds)]
        print(f"{label:18s} {N:6d} panoramas {H:7d} subsets {V:7d} vertices, {int((fo['best'] >= 0).sum()):4d} aligned, mean IoU {float(io['iou'].mean()):.3f}   "
              + "  ".join(f"{a:8.4f} | {b:8.4f} | {c:7.4f}" for a, b, c in ms) + " ms", flush=True)


def differences():
    import numpy as np

    from tests import floor_report_cases as fc
    from tests import test_gpu_floor_report as gpu

    worst_all = 0.0
    print("# (b) the largest absolute difference of a float64 output from the numpy emulator, per case")
    for c in fc.cases():
        got, _ = gpu.align_on_gpu(c)
        diffs, worst = fc.differences(got, fc.expected_align(c["name"])[0], f64_atol=1e-9)
        igot, _ = gpu.iou_on_gpu(c, fc.raster_est(c))
        idiffs, _ = fc.differences(igot, fc.expected_iou(c["name"])[0])
        print(f"{c['name']:22s} align {worst:.3e}  {'ok' if not diffs else diffs}   iou {'exact' if not idiffs else idiffs}", flush=True)
        worst_all = max(worst_all, worst)
    c, align, _, _ = fc.emulated_1210(str(ROOT / "tests" / "golden"))
    got, _ = gpu.align_on_gpu(c)
    diffs, worst = fc.differences(got, align, f64_atol=1e-9)
    print(f"{'zind-1210-floor-02':22s} align {worst:.3e}  {'ok' if not diffs else diffs}", flush=True)
    worst_all = max(worst_all, worst)
    print(f"# largest over all: {worst_all:.3e} (tests/test_gpu_floor_report.py: MEASURED_F64_DIFF, asserted at four times; the condition caps it at 1e-9)")
    assert np.isfinite(worst_all)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--subsets", type=int, default=1000, help="alignment subsets per floor")
    ap.add_argument("--differences", action="store_true", help="only (b): the float64 differences over the test cases")
    args = ap.parse_args()
    for p in (ROOT, ROOT / "tests"):
        sys.path.insert(0, str(p))
    if args.differences:
        differences()
    else:
        calls_alone(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
