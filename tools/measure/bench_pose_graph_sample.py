"""GPU box: what RANSAC over random spanning trees costs (salve_pose_graph_sample_trees; results in
profiles/r20_pose_graph_sample.txt).

  python tools/measure/bench_pose_graph_sample.py                    (a) the call alone, beside salve_pose_graph_solve on the same tables
  python tools/measure/bench_pose_graph_sample.py --restatement      (b) also the host restatement of the reference's loop on the one floor
  python tools/measure/bench_pose_graph_sample.py --atan2            (c) the device's atan2f against numpy's over the test cases' measured rows

(a) HIP events around `iters` calls through the C ABI, tables uploaded once, the two entries ALTERNATING round by round on one box: 100
    hypotheses (half of the rows each) on 1 floor of 64 panoramas and 2048 rows; 512 such floors (51 200 hypotheses) in one call; 100
    hypotheses on the 256-panorama sparse floor of tests/pose_graph_cases.py, and 100 times the whole 256-panorama path (the deepest tree a
    floor can have).  The winner of the first call on the one floor is compared with the numpy emulator's.
(b) tests/test_pose_graph_sample_host.py's dict-and-Sim2 restatement of the reference's loop with networkx, a host clock around it: a
    RESTATEMENT's time, labelled as one; the reference itself is not on this box.
(c) avg_rot_err of every launched case of tests/pose_graph_sample_cases.py against the emulator: the largest absolute difference in degrees,
    beside the bound the test derives (ROT_ERR_ATOL)."""
import argparse
import ctypes
import sys
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


def floor_of_64(pc, np, seed, n_rows=2048):
    """64 panoramas, band 3 plus 64 chords (256 pairs), n_rows rows: every pair with 8 noisy candidates above the threshold."""
    rng = np.random.default_rng(seed)
    rows, n = pc._banded(rng, 64, 3, 64, 4).build()
    rows = np.repeat(rows, -(-n_rows // len(rows)))[:n_rows]
    rows["prob"] = rng.uniform(0.55, 1.0, size=len(rows)).astype(np.float32)
    rows["t"] += rng.normal(0, 0.02, size=(len(rows), 2)).astype(np.float32)
    return rows[np.lexsort((rows["i2"], rows["i1"]))], n


def shapes(np, pc, sc, n_hyps):
    subsets = lambda rows, seed: sc.random_subsets(np.random.default_rng(seed), len(rows), n_hyps)
    one = floor_of_64(pc, np, 0)
    many = [floor_of_64(pc, np, k) for k in range(512)]
    out = [("1 floor of 64", sc.make_case("one-64", [one], [subsets(one[0], 0)]), True, 1),
           ("512 floors of 64", sc.make_case("512-64", many, [subsets(r, k) for k, (r, _) in enumerate(many)]), False, 1)]
    c = pc.case("256-nodes-sparse")
    fl = (c["rows"], int(c["n_nodes"][0]))
    out.append(("256-nodes-sparse", sc.make_case("256-nodes-sparse", [fl], [subsets(fl[0], 1)]), False, 1))
    # the 256-panorama path, every hypothesis ALL of its 255 rows: 255 label-propagation steps and 255 BFS levels per workgroup (half of the
    # rows would cut the path into short pieces); pose_graph_solve beside it without its cycle filter, or it would chain nothing
    c = pc.case("path-256")
    fl = (c["rows"], int(c["n_nodes"][0]))
    out.append(("path-256, all rows", sc.make_case("path-256", [fl], [[np.arange(len(fl[0]))] * n_hyps]), False, 0))
    return out


def call_alone(args):
    import numpy as np
    import torch

    from salve_amd import _lib, status
    from tests import pose_graph_cases as pc
    from tests import pose_graph_sample_cases as sc

    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    print(f"# (a) ms per call (HIP events), {args.iters} calls per round, the two entries alternating: sample_trees ({args.hypotheses} hypotheses per floor) | "
          "pose_graph_solve on the same rows (with its cycle filter; without it on the path)")
    for label, case, compare, cycle_filter in shapes(np, pc, sc, args.hypotheses):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
        t = {k: up(case[k]) for k in ("rows", "floor_start", "n_nodes", "hyp_start", "masks")}
        F, M, N, H, words = len(case["n_nodes"]), case["max_nodes"], len(case["rows"]), len(case["masks"]), case["mask_words"]
        mk = lambda count, dt: torch.empty(max(1, count) * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev)
        outs = [mk(H, sc.TREE_OUT), mk(N, np.int32), mk(F * M, sc.NODE_OUT), mk(F, sc.FLOOR_OUT)]
        solve_outs = [mk(N, pc.ROW_OUT), mk(F * M, pc.NODE_OUT), mk(F, pc.FLOOR_OUT)]
        ws_bytes = int(lib.salve_pose_graph_sample_workspace_bytes(H, M))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        conf = float(case["confidence_threshold"])

        def sample():
            _lib.check(lib.salve_pose_graph_sample_trees(vp(t["rows"]), N, vp(t["floor_start"]), vp(t["n_nodes"]), F, M, conf, vp(t["hyp_start"]),
                                                         vp(t["masks"]), H, words, vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(outs[3]), vp(ws), ws_bytes,
                                                         status.ptr(dev), stream), "salve_pose_graph_sample_trees")

        def solve():
            _lib.check(lib.salve_pose_graph_solve(vp(t["rows"]), N, vp(t["floor_start"]), vp(t["n_nodes"]), F, M, conf, 0.5, 0.01, cycle_filter, vp(solve_outs[0]),
                                                  vp(solve_outs[1]), vp(solve_outs[2]), None, 0, status.ptr(dev), stream), "salve_pose_graph_solve")

        for _ in range(3):
            sample()
            solve()
        status.check(dev, label)
        fo = outs[3].cpu().numpy().view(sc.FLOOR_OUT)
        if compare:
            want = sc.run_case(case, sc.emulated())[0]
            assert fo["best"].tolist() == want[3]["best"][sc.GUARD:-sc.GUARD].tolist()
            assert outs[1].cpu().numpy().view(np.int32)[:N].tobytes() == want[1][sc.GUARD:-sc.GUARD].tobytes()
        ms = []
        for _ in range(args.rounds):
            ms.append((events_ms(torch, sample, args.iters), events_ms(torch, solve, args.iters)))
        print(f"{label:20s} {N:8d} rows {H:6d} hypotheses {int((fo['best'] >= 0).sum()):4d} winners {ws_bytes / 2 ** 20:8.1f} MiB workspace   "
              + "  ".join(f"{a:8.4f} | {b:7.4f}" for a, b in ms) + " ms", flush=True)
        if compare and args.restatement:
            from tests import test_pose_graph_sample_host as host

            rows = case["rows"]
            meas, idx = host.as_measurements(rows, conf)
            hyps = [{k for k, r in enumerate(idx) if sc.mask_bit(m, int(r))} for m in case["masks"]]
            t0 = time.perf_counter()
            best = host.ransac(meas, hyps)[0]
            print(f"# (b) the host RESTATEMENT of the reference's loop on this floor (networkx, numpy objects; not the reference itself): "
                  f"{1e3 * (time.perf_counter() - t0):.0f} ms, winner {best} (device {int(fo['best'][0])})", flush=True)


def atan2_differences():
    import numpy as np
    import torch

    from tests import pose_graph_sample_cases as sc
    from tests import test_gpu_pose_graph_sample as gpu

    worst = 0.0
    for c in sc.cases():
        if c["refused"]:
            continue
        got, _ = gpu.on_gpu(c)
        want = sc.expected(c)[0]
        for g, w in ((got[0], want[0]), (got[3], want[3])):
            a, b = g["avg_rot_err"][sc.GUARD:-sc.GUARD], w["avg_rot_err"][sc.GUARD:-sc.GUARD]
            m = ~np.isnan(a) & ~np.isnan(b)
            if m.any():
                worst = max(worst, float(np.abs(a[m] - b[m]).max()))
    torch.cuda.synchronize()
    print(f"# (c) avg_rot_err, device against numpy, over every launched test case: largest difference {worst:.3e} degrees "
          f"(the test's derived bound: {sc.ROT_ERR_ATOL:.3e})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20, help="calls per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hypotheses", type=int, default=100, help="hypotheses per floor")
    ap.add_argument("--restatement", action="store_true", help="also time the host restatement of the reference's loop on the one floor")
    ap.add_argument("--atan2", action="store_true", help="also report the device's atan2f difference over the test cases")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    call_alone(args)
    if args.atan2:
        atan2_differences()
    return 0


if __name__ == "__main__":
    sys.exit(main())
