"""GPU box: what the floor pose graph costs (salve_pose_graph_solve; results in profiles/r19_pose_graph.txt).

  python tools/measure/bench_pose_graph.py                      (a) the launch alone, (b) score_floor with the keyword off / on
  python tools/measure/bench_pose_graph.py --ab-parent DIR      score_floor WITHOUT the keyword: the tree at DIR (the parent commit, built)
                                                                against this tree, alternating child processes

(a) HIP events around `iters` launches through the C ABI, tables uploaded once: 1 floor of 64 panoramas, 512 such floors in one launch (8 rows
    per pair: 7 losing candidates beside the chosen one), and the K_48, 256-panorama sparse and 256-panorama path cases of
    tests/pose_graph_cases.py.  The outputs of the first launch are compared with the numpy emulator's for the three cases.
(b) the synthetic floor of tests/test_gpu_pose_graph_floor.py on disk (3 panoramas, 3 hypotheses, ResNet-18): whole ingest.score_floor calls,
    a host clock around each (the call ends in file writes behind a device synchronise), keyword off and on alternating in ONE process.
    The floor is tiny: the figure is what the keyword ADDS to a call (one upload, one launch, one status read, one download, one JSON
    file), not a share of a real floor's time.
--ab-parent: (b)'s OFF path in child processes of both trees, alternating, on one box: is the keyword-off time inside the parent's
    run-to-run spread.  The driver process opens no GPU."""
import argparse
import ctypes
import subprocess
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]


def events_ms(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def floor_of_64(pc, np, seed, rows_per_pair=8):
    """64 panoramas, band 3 plus 64 chords, 4 corrupted edges; every pair with 7 more, less probable and misplaced, candidates."""
    rng = np.random.default_rng(seed)
    rows, n = pc._banded(rng, 64, 3, 64, 4).build()
    more = np.repeat(rows, rows_per_pair - 1)
    more["prob"] = (more["prob"] * rng.uniform(0.5, 0.99, size=len(more))).astype(np.float32)
    more["t"] += rng.uniform(-1, 1, size=(len(more), 2)).astype(np.float32)
    rows = np.concatenate([rows, more])
    return rows[np.lexsort((rows["i2"], rows["i1"]))], n


def launch_alone(args):
    import numpy as np
    import torch

    from salve_amd import _lib, status
    from tests import pose_graph_cases as pc

    dev = torch.device("cuda:0")
    lib = _lib.load()
    shapes = [("1 floor of 64", pc.make_case("one-64", [floor_of_64(pc, np, 0)]), False),
              ("512 floors of 64", pc.make_case("512-64", [floor_of_64(pc, np, k) for k in range(512)]), False)]
    shapes += [(name, pc.case(name), True) for name in ("k48-dense", "256-nodes-sparse", "path-256")]
    print(f"# (a) salve_pose_graph_solve alone: {args.iters} launches per round, ms per launch (HIP events)")
    for label, case, compare in shapes:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
        rows, floor_start, n_nodes = up(case["rows"]), up(case["floor_start"]), up(case["n_nodes"])
        F, M, N = len(case["n_nodes"]), case["max_nodes"], len(case["rows"])
        outs = [torch.empty(max(1, k) * dt.itemsize, dtype=torch.uint8, device=dev) for k, dt in ((N, pc.ROW_OUT), (F * M, pc.NODE_OUT), (F, pc.FLOOR_OUT))]
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def fn():
            _lib.check(lib.salve_pose_graph_solve(vp(rows), N, vp(floor_start), vp(n_nodes), F, M, float(case["confidence_threshold"]),
                                                  float(case["rot_threshold_deg"]), float(case["trans_threshold"]), case["cycle_filter"], vp(outs[0]),
                                                  vp(outs[1]), vp(outs[2]), None, 0, status.ptr(dev), stream), "salve_pose_graph_solve")

        for _ in range(3):
            fn()
        status.check(dev, label)
        fo = outs[2].cpu().numpy().view(pc.FLOOR_OUT)
        if compare:
            want = pc.expected(case)[0]
            assert fo.tobytes() == want[2][pc.GUARD:-pc.GUARD].tobytes()
            assert outs[1].cpu().numpy().view(pc.NODE_OUT)[:F * M].tobytes() == want[1][pc.GUARD:-pc.GUARD].tobytes()
        ms = [events_ms(torch, fn, args.iters) for _ in range(args.rounds)]
        print(f"{label:20s} {N:7d} rows {int(fo['n_chosen'].sum()):6d} edges {int(fo['n_triplets'].sum()):7d} cycles {int(fo['n_localized'].sum()):6d} localized   "
              + "  ".join(f"{m:8.4f}" for m in ms) + " ms", flush=True)


def make_floor_on_disk(tmp):
    from tests.test_gpu_ingest import make_floor

    raw, depth_root, hyp_root, _ = make_floor(Path(tmp), n_panos=3, n_hyp=3)
    return SimpleNamespace(tmp=Path(tmp), raw=raw, depth_root=depth_root, hyp_root=hyp_root)


def score_floor_times(floor, calls, keywords, tag):
    """ms of `calls` score_floor calls per entry of `keywords` (None: without the keyword), alternating; one model, one process."""
    import torch

    from salve_amd import ingest, synthetic
    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-20.0, 20.0]))
    ms = {k: [] for k in range(len(keywords))}
    for c in range(calls + 2):   # (two warm-up rounds)
        for k, kw in enumerate(keywords):
            t0 = time.perf_counter()
            ingest.score_floor(model, torch.device("cuda:0"), str(floor.raw), str(floor.depth_root), str(floor.hyp_root), str(floor.tmp / "bev"), "0003",
                               "floor_01", str(floor.tmp / f"preds_{tag}_{k}"), batch_size=2, chunk=4, **({} if kw is None else {"pose_graph": kw}))
            torch.cuda.synchronize()
            if c >= 2:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return ms


def fmt(ms):
    return "  ".join(f"{m:7.2f}" for m in ms) + f"   mean {sum(ms) / len(ms):7.2f}  spread {max(ms) - min(ms):6.2f} ms"


def score_on_off(args):
    with tempfile.TemporaryDirectory() as tmp:
        floor = make_floor_on_disk(tmp)
        ms = score_floor_times(floor, args.calls, [None, {"confidence_threshold": 0.5, "cycle_filter": False}], "onoff")
    print(f"# (b) ingest.score_floor on the synthetic floor (3 panoramas, 3 hypotheses, ResNet-18): {args.calls} calls each, alternating, ms per call")
    print("keyword off  " + fmt(ms[0]))
    print("keyword on   " + fmt(ms[1]), flush=True)


def child(args):
    """One tree's OFF path: its salve_amd, this file's floor and timing."""
    sys.path.insert(0, str(Path(args.child).resolve()))
    floor = SimpleNamespace(tmp=Path(args.floor), raw=Path(args.floor) / "zind", depth_root=Path(args.floor) / "depth", hyp_root=Path(args.floor) / "hyp")
    import salve_amd

    assert Path(salve_amd.__file__).resolve().parents[1] == Path(args.child).resolve()
    print(fmt(score_floor_times(floor, args.calls, [None], args.tag)[0]), flush=True)
    return 0


def ab_parent(args):
    trees = [("parent", Path(args.ab_parent).resolve()), ("product", ROOT)]
    with tempfile.TemporaryDirectory() as tmp:
        sys.path.insert(0, str(ROOT))
        make_floor_on_disk(tmp)   # (host work only: files)
        print(f"# ingest.score_floor WITHOUT the keyword, {args.calls} calls per child process, ms per call: the parent commit's tree and this one, alternating")
        for r in range(args.rounds):
            for tag, tree in trees:
                p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(tree), "--floor", tmp, "--tag", f"{tag}{r}", "--calls",
                                    str(args.calls)], cwd=str(tree), capture_output=True, text=True, timeout=400)
                if p.returncode != 0:
                    print(f"{tag} failed ({p.returncode}):", p.stderr[-2000:], flush=True)
                    return 1
                print(f"{tag:8s} {p.stdout.strip().splitlines()[-1]}", flush=True)
        a, b = (sorted(Path(tmp).glob(f"preds_{tag}0_0/batch_*.json")) for tag, _ in trees)
        same = [x.read_bytes() for x in a] == [x.read_bytes() for x in b] and len(a) > 0
        print(f"# prediction files of the two trees byte for byte equal: {same}", flush=True)
        return 0 if same else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50, help="launches per round of (a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=6, help="score_floor calls per variant of (b), per child of --ab-parent")
    ap.add_argument("--only", choices=("launch", "score"), help="one of the two parts")
    ap.add_argument("--ab-parent", metavar="DIR", help="a built checkout of the parent commit")
    ap.add_argument("--child", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--floor", help=argparse.SUPPRESS)
    ap.add_argument("--tag", default="child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.ab_parent:
        return ab_parent(args)
    sys.path.insert(0, str(ROOT))
    if args.only != "score":
        launch_alone(args)
    if args.only != "launch":
        score_on_off(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
