"""GPU box: what the visual-overlap count costs (salve_bev_pair_overlap; results in profiles/r16_pair_overlap.txt).

  python tools/measure/bench_pair_overlap.py                      (a) the launch alone, (b) score() with visual_overlap off / on
  python tools/measure/bench_pair_overlap.py --ab-parent DIR      bench.py of the tree at DIR (the parent commit, built) against this tree's

(a) 4096 jobs at 501 x 501 over 64 shared b images, HIP events around `iters` launches, `rounds` rounds.  The rate is quoted at the NOMINAL
    2 x 1 004 004 bytes per job; the b images (64 x 1 MB) stay in the caches, so about half of that comes from HBM.  No read-only roof has
    been measured on this box and none is measured here: the figure to set it beside is the float4 copy roof of the bench line (README:
    5.3 TB/s), which counts read + write -- its READ side is half of it.
(b) bench.py's shape (4096 hypotheses, 64 panoramas, ResNet-50, one floor surface, the pipeline's own launch size), one stream and three:
    whole score() calls, synchronised, visual_overlap off and on alternating in ONE process; asserts equal logits.
--ab-parent: the OFF path against the parent commit -- bench.py (which never asks for the overlap) of both trees as child processes in
    alternating rounds on one box, as profiles/r07_owned_half_ab.txt; compares the dumped logits byte for byte.  This mode opens no GPU in
    the driver process."""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def events_ms(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def launch_alone(args):
    import numpy as np
    import torch

    from salve_amd.rasteriser import BevRasteriser

    dev = torch.device("cuda:0")
    ras = BevRasteriser(dev)
    h, w = ras.bev_hw
    n, nb = args.jobs, 64
    g = torch.Generator(device=dev).manual_seed(0)
    mk = lambda k: (torch.randint(1, 1 << 24, (k, h, w), device=dev, generator=g, dtype=torch.int32)
                    * (torch.rand((k, h, w), device=dev, generator=g) < 0.45)).contiguous()
    a, b = mk(n), mk(nb)
    jobs = ras.upload_overlap_jobs(np.arange(n), np.arange(n) % nb)
    out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    fn = lambda: ras.pair_overlap(a, b, jobs, n, out=out)
    for _ in range(3):
        fn()
    nominal = n * 2 * h * w * 4
    print(f"# (a) salve_bev_pair_overlap alone: {n} jobs at {h} x {w} over {nb} shared b images, {args.iters} launches per round")
    for r in range(args.rounds):
        ms = events_ms(torch, fn, args.iters)
        print(f"launch   {ms:7.3f} ms   {nominal / ms / 1e9:6.2f} TB/s nominal (2 x {h * w * 4} B per job)   {nominal / 2 / ms / 1e9:6.2f} TB/s of a images alone", flush=True)
    ras.check("bench_pair_overlap")
    first = out.cpu()
    fn()
    assert torch.equal(out.cpu(), first)
    j = 17
    oa, ob = (a[j] & 0xFFFFFF) != 0, (b[j % nb] & 0xFFFFFF) != 0
    assert first[j].tolist() == [int((oa & ob).sum()), int((oa | ob).sum()), int(oa.sum()), int(ob.sum())]


def score_on_off(args):
    import numpy as np
    import torch

    from salve_amd import synthetic
    from salve_amd.models.early_fusion import EarlyFusionCEResnet
    from salve_amd.pipeline import RenderVerifyPipeline

    dev = torch.device("cuda:0")
    panos = synthetic.make_panos(args.panos)
    rgb, depth = np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    hyp = synthetic.make_hypotheses(args.hyps, args.panos, seed=0)
    model = EarlyFusionCEResnet(args.layers, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    for streams in (1, 3):
        pipe = RenderVerifyPipeline(model, dev, chunk=None, overlap=streams > 1, streams=streams, n_hypotheses=args.hyps)
        pipe.load_panos(rgb, depth)
        prepared = pipe.prepare(hyp)
        run = {False: lambda: pipe.score(prepared), True: lambda: pipe.score(prepared, visual_overlap=True)}
        logits = {}
        for on in (False, True):
            for _ in range(2):
                logits[on] = run[on]().clone()
            torch.cuda.synchronize()
        assert torch.equal(logits[False], logits[True])
        pipe.check("bench_pair_overlap")
        print(f"# (b) score(): {args.hyps} hypotheses, {args.panos} panoramas, ResNet-{args.layers}, streams = {streams}, launches of {pipe.chunk}; "
              f"{args.steps} calls per round, ms per call")
        ms = {False: [], True: []}
        for r in range(args.rounds):
            for on in (False, True):
                ms[on].append(events_ms(torch, run[on], args.steps))
            print(f"streams {streams}   off {ms[False][-1]:8.3f}   on {ms[True][-1]:8.3f}   difference {ms[True][-1] - ms[False][-1]:+7.3f} ms", flush=True)
        off, on = sum(ms[False]) / args.rounds, sum(ms[True]) / args.rounds
        print(f"streams {streams}   mean off {off:.3f}, on {on:.3f}: +{on - off:.3f} ms per {args.hyps} = {100 * (on - off) / off:.2f} % of the step; "
              f"spread of off {max(ms[False]) - min(ms[False]):.3f} ms, of on {max(ms[True]) - min(ms[True]):.3f} ms", flush=True)
        counts = pipe.visual_overlap(prepared)
        print(f"streams {streams}   IoU of the {args.hyps} pairs: median {float(np.median(counts[:, 0, 0] / (counts[:, 0, 1] + 1e-12))):.3f}", flush=True)
        del pipe, prepared
        torch.cuda.empty_cache()


def ab_parent(args):
    trees = [("parent", Path(args.ab_parent).resolve()), ("product", ROOT)]
    flags = ["--gpus", "1", "--steps", str(args.steps), "--warmup", "2", "--no-cpu-baseline", "--no-calibration", "--no-config5", "--no-power-probe"]
    for streams in (1, 3):
        print(f"# bench.py {' '.join(flags)} --streams {streams}: the parent commit's tree and this one, alternating child processes")
        dumps = {}
        for r in range(args.rounds):
            for tag, tree in trees:
                with tempfile.TemporaryDirectory() as d:
                    p = subprocess.run([sys.executable, str(tree / "bench.py"), *flags, "--streams", str(streams), "--dump-outputs", d], cwd=str(tree),
                                       capture_output=True, text=True, timeout=400)
                    if p.returncode != 0:
                        print(f"{tag} failed ({p.returncode}):", p.stderr[-2000:], flush=True)
                        return 1
                    line = json.loads(p.stdout.strip().splitlines()[-1])
                    dumps.setdefault(tag, set()).add((Path(d) / "logits.npy").read_bytes())
                roof, ver = line.get("roofline") or {}, line.get("roofline_verifier") or {}
                print(f"{tag:8s} {line['value']:9.0f} hyp/s  scatter {roof.get('scatter_ms', float('nan')):.3f}  densify {roof.get('densify_ms', float('nan')):.3f}  "
                      f"verifier {ver.get('launch_ms', float('nan')):.2f} ms", flush=True)
        same = len(dumps["parent"] | dumps["product"]) == 1
        print(f"# streams {streams}: logits of all {2 * args.rounds} runs byte for byte equal: {same}", flush=True)
        if not same:
            return 1
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--hyps", type=int, default=4096)
    ap.add_argument("--panos", type=int, default=64)
    ap.add_argument("--layers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20, help="launches per round of (a)")
    ap.add_argument("--steps", type=int, default=8, help="score() calls per round of (b); bench.py --steps of --ab-parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("launch", "score"), help="one of the two parts")
    ap.add_argument("--ab-parent", metavar="DIR", help="a built checkout of the parent commit: bench.py of both trees, alternating")
    args = ap.parse_args()
    if args.ab_parent:
        return ab_parent(args)
    if args.only != "score":
        launch_alone(args)
    if args.only != "launch":
        score_on_off(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
