"""Time the device JPEG coder (salve_bev_jpeg_encode) and the dataset driver's two JPEG routes on one MI355X:

  * --encode: `BevRasteriser.jpeg_encode` of N 501 x 501 images per call, on real renders of the synthetic scene and on full-frame
    noise: HIP events around the call, per image; the scans' sizes; and against them the pixel download the host route makes
    (`export_u8(bev).cpu()`) and the scan download the device route makes (one 2-D copy of [n, longest scan] bytes); and, on the same
    images, `BevRasteriser.jpeg_roundtrip`, which has no tool of its own, by events likewise;
  * --floor FILES: `render_dataset.render_building_floor_pairs` on one synthetic floor on disk with at least FILES tile files (four
    panoramas, FILES / 4 hypotheses, two surfaces), every route of --routes into a fresh directory, alternating, --rounds times:
    files / s by the host clock (the call ends with the files written), and the device route's files compared byte for byte
    with the host route's.  Route "host" passes no `jpeg` argument, so the same command times a checkout from before the
    argument existed: `--repo PATH` imports salve_amd from that tree.

    python tools/measure/bench_jpeg_encode.py --encode [--n 1024] [--reps 5]
    python tools/measure/bench_jpeg_encode.py --floor 2048 [--routes host,device] [--rounds 2] [--repo PATH]

Per-launch times: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/measure/bench_jpeg_encode.py --encode --reps 1`.
Medians; run the command twice for the spread.
"""

from __future__ import annotations

import argparse
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--floor", type=int, default=0)
    ap.add_argument("--routes", default="host,device")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repo", default=str(Path(__file__).resolve().parents[2]))
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, ARGS.repo)

import torch  # noqa: E402

from salve_amd import ingest, render_dataset, synthetic  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")


def _timed(fn, reps: int):
    """Median milliseconds of fn() by HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def _host_timed(fn, reps: int):
    """Median milliseconds of fn() by the host clock; fn ends with a download (a synchronise)."""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def bench_encode(n: int, reps: int) -> None:
    ras = BevRasteriser(DEV)
    Hb, Wb = ras.bev_hw
    panos = synthetic.make_panos(4)
    rgb = torch.from_numpy(np.stack([p[0] for p in panos])).to(DEV)
    depth = torch.from_numpy(np.stack([p[1] for p in panos]).view(np.int16)).to(DEV)
    hyp = synthetic.make_hypotheses(n, 4, seed=7)
    h = pack_hypotheses(hyp.i1, [SURFACES["floor"] if k % 2 == 0 else SURFACES["ceiling"] for k in range(n)], hyp.R, hyp.t, [1] * n)
    renders = torch.empty((n, Hb, Wb), dtype=torch.int32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    for lo in range(0, n, 256):
        m = min(256, n - lo)
        ras.render_counted(rgb, depth, ras.upload_hypotheses(h[lo:lo + m]), m, renders[lo:lo + m], counts[lo:lo + m])
    ras.check("bench_jpeg_encode renders")
    noise = torch.randint(0, 1 << 24, (n, Hb, Wb), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    print(f"n = {n} images of {Hb} x {Wb}; bound {ras.lib.salve_bev_jpeg_encode_max_bytes(Hb, Wb)} bytes, default slot "
          f"{ras.jpeg_encode(renders[:1])[0].shape[1]} bytes, workspace {ras.lib.salve_bev_jpeg_encode_workspace_bytes(n, Hb, Wb) / 2**20:.0f} MiB")
    rt_out = torch.empty_like(renders)
    for name, imgs in (("renders", renders), ("noise", noise)):
        med, lo, hi = _timed(lambda: ras.jpeg_roundtrip(imgs, 75, out=rt_out), reps)
        print(f"{name:8s} roundtrip {med:8.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {med / n * 1e3:7.2f} us per image")
        scan, nbytes = ras.jpeg_encode(imgs, 75)
        lens = nbytes.cpu().numpy()
        med, lo, hi = _timed(lambda: ras.jpeg_encode(imgs, 75), reps)
        longest = int(lens.max())
        px = _host_timed(lambda: ras.export_u8(imgs).cpu(), max(2, reps // 2))
        sc = _host_timed(lambda: scan[:, :longest].cpu(), max(2, reps // 2))
        print(f"{name:8s} encode {med:8.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {med / n * 1e3:7.2f} us per image | scan bytes mean {lens.mean():9.0f} "
              f"min {lens.min()} max {longest} overflowed {int((lens > scan.shape[1]).sum())} | download per image: pixels {Hb * Wb * 3} B in "
              f"{px[0] / n * 1e3:7.2f} us (export + copy), scans {longest} B in {sc[0] / n * 1e3:7.2f} us")


def make_floor(root: Path, n_hyp: int):
    """The reference's on-disk layout for one floor: four 2048 x 1024 JPEG panoramas, 1024 x 512 depth maps, n_hyp Sim(2) files."""
    raw, depth_root, hyp_root = root / "zind", root / "depth", root / "hyp"
    (raw / "0003" / "panos").mkdir(parents=True)
    for i in range(4):
        rgb, depth = synthetic.make_pano(i)
        fp = raw / "0003" / "panos" / f"floor_01_partial_room_{i:02d}_pano_{i + 3}.jpg"
        image_io.write_jpeg(str(fp), np.repeat(np.repeat(rgb, 2, axis=0), 2, axis=1))
        image_io.write_depth_png(str(depth_root / "0003" / f"{fp.stem}.depth.png"), depth)
    hyp = synthetic.make_hypotheses(n_hyp, 4, seed=2)
    for j in range(n_hyp):
        d = hyp_root / "0003" / "floor_01" / ("gt_alignment_approx" if j % 3 == 0 else "incorrect_alignment")
        d.mkdir(parents=True, exist_ok=True)
        Sim2(hyp.R[j].astype(np.float64), hyp.t[j].astype(np.float64), 1.0).save_as_json(
            str(d / f"{int(hyp.i1[j]) + 3}_{int(hyp.i2[j]) + 3}__door_{j}_0_{'identity' if j % 2 else 'rotated'}.json"))
    return str(raw), str(depth_root), str(hyp_root)


def bench_floor(files: int, routes, rounds: int) -> None:
    root = Path(tempfile.mkdtemp(prefix="jpeg_floor_"))
    try:
        raw, depth_root, hyp_root = make_floor(root, -(-files // 4))
        times = {r: [] for r in routes}
        kept = {}
        for rnd in range(rounds + 1):   # round 0 warms up (code objects, the allocator, the page cache of the panoramas)
            for r in routes:
                out = root / f"bev_{r}_{rnd}"
                kw = {} if r == "host" else {"jpeg": r}
                torch.cuda.synchronize()
                t = time.perf_counter()
                n = render_dataset.render_building_floor_pairs(depth_root, str(out), hyp_root, raw, "0003", "floor_01", None, ["rgb_texture"],
                                                               device=DEV, **kw)
                dt = time.perf_counter() - t
                if rnd:
                    times[r].append(n / dt)
                if rnd == rounds:
                    kept[r] = out
                else:
                    shutil.rmtree(out)
                print(f"round {rnd} route {r:6s}: {n} files in {dt:7.3f} s = {n / dt:8.1f} files/s{'  (warm-up)' if rnd == 0 else ''}", flush=True)
        for r in routes:
            print(f"route {r:6s}: median {statistics.median(times[r]):8.1f} files/s over {rounds} rounds (min {min(times[r]):.1f}, max {max(times[r]):.1f})")
        sizes = np.array([p.stat().st_size for p in sorted(kept[routes[0]].rglob("*.jpg"))])
        print(f"files: {len(sizes)}, bytes mean {sizes.mean():.0f} min {sizes.min()} max {sizes.max()}; host route downloads {501 * 501 * 3} B of pixels "
              f"per image, the device route one [n, longest scan] copy per batch: at most {sizes.max() - 625} B per image, mean scan {sizes.mean() - 625:.0f} B")
        if len(kept) == 2:
            a, b = (sorted(kept[r].rglob("*.jpg")) for r in routes)
            same = [p.relative_to(kept[routes[0]]) for p in a] == [p.relative_to(kept[routes[1]]) for p in b] and all(
                p.read_bytes() == q.read_bytes() for p, q in zip(a, b))
            print(f"the two routes' files are {'IDENTICAL byte for byte' if same else 'DIFFERENT'}")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the MI355X"
    if ARGS.encode:
        bench_encode(ARGS.n, ARGS.reps)
    if ARGS.floor:
        bench_floor(ARGS.floor, ARGS.routes.split(","), ARGS.rounds)
