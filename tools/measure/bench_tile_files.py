"""Time a training batch from the rendered tile data set on disk, host-decoded against device-decoded, on one MI355X:

  * the on-disk DataLoader (`training.get_dataloader`: Pillow decodes every tile, one upload and one tile launch per example) -- what a
    checkout from before `decode="device"` does, and the yardstick;
  * `train_files.TileFileSource`: thread-pool read + header parse, one pinned upload, `BevRasteriser.jpeg_decode`, one tile launch.
    Its stages are timed by a subclass kept here (`TimedSource`: the library class knows nothing about clocks) that wraps the
    source's steps: file read and header parse as seconds summed over the reader threads plus the wall time of the pool (the two
    overlap across threads, so only their thread-seconds can be told apart), packing the pinned buffer by the host clock; and by
    HIP events on the stream: the upload, the ENTROPY kernel and the INVERSE kernels -- the timed subclass issues the decode call's
    two stages apart (`jpeg_decode(stages=)`: the same three launches, an event between them) -- and the tile launch.

Workload: a synthetic data set of 501 x 501 `disc` (a render-like textured disc) and `layout` (flat colours and lines) tiles written
with Pillow at quality 75 in the reference's naming, ceiling + floor (4 tiles per example), batch 256 = 1024 tiles per batch.  The files
were written moments before they are read: the reads come from the page cache, not from a disk.

    python tools/measure/bench_tile_files.py [--examples 768] [--batch 256] [--host-batches 2] [--device-batches 6] [--keep DIR]
    python tools/measure/bench_tile_files.py --decode-only [--n 1024] [--reps 5]      # jpeg_decode alone on n tiles, by events
    python tools/measure/bench_tile_files.py --decode-only --entropy both --n 1024,256,64   # ... both entropy stages
    python tools/measure/bench_tile_files.py --panos 32 [--reps 5]                    # 2048 x 1024 panoramas: the entropy stages, Pillow, PanoStore.load

--entropy image (default) is salve_bev_jpeg_decode's one wavefront per tile, lanes the lane-parallel stage (salve_bev_jpeg_decode_lanes);
the feed benchmark takes one of them, --decode-only and --panos also `both` (the same data through one, then the other).
--panos N writes N synthetic panoramas (synthetic.make_pano doubled to 2048 x 1024, the ingest tests' files) and times, on the same
files: the two entropy stages alone by events; Pillow decoding the files in the host route's loop by the host clock; and
ingest.PanoStore.load end to end, decode="host" against decode="device", by the host clock around a call that ends in a synchronise.

--decode-only times the whole call and, in the same run, its two stages apart.  (The inverse stage's two launches, jpeg_idct_kernel and
jpeg_pixels_kernel, can be told apart by `rocprofv3 --kernel-trace --stats -- python tools/measure/bench_tile_files.py --decode-only
--reps 2`, a run of its own.)  Calling the stages apart needs the coefficients to stay in the stream's JPEG workspace, which the
rasteriser's three JPEG methods share: nothing here calls one of them between an entropy stage and its inverse stage.
Medians (min .. max); run the command twice for the spread.
"""

from __future__ import annotations

import argparse
import random
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))   # jpeg_cases.make_image: the test table's disc and layout images

import torch  # noqa: E402

import jpeg_cases as jc  # noqa: E402
from salve_amd import _lib, jpeg, training  # noqa: E402
from salve_amd.dataset.zind_data import ZindData  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402
from salve_amd.train_files import TileFileSource  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402

DEV = torch.device("cuda:0")
H = W = 501


def _stat(ms):
    return f"{statistics.median(ms):9.2f} ms  ({min(ms):.2f} .. {max(ms):.2f}, {len(ms)} batches)"


class TimedSource(TileFileSource):
    """TileFileSource with a clock around each of its steps; `times`: tag -> host seconds, or (start, end) event pairs."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.times = {}

    def _events(self, tag, fn):
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        pair[0].record()
        out = fn()
        pair[1].record()
        self.times.setdefault(tag, []).append(pair)
        return out

    def _clock(self, tag, fn):
        t = time.perf_counter()
        out = fn()
        self.times.setdefault(tag, []).append(time.perf_counter() - t)
        return out

    def _read_one(self, path):   # runs in the reader threads: list.append is atomic
        t0 = time.perf_counter()
        with open(path, "rb") as f:
            data = f.read()
        t1 = time.perf_counter()
        try:
            parsed = jpeg.parse_file(data, restart=self.entropy == "lanes")
        except jpeg.Unsupported:
            parsed = None
        self._per_file.append((t1 - t0, time.perf_counter() - t1))
        return data, parsed

    _read_one_restart = _read_one

    def _read(self, paths):
        self._per_file = []
        out = self._clock("file read + parse: wall time of the thread pool (host)", lambda: super(TimedSource, self)._read(paths))
        self.times.setdefault("    file read, thread-seconds summed (host)", []).append(sum(r for r, _ in self._per_file))
        self.times.setdefault("    parse_file, thread-seconds summed (host)", []).append(sum(p for _, p in self._per_file))
        return out

    def _pack(self, paths, read):
        return self._clock("pack the pinned buffer (host)", lambda: super(TimedSource, self)._pack(paths, read))

    def _upload(self, b):
        return self._events("upload (events)", lambda: super(TimedSource, self)._upload(b))

    def _decode_group(self, *a, **kw):
        st = self._events("entropy kernel (events)", lambda: self.ras.jpeg_decode(*a, stages=_lib.JPEG_STAGE_ENTROPY, **kw)[1])
        self._events("inverse kernels (events)", lambda: self.ras.jpeg_decode(*a, stages=_lib.JPEG_STAGE_INVERSE, **kw))
        return st

    def _tile_launch(self, *a):
        return self._events("tile launch (events)", lambda: super(TimedSource, self)._tile_launch(*a))


def _tile(kind: str, seed: int) -> np.ndarray:
    img = jc.make_image(kind, H, W, seed)
    return np.roll(img, (7 * seed) % 97, axis=1) if kind == "layout" else img   # (layout has no seed of its own)


def write_dataset(root: Path, examples: int) -> None:
    """`examples` pairs of building 1208 (train split), alternating positive / negative; ceiling tiles are discs, floor tiles
    alternate disc / layout."""
    from PIL import Image

    for i in range(examples):
        label = "gt_alignment_approx" if i % 2 == 0 else "incorrect_alignment"
        d = root / label / "1208"
        d.mkdir(parents=True, exist_ok=True)
        for s, surface in enumerate(("ceiling", "floor")):
            for k, (room, pano) in enumerate(((4, 5), (7, 8))):
                kind = "layout" if (surface == "floor" and i % 2) else "disc"
                name = f"pair_{i}___door_0_0_rotated_{surface}_rgb_floor_01_partial_room_{room:02d}_pano_{pano}.jpg"
                Image.fromarray(_tile(kind, 4 * i + 2 * s + k)).save(d / name, quality=75)


def config(root: Path, batch: int) -> TrainingConfig:
    return TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=152, pretrained=False, dataparallel=False, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=("ceiling_rgb_texture", "floor_rgb_texture"),
                          cfg_stem="bench", num_epochs=1, workers=0, batch_size=batch, data_root=str(root), layout_data_root="",
                          model_save_dirpath="")


def bench_feed(a) -> None:
    keep = Path(a.keep) if a.keep else None
    with tempfile.TemporaryDirectory() as tmp:
        root = keep or Path(tmp) / "bev"
        if not (root / "gt_alignment_approx").exists():
            t = time.perf_counter()
            write_dataset(root, a.examples)
            print(f"wrote {4 * a.examples} tiles in {time.perf_counter() - t:.1f} s")
        args = config(root, a.batch)
        sizes = [p.stat().st_size for p in root.rglob("*.jpg")]
        print(f"{len(sizes)} files, {np.mean(sizes) / 1024:.1f} KB on average ({min(sizes) / 1024:.1f} .. {max(sizes) / 1024:.1f}); batch {a.batch} = {4 * a.batch} tiles")

        # ---- the on-disk DataLoader (the parent's path): host clock around batches that end in a device synchronise
        random.seed(0)
        loader = training.get_dataloader(args, "train", seed=0)
        host_ms = []
        it = iter(loader)
        next(it)   # warm-up: code objects, the transform's tables
        torch.cuda.synchronize()
        for _ in range(min(a.host_batches, len(loader) - 1)):
            t = time.perf_counter()
            batch = next(it)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t) * 1e3)
        del it
        print(f"on-disk DataLoader (Pillow, per-example launches)   {_stat(host_ms)}")

        # ---- TileFileSource: whole batches by the host clock (the product class), then its stages (the timed subclass)
        data = ZindData(split="train", transform=None, args=args)
        plan = [np.arange(lo, lo + a.batch) % len(data.data_list) for lo in range(0, a.batch * (a.device_batches + 1), a.batch)]
        for cls in (TileFileSource, TimedSource):
            with cls(DEV, data.data_list, batch_size=a.batch, split="train", seed=0, entropy=a.entropy) as src:
                random.seed(0)
                src.batch(plan[0], src.draws(a.batch))   # warm-up: the pinned buffer, the workspace, code objects
                torch.cuda.synchronize()
                if cls is TimedSource:
                    src.times = {}
                ms = []
                for idx in plan[1:]:
                    t = time.perf_counter()
                    src.batch(idx, src.draws(a.batch))
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t) * 1e3)
                src._check_epoch("bench_tile_files")
                if cls is TileFileSource:
                    dev_ms = ms
                    print(f"TileFileSource (device decode, entropy={a.entropy}, one tile launch)      {_stat(dev_ms)}")
                    print(f"speed-up of the batch: {statistics.median(host_ms) / statistics.median(dev_ms):.1f} x;  files decoded by Pillow in the device route: {src.fallbacks}")
                else:
                    print(f"its stages (TimedSource; the batch itself            {_stat(ms)}):")
                    for tag, vals in src.times.items():
                        print(f"    {tag:<62} {_stat([v * 1e3 if isinstance(v, float) else v[0].elapsed_time(v[1]) for v in vals])}")

        # ---- the same batch both ways: the feed must not change what the model sees
        random.seed(5)
        ref = next(iter(training.get_dataloader(args, "train", seed=0)))
        src2 = TileFileSource(DEV, data.data_list, batch_size=a.batch, split="train", seed=0, entropy=a.entropy)
        random.seed(5)
        x, y = next(iter(src2))
        src2.close()
        want = torch.cat([t.to(DEV) for t in ref[:4]], 1).permute(0, 2, 3, 1)
        same = torch.equal(x[..., :12], want) and bool((x[..., 12:] == 0).all()) and torch.equal(y.reshape(-1).cpu(), ref[4].reshape(-1))
        print(f"first batch of the epoch, DataLoader against TileFileSource (seed 0): {'bit-identical' if same else 'DIFFERENT'}")
        if not same:
            raise SystemExit(1)


def _time_stages(ras, args, kw, reps):
    """Medians by events of the whole jpeg_decode call and of its two stages called apart -> (whole, entropy, inverse) lists of ms."""
    fn = lambda **more: ras.jpeg_decode(*args, **kw, **more)
    for _ in range(2):
        _, st = fn()
    torch.cuda.synchronize()
    assert not bool(st.any())
    whole, ent, inv = [], [], []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        whole.append(s.elapsed_time(e))
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        fn(stages=_lib.JPEG_STAGE_ENTROPY)
        ev[1].record()
        fn(stages=_lib.JPEG_STAGE_INVERSE)
        ev[2].record()
        ev[2].synchronize()
        ent.append(ev[0].elapsed_time(ev[1]))
        inv.append(ev[1].elapsed_time(ev[2]))
    return whole, ent, inv


def _entropies(a):
    return ("image", "lanes") if a.entropy == "both" else (a.entropy,)


def _report(tag, whole, ent, inv, n):
    med = statistics.median
    print(f"{tag}, entropy + inverse: {med(whole):.2f} ms ({min(whole):.2f} .. {max(whole):.2f}); {med(whole) * 1e3 / n:.1f} us per image")
    print(f"    {'entropy stage':<34} {med(ent):.3f} ms ({min(ent):.3f} .. {max(ent):.3f})")
    print(f"    {'inverse kernels (idct + pixels)':<34} {med(inv):.3f} ms ({min(inv):.3f} .. {max(inv):.3f})")


def bench_decode(a) -> None:
    import io

    from PIL import Image

    ras = BevRasteriser(DEV)
    print(f"subsequence: {ras.lib.salve_bev_jpeg_subseq_bytes()} bytes")
    files = []
    for i in range(16):
        buf = io.BytesIO()
        Image.fromarray(_tile("layout" if i % 4 == 3 else "disc", i)).save(buf, format="JPEG", quality=75)
        files.append(buf.getvalue())
    parsed = [jpeg.parse_file(f) for f in files]
    scans = [f[p.scan_offset:p.scan_offset + p.scan_bytes] for f, p in zip(files, parsed)]
    p = parsed[0]
    for n in a.n:
        pick = [i % 16 for i in range(n)]
        off = np.cumsum([0] + [len(scans[i]) for i in pick])
        blob = b"".join(scans[i] for i in pick) + bytes(jpeg.SCAN_PADDING)
        dev = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)
        nb = np.array([len(scans[i]) for i in pick])
        out = torch.empty((n, H, W), dtype=torch.int32, device=DEV)
        results = {}
        for entropy in _entropies(a):
            kw = dict(out=out) if entropy == "image" else dict(out=out, entropy=entropy)
            whole, ent, inv = _time_stages(ras, (dev, off[:-1], nb, H, W, p.qtab, p.huffman), kw, a.reps)
            results[entropy] = out.clone()
            _report(f"jpeg_decode(entropy={entropy!r}) of {n} tiles of 501 x 501 ({len(blob) / n / 1024:.1f} KB of scan each)", whole, ent, inv, n)
        if len(results) == 2:
            print(f"    the two routes' images: {'bit-identical' if torch.equal(results['image'], results['lanes']) else 'DIFFERENT'}")


def bench_panos(a) -> None:
    from PIL import Image

    from salve_amd import ingest, synthetic
    from salve_amd.utils import image_io

    n = a.panos
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        (root / "zind" / "0003" / "panos").mkdir(parents=True)
        fpaths = {}
        for i in range(n):
            rgb, depth = synthetic.make_pano(i)
            fp = root / "zind" / "0003" / "panos" / f"floor_01_partial_room_{i:02d}_pano_{i}.jpg"
            image_io.write_jpeg(str(fp), np.repeat(np.repeat(rgb, 2, axis=0), 2, axis=1))
            image_io.write_depth_png(str(root / "depth" / "0003" / f"{fp.stem}.depth.png"), depth)
            fpaths[i] = str(fp)
        files = [Path(fpaths[i]).read_bytes() for i in range(n)]
        parsed = [jpeg.parse_file(f) for f in files]
        p = parsed[0]
        assert len({q.header_key for q in parsed}) == 1 and (p.h, p.w) == (1024, 2048)
        nb = np.array([q.scan_bytes for q in parsed])
        off = np.cumsum(np.r_[0, nb])
        blob = b"".join(f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)) + bytes(jpeg.SCAN_PADDING)
        print(f"{n} panoramas of 2048 x 1024, {nb.mean() / 1024:.0f} KB of scan each ({nb.min() / 1024:.0f} .. {nb.max() / 1024:.0f}); subsequence: "
              f"{_lib.load().salve_bev_jpeg_subseq_bytes()} bytes")
        ras = BevRasteriser(DEV)
        dev = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)
        out = torch.empty((n, p.h, p.w), dtype=torch.int32, device=DEV)
        results = {}
        for entropy in _entropies(a):
            kw = dict(out=out) if entropy == "image" else dict(out=out, entropy=entropy)
            whole, ent, inv = _time_stages(ras, (dev, off[:-1], nb, p.h, p.w, p.qtab, p.huffman), kw, a.reps)
            results[entropy] = out.clone()
            _report(f"jpeg_decode(entropy={entropy!r}) of the {n} panoramas", whole, ent, inv, n)
        if len(results) == 2:
            print(f"    the two routes' images: {'bit-identical' if torch.equal(results['image'], results['lanes']) else 'DIFFERENT'}")
        del out, results
        ms = []
        for _ in range(max(2, a.reps // 2)):
            t = time.perf_counter()
            for i in range(n):
                image_io.read_rgb(fpaths[i])
            ms.append((time.perf_counter() - t) * 1e3)
        print(f"Pillow decoding the {n} files, one after the other (host clock): {statistics.median(ms):.1f} ms ({min(ms):.1f} .. {max(ms):.1f}); "
              f"{statistics.median(ms) / n:.1f} ms per panorama")
        stores = {}
        for decode in ("host", "device"):
            ms = []
            for r in range(a.reps + 1):   # (the first call warms up: code objects, the workspace)
                torch.cuda.synchronize()
                t = time.perf_counter()
                stores[decode] = ingest.PanoStore(DEV).load(fpaths, str(root / "depth"), "0003", list(range(n)), decode=decode)
                torch.cuda.synchronize()
                if r:
                    ms.append((time.perf_counter() - t) * 1e3)
            print(f"PanoStore.load(decode={decode!r}) of the {n} panoramas, end to end (host clock): {statistics.median(ms):.1f} ms ({min(ms):.1f} .. {max(ms):.1f})")
        same = torch.equal(stores["host"].rgb, stores["device"].rgb) and torch.equal(stores["host"].depth, stores["device"].depth)
        print(f"    the two stores: {'bit-identical' if same else 'DIFFERENT'}; files Pillow decoded in the device route: {stores['device'].host_decoded}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--examples", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-batches", type=int, default=2)
    ap.add_argument("--device-batches", type=int, default=6)
    ap.add_argument("--keep", default=None, help="write the data set here and keep it (reused if it exists)")
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--n", type=lambda v: [int(x) for x in v.split(",")], default=[1024], help="--decode-only: tiles per call; several sizes separated by commas")
    ap.add_argument("--entropy", choices=("image", "lanes", "both"), default="image")
    ap.add_argument("--panos", type=int, default=0, help="time this many 2048 x 1024 panoramas instead of tiles")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tile_files needs the MI355X: there is nothing to time without it")
    if a.entropy == "both" and not (a.decode_only or a.panos):
        raise SystemExit("--entropy both compares the two stages on the same data: with --decode-only or --panos")
    bench_panos(a) if a.panos else bench_decode(a) if a.decode_only else bench_feed(a)
