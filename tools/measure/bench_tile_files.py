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
    python tools/measure/bench_tile_files.py --read-ahead [--examples 2048] [--reps 3] [--write-workers 16]   # the pipelined feed

--entropy image (default) is salve_bev_jpeg_decode's one wavefront per tile, lanes the lane-parallel stage (salve_bev_jpeg_decode_lanes);
the feed benchmark takes one of them, --decode-only and --panos also `both` (the same data through one, then the other).
--panos N writes N synthetic panoramas (synthetic.make_pano doubled to 2048 x 1024, the ingest tests' files) and times, on the same
files: the two entropy stages alone by events; Pillow decoding the files in the host route's loop by the host clock; and
ingest.PanoStore.load end to end, decode="host" against decode="device", by the host clock around a call that ends in a synchronise.

--decode-only times the whole call and, in the same run, its two stages apart.  (The inverse stage's two launches, jpeg_idct_kernel and
jpeg_pixels_kernel, can be told apart by `rocprofv3 --kernel-trace --stats -- python tools/measure/bench_tile_files.py --decode-only
--reps 2`, a run of its own.)  Calling the stages apart needs the coefficients to stay in the stream's JPEG workspace, which the
rasteriser's three JPEG methods share: nothing here calls one of them between an entropy stage and its inverse stage.
--read-ahead times the feed THROUGH a training step that consumes it (ResNet-152, ceiling + floor, batch 256, bf16, HIP norm, optimiser
and head): the host clock per batch from one device synchronise behind a step to the next, over epochs of at least eight batches, the
median of an epoch's batches after its first two.  Four feeds, both entropy stages, alternating within each repeat: the serial feed with
the full marker walk per file (what a checkout from before HeaderCache and read_ahead does: the baseline), the serial feed, the
pipelined feed (read_ahead=True), and the same step on one resident batch (no feed: the floor).  Beside them the epoch's wall time with
no synchronise between batches (the way `training.run_epoch` drives a HIP head), and the parse thread-seconds per batch with and without
HeaderCache.  The pipelined feed counts as faster only if its median lies below the baseline's by more than the spread of the baseline's
repeats; the verdict line says which.  The first epoch of every feed warms up (pinned buffers, workspaces, code objects) and carries the
check that the pipelined batches are the serial ones.
Medians (min .. max); run the command twice for the spread.
"""

from __future__ import annotations

import argparse
import concurrent.futures
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


def _write_example(root: Path, i: int) -> None:
    from PIL import Image

    label = "gt_alignment_approx" if i % 2 == 0 else "incorrect_alignment"
    d = root / label / "1208"
    d.mkdir(parents=True, exist_ok=True)
    for s, surface in enumerate(("ceiling", "floor")):
        for k, (room, pano) in enumerate(((4, 5), (7, 8))):
            kind = "layout" if (surface == "floor" and i % 2) else "disc"
            name = f"pair_{i}___door_0_0_rotated_{surface}_rgb_floor_01_partial_room_{room:02d}_pano_{pano}.jpg"
            Image.fromarray(_tile(kind, 4 * i + 2 * s + k)).save(d / name, quality=75)


def _write_examples(root: Path, lo: int, hi: int) -> None:
    for i in range(lo, hi):
        _write_example(root, i)


def write_dataset(root: Path, examples: int, workers: int = 1) -> None:
    """`examples` pairs of building 1208 (train split), alternating positive / negative; ceiling tiles are discs, floor tiles
    alternate disc / layout.  workers > 1: that many processes write a share each (they never touch the device)."""
    if workers <= 1:
        return _write_examples(root, 0, examples)
    import multiprocessing

    share = -(-examples // (4 * workers))
    with concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn")) as pool:
        list(pool.map(_write_examples, *zip(*[(root, lo, min(lo + share, examples)) for lo in range(0, examples, share)])))


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
            write_dataset(root, a.examples, a.write_workers)
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


class FeedSource(TileFileSource):
    """TileFileSource whose reader threads clock their two halves per file; `parse_s` / `read_s`: thread-seconds summed per batch.
    cache=False parses every file with the full marker walk (jpeg.parse_file), as the source did before HeaderCache."""

    def __init__(self, *a, cache=True, **kw):
        super().__init__(*a, **kw)
        self.cache, self.parse_s, self.read_s = cache, [], []

    def _read_one(self, path):
        t0 = time.perf_counter()
        with open(path, "rb") as f:
            data = f.read()
        t1 = time.perf_counter()
        try:
            parsed = self.headers.parse(data) if self.cache else jpeg.parse_file(data, restart=self.entropy == "lanes")
        except jpeg.Unsupported:
            parsed = None
        return data, parsed, t1 - t0, time.perf_counter() - t1

    def _read(self, paths):   # (one batch at a time, in the iterating thread or in the one thread that packs)
        out = super()._read(paths)
        self.read_s.append(sum(r[2] for r in out))
        self.parse_s.append(sum(r[3] for r in out))
        return [r[:2] for r in out]


def bench_read_ahead(a) -> None:
    from salve_amd.evaluate import DeviceClassMeter

    keep = Path(a.keep) if a.keep else None
    with tempfile.TemporaryDirectory() as tmp:
        root = keep or Path(tmp) / "bev"
        if not (root / "gt_alignment_approx").exists():
            t = time.perf_counter()
            write_dataset(root, a.examples, a.write_workers)
            print(f"wrote {4 * a.examples} tiles in {time.perf_counter() - t:.1f} s ({a.write_workers} process(es))")
        args = config(root, a.batch)
        sizes = [p.stat().st_size for p in root.rglob("*.jpg")]
        data = ZindData(split="train", transform=None, args=args)
        per_epoch = len(data.data_list) // a.batch
        print(f"{len(sizes)} files, {np.mean(sizes) / 1024:.1f} KB on average ({min(sizes) / 1024:.1f} .. {max(sizes) / 1024:.1f}); batch {a.batch} = "
              f"{4 * a.batch} tiles, {per_epoch} batches per epoch")
        if per_epoch < 8:
            raise SystemExit(f"--read-ahead wants at least eight batches per epoch for a steady state: --examples {8 * a.batch} or more")
        torch.manual_seed(0)
        model = training.get_model(args, "bf16", "hip", "hip").train()
        optimizer = training.get_optimizer(args, model, "hip")
        meter = DeviceClassMeter(args.num_ce_classes, DEV)

        def step(x, y):
            _, loss = training.cross_entropy_forward_packed(model, "train", x, y, meters=meter, accumulate_loss=True)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()

        def epoch(batches, synchronise=True):
            """Host ms per batch, from the synchronise behind one step to the one behind the next -- or, free-running, the epoch's ms
            per batch with one synchronise at its end -- and a checksum of the batches' bits."""
            ms, sums = [], []
            torch.cuda.synchronize()
            start = t = time.perf_counter()
            for x, y in batches:
                sums.append(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).sum(dtype=torch.int64))
                step(x, y)
                if synchronise:
                    torch.cuda.synchronize()
                    now = time.perf_counter()
                    ms.append((now - t) * 1e3)
                    t = now
            torch.cuda.synchronize()
            if not synchronise:
                ms = [(time.perf_counter() - start) * 1e3 / max(1, len(sums))]
            return ms, [int(s) for s in sums]

        steady = lambda ms: ms[2:]
        for entropy in ("image", "lanes"):
            kw = dict(batch_size=a.batch, precision="bf16", split="train", seed=0, entropy=entropy)
            feeds = {"serial, full marker walk (baseline)": FeedSource(DEV, data.data_list, cache=False, **kw),
                     "serial": FeedSource(DEV, data.data_list, **kw),
                     "read_ahead": FeedSource(DEV, data.data_list, read_ahead=True, **kw)}
            print(f"---- entropy={entropy}")
            first = {}
            for name, src in feeds.items():   # warm-up epoch: pinned buffers, workspaces, code objects; the same seeds, so the same batches
                random.seed(0)
                _, first[name] = epoch(src)
                src.parse_s, src.read_s = [], []
            same = first["read_ahead"] == first["serial"] == first["serial, full marker walk (baseline)"]
            print(f"first epoch, the three feeds' batches by checksum: {'bit-identical' if same else 'DIFFERENT'}")
            if not same:
                raise SystemExit(1)
            resident = feeds["serial"].batch(np.arange(a.batch), feeds["serial"].draws(a.batch))
            feeds["serial"]._check_epoch("bench_tile_files")
            feeds["serial"].parse_s, feeds["serial"].read_s = [], []
            medians = {name: [] for name in list(feeds) + ["resident batch (no feed)"]}
            free = {name: [] for name in feeds}
            for r in range(a.reps):
                for name, src in feeds.items():   # alternating: one epoch of each feed per repeat
                    ms, _ = epoch(src)
                    medians[name].append(statistics.median(steady(ms)))
                    print(f"  repeat {r}  {name:<38} {_stat(steady(ms))}")
                ms, _ = epoch([resident] * per_epoch)
                medians["resident batch (no feed)"].append(statistics.median(steady(ms)))
                print(f"  repeat {r}  {'resident batch (no feed)':<38} {_stat(steady(ms))}")
                for name, src in feeds.items():
                    free[name].append(epoch(src, synchronise=False)[0][0])
            for name, m in medians.items():
                print(f"{name:<40} median of {len(m)} repeats' medians {statistics.median(m):8.2f} ms per batch  ({min(m):.2f} .. {max(m):.2f})")
            for name, m in free.items():
                print(f"{name:<40} free-running epoch {statistics.median(m):8.2f} ms per batch  ({min(m):.2f} .. {max(m):.2f})")
            for name, src in feeds.items():
                print(f"{name:<40} parse, thread-seconds per batch {_stat([v * 1e3 for v in src.parse_s])};  read {_stat([v * 1e3 for v in src.read_s])}")
            base = medians["serial, full marker walk (baseline)"]
            gain, spread = statistics.median(base) - statistics.median(medians["read_ahead"]), max(base) - min(base)
            print(f"verdict, entropy={entropy}: read_ahead is {gain:.2f} ms per batch below the baseline, whose repeats spread over {spread:.2f} ms: "
                  f"{'FASTER' if gain > spread else 'NOT FASTER'}")
            for src in feeds.values():
                src.close()


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
    ap.add_argument("--read-ahead", action="store_true", help="time the serial and the pipelined feed through a ResNet-152 training step")
    ap.add_argument("--write-workers", type=int, default=1, help="processes that write the data set")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tile_files needs the MI355X: there is nothing to time without it")
    if a.entropy == "both" and not (a.decode_only or a.panos):
        raise SystemExit("--entropy both compares the two stages on the same data: with --decode-only or --panos")
    if a.read_ahead and a.examples < 8 * a.batch:
        a.examples = 8 * a.batch   # r10's workload, enlarged to eight batches per epoch
    bench_read_ahead(a) if a.read_ahead else bench_panos(a) if a.panos else bench_decode(a) if a.decode_only else bench_feed(a)
