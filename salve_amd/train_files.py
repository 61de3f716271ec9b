"""Batches straight from the rendered tile data set on disk, decoded on the device (opt-in: training.train(decode="device"),
`python -m salve_amd.train --decode device`, train_utils.get_dataloader(decode="device")).

The reference trains and evaluates from 501 x 501 JPEG tiles on disk and decodes each with Pillow in its DataLoader
(zind_data.py:306-315); so does `salve_amd.dataset.zind_data.ZindData`, one file, one upload and one tile launch per example at a
time.  Here a batch is: a bounded thread pool reads the batch's files and parses their headers (salve_amd.jpeg.HeaderCache: the
marker walk once per distinct header, the per-file checks on every file); the
entropy-coded scans go into ONE pinned buffer and up in ONE copy; `BevRasteriser.jpeg_decode` decodes them, one call per group of
files that share size and tables (in a data set written by one program: one call); ONE tile launch makes the batch.
The grouping and ordering of the examples stay `ZindData`'s: both classes are built from its `data_list`.

  TileFileSource   the iteration contract of train_render.RenderedTrainSource: `(x_packed, is_match)` for `training.run_epoch`.
                   train: a seeded shuffle (the DataLoader's own order for that seed), the last partial batch dropped, one
                   `TrainTransform.draw()` per example in the reference's order; val / test: in order, centre crop, nothing dropped.
  TileFileLoader   the evaluation DataLoader's tuples `(x1, x2[, x3, x4[, x5, x6]], is_match, fp0, fp1)`: float32 NCHW tiles from
                   one salve_bev_tiles launch per batch, for `evaluate.run_test_epoch`.

`entropy="lanes"` (both classes) takes the lane-parallel entropy stage (salve_bev_jpeg_decode_lanes): the same
batches bit for bit, and files with restart intervals stay on the device.
A file the device does not decode (`parse_file` raises Unsupported: progressive, restart markers unless entropy="lanes", other
subsamplings, greyscale ...) is decoded by Pillow and uploaded into its image slot with the same copy.  Every tile of a data set has one size (the first file's);
a file of another size raises, naming it.  The decoder's per-image status is read ONCE per epoch, after the last batch; a non-zero
entry raises, naming the file.  `close()` (or a `with` block) ends the reader threads; `training.train` and `evaluate_model` call it.

`read_ahead=True` (both classes; opt-in) turns iteration into a pipeline over the epoch's plan -- the same batches bit
for bit, the same `fallbacks` at the end of the epoch, the same errors at the same batch:

  stage R  host threads: batches k + 1 and k + 2 are read, parsed and packed into a ring of three pinned buffers while batch k
           trains (the reader pool, plus one thread that packs; Pillow's files are decoded here).  No device call.
  stage D  the iterating thread, on ONE side stream the source owns: batch k + 1's upload and decode calls are issued when batch
           k is asked for, an event behind them.
  stage T  the iterating thread, current stream: waits for batch k's event, takes the draws, ONE tile launch, yields.

ONE more batch of decoded images and ONE more decode workspace than without it live on the device (at 1024 tiles of 501 x 501 about
1 GB + 1.2 GB), and three pinned buffers instead of one on the host.  `batch(idx, draws)` stays serial.  An iteration that ends early
-- an error, a closed generator -- leaves the source clean: the reads in flight are cancelled or awaited, the side stream is
synchronised, the status of the batches it did yield is dropped, and the next iteration starts from the plan's first batch.
"""

from __future__ import annotations

import concurrent.futures
import contextlib
import threading
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, jpeg, status, tracing, train_feed
from salve_amd.common.bevparams import BEVParams
from salve_amd.rasteriser import BevRasteriser
from salve_amd.train_feed import batches_per_epoch, plan_epoch
from salve_amd.transforms import TrainTransform
from salve_amd.utils import image_io

MAX_READ_THREADS = 16
SPLITS = ("train", "val", "test")
ENTROPY_STAGES = ("image", "lanes")   # BevRasteriser.jpeg_decode(entropy=)
RING_SLOTS = 3                        # read_ahead: the batch being uploaded and the two that stage R works on


class _Slot:
    """One pinned staging buffer and the event behind the last copy that read it."""

    def __init__(self) -> None:
        self.pinned: Optional[torch.Tensor] = None
        self.copied: Optional[torch.cuda.Event] = None

    def fits(self, nbytes: int) -> bool:
        return self.pinned is not None and self.pinned.numel() >= nbytes

    def grow(self, nbytes: int) -> None:
        if not self.fits(nbytes):
            self.pinned = torch.empty(max(nbytes, 2 * (self.pinned.numel() if self.pinned is not None else 0)), dtype=torch.uint8).pin_memory()

    def wait(self) -> None:
        if self.copied is not None:
            self.copied.synchronize()   # the last copy has read the buffer


@dataclass
class _Batch:
    """One batch's files as `_layout` places them in a pinned buffer."""
    n: int
    position: np.ndarray                      # image slot of each path
    offsets: np.ndarray                       # [:decoded]: each decoded image's scan in the buffer
    lengths: np.ndarray
    groups: list = field(default_factory=list)   # (images, qtab, huffman, segment rows or None) per decode call, in slot order
    names: list = field(default_factory=list)    # path by image slot
    decoded: int = 0                          # images the device decodes; the host route's follow them
    host_route: int = 0
    scans_end: int = 0                        # the scans and their padding
    pixels_at: int = 0                        # the host route's pixels
    total: int = 0
    slot: Optional[_Slot] = None              # the pinned buffer that holds it
    status: Optional[torch.Tensor] = None     # the decoder's per-image status, once `_decode` has been issued


@dataclass
class _Ahead:
    """One batch of a read_ahead iteration on its way through the stages."""
    slot: _Slot
    entered: threading.Event = field(default_factory=threading.Event)   # stage R has begun to read it
    future: Optional[concurrent.futures.Future] = None                  # stage R: (_Batch, fill or None)
    batch: Optional[_Batch] = None                                      # stage D: issued on the side stream ...
    images: Optional[torch.Tensor] = None
    ready: Optional[torch.cuda.Event] = None                            # ... with this event behind it


class _TileFiles:
    """What the two batch sources share: the files of a batch -> int32 [n, H, W] images on the device."""

    def __init__(self, device, data_list: Sequence[tuple], resize_hw: Tuple[int, int], crop_hw: Tuple[int, int], read_threads: int,
                 entropy: str = "image", read_ahead: bool = False, photometric: Optional[str] = None, rank: int = 0, world: int = 1) -> None:
        train_feed.check_photometric(photometric)
        train_feed.shard_bounds(0, rank, world)   # (refuses a rank outside its world)
        self.rank, self.world = int(rank), int(world)
        if not 1 <= int(read_threads) <= MAX_READ_THREADS:
            raise ValueError(f"read_threads must be 1 .. {MAX_READ_THREADS}, got {read_threads}")
        if entropy not in ENTROPY_STAGES:
            raise ValueError(f"entropy must be one of {ENTROPY_STAGES}, got {entropy!r}")
        self.entropy = entropy                          # "lanes": salve_bev_jpeg_decode_lanes, which also takes files with restart intervals
        self.read_ahead = bool(read_ahead)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SalveHipError("decode=\"device\" needs a HIP device ('cuda:N'); there is no CPU path")
        self.data_list = list(data_list)
        widths = {len(e) for e in self.data_list}
        if len(widths) > 1 or (widths and next(iter(widths)) not in (3, 5, 7)):
            raise RuntimeError(f"examples are (2, 4 or 6 tile paths, is_match) tuples of one length, got lengths {sorted(widths)}")
        self.images_per_example = (next(iter(widths)) - 1) if widths else 2
        self.photometric = photometric   # (a source that yields train batches jitters them; the others only accept the keyword)
        # the draws (and the square / no-padding refusals); its kernels are not used
        self.tf = TrainTransform(resize_hw, crop_hw, jitter_types=train_feed.JITTER_TYPES if photometric else None)
        self.read_threads = int(read_threads)
        self.ras: Optional[BevRasteriser] = None       # made with the first batch: its image size is the first file's
        self.fallbacks = 0                              # files decoded by Pillow so far
        self.headers = jpeg.HeaderCache(restart=entropy == "lanes")   # one per source: the options are the source's
        self._pool: Optional[concurrent.futures.ThreadPoolExecutor] = None
        self._slot = _Slot()                            # the serial path's pinned buffer
        self._epoch_status: List[Tuple[torch.Tensor, List[str]]] = []
        # read_ahead: the ring, the thread that packs, the side stream, and the batches of the running iteration by number
        self._ring = [_Slot() for _ in range(RING_SLOTS)] if self.read_ahead else []
        self._ring_bytes = 0
        self._packer: Optional[concurrent.futures.ThreadPoolExecutor] = None
        self._side: Optional[torch.cuda.Stream] = None
        self._ahead: Dict[int, _Ahead] = {}
        self._in_stage_r = threading.local()
        # (a bit an earlier, unchecked caller left in the device's status word is reported as ITS failure, not as this source's)
        status.check(self.device, "a launch issued before this tile file source was created")

    def close(self) -> None:
        """Ends the threads the source started (they start with the first batch); with read_ahead, what an unfinished iteration
        left in flight is cancelled or awaited first.  The object stays usable: the next batch starts new threads."""
        self._drain()
        if self._packer is not None:
            self._packer.shutdown(wait=True)
            self._packer = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # ------------------------------------------------------------------ one batch's images, step by step
    # (tools/measure/bench_tile_files.py times the steps by overriding them: nothing here knows about clocks)
    def _read(self, paths: List[str]) -> list:
        """[(file bytes, ParsedFile or None)] of the batch's files, by the thread pool."""
        entered = getattr(self._in_stage_r, "entered", None)
        if entered is not None:
            entered.set()
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.read_threads, thread_name_prefix="salve-tile-files")
        return list(self._pool.map(self._read_one, paths))

    def _read_one(self, path: str):
        with open(path, "rb") as f:
            data = f.read()
        try:
            return data, self.headers.parse(data)
        except jpeg.Unsupported:
            return data, None

    def _rasteriser(self, path: str, parsed) -> None:
        """Makes the rasteriser with the first file there is: the data set's image size is that file's."""
        if self.ras is None:
            h, w = (parsed.h, parsed.w) if parsed is not None else image_io.read_rgb(path).shape[:2]
            self.ras = BevRasteriser(self.device, bev_params=BEVParams(img_h=h - 1, img_w=w - 1), resize=self.tf.resize, crop=self.tf.crop)

    def _layout(self, paths: List[str], read: list) -> Tuple["_Batch", Callable[[np.ndarray], None]]:
        """Groups the files by `header_key` and lays the batch out: the groups' scans one behind the other, the padding, then (4-byte
        aligned) the pixels of the files that take the host route, which Pillow decodes here.  -> (the layout, `fill(host)` that
        writes those `total` bytes into a buffer).  Host work only: the rasteriser exists by now."""
        H, W = self.ras.bev_hw
        groups: Dict[bytes, List[int]] = {}
        host_route: List[int] = []
        for i, (_, parsed) in enumerate(read):
            if parsed is None:
                host_route.append(i)
            elif (parsed.h, parsed.w) != (H, W):
                raise RuntimeError(f"{paths[i]} is {parsed.h} x {parsed.w}; the tiles of this data set are {H} x {W}")
            else:
                groups.setdefault(parsed.header_key, []).append(i)
        n = len(paths)
        b = _Batch(n=n, position=np.empty(n, dtype=np.int64), offsets=np.zeros(n, dtype=np.int64), lengths=np.zeros(n, dtype=np.int64))
        at = k = 0
        order: List[int] = []
        for members in groups.values():
            rows = None
            if self.entropy == "lanes":   # the restart intervals (one per file without markers), where `at` will put them
                rows, to = [], at
                for j, i in enumerate(members):
                    parsed = read[i][1]
                    rows += [(to + off - parsed.scan_offset, nbytes, j, first, count) for off, nbytes, first, count in parsed.segments]
                    to += parsed.scan_bytes
            b.groups.append((len(members), read[members[0]][1].qtab, read[members[0]][1].huffman, rows))
            for i in members:
                b.position[i], b.offsets[k], b.lengths[k] = k, at, read[i][1].scan_bytes
                at += read[i][1].scan_bytes
                order.append(i)
                k += 1
        b.decoded, b.host_route = k, len(host_route)
        b.scans_end = at + jpeg.SCAN_PADDING
        b.pixels_at = (b.scans_end + 3) // 4 * 4
        b.total = b.pixels_at + len(host_route) * H * W * 4
        pixels = []
        for j, i in enumerate(host_route):
            rgb = image_io.read_rgb(paths[i])
            if rgb.shape[:2] != (H, W):
                raise RuntimeError(f"{paths[i]} is {rgb.shape[0]} x {rgb.shape[1]}; the tiles of this data set are {H} x {W}")
            p = rgb.astype(np.uint32)
            pixels.append((p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)).view(np.uint8).reshape(-1))
            b.position[i] = k + j
        b.names = [""] * n
        for i in range(n):
            b.names[int(b.position[i])] = paths[i]

        def fill(host: np.ndarray) -> None:
            for j, i in enumerate(order):
                data, parsed = read[i]
                host[b.offsets[j]:b.offsets[j] + b.lengths[j]] = np.frombuffer(data, dtype=np.uint8, count=parsed.scan_bytes, offset=parsed.scan_offset)
            host[at:b.pixels_at] = 0
            for j, p in enumerate(pixels):
                host[b.pixels_at + j * H * W * 4:b.pixels_at + (j + 1) * H * W * 4] = p

        return b, fill

    def _pack(self, paths: List[str], read: list) -> "_Batch":
        """The serial path: `_layout`, then the pinned buffer filled once the last batch's copy has read it."""
        self._rasteriser(paths[0], read[0][1])
        b, fill = self._layout(paths, read)
        b.slot = self._slot
        b.slot.wait()
        b.slot.grow(b.total)
        fill(b.slot.pinned.numpy())
        self.fallbacks += b.host_route
        return b

    def _upload(self, b: "_Batch") -> torch.Tensor:
        """The `total` bytes of the batch's pinned buffer to the device, ONE copy, on the current stream."""
        with tracing.range("salve.tile_files_upload"):
            dev = torch.empty(b.total, dtype=torch.uint8, device=self.device)
            dev.copy_(b.slot.pinned[:b.total], non_blocking=True)
            b.slot.copied = torch.cuda.Event()
            b.slot.copied.record()
        return dev

    def _decode_group(self, *args, **kw) -> torch.Tensor:
        """One `BevRasteriser.jpeg_decode` call (a group of files that share size and tables) -> its status."""
        return self.ras.jpeg_decode(*args, **kw)[1]

    def _decode(self, b: "_Batch", dev: torch.Tensor) -> torch.Tensor:
        """int32 [n, H, W] images: one decode call per group, then the host route's pixels copied into their slots; the per-image
        status goes into `b.status`.  On the current stream."""
        H, W = self.ras.bev_hw
        images = torch.empty((b.n, H, W), dtype=torch.int32, device=self.device)
        image_status = torch.zeros(b.n, dtype=torch.int32, device=self.device)
        with tracing.range("salve.jpeg_decode"):
            lo = 0
            for m, qtab, huffman, rows in b.groups:
                kw = {} if self.entropy == "image" else dict(entropy=self.entropy, segments=rows)
                image_status[lo:lo + m] = self._decode_group(dev[:b.scans_end], b.offsets[lo:lo + m], b.lengths[lo:lo + m], H, W, qtab, huffman,
                                                             out=images[lo:lo + m], **kw)
                lo += m
        if b.host_route:
            images[b.decoded:] = dev[b.pixels_at:].view(torch.int32).view(b.host_route, H, W)
        b.status = image_status
        return images

    def _load(self, paths: List[str]) -> Tuple[torch.Tensor, np.ndarray]:
        """The files `paths` -> (int32 [n, H, W] images on the device, position [n] of each path's image in that array)."""
        b = self._pack(paths, self._read(paths))
        images = self._decode(b, self._upload(b))
        self._epoch_status.append((b.status, b.names))
        return images, b.position

    def _check_epoch(self, what: str) -> None:
        """The decoder's per-image status of every batch since the last check, read once; then the device status word."""
        kept, self._epoch_status = self._epoch_status, []
        if kept:
            words = torch.cat([s for s, _ in kept]).cpu().numpy()
            bad = np.flatnonzero(words)
            if bad.size:
                names = [n for _, ns in kept for n in ns]
                lines = [f"{names[i]}: {jpeg.describe_status(int(words[i]))}" for i in bad[:8]]
                raise RuntimeError(f"{what}: {bad.size} malformed JPEG file(s) -- " + " | ".join(lines))
        status.check(self.device, what)

    def _paths(self, idx: np.ndarray) -> List[str]:
        return [p for i in idx for p in self.data_list[int(i)][:-1]]

    # ------------------------------------------------------------------ an epoch's batches, one behind the other or pipelined
    def _batches(self, plan: Sequence[np.ndarray]):
        """(idx, images, position) for each batch of the plan; `contextlib.closing` around it ends a pipelined iteration with its caller's."""
        if self.read_ahead:
            return self._batches_ahead(list(plan))
        return ((idx, *self._load(self._paths(idx))) for idx in plan)

    def _stage_r(self, paths: List[str], item: "_Ahead"):
        """Stage R, in the packing thread: read, parse, lay out, and fill the slot if it is large enough (growing it pins memory, a
        call into the runtime, which is the iterating thread's to make: `fill` goes back to it then).  No device call."""
        self._in_stage_r.entered = item.entered
        try:
            b, fill = self._layout(paths, self._read(paths))
            b.slot = item.slot
            if b.slot.fits(b.total):
                fill(b.slot.pinned.numpy())
                fill = None
            return b, fill
        finally:
            self._in_stage_r.entered = None
            item.entered.set()   # (an error in front of the read: nobody waits for it in vain)

    def _submit(self, plan: List[np.ndarray], j: int) -> None:
        """Hands batch j to stage R.  Its slot is free: the copy that last read it (batch j - 3's) has completed, awaited here."""
        if j >= len(plan):
            return
        slot = self._ring[j % RING_SLOTS]
        slot.wait()
        if self._ring_bytes:
            slot.grow(self._ring_bytes)   # (what a sibling needed: so that only an epoch's first batches are filled by the iterating thread)
        item = self._ahead[j] = _Ahead(slot)
        item.future = self._packer.submit(self._stage_r, self._paths(plan[j]), item)

    def _stage_d(self, item: "_Ahead") -> None:
        """Stage D, iterating thread: awaits the batch's pack (raising stage R's error), then issues its upload and its decode calls
        on the side stream with an event behind them."""
        b, fill = item.future.result()
        if fill is not None:
            self._ring_bytes = max(self._ring_bytes, b.total + b.total // 8)
            b.slot.grow(self._ring_bytes)
            fill(b.slot.pinned.numpy())
        with torch.cuda.stream(self._side):
            item.images = self._decode(b, self._upload(b))
            item.ready = torch.cuda.Event()
            item.ready.record()
        item.batch = b

    def _drain(self, unfinished: bool = False) -> None:
        """Leaves nothing of an unfinished read_ahead iteration behind: stage R's queued batches are cancelled and the running one
        awaited (its error, if any, dies with it), the side stream is synchronised, the status of the batches the iteration yielded is
        dropped.  Nothing to do where no iteration is under way."""
        if not (unfinished or self._ahead):
            return
        for item in self._ahead.values():
            if item.future is not None and not item.future.cancel():
                concurrent.futures.wait([item.future])
        self._ahead = {}
        if self._side is not None:
            self._side.synchronize()
        self._epoch_status = []

    def _batches_ahead(self, plan: List[np.ndarray]):
        self._drain()   # (an earlier iteration whose generator is still around)
        if not plan:
            return
        current = torch.cuda.current_stream(self.device)
        if self.ras is None:   # the image size is the first file's; stage R makes no device call, so the rasteriser is made here
            first = self._paths(plan[0])[0]
            self._rasteriser(first, self._read_one(first)[1])
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        if self._packer is None:
            self._packer = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="salve-tile-files-pack")
        self._side.wait_stream(current)   # the rasteriser's tables, and whatever this thread issued before, come first
        whole = False
        try:
            for j in range(RING_SLOTS):
                self._submit(plan, j)
            self._stage_d(self._ahead[0])
            for k, idx in enumerate(plan):
                if k:
                    self._submit(plan, k + 2)
                failed = None
                if k + 1 < len(plan):
                    try:
                        self._stage_d(self._ahead[k + 1])
                    except Exception as e:   # batch k + 1's: raised when that batch is asked for, behind batch k
                        failed = e
                item = self._ahead.pop(k)
                b, images = item.batch, item.images
                current.wait_event(item.ready)
                images.record_stream(current)      # made on the side stream, read by the tile launch and whatever follows it here
                b.status.record_stream(current)    # ... and by `_check_epoch`'s read-back
                self._epoch_status.append((b.status, b.names))
                self.fallbacks += b.host_route
                if k + 2 in self._ahead:
                    self._ahead[k + 2].entered.wait()   # stage R is two batches ahead by the time this one is handed out
                yield idx, images, b.position
                if failed is not None:
                    raise failed
            whole = True
        finally:
            if not whole:
                self._drain(unfinished=True)


class TileFileSource(_TileFiles):
    """Iterating yields `(x_packed, is_match)`: x_packed [B, crop, crop, Cp] float32 / bfloat16 on the device (the trainable model's
    packed input, `forward_packed`: the example's images in the order of its tuple, three channels each, zero-padded to a multiple of
    8), is_match int64 [B, 1].  One epoch per iteration; `len()` = batches per epoch.  Everything runs on the current stream.
    data_list: `ZindData(...).data_list`.
    read_ahead=True: the next two batches' files are read, and the next batch decoded on a side stream, while the current batch trains
    (the module's docstring): the same batches, one more batch of decoded images and one more decode workspace on the
    device (about 1 GB + 1.2 GB at 1024 tiles of 501 x 501).  The yielded tensors belong to the current stream as always.
    photometric: None (default), or "device": the train split's batches take the reference's PhotometricShift inside the train-tile call
    (RenderedTrainSource's keyword), read_ahead or not; every other split never jitters.
    rank, world (data-parallel training): RenderedTrainSource's keywords -- the whole epoch is planned and the whole
    batch's draws are taken, rows [lo, hi) of every batch are read, decoded and yielded; read_ahead reads this rank's files only."""

    def __init__(self, device, data_list: Sequence[tuple], batch_size: int = 256, precision: str = "fp32", split: str = "train", seed: int = 0,
                 resize_hw: Tuple[int, int] = (234, 234), crop_hw: Tuple[int, int] = (224, 224), read_threads: int = MAX_READ_THREADS,
                 entropy: str = "image", read_ahead: bool = False, photometric: Optional[str] = None, rank: int = 0, world: int = 1) -> None:
        train_feed.check_arguments(batch_size, split, SPLITS, precision)
        train_feed.check_shard(batch_size, split, rank, world)
        super().__init__(device, data_list, resize_hw, crop_hw, read_threads, entropy, read_ahead, photometric if split == "train" else None,
                         rank, world)
        self._rows: List[Tuple[int, int, int]] = []   # the running epoch: (rows of the whole batch, lo, hi) per batch of this rank
        self.split, self.batch_size = split, int(batch_size)
        self.dtype = torch.bfloat16 if precision == "bf16" else torch.float32
        self.per_sample = self.images_per_example // 2            # image PAIRS per example
        self.out_c = (3 * self.images_per_example + 7) // 8 * 8
        self.gen = torch.Generator()
        self.gen.manual_seed(seed)
        self.labels = np.array([int(e[-1]) for e in self.data_list], dtype=np.int64)

    def __len__(self) -> int:
        return batches_per_epoch(len(self.data_list), self.batch_size, "train" if self.split == "train" else "val")

    def draws(self, n: int) -> List[Tuple[int, int, bool, bool]]:
        """One draw per example of a batch (`train_feed.draws`)."""
        return train_feed.draws(self.tf, self.split, n)

    def jitter_draws(self, n: int) -> Optional[List[train_feed.JitterDraw]]:
        """The jitter draws of a batch of n examples (`train_feed.jitter_draws`), or None where the source does not jitter."""
        return train_feed.jitter_draws(self.tf, n, self.images_per_example) if self.photometric else None

    def _shard_draws(self, b: int):
        """(draws, jitter draws) of batch `b` of this rank's plan: the whole batch's are taken, this rank's rows are kept."""
        n, lo, hi = self._rows[b]
        return train_feed.shard_draws(self.draws(n), self.jitter_draws(n), self.images_per_example, lo, hi)

    def batch(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]],
              jitter: Optional[Sequence[train_feed.JitterDraw]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Examples `idx` with one draw (crop_y, crop_x, hflip, vflip) each: (x_packed, is_match).  Serial, whatever `read_ahead`.
        jitter (photometric="device"): one `TrainTransform.draw_jitter()` per image, example by example in the order of its tuple."""
        idx = np.asarray(idx, dtype=np.int64)
        if len(draws) != len(idx):
            raise ValueError(f"{len(idx)} examples, {len(draws)} draws")
        return self._tile(idx, draws, *self._load(self._paths(idx)), jitter=jitter)

    def tile_tables(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]], position: np.ndarray):
        """The host tables of one batch whose example b's images lie at `position[E b : E (b + 1)]` of the decoded array, in the order of
        its tuple: (tile jobs [2][B][K], draws [B]).  Host arithmetic only."""
        B, K = len(idx), self.per_sample
        if len(draws) != B:
            raise ValueError(f"{B} examples, {len(draws)} draws")
        H, W = self.ras.bev_hw
        pos = np.asarray(position).reshape(B, K, 2)
        jobs = np.zeros((2, B, K), dtype=_lib.TILE_JOB_DTYPE)   # [first | second image of a pair][sample][pair]
        jobs["bev_offset"][0], jobs["bev_offset"][1] = pos[:, :, 0] * (H * W), pos[:, :, 1] * (H * W)
        jobs["slot"][:] = np.arange(B, dtype=np.int64)[None, :, None]
        jobs["chan"][0] = 6 * np.arange(K)[None, :]
        jobs["chan"][1] = 6 * np.arange(K)[None, :] + 3
        return jobs, train_feed.aug_table(draws)

    def _tile(self, idx: np.ndarray, draws, images: torch.Tensor, position: np.ndarray, jitter=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The batch from its decoded images: the tables in ONE upload, ONE train-tile call, on the current stream."""
        B, K = len(idx), self.per_sample
        if jitter is not None and len(jitter) != 2 * K * B:
            raise ValueError(f"{B} examples of {2 * K} images, {len(jitter)} jitter draws")
        jobs, aug = self.tile_tables(idx, draws, position)
        buf, o = train_feed.upload_tables([jobs, aug, self.labels[idx], train_feed.jitter_table(jitter or [])], self.device)
        out = torch.empty((B, self.ras.crop, self.ras.crop, self.out_c), dtype=self.dtype, device=self.device)
        self._tile_launch(images, buf[:o[1] // 2], buf[o[1] // 2:o[1]], K, buf[o[1]:o[2]], B, out, None if jitter is None else buf[o[3]:o[4]])
        return out, buf[o[2]:o[3]].view(torch.int64).view(B, 1)

    def _tile_launch(self, images, jobs_a, jobs_b, per_sample, aug, batch, out, jitter=None) -> None:
        """ONE salve_bev_train_tiles (or, with jitter records, salve_bev_train_tiles_jitter) call: both arrays of image pairs are the
        decoded images."""
        with tracing.range("salve.train_tiles"):
            self.ras.train_tiles(images, images, jobs_a, jobs_b, per_sample, aug, batch, out, jitter=jitter)

    def __iter__(self):
        # the whole epoch is planned (the generator stands where the single process's stands), then cut to this rank's rows
        plan, self._rows = train_feed.shard_plan(plan_epoch(len(self.data_list), self.batch_size, "train" if self.split == "train" else "val", self.gen),
                                                 self.rank, self.world)
        if not self.read_ahead:
            for b, idx in enumerate(plan):
                yield self.batch(idx, *self._shard_draws(b))
        else:
            with contextlib.closing(self._batches(plan)) as batches:
                for b, (idx, images, position) in enumerate(batches):   # (the draws now: Python's `random` is consumed batch by batch, as above)
                    draws, jitter = self._shard_draws(b)
                    yield self._tile(np.asarray(idx, dtype=np.int64), draws, images, position, jitter)
        self._check_epoch(f"tile files, {self.split} batches")


class TileFileLoader(_TileFiles):
    """Iterating yields what the evaluation DataLoader over `ZindData` yields: `(x1, x2[, x3, x4[, x5, x6]], is_match, fp0, fp1)` --
    float32 [B, 3, crop, crop] tiles on the device (Resize -> centre Crop -> ToTensor -> Normalize, ONE salve_bev_tiles launch per
    batch), is_match int64 [B], and the two lists of tile paths that name the hypothesis (the floor pair where there is one).  In order,
    nothing dropped.  data_list: `ZindData(...).data_list`, or a slice of it (a rank's block of whole batches).
    read_ahead=True: TileFileSource's, with the same cost in device memory.  photometric: TileFileSource's keyword, checked and without
    effect: evaluation never jitters.  rank, world: rows [lo, hi) of every batch (train_feed.shard_bounds), as TileFileSource's val split."""

    def __init__(self, device, data_list: Sequence[tuple], batch_size: int, resize_hw: Tuple[int, int], crop_hw: Tuple[int, int],
                 read_threads: int = MAX_READ_THREADS, entropy: str = "image", read_ahead: bool = False, photometric: Optional[str] = None,
                 rank: int = 0, world: int = 1) -> None:
        train_feed.check_arguments(batch_size)
        train_feed.check_photometric(photometric)   # (accepted so that one set of keywords builds every loader; evaluation batches never jitter)
        super().__init__(device, data_list, resize_hw, crop_hw, read_threads, entropy, read_ahead, rank=rank, world=world)
        self.batch_size = int(batch_size)

    def __len__(self) -> int:
        return batches_per_epoch(len(self.data_list), self.batch_size, "val")

    def __iter__(self):
        E = self.images_per_example
        plan, _ = train_feed.shard_plan(plan_epoch(len(self.data_list), self.batch_size, "val"), self.rank, self.world)
        with contextlib.closing(self._batches(plan)) as batches:
            for idx, images, position in batches:
                B = len(idx)
                out = torch.empty((E, B, 3, self.ras.crop, self.ras.crop), dtype=torch.float32, device=self.device)
                b, j = np.divmod(np.arange(B * E), E)
                jobs = self.ras.upload_tile_jobs(position, j * B + b, np.zeros(B * E, dtype=np.int64))
                with tracing.range("salve.tiles"):
                    self.ras.tiles(images, jobs, B * E, out, _lib.TILE_F32_NCHW, 3)
                examples = [self.data_list[int(i)] for i in idx]
                names = [(e[0], e[1]) if E == 2 else (e[2], e[3]) for e in examples]   # (c1, c2, f1, f2[, l1, l2]): the floor pair
                yield (*(out[k] for k in range(E)), torch.tensor([int(e[-1]) for e in examples], dtype=torch.int64), [n[0] for n in names],
                       [n[1] for n in names])
        self._check_epoch("tile files, evaluation batches")
