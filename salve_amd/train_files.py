"""Batches straight from the rendered tile data set on disk, decoded on the device (opt-in: training.train(decode="device"),
`python -m salve_amd.train --decode device`, train_utils.get_dataloader(decode="device")).

The reference trains and evaluates from 501 x 501 JPEG tiles on disk and decodes each with Pillow in its DataLoader
(zind_data.py:306-315); so does `salve_amd.dataset.zind_data.ZindData`, one file, one upload and one tile launch per example at a
time.  Here a batch is: a bounded thread pool reads the batch's files and parses their headers (salve_amd.jpeg.parse_file); the
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
"""

from __future__ import annotations

import concurrent.futures
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, jpeg, status, tracing
from salve_amd.common.bevparams import BEVParams
from salve_amd.rasteriser import BevRasteriser
from salve_amd.train_render import batches_per_epoch, plan_epoch
from salve_amd.transforms import TrainTransform
from salve_amd.utils import image_io

MAX_READ_THREADS = 16
SPLITS = ("train", "val", "test")
ENTROPY_STAGES = ("image", "lanes")   # BevRasteriser.jpeg_decode(entropy=)


def _read_and_parse(path: str, restart: bool = False):
    with open(path, "rb") as f:
        data = f.read()
    try:
        return data, jpeg.parse_file(data, restart=restart)
    except jpeg.Unsupported:
        return data, None


def _read_and_parse_restart(path: str):
    return _read_and_parse(path, restart=True)


@dataclass
class _Batch:
    """One batch's files as `_pack` laid them out in the pinned buffer."""
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


class _TileFiles:
    """What the two batch sources share: the files of a batch -> int32 [n, H, W] images on the device."""

    def __init__(self, device, data_list: Sequence[tuple], resize_hw: Tuple[int, int], crop_hw: Tuple[int, int], read_threads: int,
                 entropy: str = "image") -> None:
        if not 1 <= int(read_threads) <= MAX_READ_THREADS:
            raise ValueError(f"read_threads must be 1 .. {MAX_READ_THREADS}, got {read_threads}")
        if entropy not in ENTROPY_STAGES:
            raise ValueError(f"entropy must be one of {ENTROPY_STAGES}, got {entropy!r}")
        self.entropy = entropy                          # "lanes": salve_bev_jpeg_decode_lanes, which also takes files with restart intervals
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SalveHipError("decode=\"device\" needs a HIP device ('cuda:N'); there is no CPU path")
        self.data_list = list(data_list)
        widths = {len(e) for e in self.data_list}
        if len(widths) > 1 or (widths and next(iter(widths)) not in (3, 5, 7)):
            raise RuntimeError(f"examples are (2, 4 or 6 tile paths, is_match) tuples of one length, got lengths {sorted(widths)}")
        self.images_per_example = (next(iter(widths)) - 1) if widths else 2
        self.tf = TrainTransform(resize_hw, crop_hw)   # the draws (and the square / no-padding refusals); its kernels are not used
        self.read_threads = int(read_threads)
        self.ras: Optional[BevRasteriser] = None       # made with the first batch: its image size is the first file's
        self.fallbacks = 0                              # files decoded by Pillow so far
        self._pool: Optional[concurrent.futures.ThreadPoolExecutor] = None
        self._pinned: Optional[torch.Tensor] = None
        self._copied: Optional[torch.cuda.Event] = None
        self._epoch_status: List[Tuple[torch.Tensor, List[str]]] = []
        # (a bit an earlier, unchecked caller left in the device's status word is reported as ITS failure, not as this source's)
        status.check(self.device, "a launch issued before this tile file source was created")

    def close(self) -> None:
        """Ends the reader threads (they start with the first batch).  The object stays usable: the next batch starts new ones."""
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
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.read_threads, thread_name_prefix="salve-tile-files")
        return list(self._pool.map(self._read_one if self.entropy == "image" else self._read_one_restart, paths))

    _read_one = staticmethod(_read_and_parse)
    _read_one_restart = staticmethod(_read_and_parse_restart)

    def _pack(self, paths: List[str], read: list) -> "_Batch":
        """Groups the files by `header_key` and fills the pinned buffer: the groups' scans one behind the other, the padding, then
        (4-byte aligned) the pixels of the files that take the host route."""
        if self.ras is None:
            first = read[0][1]
            h, w = (first.h, first.w) if first is not None else image_io.read_rgb(paths[0]).shape[:2]
            self.ras = BevRasteriser(self.device, bev_params=BEVParams(img_h=h - 1, img_w=w - 1), resize=self.tf.resize, crop=self.tf.crop)
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
        if self._copied is not None:
            self._copied.synchronize()   # the last batch's copy has read the buffer
        if self._pinned is None or self._pinned.numel() < b.total:
            self._pinned = torch.empty(max(b.total, 2 * (self._pinned.numel() if self._pinned is not None else 0)), dtype=torch.uint8).pin_memory()
        host = self._pinned.numpy()
        for j, i in enumerate(order):
            data, parsed = read[i]
            host[b.offsets[j]:b.offsets[j] + b.lengths[j]] = np.frombuffer(data, dtype=np.uint8, count=parsed.scan_bytes, offset=parsed.scan_offset)
        host[at:b.pixels_at] = 0
        for j, i in enumerate(host_route):
            rgb = image_io.read_rgb(paths[i])
            if rgb.shape[:2] != (H, W):
                raise RuntimeError(f"{paths[i]} is {rgb.shape[0]} x {rgb.shape[1]}; the tiles of this data set are {H} x {W}")
            p = rgb.astype(np.uint32)
            host[b.pixels_at + j * H * W * 4:b.pixels_at + (j + 1) * H * W * 4] = (p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)).view(np.uint8).reshape(-1)
            b.position[i] = k + j
        self.fallbacks += len(host_route)
        b.names = [""] * n
        for i in range(n):
            b.names[int(b.position[i])] = paths[i]
        return b

    def _upload(self, b: "_Batch") -> torch.Tensor:
        """The pinned buffer's `total` bytes to the device, ONE copy."""
        with tracing.range("salve.tile_files_upload"):
            dev = torch.empty(b.total, dtype=torch.uint8, device=self.device)
            dev.copy_(self._pinned[:b.total], non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
        return dev

    def _decode_group(self, *args, **kw) -> torch.Tensor:
        """One `BevRasteriser.jpeg_decode` call (a group of files that share size and tables) -> its status."""
        return self.ras.jpeg_decode(*args, **kw)[1]

    def _decode(self, b: "_Batch", dev: torch.Tensor) -> torch.Tensor:
        """int32 [n, H, W] images: one decode call per group, then the host route's pixels copied into their slots."""
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
        self._epoch_status.append((image_status, b.names))
        return images

    def _load(self, paths: List[str]) -> Tuple[torch.Tensor, np.ndarray]:
        """The files `paths` -> (int32 [n, H, W] images on the device, position [n] of each path's image in that array)."""
        b = self._pack(paths, self._read(paths))
        return self._decode(b, self._upload(b)), b.position

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


class TileFileSource(_TileFiles):
    """Iterating yields `(x_packed, is_match)`: x_packed [B, crop, crop, Cp] float32 / bfloat16 on the device (the trainable model's
    packed input, `forward_packed`: the example's images in the order of its tuple, three channels each, zero-padded to a multiple of
    8), is_match int64 [B, 1].  One epoch per iteration; `len()` = batches per epoch.  Everything runs on the current stream.
    data_list: `ZindData(...).data_list`."""

    def __init__(self, device, data_list: Sequence[tuple], batch_size: int = 256, precision: str = "fp32", split: str = "train", seed: int = 0,
                 resize_hw: Tuple[int, int] = (234, 234), crop_hw: Tuple[int, int] = (224, 224), read_threads: int = MAX_READ_THREADS,
                 entropy: str = "image") -> None:
        if split not in SPLITS:
            raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        if int(batch_size) <= 0:
            raise ValueError(f"batch size must be positive, got {batch_size}")
        super().__init__(device, data_list, resize_hw, crop_hw, read_threads, entropy)
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
        """train: `TrainTransform.draw()` per example, from Python's `random`; val / test: the centre crop, no flips."""
        if self.split == "train":
            return [self.tf.draw() for _ in range(n)]
        off = (self.tf.resize - self.tf.crop) // 2
        return [(off, off, False, False)] * n

    def batch(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]]) -> Tuple[torch.Tensor, torch.Tensor]:
        """Examples `idx` with one draw (crop_y, crop_x, hflip, vflip) each: (x_packed, is_match)."""
        idx = np.asarray(idx, dtype=np.int64)
        B, K = len(idx), self.per_sample
        if len(draws) != B:
            raise ValueError(f"{B} examples, {len(draws)} draws")
        images, position = self._load(self._paths(idx))
        H, W = self.ras.bev_hw
        pos = position.reshape(B, K, 2)
        jobs = np.zeros((2, B, K), dtype=_lib.TILE_JOB_DTYPE)   # [first | second image of a pair][sample][pair]
        jobs["bev_offset"][0], jobs["bev_offset"][1] = pos[:, :, 0] * (H * W), pos[:, :, 1] * (H * W)
        jobs["slot"][:] = np.arange(B, dtype=np.int64)[None, :, None]
        jobs["chan"][0] = 6 * np.arange(K)[None, :]
        jobs["chan"][1] = 6 * np.arange(K)[None, :] + 3
        aug = np.zeros(B, dtype=_lib.TILE_AUG_DTYPE)
        for k, (cy, cx, hflip, vflip) in enumerate(draws):
            aug[k] = (cy, cx, (_lib.TILE_HFLIP if hflip else 0) | (_lib.TILE_VFLIP if vflip else 0), 0)
        parts = [jobs.view(np.uint8).reshape(-1), aug.view(np.uint8), self.labels[idx].view(np.uint8)]   # ONE upload of the tables
        buf = torch.from_numpy(np.concatenate(parts)).to(self.device)
        o = np.cumsum([0] + [p.nbytes for p in parts])
        out = torch.empty((B, self.ras.crop, self.ras.crop, self.out_c), dtype=self.dtype, device=self.device)
        self._tile_launch(images, buf[:o[1] // 2], buf[o[1] // 2:o[1]], K, buf[o[1]:o[2]], B, out)
        return out, buf[o[2]:o[3]].view(torch.int64).view(B, 1)

    def _tile_launch(self, images, jobs_a, jobs_b, per_sample, aug, batch, out) -> None:
        """ONE salve_bev_train_tiles launch: both arrays of image pairs are the decoded images."""
        with tracing.range("salve.train_tiles"):
            self.ras.train_tiles(images, images, jobs_a, jobs_b, per_sample, aug, batch, out)

    def __iter__(self):
        for idx in plan_epoch(len(self.data_list), self.batch_size, "train" if self.split == "train" else "val", self.gen):
            yield self.batch(idx, self.draws(len(idx)))
        self._check_epoch(f"tile files, {self.split} batches")


class TileFileLoader(_TileFiles):
    """Iterating yields what the evaluation DataLoader over `ZindData` yields: `(x1, x2[, x3, x4[, x5, x6]], is_match, fp0, fp1)` --
    float32 [B, 3, crop, crop] tiles on the device (Resize -> centre Crop -> ToTensor -> Normalize, ONE salve_bev_tiles launch per
    batch), is_match int64 [B], and the two lists of tile paths that name the hypothesis (the floor pair where there is one).  In order,
    nothing dropped.  data_list: `ZindData(...).data_list`, or a slice of it (a rank's block of whole batches)."""

    def __init__(self, device, data_list: Sequence[tuple], batch_size: int, resize_hw: Tuple[int, int], crop_hw: Tuple[int, int],
                 read_threads: int = MAX_READ_THREADS, entropy: str = "image") -> None:
        if int(batch_size) <= 0:
            raise ValueError(f"batch size must be positive, got {batch_size}")
        super().__init__(device, data_list, resize_hw, crop_hw, read_threads, entropy)
        self.batch_size = int(batch_size)

    def __len__(self) -> int:
        return batches_per_epoch(len(self.data_list), self.batch_size, "val")

    def __iter__(self):
        E = self.images_per_example
        for idx in plan_epoch(len(self.data_list), self.batch_size, "val"):
            B = len(idx)
            images, position = self._load(self._paths(idx))
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
