"""Training batches rendered on the GPU: panoramas, depth maps and labelled alignment hypotheses in, the trainable model's packed
input out, no JPEG hop.

The reference trains from a rendered dataset on disk: scripts/render_dataset_bev.py writes one JPEG per panorama, surface and
hypothesis, salve/dataset/zind_data.py:306-315 reads 2 / 4 of them per example, salve/train_utils.py:63-124 resizes, crops, flips and
normalises them on the host, and salve/models/early_fusion.py:52-60 concatenates them.  `RenderedTrainSource` yields the same
batches from the lossless BEV images instead: per batch one scatter + densify launch pair of the rasteriser for the posed renders
(the identity renders of every panorama are made once and kept, as in salve_amd.pipeline) and ONE salve_bev_train_tiles launch
that writes `[B, crop, crop, Cp]` in the training precision -- what `TrainableEarlyFusionCEResnet.forward_packed` takes.

The layout modality (`layouts=PanoLayouts`) rides along: the panoramas' rooms and W/D/Os stay on the device as flat tables, a batch's
record table goes up with its one upload, ONE salve_layout_pose launch poses the batch's layouts and ONE salve_layout_rasterise launch
draws them into the image arrays the tile jobs index, behind the texture renders; the train-tile launch then takes one more image per
sample.  Layout alone renders no texture map and uploads no panorama.

Two opt-in arguments take the feed beyond panorama sets that fit the device.  `identity="batch"` keeps no identity image per
panorama: the identity renders of the batch's distinct second panoramas ride in the batch's own scatter / densify launch pair, behind
the posed renders.  `resident_panos=N` keeps a pool of N panorama slots on the device (salve_amd.pano_pool.PanoPool): `PanoCache` plans, batch by batch, which
panoramas of the host arrays (np.memmap included) are uploaded into which slots -- the victim is the panorama whose next use in the
epoch lies furthest ahead -- and `BevRasteriser.update_panos` rebuilds the panorama index of the written slots only.  `prefetch=True`
(with a pool) does that one batch ahead, off the training step's path: worker threads gather the next batch's missed rows and the
copies, slot writes and index update run on a copy stream of the pool's own while the current batch trains.

Shuffle order and augmentation draws are those of `training.get_dataloader` + `transforms.TrainTransform` (salve_amd.train_feed, shared
with the tile-file feed).  The planning functions are pure and need no device: `plan_examples` and `check_launch` here, `plan_epoch`
(train_feed), `PanoCache` and `epoch_next_use` (pano_pool) -- the moved names still resolve in this module.
"""

from __future__ import annotations

import contextlib
import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, status, tracing, train_feed
from salve_amd.pano_pool import MAX_GATHER_THREADS, NEVER, PanoCache, PanoPool, epoch_next_use  # noqa: F401  (NEVER: re-exported)
from salve_amd.pipeline import surfaces_for
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses
from salve_amd.synthetic import HypothesisTable
from salve_amd.train_feed import SPLITS, batches_per_epoch, plan_epoch
from salve_amd.transforms import TrainTransform

MAX_RENDERS_PER_CALL = 65535   # include/salve_hip.h: renders per scatter / densify call
MAX_LAYOUTS_PER_LAUNCH = 65535  # include/salve_hip.h: images per salve_layout_pose / salve_layout_rasterise call


def check_launch(batch_size: int, n_surfaces: int, identity_rows: int = 0, layout: bool = False) -> None:
    """A batch's posed renders -- and, with identity="batch", the identity renders of up to `identity_rows` distinct second panoramas
    behind them -- go through ONE scatter / densify call; with `layout`, its layout images (one per sample and identity panorama) go
    through ONE pose / rasterise call of the same limit."""
    if batch_size <= 0:
        raise ValueError(f"batch size must be positive, got {batch_size}")
    if identity_rows < 0:
        raise ValueError(f"identity_rows must not be negative, got {identity_rows}")
    n = (batch_size + identity_rows) * n_surfaces
    if n > MAX_RENDERS_PER_CALL:
        what = f"batch_size {batch_size}" if identity_rows == 0 else f"(batch_size {batch_size} + {identity_rows} identity panoramas)"
        raise RuntimeError(f"{what} x {n_surfaces} surfaces = {n} renders per batch; the library takes at most {MAX_RENDERS_PER_CALL} per call")
    if layout and batch_size + identity_rows > MAX_LAYOUTS_PER_LAUNCH:
        raise RuntimeError(f"batch_size {batch_size} + {identity_rows} identity panoramas = {batch_size + identity_rows} layout images per batch; "
                           f"the library takes at most {MAX_LAYOUTS_PER_LAUNCH} per call")


def train_surfaces(modalities: Sequence[str], with_layouts: bool = False) -> List[str]:
    """The texture surfaces of a configuration's modalities.  "layout" is served only when the panoramas' layouts are given
    (`RenderedTrainSource(layouts=...)`): alone (no surface) or behind ceiling + floor."""
    if "layout" in set(modalities) and not with_layouts:
        raise RuntimeError('RenderedTrainSource does not render the "layout" modality (floor, ceiling, ceiling + floor only) without the '
                           "panoramas' layouts (layouts=PanoLayouts; --render-from: layouts.npz): train it from the rendered dataset on disk")
    return surfaces_for(modalities)


def plan_examples(hyp: HypothesisTable, is_match, n_panos: int) -> Dict[str, np.ndarray]:
    """The validated host arrays of a labelled example table: one example per row of `hyp`, label is_match[row]."""
    n = len(hyp)
    labels = np.asarray(is_match)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise RuntimeError(f"is_match must hold one label per hypothesis: {n} rows, labels of shape {labels.shape}")
    i1, i2 = np.asarray(hyp.i1).astype(np.int64), np.asarray(hyp.i2).astype(np.int64)
    for name, v in (("i1", i1), ("i2", i2)):
        if n and (int(v.min()) < 0 or int(v.max()) >= n_panos):
            raise RuntimeError(f"{name} names panorama {int(v.min()) if int(v.min()) < 0 else int(v.max())}; {n_panos} panoramas are loaded")
    R, t = np.asarray(hyp.R, dtype=np.float32).reshape(n, 2, 2), np.asarray(hyp.t, dtype=np.float32).reshape(n, 2)
    swap = np.zeros(n, dtype=np.int64) if hyp.swap is None else np.asarray(hyp.swap).astype(np.int64)
    if swap.shape != (n,):
        raise RuntimeError(f"swap must hold one flag per hypothesis, got shape {swap.shape}")
    return {"i1": i1, "i2": i2, "R": R, "t": t, "swap": swap, "is_match": labels.astype(np.int64)}


IDENTITIES = ("kept", "batch")


class RenderedTrainSource:
    """Iterating yields `(x_packed, is_match)`: x_packed [B, crop, crop, Cp] float32 / bfloat16 on the device, is_match int64 [B, 1].
    One epoch per iteration; `len()` = batches per epoch.  Everything runs on the current stream.  The device status word is checked
    once per epoch, after the last batch (a bad render row, tile job or pool slot raises there).

    layouts: salve_amd.layout.PanoLayouts of the same panoramas -- required iff the modalities include "layout" (["layout"] alone: no
    texture map is rendered and no panorama uploaded; ceiling + floor + layout: 18 channels, the layout pair behind the texture maps).
    identity: "kept" (default) renders the identity image of every panorama once and keeps it; "batch" renders the identity images of
    the batch's distinct second panoramas with the batch -- the same images, no P x S image array.  resident_panos: None (default)
    uploads every panorama up front; an integer keeps a pool of that many panorama slots on the device, filled on first use from the
    host arrays `load_panos` was given (needs identity="batch"; at least min(2 x batch_size, P) slots).
    prefetch (needs resident_panos; at least min(4 x batch_size, P) slots): while batch b trains, batch b + 1's misses are gathered by
    `gather_threads` host threads and uploaded on a copy stream the pool owns; the batches are the same.
    jpeg_quality: None (default): the tiles come from the lossless images.  An integer (the reference's files: 75): every render and
    layout image takes the reference's JPEG round trip on the device (BevRasteriser.jpeg_roundtrip) between densify / rasterise and the
    train-tile launch -- kept identity images once, everything else with its batch -- so the batches equal the on-disk DataLoader's
    (DESIGN.md 4.17).  It runs on the compute stream: prefetch and the resident pool are unaffected.
    photometric: None (default), or "device": train batches take the reference's PhotometricShift -- ColorJitter on every resized image,
    with draws of its own, in front of the crop -- inside the train-tile call (salve_bev_train_tiles_jitter), the draws
    those of `TrainTransform.draw_jitter` per image in x1 .. x6 order from torch's global generator.  Val batches never jitter.
    rank, world (data-parallel training): the source plans the whole epoch and takes the whole batch's draws, then yields
    rows [lo, hi) of every batch (train_feed.shard_bounds) -- bit for bit those rows of the world-1 source's batch; the pool plans for
    this rank's panoramas only.  `len()` stays the number of whole batches; a train batch size must be a multiple of `world`; a val
    batch that leaves the rank no row is not yielded."""

    def __init__(self, device, modalities: Sequence[str], pano_hw: Tuple[int, int] = (512, 1024), batch_size: int = 256,
                 precision: str = "fp32", split: str = "train", seed: int = 0, resize_hw: Tuple[int, int] = (234, 234),
                 crop_hw: Tuple[int, int] = (224, 224), identity: str = "kept", resident_panos: Optional[int] = None, layouts=None,
                 prefetch: bool = False, gather_threads: int = 4, jpeg_quality: Optional[int] = None, photometric: Optional[str] = None,
                 rank: int = 0, world: int = 1) -> None:
        train_feed.check_arguments(batch_size, split, SPLITS, precision)
        train_feed.check_photometric(photometric)
        train_feed.check_shard(batch_size, split, rank, world)
        self.rank, self.world = int(rank), int(world)
        self._rows: List[Tuple[int, int, int]] = []   # the running epoch: (rows of the whole batch, lo, hi) per batch of this rank
        if identity not in IDENTITIES:
            raise ValueError(f"identity must be one of {IDENTITIES}, got {identity!r}")
        if resident_panos is not None:
            if identity != "batch":
                raise ValueError('resident_panos needs identity="batch": keeping an identity image per panorama is what does not fit')
            if int(resident_panos) <= 0:
                raise ValueError(f"resident_panos must be positive, got {resident_panos}")
        if prefetch and resident_panos is None:
            raise ValueError("prefetch needs resident_panos: without a pool every panorama is resident and nothing is uploaded per batch")
        if not 1 <= int(gather_threads) <= MAX_GATHER_THREADS:
            raise ValueError(f"gather_threads must be 1 .. {MAX_GATHER_THREADS}, got {gather_threads}")
        self.prefetch, self.gather_threads = bool(prefetch), int(gather_threads)
        self.jpeg_quality = None if jpeg_quality is None else int(jpeg_quality)
        self.surfaces = train_surfaces(modalities, with_layouts=layouts is not None)
        self.has_layout = "layout" in set(modalities)
        self.layouts = layouts if self.has_layout else None   # salve_amd.layout.PanoLayouts, indexed by panorama
        self.per_sample = len(self.surfaces) + (1 if self.has_layout else 0)   # images per sample and array: texture maps, then the layout
        check_launch(batch_size, len(self.surfaces), batch_size if identity == "batch" else 0, layout=self.has_layout)
        self.photometric = photometric if split == "train" else None   # (val batches never jitter)
        # the draws (and the square / no-padding refusals); its kernels are not used
        self.tf = TrainTransform(resize_hw, crop_hw, jitter_types=train_feed.JITTER_TYPES if self.photometric else None)
        self.split, self.batch_size = split, int(batch_size)
        self.identity, self.resident_panos = identity, None if resident_panos is None else int(resident_panos)
        self.dtype = torch.bfloat16 if precision == "bf16" else torch.float32
        self.out_c = (6 * self.per_sample + 7) // 8 * 8
        self.gen = torch.Generator()
        self.gen.manual_seed(seed)
        self.device = torch.device(device)
        # (a bit an earlier, unchecked caller left in the device's status word is reported as ITS failure, not as this source's)
        status.check(self.device, "a launch issued before this RenderedTrainSource was created")
        self.ras = BevRasteriser(self.device, pano_hw=pano_hw, resize=self.tf.resize, crop=self.tf.crop)
        self.pano_rgb = self.pano_depth = self.ref_bev = self.bev = None
        self.lay = None           # layout.DeviceLayouts: the resident tables and one batch's output tables
        self.lay_base = (0, 0)    # first layout image inside self.bev / self.ref_bev: they lie behind the texture renders
        self.n_panos: Optional[int] = None
        self.examples: Optional[Dict[str, np.ndarray]] = None
        self.pool: Optional[PanoPool] = None   # resident_panos: host arrays, PanoCache, slots, staging buffers -- shared by share_panos
        self.timers = None   # a list: every launch appends (tag, start event, end event) -- tools/measure/bench_train_feed.py

    # ------------------------------------------------------------------ panoramas
    def _refuse_if_too_large(self, need: int, what: str) -> None:
        free = int(torch.cuda.mem_get_info(self.device)[0])
        if need > free:
            hint = ("a smaller --resident-panos pool fits" if self.resident_panos is not None else
                    "panorama sets that do not fit at once train with --resident-panos N (which selects --identity batch)")
            raise RuntimeError(f"{what} need {need} bytes of device memory, {free} are free: {hint}")

    def _batch_images(self, n_slots: int) -> int:
        """Images of one batch's buffer: the posed renders, and with identity="batch" the identity renders behind them."""
        return (self.batch_size + (min(self.batch_size, n_slots) if self.identity == "batch" else 0)) * len(self.surfaces)

    def _layout_images(self, n_slots: int) -> int:
        """Layout images of one batch's buffer: one per sample, and with identity="batch" one per distinct second panorama."""
        return (self.batch_size + (min(self.batch_size, n_slots) if self.identity == "batch" else 0)) if self.has_layout else 0

    def layout_bases(self, P: int, n_slots: int) -> Tuple[int, int]:
        """First layout image inside (the batch's array, the kept identity array): behind the texture renders of each."""
        S = len(self.surfaces)
        return (self._batch_images(n_slots) if self.identity == "batch" else self.batch_size * S), P * S

    def _alloc_images(self, P: int, n_slots: int) -> None:
        """self.bev (one batch: texture renders | layout images) and, identity="kept", self.ref_bev (P x S identity renders | P identity
        layout images, drawn here once); the layout tables go to the device."""
        S = len(self.surfaces)
        Hb, Wb = self.ras.bev_hw
        self.lay_base = self.layout_bases(P, n_slots)
        self.bev = torch.empty((self.lay_base[0] + self._layout_images(n_slots), Hb, Wb), dtype=torch.int32, device=self.device)
        self.ref_bev = torch.empty((P * self.per_sample, Hb, Wb), dtype=torch.int32, device=self.device) if self.identity == "kept" else None
        if not self.has_layout:
            return
        from salve_amd import layout as layout_mod

        if self.layouts.P != P:
            raise RuntimeError(f"the layout tables hold {self.layouts.P} panoramas, {P} panoramas are loaded")
        self.lay = layout_mod.DeviceLayouts(self.layouts, self.device, max(1, self._layout_images(n_slots)))
        if self.identity == "kept":
            with tracing.range("salve.identity_layouts"):
                for lo in range(0, P, self.lay.n_max):
                    ids = np.arange(lo, min(lo + self.lay.n_max, P))
                    self.lay.draw(layout_mod.pose_records(self.layouts, ids), self.ref_bev[P * S + lo:])
                self._jpeg(self.ref_bev[P * S:P * S + P])

    def load_panos(self, rgb: np.ndarray, depth: np.ndarray) -> None:
        """P panoramas (uint8 [P, H, W, 3], uint16 [P, H, W]).  Default: upload them all (and, identity="kept", render their identity
        BEV images).  resident_panos: keep the host arrays (np.memmap included) and upload nothing -- slots fill on first use.
        Layout alone: only P is taken from the arrays, nothing is uploaded."""
        if not self.surfaces:
            self._set_no_panos(int(rgb.shape[0]))
            return
        if self.resident_panos is None:
            self._refuse_if_too_large(int(rgb.nbytes) + int(depth.nbytes), f"{len(rgb)} panoramas")
            self.set_panos(*self.ras.upload_panos(rgb, depth))
            return
        H, W = self.ras.pano_hw
        if rgb.dtype != np.uint8 or depth.dtype != np.uint16 or tuple(rgb.shape[1:]) != (H, W, 3) or tuple(depth.shape) != tuple(rgb.shape[:3]):
            raise RuntimeError(f"panoramas must be uint8 [P, {H}, {W}, 3] and uint16 [P, {H}, {W}], got {rgb.dtype} {tuple(rgb.shape)} / "
                               f"{depth.dtype} {tuple(depth.shape)}")
        P, S = int(rgb.shape[0]), len(self.surfaces)
        Hb, Wb = self.ras.bev_hw
        try:
            cache = PanoCache(P, self.resident_panos, self.batch_size, bytes_per_pano=H * W * 5, prefetch=self.prefetch)
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        n_slots, n_stage = cache.capacity, min(2 * self.batch_size, cache.capacity)
        index_bytes = self.ras.pano_index_bytes(n_slots)
        # (prefetch: the rows of the batch ahead are allocated on the copy stream, those of an epoch's first batch on the compute stream, and
        # the caching allocator keeps the two streams' blocks apart: two batches' upload rows and their int64 slot lists can be held at once)
        n_rows = 2 * n_stage if self.prefetch else n_stage
        self._refuse_if_too_large((n_slots + n_rows) * H * W * 5 + n_rows * 12 + index_bytes
                                  + (self._batch_images(n_slots) + self._layout_images(n_slots)) * Hb * Wb * 4,
                                  f"a pool of {n_slots} panorama slots, its index, {'two batches' if self.prefetch else 'one batch'}'s uploads and one batch's BEV images")
        self.pool = PanoPool(self.ras, rgb, depth, cache, n_stage, prefetch=self.prefetch)
        self.pano_rgb, self.pano_depth = self.pool.pano_rgb, self.pool.pano_depth
        self.n_panos, self.examples = P, None
        self._alloc_images(P, n_slots)
        self.ras._workspace(self._batch_images(n_slots))

    def _set_no_panos(self, P: int) -> None:
        """Layout alone: P panoramas are known by their layouts only; no texture map is rendered, so none is uploaded and a resident
        pool has nothing to hold."""
        Hb, Wb = self.ras.bev_hw
        self._refuse_if_too_large((self._layout_images(P) + (P if self.identity == "kept" else 0)) * Hb * Wb * 4, "the layout images")
        self.n_panos, self.examples = P, None
        self._alloc_images(P, P)

    def set_panos(self, rgb_dev: torch.Tensor, depth_dev: torch.Tensor) -> None:
        """Panoramas on the device (as RenderVerifyPipeline.set_panos takes them).  identity="kept": the identity render of every
        panorama and surface is made once and kept; identity="batch": nothing is rendered here."""
        if not self.surfaces:
            self._set_no_panos(int(rgb_dev.shape[0]))
            return
        if self.resident_panos is not None:
            raise RuntimeError("resident_panos takes the panoramas as host arrays: load_panos(rgb, depth)")
        if tuple(rgb_dev.shape[1:3]) != tuple(self.ras.pano_hw) or tuple(depth_dev.shape[1:]) != tuple(self.ras.pano_hw):
            raise RuntimeError(f"panoramas must be {self.ras.pano_hw}, got {tuple(rgb_dev.shape[1:3])} / {tuple(depth_dev.shape[1:])}")
        P, S = int(rgb_dev.shape[0]), len(self.surfaces)
        Hb, Wb = self.ras.bev_hw
        if self.identity == "batch":
            self._refuse_if_too_large((self._batch_images(P) + self._layout_images(P)) * Hb * Wb * 4, "the BEV images of one batch")
            self.pano_rgb, self.pano_depth = rgb_dev.contiguous(), depth_dev.contiguous()
            self.n_panos, self.examples = P, None
            self._alloc_images(P, P)   # posed | identity renders of one batch (| its layout images)
            self.ras._workspace(self._batch_images(P))
            return
        self._refuse_if_too_large((P + self.batch_size) * self.per_sample * Hb * Wb * 4, f"the BEV images of {P} panoramas and one batch")
        self.pano_rgb, self.pano_depth = rgb_dev.contiguous(), depth_dev.contiguous()
        self.n_panos, self.examples = P, None
        rows = pack_hypotheses(np.repeat(np.arange(P), S), np.tile([SURFACES[s] for s in self.surfaces], P),
                               np.tile(np.eye(2, dtype=np.float32), (P * S, 1, 1)), np.zeros((P * S, 2), np.float32), np.zeros(P * S))
        rows_dev = self.ras.upload_hypotheses(rows)
        self._alloc_images(P, P)   # one batch's posed renders; the identity renders of every panorama
        with tracing.range("salve.identity_renders"):
            for lo in range(0, P * S, 256):
                n = min(256, P * S - lo)
                self.ras.render(self.pano_rgb, self.pano_depth, rows_dev[lo * _lib.HYP_DTYPE.itemsize:], n, self.ref_bev[lo:lo + n])
            self._jpeg(self.ref_bev[:P * S])

    def share_panos(self, other: "RenderedTrainSource") -> None:
        """Use the panoramas, identity renders and batch buffer `other` holds (the val source beside the train source: one copy on
        the device; both run on the same stream, one batch at a time).  With a resident pool the slots and their `PanoCache` are
        shared too: whichever source is iterating plans with its own epoch's next uses."""
        if other.n_panos is None:
            raise RuntimeError("the other source has no panoramas yet")
        if (other.device, other.surfaces, other.has_layout, other.ras.pano_hw, other.ras.bev_hw) != \
                (self.device, self.surfaces, self.has_layout, self.ras.pano_hw, self.ras.bev_hw) \
                or other.batch_size < self.batch_size:
            raise RuntimeError("share_panos needs the same device, modalities and panorama size, and a batch size not above the other's")
        if (other.identity, other.resident_panos) != (self.identity, self.resident_panos):
            raise RuntimeError("share_panos needs the same identity and resident_panos arguments on both sources")
        if other.prefetch != self.prefetch:
            raise RuntimeError("share_panos needs the same prefetch argument on both sources")
        if other.jpeg_quality != self.jpeg_quality:
            raise RuntimeError("share_panos needs the same jpeg_quality argument on both sources (the kept identity images are shared)")
        self.pano_rgb, self.pano_depth, self.ref_bev, self.bev, self.n_panos, self.examples = (other.pano_rgb, other.pano_depth, other.ref_bev,
                                                                                               other.bev, other.n_panos, None)
        self.pool, self.lay, self.lay_base, self.layouts = other.pool, other.lay, other.lay_base, other.layouts

    @property
    def cache(self) -> Optional[PanoCache]:
        return None if self.pool is None else self.pool.cache

    @property
    def uploads(self) -> int:
        """Panoramas uploaded into the pool so far (0 without one)."""
        return 0 if self.pool is None else self.pool.uploads

    # ------------------------------------------------------------------ examples
    def set_examples(self, hyp: HypothesisTable, is_match) -> None:
        """One labelled example per row: panorama i1 rendered under the pose, panorama i2 at identity, label is_match[row].  The
        two tiles of a surface go to the model in (i1, i2) order, or (i2, i1) where `hyp.swap` says so -- the file-name order of
        salve/dataset/zind_data.py:110, exactly as RenderVerifyPipeline.prepare orders them."""
        if self.n_panos is None:
            raise RuntimeError("set_panos / load_panos first: the examples are checked against the loaded panoramas")
        self.examples = plan_examples(hyp, is_match, self.n_panos)

    def __len__(self) -> int:
        return 0 if self.examples is None else batches_per_epoch(len(self.examples["i1"]), self.batch_size, self.split)

    # ------------------------------------------------------------------ batches
    def _jpeg(self, images: torch.Tensor) -> None:
        """The reference's JPEG round trip of `images`, in place, if this source was asked for it."""
        if self.jpeg_quality is None or images.shape[0] == 0:
            return
        with self._launch("jpeg", "salve.jpeg"):
            self.ras.jpeg_roundtrip(images, self.jpeg_quality, out=images)

    @contextlib.contextmanager
    def _launch(self, tag: str, name: str):
        """Around one launch: the trace range `name`, and -- while `timers` is a list -- two HIP events around it, filed under `tag`."""
        timed = self.timers is not None
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.timers.append((tag, e0, e1))
            e0.record()
        with tracing.range(name):
            yield
        if timed:
            e1.record()

    # ------------------------------------------------------------------ prefetch
    def _iter_prefetch(self, plan: List[np.ndarray]):
        """The epoch with the uploads one batch ahead: batch 0 is made resident on the compute stream as without prefetch; right behind
        batch b's launches batch b + 1 is planned and its upload started.  The copy stream writes only slots that neither batch b nor
        batch b + 1 names, behind the event of batch b - 1's last launch (the last batch of the epoch before, for b = 0)."""
        pool = self.pool
        panos = [self.batch_panos(idx) for idx in plan]
        next_use, after = epoch_next_use(panos, self.n_panos)
        mine, planned = pool.begin(self.gather_threads), False
        try:
            for b, idx in enumerate(plan):
                pool.check(mine)   # one iteration at a time plans this pool: one that was suspended meanwhile refuses to go on
                if planned:
                    ready = pool.drain(raise_errors=True)
                    if ready is not None:
                        torch.cuda.current_stream(self.device).wait_event(ready)
                draws, jitter = self._shard_draws(b)
                out = self.batch(idx, draws, next_use, planned=planned, jitter=jitter)
                next_use[panos[b]] = after[b]
                before = pool.mark_done()
                planned = b + 1 < len(plan)
                if planned:
                    pool.plan_ahead(panos[b + 1], next_use, panos[b], before, mine)
                yield out
        finally:
            pool.end(mine)

    def _shard_draws(self, b: int):
        """(draws, jitter draws) of batch `b` of this rank's plan: the whole batch's are taken, this rank's rows are kept."""
        n, lo, hi = self._rows[b]
        return train_feed.shard_draws(self.draws(n), self.jitter_draws(n), 2 * self.per_sample, lo, hi)

    def batch(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]], next_use: Optional[np.ndarray] = None,
              planned: bool = False, jitter: Optional[Sequence[train_feed.JitterDraw]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Render examples `idx` with one draw (crop_y, crop_x, hflip, vflip) each: (x_packed, is_match).  `next_use` (resident pool
        only): the batch of every panorama's next use, for the planner (`epoch_next_use`).  `planned`: the batch's panoramas were made
        resident ahead (prefetch): their slots are looked up, nothing is planned or uploaded here.  `jitter` (photometric="device"): one
        `TrainTransform.draw_jitter()` per image, [B * 2 K] in example order, an example's images by channel group (`jitter_draws`)."""
        B, S, K = len(idx), len(self.surfaces), self.per_sample
        if jitter is not None and len(jitter) != 2 * K * B:
            raise ValueError(f"{B} examples of {2 * K} images, {len(jitter)} jitter draws")
        jobs, aug, rows, lay_recs, n = self.batch_tables(idx, draws, next_use, planned)
        bev_b = self.ref_bev if self.identity == "kept" else self.bev
        # ONE upload per batch; every table starts on a multiple of 16 bytes (the 40-byte render rows come last)
        # (the 48-byte layout records hold a double: every table in front of them is a multiple of 8 bytes long)
        # (the 40-byte jitter records hold 4-byte fields only: they come behind everything else)
        buf, o = train_feed.upload_tables([jobs, aug, self.examples["is_match"][idx], rows, lay_recs, train_feed.jitter_table(jitter or [])], self.device)
        jobs_a, jobs_b = buf[:o[1] // 2], buf[o[1] // 2:o[1]]
        labels = buf[o[2]:o[3]].view(torch.int64).view(B, 1)
        if S:   # (layout alone: no texture map, as RenderVerifyPipeline)
            with self._launch("scatter", "salve.scatter"):
                self.ras.scatter(self.pano_rgb, self.pano_depth, buf[o[3]:o[4]], n, self.bev, index=None if self.pool is None else self.pool.index)
            with self._launch("densify", "salve.densify"):
                self.ras.densify(n, self.bev)
            self._jpeg(self.bev[:n])
        if self.has_layout:
            with self._launch("layout pose", "salve.layout_pose"):
                self.lay.pose(buf[o[4]:o[5]], len(lay_recs))
            with self._launch("layout rasterise", "salve.layout_rasterise"):
                self.lay.rasterise(len(lay_recs), self.bev[self.lay_base[0]:])
            self._jpeg(self.bev[self.lay_base[0]:self.lay_base[0] + len(lay_recs)])
        out = torch.empty((B, self.ras.crop, self.ras.crop, self.out_c), dtype=self.dtype, device=self.device)
        with self._launch("tiles", "salve.train_tiles"):
            self.ras.train_tiles(self.bev, bev_b, jobs_a, jobs_b, K, buf[o[1]:o[2]], B, out,   # (identity="batch": one buffer, only read)
                                 jitter=None if jitter is None else buf[o[5]:o[6]])
        return out, labels

    def batch_tables(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]], next_use: Optional[np.ndarray] = None, planned: bool = False):
        """The host tables of one batch: (tile jobs [2][B][K], draws [B], render rows, layout pose records, renders).  Host arithmetic,
        except that a resident pool uploads its misses here (`PanoPool.make_resident`)."""
        ex, S, B, K = self.examples, len(self.surfaces), len(idx), self.per_sample
        if len(draws) != B:
            raise ValueError(f"{B} examples, {len(draws)} draws")
        Hb, Wb = self.ras.bev_hw
        i1 = ex["i1"][idx]
        surf = [SURFACES[s] for s in self.surfaces]
        si = np.tile(np.arange(S, dtype=np.int64), B)
        # sample-major [B][K]: posed renders of this batch | identity renders; a sample's layout image (K = S + 1) is its last job
        jobs = np.zeros((2, B, K), dtype=_lib.TILE_JOB_DTYPE)
        tex = lambda v: np.asarray(v).reshape(B, S)
        lay_recs = np.zeros(0, dtype=_lib.LAYOUT_POSE_DTYPE)
        if self.identity == "kept":
            # renders in the order of their panorama (as RenderVerifyPipeline.prepare issues them: the workgroups of one panorama run
            # side by side and share its depth blocks through the L2s); the tile jobs name each sample's render by its rank
            order = np.argsort(i1, kind="stable")
            rank = np.empty(B, dtype=np.int64)
            rank[order] = np.arange(B)
            src = idx[order]
            rows = pack_hypotheses(np.repeat(ex["i1"][src], S), np.tile(surf, B), np.repeat(ex["R"][src], S, axis=0),
                                   np.repeat(ex["t"][src], S, axis=0), np.ones(B * S))
            n = B * S
            jobs["bev_offset"][0, :, :S] = tex((np.repeat(rank, S) * S + si) * (Hb * Wb))
            jobs["bev_offset"][1, :, :S] = tex((np.repeat(ex["i2"][idx], S) * S + si) * (Hb * Wb))
            if self.has_layout:   # sample k's posed layout is image k of the batch's; panorama i2's own layout was drawn when the layouts were loaded
                lay_recs = self._layout_records(i1, ex["R"][idx], ex["t"][idx], 0)
                jobs["bev_offset"][0, :, S] = (self.lay_base[0] + np.arange(B)) * (Hb * Wb)
                jobs["bev_offset"][1, :, S] = (self.lay_base[1] + ex["i2"][idx]) * (Hb * Wb)
        else:
            # B posed renders and the identity renders of the U distinct second panoramas, ONE launch pair; a group of S renders per
            # entry, the groups in the order of their panorama's slot (the pool's slot, or the panorama itself when all are resident)
            uniq, inv = np.unique(ex["i2"][idx], return_inverse=True)
            U = len(uniq)
            pano = np.concatenate([i1, uniq])
            where = pano if self.pool is None else self.pool.lookup(pano) if planned else self.pool.make_resident(pano, next_use, self._launch)
            order = np.argsort(where, kind="stable")
            rank = np.empty(B + U, dtype=np.int64)
            rank[order] = np.arange(B + U)
            R = np.concatenate([ex["R"][idx], np.tile(np.eye(2, dtype=np.float32), (U, 1, 1))])[order]
            t = np.concatenate([ex["t"][idx], np.zeros((U, 2), np.float32)])[order]
            posed = (np.arange(B + U) < B).astype(np.int32)[order]
            rows = pack_hypotheses(np.repeat(where[order], S), np.tile(surf, B + U), np.repeat(R, S, axis=0), np.repeat(t, S, axis=0), np.repeat(posed, S))
            n = (B + U) * S
            jobs["bev_offset"][0, :, :S] = tex((np.repeat(rank[:B], S) * S + si) * (Hb * Wb))
            jobs["bev_offset"][1, :, :S] = tex((np.repeat(rank[B + inv], S) * S + si) * (Hb * Wb))
            if self.has_layout:   # B posed layouts and the U distinct identity layouts behind them, ONE pose and ONE rasterise launch
                lay_recs = self._layout_records(np.concatenate([i1, uniq]), ex["R"][idx], ex["t"][idx], U)
                jobs["bev_offset"][0, :, S] = (self.lay_base[0] + np.arange(B)) * (Hb * Wb)
                jobs["bev_offset"][1, :, S] = (self.lay_base[0] + B + inv) * (Hb * Wb)
        check_launch(B, S, (n // S - B) if S else (len(lay_recs) - B), layout=self.has_layout)
        swap = ex["swap"][idx]
        jobs["slot"][:] = np.arange(B, dtype=np.int64)[None, :, None]
        jobs["chan"][0] = 6 * np.arange(K)[None, :] + 3 * swap[:, None]   # the layout pair follows the texture maps (zind_data.py:26)
        jobs["chan"][1] = 6 * np.arange(K)[None, :] + 3 * (1 - swap)[:, None]
        return jobs, train_feed.aug_table(draws), rows, lay_recs, n

    def _layout_records(self, pano: np.ndarray, R: np.ndarray, t: np.ndarray, n_identity: int) -> np.ndarray:
        """salve_layout_pose_t rows of a batch: its posed layouts under (R, t) (alignment hypotheses are SE(2): scale 1), then
        `n_identity` panoramas' own layouts -- indexed by PANORAMA, not by pool slot: the layout tables are fully resident."""
        from salve_amd import layout as layout_mod

        return layout_mod.pose_records(self.layouts, pano, np.concatenate([R, np.zeros((n_identity, 2, 2), np.float32)]),
                                       np.concatenate([t, np.zeros((n_identity, 2), np.float32)]), None, np.arange(len(pano)) < len(R))

    def draws(self, n: int) -> List[Tuple[int, int, bool, bool]]:
        """One draw per example of a batch (`train_feed.draws`)."""
        return train_feed.draws(self.tf, self.split, n)

    def jitter_draws(self, n: int) -> Optional[List[train_feed.JitterDraw]]:
        """The jitter draws of a batch of n examples (`train_feed.jitter_draws`), or None where the source does not jitter."""
        return train_feed.jitter_draws(self.tf, n, 2 * self.per_sample) if self.photometric else None

    def batch_panos(self, idx: np.ndarray) -> np.ndarray:
        """The distinct panoramas examples `idx` name."""
        return np.unique(np.concatenate([self.examples["i1"][idx], self.examples["i2"][idx]]))

    def __iter__(self):
        if self.examples is None:
            raise RuntimeError("set_examples first")
        # the whole epoch is planned (the generator stands where the single process's stands), then cut to this rank's rows
        plan, self._rows = train_feed.shard_plan(plan_epoch(len(self.examples["i1"]), self.batch_size, self.split, self.gen), self.rank, self.world)
        if self.pool is None:
            for b, idx in enumerate(plan):
                draws, jitter = self._shard_draws(b)
                yield self.batch(idx, draws, jitter=jitter)
        elif self.pool.prefetch:
            yield from self._iter_prefetch(plan)
        else:   # the epoch's order is known here, before its first batch: every panorama's next use, for the planner
            panos = [self.batch_panos(idx) for idx in plan]
            next_use, after = epoch_next_use(panos, self.n_panos)
            for b, idx in enumerate(plan):
                draws, jitter = self._shard_draws(b)
                out = self.batch(idx, draws, next_use, jitter=jitter)
                next_use[panos[b]] = after[b]
                yield out
        status.check(self.device, f"rendered {self.split} batches")


# ---------------------------------------------------------------------------------------------------- --render-from DIR
RENDER_DIR_FILES = ("panos_rgb.npy", "panos_depth.npy", "train.json", "val.json")
LAYOUTS_FILE = "layouts.npz"   # the optional fifth file: read only when the configuration's modalities include "layout"


def load_example_json(path: Path) -> Tuple[HypothesisTable, np.ndarray]:
    """{"i1": [N], "i2": [N], "R": [N][2][2], "t": [N][2], "is_match": [N], optional "swap": [N]} -> (table, labels)."""
    with open(path, "r") as f:
        d = json.load(f)
    missing = [k for k in ("i1", "i2", "R", "t", "is_match") if k not in d]
    if missing:
        raise SystemExit(f"{path}: missing key(s) {missing}")
    n = len(d["i1"])
    R = np.asarray(d["R"], dtype=np.float32).reshape(n, 2, 2)
    table = HypothesisTable(np.asarray(d["i1"], dtype=np.int32), np.asarray(d["i2"], dtype=np.int32), R,
                            np.asarray(d["t"], dtype=np.float32).reshape(n, 2), np.degrees(np.arctan2(R[:, 1, 0], R[:, 0, 0])).astype(np.float64),
                            np.asarray(d["swap"]).astype(bool) if d.get("swap") is not None else None)
    return table, np.asarray(d["is_match"], dtype=np.int64)


def load_render_dir(path: str, mmap: bool = False):
    """(rgb uint8 [P, H, W, 3], depth uint16 [P, H, W], {"train" | "val": (HypothesisTable, labels)}) of a --render-from directory
    (format: INTEGRATION.md).  A missing file ends the program with one line.  mmap: the two arrays are np.memmap views of their
    files (only the headers are read here) -- for `RenderedTrainSource(resident_panos=N)`, which reads a panorama when it uploads it."""
    root = Path(path)
    for name in RENDER_DIR_FILES:
        if not (root / name).is_file():
            raise SystemExit(f"--render-from {root}: {name} is missing (expected {', '.join(RENDER_DIR_FILES)})")
    mode = "r" if mmap else None
    rgb, depth = np.load(root / "panos_rgb.npy", mmap_mode=mode), np.load(root / "panos_depth.npy", mmap_mode=mode)
    if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or depth.dtype != np.uint16 or depth.shape != rgb.shape[:3]:
        raise SystemExit(f"--render-from {root}: panos_rgb.npy must be uint8 [P, H, W, 3] and panos_depth.npy uint16 [P, H, W], got "
                         f"{rgb.dtype} {rgb.shape} / {depth.dtype} {depth.shape}")
    return rgb, depth, {split: load_example_json(root / f"{split}.json") for split in SPLITS}


def load_render_layouts(path: str, n_panos: int):
    """The `layout.PanoLayouts` of a --render-from directory's optional fifth file, layouts.npz (format: INTEGRATION.md), for
    configurations whose modalities include "layout".  A missing or malformed file, or tables for another number of panoramas than
    the panorama arrays hold, ends the program with one line."""
    from salve_amd.layout import PanoLayouts

    root = Path(path)
    if not (root / LAYOUTS_FILE).is_file():
        raise SystemExit(f'--render-from {root}: {LAYOUTS_FILE} is missing (the "layout" modality needs it beside {", ".join(RENDER_DIR_FILES)})')
    try:
        layouts = PanoLayouts.load(root / LAYOUTS_FILE)
    except Exception as e:   # (a truncated or foreign file raises whatever numpy's reader raises)
        raise SystemExit(f"--render-from {root}: {LAYOUTS_FILE}: {e}") from None
    if layouts.P != n_panos:
        raise SystemExit(f"--render-from {root}: {LAYOUTS_FILE} holds the layouts of {layouts.P} panoramas, panos_rgb.npy holds {n_panos}")
    return layouts
