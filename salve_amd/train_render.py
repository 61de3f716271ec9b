"""Training batches rendered on the GPU: panoramas, depth maps and labelled alignment hypotheses in, the trainable model's packed
input out, no JPEG hop.

The reference trains from a rendered dataset on disk: scripts/render_dataset_bev.py writes one JPEG per panorama, surface and
hypothesis, salve/dataset/zind_data.py:306-315 reads 2 / 4 of them per example, salve/train_utils.py:63-124 resizes, crops, flips and
normalises them on the host, and salve/models/early_fusion.py:52-60 concatenates them.  `RenderedTrainSource` yields the same
batches from the lossless BEV images instead: per batch one scatter + densify launch pair of the rasteriser for the posed renders
(the identity renders of every panorama are made once and kept, as in salve_amd.pipeline) and ONE salve_bev_train_tiles launch
that writes `[B, crop, crop, Cp]` in the training precision -- what `TrainableEarlyFusionCEResnet.forward_packed` takes.

Shuffle order and augmentation draws are those of `training.get_dataloader` + `transforms.TrainTransform`: the order of a
`DataLoader(shuffle=True, generator=<seeded>)`, one `TrainTransform.draw()` per example in batch order from Python's `random`.
The planning functions (`plan_epoch`, `plan_examples`, `check_launch`) are pure and need no device.
"""

from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, status, tracing
from salve_amd.pipeline import surfaces_for
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses
from salve_amd.synthetic import HypothesisTable
from salve_amd.transforms import TrainTransform

MAX_RENDERS_PER_CALL = 65535   # include/salve_hip.h: renders per scatter / densify call
SPLITS = ("train", "val")


def plan_epoch(n: int, batch: int, split: str, gen: Optional[torch.Generator] = None) -> List[np.ndarray]:
    """Example indices of every batch of one epoch.  "train": the order `training.get_dataloader` gives its examples -- a
    DataLoader(shuffle=True, generator=gen, drop_last=True) over the indices themselves, so that every draw the loader and its
    sampler take from `gen` is taken here too -- the last partial batch dropped.  "val": table order, nothing dropped."""
    if split not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
    if batch <= 0:
        raise ValueError(f"batch size must be positive, got {batch}")
    if split == "val":
        return [np.arange(lo, min(lo + batch, n), dtype=np.int64) for lo in range(0, n, batch)]
    if gen is None:
        raise ValueError('plan_epoch(split="train") needs the seeded torch.Generator')
    if n == 0:
        return []
    loader = torch.utils.data.DataLoader(range(n), batch_size=batch, shuffle=True, generator=gen, num_workers=0, drop_last=True)
    return [b.numpy().astype(np.int64) for b in loader]


def batches_per_epoch(n: int, batch: int, split: str) -> int:
    return n // batch if split == "train" else (n + batch - 1) // batch


def check_launch(batch_size: int, n_surfaces: int) -> None:
    """A batch's posed renders go through ONE scatter / densify call."""
    if batch_size <= 0:
        raise ValueError(f"batch size must be positive, got {batch_size}")
    if batch_size * n_surfaces > MAX_RENDERS_PER_CALL:
        raise RuntimeError(f"batch_size {batch_size} x {n_surfaces} surfaces = {batch_size * n_surfaces} renders per batch; the library "
                           f"takes at most {MAX_RENDERS_PER_CALL} per call")


def train_surfaces(modalities: Sequence[str]) -> List[str]:
    if "layout" in set(modalities):
        raise RuntimeError('RenderedTrainSource does not render the "layout" modality (floor, ceiling, ceiling + floor only): train it from '
                           "the rendered dataset on disk")
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


class RenderedTrainSource:
    """Iterating yields `(x_packed, is_match)`: x_packed [B, crop, crop, Cp] float32 / bfloat16 on the device, is_match int64 [B, 1].
    One epoch per iteration; `len()` = batches per epoch.  Everything runs on the current stream.  The device status word is checked
    once per epoch, after the last batch (a bad render row or tile job raises there)."""

    def __init__(self, device, modalities: Sequence[str], pano_hw: Tuple[int, int] = (512, 1024), batch_size: int = 256,
                 precision: str = "fp32", split: str = "train", seed: int = 0, resize_hw: Tuple[int, int] = (234, 234),
                 crop_hw: Tuple[int, int] = (224, 224)) -> None:
        if split not in SPLITS:
            raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        self.surfaces = train_surfaces(modalities)
        check_launch(batch_size, len(self.surfaces))
        self.tf = TrainTransform(resize_hw, crop_hw)   # the draws (and the square / no-padding refusals); its kernels are not used
        self.split, self.batch_size = split, int(batch_size)
        self.dtype = torch.bfloat16 if precision == "bf16" else torch.float32
        self.out_c = (6 * len(self.surfaces) + 7) // 8 * 8
        self.gen = torch.Generator()
        self.gen.manual_seed(seed)
        self.device = torch.device(device)
        # (a bit an earlier, unchecked caller left in the device's status word is reported as ITS failure, not as this source's)
        status.check(self.device, "a launch issued before this RenderedTrainSource was created")
        self.ras = BevRasteriser(self.device, pano_hw=pano_hw, resize=self.tf.resize, crop=self.tf.crop)
        self.pano_rgb = self.pano_depth = self.ref_bev = self.bev = None
        self.n_panos: Optional[int] = None
        self.examples: Optional[Dict[str, np.ndarray]] = None
        self.timers = None   # a list: every launch appends (tag, start event, end event) -- tools/measure/bench_train_feed.py

    # ------------------------------------------------------------------ panoramas
    def _refuse_if_too_large(self, need: int, what: str) -> None:
        free = int(torch.cuda.mem_get_info(self.device)[0])
        if need > free:
            raise RuntimeError(f"{what} need {need} bytes of device memory, {free} are free: panorama sets that do not fit at once are not supported")

    def load_panos(self, rgb: np.ndarray, depth: np.ndarray) -> None:
        """Upload P panoramas (uint8 [P, H, W, 3], uint16 [P, H, W]) and render their identity BEV images."""
        self._refuse_if_too_large(int(rgb.nbytes) + int(depth.nbytes), f"{len(rgb)} panoramas")
        self.set_panos(*self.ras.upload_panos(rgb, depth))

    def set_panos(self, rgb_dev: torch.Tensor, depth_dev: torch.Tensor) -> None:
        """Panoramas on the device (as RenderVerifyPipeline.set_panos takes them); the identity render of every panorama and
        surface is made once and kept."""
        if tuple(rgb_dev.shape[1:3]) != tuple(self.ras.pano_hw) or tuple(depth_dev.shape[1:]) != tuple(self.ras.pano_hw):
            raise RuntimeError(f"panoramas must be {self.ras.pano_hw}, got {tuple(rgb_dev.shape[1:3])} / {tuple(depth_dev.shape[1:])}")
        P, S = int(rgb_dev.shape[0]), len(self.surfaces)
        Hb, Wb = self.ras.bev_hw
        self._refuse_if_too_large((P + self.batch_size) * S * Hb * Wb * 4, f"the BEV images of {P} panoramas and one batch")
        self.pano_rgb, self.pano_depth = rgb_dev.contiguous(), depth_dev.contiguous()
        self.n_panos, self.examples = P, None
        rows = pack_hypotheses(np.repeat(np.arange(P), S), np.tile([SURFACES[s] for s in self.surfaces], P),
                               np.tile(np.eye(2, dtype=np.float32), (P * S, 1, 1)), np.zeros((P * S, 2), np.float32), np.zeros(P * S))
        rows_dev = self.ras.upload_hypotheses(rows)
        self.ref_bev = torch.empty((P * S, Hb, Wb), dtype=torch.int32, device=self.device)
        with tracing.range("salve.identity_renders"):
            for lo in range(0, P * S, 256):
                n = min(256, P * S - lo)
                self.ras.render(self.pano_rgb, self.pano_depth, rows_dev[lo * _lib.HYP_DTYPE.itemsize:], n, self.ref_bev[lo:lo + n])
        self.bev = torch.empty((self.batch_size * S, Hb, Wb), dtype=torch.int32, device=self.device)   # one batch's posed renders

    def share_panos(self, other: "RenderedTrainSource") -> None:
        """Use the panoramas, identity renders and batch buffer `other` holds (the val source beside the train source: one copy on
        the device; both run on the same stream, one batch at a time)."""
        if other.n_panos is None:
            raise RuntimeError("the other source has no panoramas yet")
        if (other.device, other.surfaces, other.ras.pano_hw, other.ras.bev_hw) != (self.device, self.surfaces, self.ras.pano_hw, self.ras.bev_hw) \
                or other.batch_size < self.batch_size:
            raise RuntimeError("share_panos needs the same device, modalities and panorama size, and a batch size not above the other's")
        self.pano_rgb, self.pano_depth, self.ref_bev, self.bev, self.n_panos, self.examples = (other.pano_rgb, other.pano_depth, other.ref_bev,
                                                                                               other.bev, other.n_panos, None)

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
    def _timed(self, tag: str):
        if self.timers is None:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.timers.append((tag, e0, e1))
        e0.record()
        return e1

    def batch(self, idx: np.ndarray, draws: Sequence[Tuple[int, int, bool, bool]]) -> Tuple[torch.Tensor, torch.Tensor]:
        """Render examples `idx` with one draw (crop_y, crop_x, hflip, vflip) each: (x_packed, is_match)."""
        ex, S, B = self.examples, len(self.surfaces), len(idx)
        Hb, Wb = self.ras.bev_hw
        i1 = ex["i1"][idx]
        # renders in the order of their panorama (as RenderVerifyPipeline.prepare issues them: the workgroups of one panorama run
        # side by side and share its depth blocks through the L2s); the tile jobs name each sample's render by its rank
        order = np.argsort(i1, kind="stable")
        rank = np.empty(B, dtype=np.int64)
        rank[order] = np.arange(B)
        src = idx[order]
        rows = pack_hypotheses(np.repeat(ex["i1"][src], S), np.tile([SURFACES[s] for s in self.surfaces], B), np.repeat(ex["R"][src], S, axis=0),
                               np.repeat(ex["t"][src], S, axis=0), np.ones(B * S))
        si = np.tile(np.arange(S, dtype=np.int64), B)
        smp = np.repeat(np.arange(B, dtype=np.int64), S)
        swap = np.repeat(ex["swap"][idx], S)
        jobs = np.zeros((2, B * S), dtype=_lib.TILE_JOB_DTYPE)   # sample-major [B][S]: posed renders of this batch | identity renders
        jobs["bev_offset"][0] = (np.repeat(rank, S) * S + si) * (Hb * Wb)
        jobs["bev_offset"][1] = (np.repeat(ex["i2"][idx], S) * S + si) * (Hb * Wb)
        jobs["slot"][:] = smp
        jobs["chan"][0] = 6 * si + 3 * swap
        jobs["chan"][1] = 6 * si + 3 * (1 - swap)
        aug = np.zeros(B, dtype=_lib.TILE_AUG_DTYPE)
        for k, (cy, cx, hflip, vflip) in enumerate(draws):
            aug[k] = (cy, cx, (_lib.TILE_HFLIP if hflip else 0) | (_lib.TILE_VFLIP if vflip else 0), 0)
        # ONE upload per batch; every table starts on a multiple of 16 bytes (the 40-byte render rows come last)
        parts = [jobs.view(np.uint8).reshape(-1), aug.view(np.uint8), ex["is_match"][idx].view(np.uint8), rows.view(np.uint8)]
        buf = torch.from_numpy(np.concatenate(parts)).to(self.device)
        o = np.cumsum([0] + [p.nbytes for p in parts])
        jobs_a, jobs_b = buf[:o[1] // 2], buf[o[1] // 2:o[1]]
        labels = buf[o[2]:o[3]].view(torch.int64).view(B, 1)
        e1 = self._timed("scatter")
        with tracing.range("salve.scatter"):
            self.ras.scatter(self.pano_rgb, self.pano_depth, buf[o[3]:], B * S, self.bev)
        if e1 is not None:
            e1.record()
        e1 = self._timed("densify")
        with tracing.range("salve.densify"):
            self.ras.densify(B * S, self.bev)
        if e1 is not None:
            e1.record()
        out = torch.empty((B, self.ras.crop, self.ras.crop, self.out_c), dtype=self.dtype, device=self.device)
        e1 = self._timed("tiles")
        with tracing.range("salve.train_tiles"):
            self.ras.train_tiles(self.bev, self.ref_bev, jobs_a, jobs_b, S, buf[o[1]:o[2]], B, out)
        if e1 is not None:
            e1.record()
        return out, labels

    def draws(self, n: int) -> List[Tuple[int, int, bool, bool]]:
        """train: `TrainTransform.draw()` per example, from Python's `random`; val: the centre crop, no flips (ValTestTransform)."""
        if self.split == "train":
            return [self.tf.draw() for _ in range(n)]
        off = (self.tf.resize - self.tf.crop) // 2
        return [(off, off, False, False)] * n

    def __iter__(self):
        if self.examples is None:
            raise RuntimeError("set_examples first")
        for idx in plan_epoch(len(self.examples["i1"]), self.batch_size, self.split, self.gen):
            yield self.batch(idx, self.draws(len(idx)))
        status.check(self.device, f"rendered {self.split} batches")


# ---------------------------------------------------------------------------------------------------- --render-from DIR
RENDER_DIR_FILES = ("panos_rgb.npy", "panos_depth.npy", "train.json", "val.json")


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


def load_render_dir(path: str):
    """(rgb uint8 [P, H, W, 3], depth uint16 [P, H, W], {"train" | "val": (HypothesisTable, labels)}) of a --render-from directory
    (format: INTEGRATION.md).  A missing file ends the program with one line."""
    root = Path(path)
    for name in RENDER_DIR_FILES:
        if not (root / name).is_file():
            raise SystemExit(f"--render-from {root}: {name} is missing (expected {', '.join(RENDER_DIR_FILES)})")
    rgb, depth = np.load(root / "panos_rgb.npy"), np.load(root / "panos_depth.npy")
    if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or depth.dtype != np.uint16 or depth.shape != rgb.shape[:3]:
        raise SystemExit(f"--render-from {root}: panos_rgb.npy must be uint8 [P, H, W, 3] and panos_depth.npy uint16 [P, H, W], got "
                         f"{rgb.dtype} {rgb.shape} / {depth.dtype} {depth.shape}")
    return rgb, depth, {split: load_example_json(root / f"{split}.json") for split in SPLITS}
