"""What the two training feeds share (salve_amd.train_render.RenderedTrainSource, salve_amd.train_files.TileFileSource): the epoch's
order, the augmentation draws and their table, the one upload of a batch's host tables, and the refusals of the arguments both take.
Shuffle order and draws are those of `training.get_dataloader` + `transforms.TrainTransform`: the order of a
`DataLoader(shuffle=True, generator=<seeded>)`, one `TrainTransform.draw()` per example in batch order from Python's `random` -- and,
where the photometric augmentation is on (`photometric="device"`), one `TrainTransform.draw_jitter()` per image from
torch's global generator, with the record table that carries them.  Nothing here needs a device."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib

SPLITS = ("train", "val")   # the orders `plan_epoch` knows; a source may name more splits and map them onto these

Draw = Tuple[int, int, bool, bool]   # (crop_y, crop_x, hflip, vflip)
JitterDraw = Tuple[Tuple[int, int, int, int], int, float, float, float, float]   # (order, mask, brightness, contrast, saturation, hue) of ONE image


def check_arguments(batch_size: int, split: Optional[str] = None, splits: Sequence[str] = SPLITS, precision: Optional[str] = None) -> None:
    """The refusals the sources share; `splits`: the caller's own tuple.  None: the caller takes no such argument."""
    if split is not None and split not in splits:
        raise ValueError(f"split must be one of {tuple(splits)}, got {split!r}")
    if precision is not None and precision not in ("fp32", "bf16"):
        raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
    if int(batch_size) <= 0:
        raise ValueError(f"batch size must be positive, got {batch_size}")


def plan_epoch(n: int, batch: int, split: str, gen: Optional[torch.Generator] = None) -> List[np.ndarray]:
    """Example indices of every batch of one epoch.  "train": the order `training.get_dataloader` gives its examples -- a
    DataLoader(shuffle=True, generator=gen, drop_last=True) over the indices themselves, so that every draw the loader and its
    sampler take from `gen` is taken here too -- the last partial batch dropped.  "val": table order, nothing dropped."""
    check_arguments(batch, split)
    if split == "val":
        return [np.arange(lo, min(lo + batch, n), dtype=np.int64) for lo in range(0, n, batch)]
    if gen is None:
        raise ValueError('plan_epoch(split="train") needs the seeded torch.Generator')
    if n == 0:
        return []
    loader = torch.utils.data.DataLoader(range(n), batch_size=batch, shuffle=True, generator=gen, num_workers=0, drop_last=True)
    return [b.numpy().astype(np.int64) for b in loader]


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Rows [lo, hi) of an n-row batch that rank `rank` of `world` data-parallel ranks trains: the contiguous block split of
    `HypothesisTable.shard_bounds` (sizes differ by at most one; a short batch may leave a rank nothing)."""
    from salve_amd.synthetic import HypothesisTable

    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of a world of {world}")
    return HypothesisTable.shard_bounds(int(n), int(rank), int(world))


def check_shard(batch_size: int, split: str, rank: int, world: int) -> None:
    """The refusals of the feeds' `rank` / `world` keywords: a train batch must split into equal blocks (every rank steps on the
    same number of rows, and the mean of the ranks' gradients is the batch's); val batches split as they come."""
    shard_bounds(0, rank, world)
    if split == "train" and int(batch_size) % int(world) != 0:
        raise ValueError(f"batch size {batch_size} is not a multiple of the {world} data-parallel ranks: the train batch is split into equal blocks")


def shard_plan(plan: Sequence[np.ndarray], rank: int, world: int) -> Tuple[List[np.ndarray], List[Tuple[int, int, int]]]:
    """An epoch's plan as rank `rank` sees it, sliced directly behind `plan_epoch`: (the rank's rows of every batch that leaves it
    any, (rows of the whole batch, lo, hi) of each such batch).  Whoever plans ahead -- the resident pool, the file reader -- then
    plans for this rank's rows only.  A batch that leaves the rank no row (a short last val batch) is left out: val takes no draw
    from a generator, so no stream falls out of step."""
    if world == 1:
        return list(plan), [(len(idx), 0, len(idx)) for idx in plan]
    mine, rows = [], []
    for idx in plan:
        lo, hi = shard_bounds(len(idx), rank, world)
        if hi > lo:
            mine.append(idx[lo:hi])
            rows.append((len(idx), lo, hi))
    return mine, rows


def shard_draws(draws: Sequence[Draw], jitter: Optional[Sequence[JitterDraw]], images_per_example: int, lo: int, hi: int):
    """Rows [lo, hi) of a whole batch's draws and of its jitter draws (per image: `images_per_example` consecutive ones per row).
    The whole batch's draws were taken, so the generators stand where the single process's stand."""
    return list(draws[lo:hi]), None if jitter is None else list(jitter[lo * images_per_example:hi * images_per_example])


def batches_per_epoch(n: int, batch: int, split: str) -> int:
    return n // batch if split == "train" else (n + batch - 1) // batch


def draws(tf, split: str, n: int) -> List[Draw]:
    """train: `TrainTransform.draw()` per example, from Python's `random`; every other split: the centre crop, no flips
    (ValTestTransform)."""
    if split == "train":
        return [tf.draw() for _ in range(n)]
    off = (tf.resize - tf.crop) // 2
    return [(off, off, False, False)] * n


def aug_table(draws: Sequence[Draw]) -> np.ndarray:
    """salve_tile_aug_t rows of a batch's draws: TILE_AUG_DTYPE [B]."""
    aug = np.zeros(len(draws), dtype=_lib.TILE_AUG_DTYPE)
    for k, (cy, cx, hflip, vflip) in enumerate(draws):
        aug[k] = (cy, cx, (_lib.TILE_HFLIP if hflip else 0) | (_lib.TILE_VFLIP if vflip else 0), 0)
    return aug


PHOTOMETRICS = (None, "device")   # the `photometric=` keyword of the feeds and of `training`: it permits, the config's field decides
JITTER_TYPES = ("brightness", "contrast", "saturation", "hue")   # what the reference's train transform names (salve/train_utils.py:110-111)


def check_photometric(photometric: Optional[str]) -> None:
    if photometric not in PHOTOMETRICS:
        raise ValueError(f"photometric must be one of {PHOTOMETRICS}, got {photometric!r}")


def jitter_draws(tf, n_examples: int, images_per_example: int, generator=None) -> List[JitterDraw]:
    """`TrainTransform.draw_jitter()` per image, example by example in batch order, an example's images in x1 .. x6 order: the draws
    the DataLoader path takes from torch's generator, flattened [n_examples * images_per_example]."""
    return [tf.draw_jitter(generator) for _ in range(n_examples * images_per_example)]


def jitter_table(draws: Sequence[JitterDraw]) -> np.ndarray:
    """salve_tile_jitter_t rows of the images' draws: TILE_JITTER_DTYPE [len(draws)].  The complements 1 - f are formed in double and
    rounded once, as torchvision's _blend forms them."""
    t = np.zeros(len(draws), dtype=_lib.TILE_JITTER_DTYPE)
    for k, (order, mask, b, c, s, h) in enumerate(draws):
        t[k] = (order, mask, b, c, s, h, *(np.float32(1.0 - float(f)) for f in (b, c, s)), 0)
    return t


def upload_tables(parts: Sequence[np.ndarray], device) -> Tuple[torch.Tensor, np.ndarray]:
    """A batch's host tables in ONE upload: (uint8 buffer on `device` holding them one behind the other, byte offsets [len(parts) + 1]);
    table k is buf[offsets[k]:offsets[k + 1]].  Nothing is padded: the caller orders the tables so that each starts where its rows
    may start."""
    raw = [np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts]
    return torch.from_numpy(np.concatenate(raw)).to(device), np.cumsum([0] + [r.nbytes for r in raw])
