"""Validation / test image transform on the GPU: Resize (cv2 INTER_LINEAR, uint8) -> centre Crop -> ToTensor ->
Normalize, i.e. what salve/train_utils.py:126-159 composes from salve/utils/transform.py:256-272, 386-420, 105-123,
177-202 -- one launch of the tile kernel (salve_bev_tiles) per call instead of four numpy / cv2 passes.

The callable takes the 2 / 4 / 6 HWC uint8 images of one example (as the reference's Pair / Quadruplet / Sextuplet
transforms do) and returns as many float32 [3, crop_h, crop_w] tensors, on the GPU.  No CPU fallback.
"""

from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, status
from salve_amd.rasteriser import linear_resize_taps, normalisation_lut
from salve_amd.train_feed import JitterDraw, aug_table, jitter_table, upload_tables


class ValTestTransform:
    def __init__(self, resize_hw: Tuple[int, int], crop_hw: Tuple[int, int], device=None) -> None:
        if resize_hw[0] != resize_hw[1] or crop_hw[0] != crop_hw[1]:
            raise RuntimeError("the tile kernel resizes / crops to squares (resize_h == resize_w, train_h == train_w)")
        if crop_hw[0] > resize_hw[0]:
            raise RuntimeError("centre crop larger than the resized image (the reference would pad with the mean)")
        self.resize, self.crop = int(resize_hw[0]), int(crop_hw[0])
        self.device = device
        self._taps: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._lut = None

    def _dev(self) -> torch.device:
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("salve_amd.transforms needs the MI355X (no CPU fallback); pass transform=None to read raw tiles")
            self.device = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self.device)

    def __call__(self, *images: np.ndarray):
        dev = self._dev()
        lib = _lib.load()
        h, w = images[0].shape[:2]
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[:2] != (h, w):
                raise RuntimeError("expected equally sized HWC uint8 RGB images")
        if (h, w) not in self._taps:
            self._taps[(h, w)] = (torch.from_numpy(linear_resize_taps(self.resize, h)).to(dev),
                                  torch.from_numpy(linear_resize_taps(self.resize, w)).to(dev))
        if self._lut is None:
            self._lut = torch.from_numpy(normalisation_lut()).to(dev)
        coef_y, coef_x = self._taps[(h, w)]
        k = len(images)
        stack = np.stack(images).astype(np.uint32)
        packed = torch.from_numpy((stack[..., 0] | (stack[..., 1] << 8) | (stack[..., 2] << 16)).astype(np.int32)).to(dev)  # 0x00BBGGRR
        jobs = np.zeros(k, dtype=_lib.TILE_JOB_DTYPE)
        jobs["bev_offset"] = np.arange(k, dtype=np.int64) * (h * w)
        jobs["slot"] = np.arange(k, dtype=np.int32)
        jobs["chan"] = 0
        jobs_dev = torch.from_numpy(jobs.view(np.uint8)).to(dev)
        out = torch.empty((k, 3, self.crop, self.crop), dtype=torch.float32, device=dev)
        st = lib.salve_bev_tiles(ctypes.c_void_p(packed.data_ptr()), h, w, ctypes.c_void_p(jobs_dev.data_ptr()), k,
                                 ctypes.c_void_p(coef_y.data_ptr()), ctypes.c_void_p(coef_x.data_ptr()), self.resize, self.crop,
                                 ctypes.c_void_p(self._lut.data_ptr()), ctypes.c_void_p(out.data_ptr()), _lib.TILE_F32_NCHW, 3,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(st, "salve_bev_tiles")
        return tuple(out[i] for i in range(k))


class TrainTransform(ValTestTransform):
    """The reference's TRAIN transform (salve/train_utils.py:63-124): Resize -> Crop(crop_type="rand") -> RandomHorizontalFlip ->
    RandomVerticalFlip -> ToTensor -> Normalize, on the GPU in one launch of salve_bev_tiles_aug.  Per example ONE set of draws,
    shared by all its images, from Python's `random` in the reference's order: randint(0, h - crop_h), randint(0, w - crop_w),
    random() < 0.5 (horizontal flip), random() < 0.5 (vertical flip).  Same taps and LUT as ValTestTransform: with the centre
    offsets and no flips the tiles are bit-identical to it.

    jitter_types (default None: no photometric augmentation): the reference's PhotometricShift (salve/utils/transform.py:619-686) between
    Resize and Crop -- torchvision's ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.05) restricted to the named
    operations, every image of an example with draws of its own (`draw_jitter`), on the device (salve_bev_train_tiles_jitter, DESIGN.md
    4.23)."""

    JITTER_RANGES = {"brightness": (0.5, 1.5), "contrast": (0.5, 1.5), "saturation": (0.5, 1.5), "hue": (-0.05, 0.05)}   # in ColorJitter's fn_id order

    def __init__(self, resize_hw: Tuple[int, int], crop_hw: Tuple[int, int], device=None, jitter_types: Optional[Sequence[str]] = None) -> None:
        super().__init__(resize_hw, crop_hw, device)
        if jitter_types is not None:
            unknown = [t for t in jitter_types if t not in self.JITTER_RANGES]
            if unknown:
                raise ValueError(f"jitter_types names {unknown}; known: {tuple(self.JITTER_RANGES)}")
            if self.resize * self.resize * 255 >= 1 << 24:
                raise RuntimeError(f"photometric augmentation needs resize <= 256 (the grey sum must stay an exact float32), got {self.resize}")
        self.jitter_types = None if jitter_types is None else tuple(jitter_types)
        self._jitter_ws = {}   # workspace of `apply(jitter=)` by stream

    def draw_jitter(self, generator=None) -> JitterDraw:
        """One image's ColorJitter draw, (order, mask, brightness, contrast, saturation, hue): the calls `ColorJitter.get_params` makes,
        in its order -- torch.randperm(4), then float(torch.empty(1).uniform_(lo, hi)) for every operation in `jitter_types` -- from
        torch's global generator or `generator`.  An operation that is not named draws nothing, is masked out and keeps factor 1 (hue 0)."""
        if self.jitter_types is None:
            raise RuntimeError("this transform was built without jitter_types")
        order = tuple(int(v) for v in torch.randperm(4, generator=generator))
        mask, factors = 0, []
        for op, (name, (lo, hi)) in enumerate(self.JITTER_RANGES.items()):
            if name in self.jitter_types:
                mask |= 1 << op
                factors.append(float(torch.empty(1).uniform_(lo, hi, generator=generator)))
            else:
                factors.append(0.0 if name == "hue" else 1.0)
        return (order, mask, *factors)

    def draw(self, rng=None):
        """(crop_y, crop_x, hflip, vflip) from `rng` (default: the `random` module), in the reference's order."""
        import random as _random

        rng = _random if rng is None else rng
        h_off = rng.randint(0, self.resize - self.crop)
        w_off = rng.randint(0, self.resize - self.crop)
        hflip = rng.random() < 0.5
        vflip = rng.random() < 0.5
        return h_off, w_off, hflip, vflip

    def apply(self, images, crop_y: int, crop_x: int, hflip: bool, vflip: bool, jitter: Optional[Sequence[JitterDraw]] = None):
        """The transform with the given draws (what __call__ does after drawing).  jitter: one `draw_jitter()` per image, applied to the
        resized image in front of the crop -- the batch entry salve_bev_train_tiles_jitter with a batch of one (2, 4 or 6 images), the
        returned tensors views of its NHWC sample."""
        dev = self._dev()
        if jitter is not None:
            return self._apply_jitter(dev, images, crop_y, crop_x, hflip, vflip, jitter)
        lib = _lib.load()
        h, w = images[0].shape[:2]
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[:2] != (h, w):
                raise RuntimeError("expected equally sized HWC uint8 RGB images")
        if not (0 <= crop_y <= self.resize - self.crop and 0 <= crop_x <= self.resize - self.crop):
            raise RuntimeError(f"crop offset ({crop_y}, {crop_x}) outside [0, {self.resize - self.crop}]")
        if (h, w) not in self._taps:
            self._taps[(h, w)] = (torch.from_numpy(linear_resize_taps(self.resize, h)).to(dev),
                                  torch.from_numpy(linear_resize_taps(self.resize, w)).to(dev))
        if self._lut is None:
            self._lut = torch.from_numpy(normalisation_lut()).to(dev)
        coef_y, coef_x = self._taps[(h, w)]
        k = len(images)
        stack = np.stack(images).astype(np.uint32)
        packed = torch.from_numpy((stack[..., 0] | (stack[..., 1] << 8) | (stack[..., 2] << 16)).astype(np.int32)).to(dev)
        jobs = np.zeros(k, dtype=_lib.TILE_JOB_DTYPE)
        jobs["bev_offset"] = np.arange(k, dtype=np.int64) * (h * w)
        jobs["slot"] = np.arange(k, dtype=np.int32)
        aug = np.zeros(k, dtype=_lib.TILE_AUG_DTYPE)
        aug["crop_y"], aug["crop_x"] = crop_y, crop_x
        aug["flags"] = (_lib.TILE_HFLIP if hflip else 0) | (_lib.TILE_VFLIP if vflip else 0)
        tables = torch.from_numpy(np.concatenate([jobs.view(np.uint8), aug.view(np.uint8)])).to(dev)
        out = torch.empty((k, 3, self.crop, self.crop), dtype=torch.float32, device=dev)
        st = lib.salve_bev_tiles_aug(ctypes.c_void_p(packed.data_ptr()), h, w, ctypes.c_void_p(tables.data_ptr()),
                                     ctypes.c_void_p(tables.data_ptr() + jobs.nbytes), k, ctypes.c_void_p(coef_y.data_ptr()),
                                     ctypes.c_void_p(coef_x.data_ptr()), self.resize, self.crop, ctypes.c_void_p(self._lut.data_ptr()),
                                     ctypes.c_void_p(out.data_ptr()), 3, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(st, "salve_bev_tiles_aug")
        return tuple(out[i] for i in range(k))

    def _apply_jitter(self, dev, images, crop_y, crop_x, hflip, vflip, jitter):
        lib = _lib.load()
        k = len(images)
        h, w = images[0].shape[:2]
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[:2] != (h, w):
                raise RuntimeError("expected equally sized HWC uint8 RGB images")
        if k not in (2, 4, 6) or len(jitter) != k:
            raise RuntimeError(f"photometric augmentation takes 2, 4 or 6 images and one jitter draw per image, got {k} images and {len(jitter)} draws")
        if not (0 <= crop_y <= self.resize - self.crop and 0 <= crop_x <= self.resize - self.crop):
            raise RuntimeError(f"crop offset ({crop_y}, {crop_x}) outside [0, {self.resize - self.crop}]")
        if (h, w) not in self._taps:
            self._taps[(h, w)] = (torch.from_numpy(linear_resize_taps(self.resize, h)).to(dev),
                                  torch.from_numpy(linear_resize_taps(self.resize, w)).to(dev))
        if self._lut is None:
            self._lut = torch.from_numpy(normalisation_lut()).to(dev)
        coef_y, coef_x = self._taps[(h, w)]
        stack = np.stack(images).astype(np.uint32)
        packed = torch.from_numpy((stack[..., 0] | (stack[..., 1] << 8) | (stack[..., 2] << 16)).astype(np.int32)).to(dev)
        jobs = np.zeros(k, dtype=_lib.TILE_JOB_DTYPE)   # image i is channel group i of the one sample: even images first (table a), then the odd ones (table b)
        idx = np.concatenate([np.arange(0, k, 2), np.arange(1, k, 2)])
        jobs["bev_offset"], jobs["chan"] = idx.astype(np.int64) * (h * w), 3 * idx
        tables, off = upload_tables([jobs, aug_table([(crop_y, crop_x, hflip, vflip)]), jitter_table(jitter)], dev)
        cp = (3 * k + 7) // 8 * 8
        out = torch.empty((1, self.crop, self.crop, cp), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        need = lib.salve_bev_train_tiles_jitter_workspace_bytes(1, k // 2)
        ws = self._jitter_ws.get(stream)
        if ws is None or ws.numel() < need:
            ws = self._jitter_ws[stream] = torch.empty(need, dtype=torch.uint8, device=dev)
        p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + int(o))
        with torch.cuda.device(dev):
            st = lib.salve_bev_train_tiles_jitter(p(packed), k, p(packed), k, h, w, p(tables), p(tables, jobs.nbytes // 2), k // 2, p(tables, off[1]), 1,
                                                  p(coef_y), p(coef_x), self.resize, self.crop, p(self._lut), p(out), _lib.TILE_F32_NHWC, cp,
                                                  p(tables, off[2]), p(ws), ws.numel(), status.ptr(dev), ctypes.c_void_p(stream))
        _lib.check(st, "salve_bev_train_tiles_jitter")
        chw = out[0].permute(2, 0, 1)
        return tuple(chw[3 * i:3 * i + 3] for i in range(k))

    def __call__(self, *images: np.ndarray):
        if self.jitter_types is None:
            return self.apply(images, *self.draw())
        return self.apply(images, *self.draw(), jitter=[self.draw_jitter() for _ in images])
