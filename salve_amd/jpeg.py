"""The quantisation tables of the reference's JPEG hop.

The reference writes every BEV render with `imageio.imwrite(path.jpg, img)` (bev_rendering_utils.py:629-630) -- Pillow's encoder
over libjpeg at quality 75, baseline, 4:2:0 -- and reads the file back (zind_data.py:306-315).  `BevRasteriser.jpeg_roundtrip`
reproduces decode(encode(img)) on the device (salve_amd/csrc/jpeg_roundtrip.hip); the tables it divides by come from here.
Pure host arithmetic, no device.
"""

from __future__ import annotations

import numpy as np

# ITU-T T.81 Annex K tables 1 and 2 in natural (row-major) order: what libjpeg's jpeg_set_defaults installs
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
STD_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)


def quality_scaling(quality: int) -> int:
    """libjpeg's jpeg_quality_scaling: quality clamped to 1..100, below 50 -> 5000 / q, from 50 -> 200 - 2 q (per cent)."""
    q = min(max(int(quality), 1), 100)
    return 5000 // q if q < 50 else 200 - 2 * q


def quality_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64] (luma, chroma; natural order): libjpeg's jpeg_set_quality(quality, force_baseline=TRUE) of the standard
    tables -- (entry * scale + 50) / 100, clamped to 1..255 -- i.e. the tables of Pillow's `save(path, quality=quality)`."""
    scale = quality_scaling(quality)
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]).astype(np.uint16)
