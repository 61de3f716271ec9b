"""The case table and the emulator of the JPEG decoder's samplings beyond 4:2:0 (4:2:2, 4:4:4, greyscale), shared by
tests/test_jpeg_sampling_host.py (parse_file(samplings=); emulator == Pillow; the host build of the two entropy decoders == emulator;
the wrong decoders fail) and tests/test_gpu_jpeg_sampling.py (BevRasteriser.jpeg_decode(sampling=) == Pillow).

`cases()` names (sampling, case) pairs; `file_of(sampling, case)` makes the file with Pillow (once per process).
`decode` is tests/jpeg_decode_cases.py's `decode` with the MCU's block pattern as an argument: blocks per MCU, the component of each
slot, a DC predictor per component; `reference_levels` runs it a restart interval at a time.  `pixels` is its `pixels` likewise:
tests/jpeg_cases.py's dequantisation, inverse DCT and colour conversion around the sampling's own plane layout and upsampling --
jdsample.c's h2v1_fancy_upsample for 4:2:2, none for 4:4:4, no colour conversion for greyscale.  `mutant=` switches one rule to a
plausible wrong variant.  `malformed(sampling)` is the ONE set of hostile inputs: the host program passes them under the sanitizers
before the GPU tests feed the same bytes to the device.
"""

from __future__ import annotations

import io
from typing import Dict, List, Optional, Tuple

import numpy as np

import jpeg_cases as jc
import jpeg_decode_cases as dc
from salve_amd import jpeg

SAMPLINGS = jpeg.SAMPLINGS
PILLOW_SUBSAMPLING = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}            # Pillow's save(subsampling=); "grey": one channel as mode L
LUMA_BLOCKS = {"4:2:0": (2, 2), "4:2:2": (1, 2), "4:4:4": (1, 1), "grey": (1, 1)}   # luma blocks of an MCU: down, across
MUTANTS = ("h2v2_for_422", "rounding_swapped", "no_replication", "order_y_cb_y_cr", "dc_shared_by_chroma", "grey_mcus_of_16")

# name -> (h, w, content, Pillow save arguments): what each covers is in the table of the module docstring of test_jpeg_sampling_host.py
CASES: Dict[str, Tuple[int, int, str, dict]] = {
    "8x8": (8, 8, "noise", dict(quality=75)),
    "8x16": (8, 16, "noise", dict(quality=75)),
    "5x3": (5, 3, "noise", dict(quality=75)),
    "7x4": (7, 4, "noise", dict(quality=75)),
    "8x5": (8, 5, "noise", dict(quality=75)),
    "9x17": (9, 17, "noise", dict(quality=75)),
    "33x47": (33, 47, "noise", dict(quality=75)),
    "24x40_disc": (24, 40, "disc", dict(quality=75)),
    "24x40_noise": (24, 40, "noise", dict(quality=75)),
    "24x40_disc_q30": (24, 40, "disc", dict(quality=30)),
    "24x40_noise_q30": (24, 40, "noise", dict(quality=30)),
    "24x40_noise_q95": (24, 40, "noise", dict(quality=95)),
    "24x40_noise_q100": (24, 40, "noise", dict(quality=100)),
    "24x40_optimised": (24, 40, "noise", dict(quality=75, optimize=True)),
    "restart_blocks1": (33, 47, "noise", dict(quality=75, restart_marker_blocks=1)),
    "restart_blocks3": (33, 47, "noise", dict(quality=75, restart_marker_blocks=3)),
    "restart_rows1": (33, 47, "noise", dict(quality=75, restart_marker_rows=1)),
    "lanes_48x64": (48, 64, "noise", dict(quality=95)),
    "pano_128x256": (128, 256, "layout", dict(quality=75)),
}
RESTART_CASES = ("restart_blocks1", "restart_blocks3", "restart_rows1")
MALFORMED_CASE = "lanes_48x64"      # the file `malformed` cuts its inputs from

_FILES: Dict[Tuple[str, str], bytes] = {}
_PILLOW: Dict[Tuple[str, str], np.ndarray] = {}


def cases() -> List[Tuple[str, str]]:
    return [(s, name) for s in SAMPLINGS for name in CASES]


def pillow_file(rgb: np.ndarray, sampling: str, **save) -> bytes:
    """An RGB image as a JPEG file of `sampling` ("grey": its first channel, as mode L)."""
    from PIL import Image

    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(rgb[..., 0]).save(buf, format="JPEG", **save)
    else:
        Image.fromarray(rgb).save(buf, format="JPEG", subsampling=PILLOW_SUBSAMPLING[sampling], **save)
    return buf.getvalue()


def file_of(sampling: str, name: str) -> bytes:
    if (sampling, name) not in _FILES:
        h, w, content, save = CASES[name]
        _FILES[sampling, name] = pillow_file(jc.make_image(content, h, w), sampling, **save)
    return _FILES[sampling, name]


def pillow_rgb3(data: bytes) -> np.ndarray:
    """What ingest._read_rgb3 makes of a file: Pillow's pixels, mode L repeated into three channels."""
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        a = np.asarray(im).copy()
    return np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else a


def pillow_reference(sampling: str, name: str) -> np.ndarray:
    """Pillow's pixels of a case, computed once per process and shared (read only)."""
    if (sampling, name) not in _PILLOW:
        _PILLOW[sampling, name] = pillow_rgb3(file_of(sampling, name))
        _PILLOW[sampling, name].setflags(write=False)
    return _PILLOW[sampling, name]


def parse(data: bytes) -> jpeg.ParsedFile:
    return jpeg.parse_file(data, restart=True, samplings=SAMPLINGS)


# ---------------------------------------------------------------------------------------------------- the entropy decoder
def slot_components(sampling: str, mutant: Optional[str] = None) -> List[int]:
    """The component (0 Y, 1 Cb, 2 Cr) of each block slot of the MCU, in the scan's order."""
    if sampling == "grey":
        return [0]
    if sampling == "4:2:2" and mutant == "order_y_cb_y_cr":
        return [0, 1, 0, 2]
    down, across = LUMA_BLOCKS[sampling]
    return [0] * (down * across) + [1, 2]


def decode(scan: bytes, huffman: np.ndarray, mcus: int, sampling: str, mutant: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """One segment (the DC predictors start at 0) -> (levels [mcus, blocks per MCU, 64] in natural order, SALVE_JPEG_* status).
    jpeg_decode_cases.decode's rules; a failing scan keeps what it had decoded."""
    comps = slot_components(sampling, mutant)
    tables = [dc._decoder_table(np.asarray(huffman[t])) for t in range(4)]
    data, status = dc._unstuff(bytes(scan), False)
    bits = dc._Bits(data)
    out = np.zeros((mcus, len(comps), 64), dtype=np.int64)
    zigzag = jpeg.ZIGZAG.tolist()

    def value(size: int) -> int:
        v = bits.take(size)
        return v + (-1 << size) + 1 if size and v < (1 << (size - 1)) else v

    def block(dst: np.ndarray, comp: int, pred: List[int]) -> int:
        t = 0 if comp == 0 else 2
        size = bits.symbol(tables[t])
        if size < 0:
            return dc.BAD_CODE
        if size > 11:
            return dc.DC_RANGE
        which = 1 if (comp and mutant == "dc_shared_by_chroma") else comp
        v = pred[which] + value(size)
        if bits.at > bits.total:
            return dc.TRUNCATED
        if not -2047 <= v <= 2047:
            return dc.DC_RANGE
        pred[which] = v
        dst[0] = v
        k = 1
        while k < 64:
            rs = bits.symbol(tables[t + 1])
            if rs < 0:
                return dc.BAD_CODE
            run, size = rs >> 4, rs & 15
            if size == 0:
                if bits.at > bits.total:
                    return dc.TRUNCATED
                if run != 15:
                    break
                k += 16
                if k > 64:
                    return dc.COEF_OVERRUN
                continue
            k += run
            if k > 63:
                return dc.COEF_OVERRUN
            v = value(size)
            if bits.at > bits.total:
                return dc.TRUNCATED
            dst[zigzag[k]] = v
            k += 1
        return 0

    pred = [0, 0, 0]
    for m in range(mcus):
        for b, comp in enumerate(comps):
            if status & ~dc.MARKER or (status and bits.at >= bits.total):
                return out, status
            status |= block(out[m, b], comp, pred)
    if not status:
        left = bits.total - bits.at
        if left > 7 or bits.take(left) != (1 << left) - 1:
            status |= dc.LEFTOVER
    return out, status


def mcu_grid(p: jpeg.ParsedFile, mutant: Optional[str] = None) -> Tuple[int, int]:
    if p.sampling == "grey" and mutant == "grey_mcus_of_16":
        return jpeg.mcu_grid(p.h, p.w, "4:2:0")
    return jpeg.mcu_grid(p.h, p.w, p.sampling)


def reference_levels(data: bytes, mutant: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """A whole file, one restart interval at a time -> (levels [MCUs, blocks per MCU, 64], status)."""
    p = parse(data)
    mh, mw = mcu_grid(p, mutant)
    out = np.zeros((mh * mw, jpeg.MCU_BLOCKS[p.sampling], 64), dtype=np.int64)
    status = 0
    for off, nb, first, count in p.segments:
        count = max(0, min(count, mh * mw - first))          # (only a wrong MCU count cuts here)
        levels, st = decode(data[off:off + nb], p.huffman, count, p.sampling, mutant)
        out[first:first + count] = levels
        status |= st
    return out, status


# ---------------------------------------------------------------------------------------------------- the inverse chain
def upsample_h2v1(c: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """jdsample.c: h2v1_fancy_upsample, per row: 3/4 of the nearer and 1/4 of the further sample, + 1 to the left and + 2 to the right,
    the row's two end pixels copied; a component of at most two samples a row is replicated (h2v1_upsample)."""
    c = c.astype(np.int64)
    cw = c.shape[1]
    out = np.repeat(c, 2, axis=1)
    if cw <= 2 and mutant != "no_replication":
        return out
    left, right = (2, 1) if mutant == "rounding_swapped" else (1, 2)
    out[:, 2::2] = (3 * c[:, 1:] + c[:, :-1] + left) >> 2
    out[:, 1:-1:2] = (3 * c[:, :-1] + c[:, 1:] + right) >> 2
    return out


def pixels(levels: np.ndarray, qtab: np.ndarray, h: int, w: int, sampling: str, mutant: Optional[str] = None) -> np.ndarray:
    """Quantised levels [MCUs, blocks per MCU, 64] -> uint8 [h, w, 3]: dequantise, jpeg_idct_islow, the sampling's upsampling, YCbCr ->
    RGB; greyscale: Y in all three channels."""
    mh, mw = jpeg.mcu_grid(h, w, sampling)
    levels = np.asarray(levels).reshape(mh, mw, -1, 64)
    q = np.asarray(qtab, dtype=np.int64)
    comps = slot_components(sampling, mutant)
    down, across = LUMA_BLOCKS[sampling]
    luma = np.zeros((down * mh, across * mw, 8, 8), dtype=np.int64)
    for j, k in enumerate(i for i, c in enumerate(comps) if c == 0):
        luma[j // across::down, j % across::across] = jc.idct_islow((levels[:, :, k] * q[0]).reshape(mh, mw, 8, 8))
    y = jc._unblocks(luma)[:h, :w]
    if sampling == "grey":
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    planes = []
    for comp in (1, 2):
        small = jc._unblocks(jc.idct_islow((levels[:, :, comps.index(comp)] * q[1]).reshape(mh, mw, 8, 8)))
        if sampling == "4:4:4":
            planes.append(small[:h, :w])
        elif sampling == "4:2:2" and mutant != "h2v2_for_422":
            planes.append(upsample_h2v1(small[:h, :(w + 1) // 2], mutant)[:, :w])
        elif sampling == "4:2:2":                              # the vertical triangle filter as well: each row blended with the one below
            planes.append(jc.upsample_h2v2(small[:h, :(w + 1) // 2])[1::2, :w])
        else:
            planes.append(jc.upsample_h2v2(small[:(h + 1) // 2, :(w + 1) // 2])[:h, :w])
    return jc.ycc_to_rgb(y, planes[0], planes[1])


def decode_file(data: bytes, mutant: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """A whole file -> (pixels uint8 [h, w, 3], status)."""
    p = parse(data)
    levels, status = reference_levels(data, mutant)
    if mutant == "grey_mcus_of_16" and p.sampling == "grey":      # its few blocks, laid out as that decoder believes
        mh, mw = jpeg.mcu_grid(p.h, p.w, "grey")
        full = np.zeros((mh * mw, 1, 64), dtype=np.int64)
        full[:min(len(levels), mh * mw)] = levels[:mh * mw]
        levels = full
    return pixels(levels, p.qtab, p.h, p.w, p.sampling, mutant), status


# ---------------------------------------------------------------------------------------------------- malformed inputs
def malformed(sampling: str) -> List[Tuple[str, bytes, List[Tuple[int, int, int, int, int]]]]:
    """[(name, scan buffer, segment rows (offset, bytes, image 0, first MCU, MCUs))] cut from the sampling's 48 x 64 noise file: the
    scan cut in half, its last 40 bytes replaced by seeded noise, and a segment table whose MCU range passes the image."""
    data = file_of(sampling, MALFORMED_CASE)
    p = parse(data)
    scan = data[p.scan_offset:p.scan_offset + p.scan_bytes]
    mcus = int(np.prod(jpeg.mcu_grid(p.h, p.w, sampling)))
    noise = np.random.RandomState(11 + SAMPLINGS.index(sampling)).randint(0, 256, size=40).astype(np.uint8).tobytes()
    return [("cut_in_half", scan[:len(scan) // 2], [(0, len(scan) // 2, 0, 0, mcus)]),
            ("noise_tail", scan[:-40] + noise, [(0, len(scan), 0, 0, mcus)]),
            ("mcu_range_passes_image", scan, [(0, len(scan), 0, 1, mcus)])]
