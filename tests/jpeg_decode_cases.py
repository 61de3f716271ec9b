"""The JPEG entropy DEcoder's emulator, shared by tests/test_jpeg_decode_host.py (emulator == the coder's coefficients == Pillow's
pixels; the host build of salve_amd/csrc/jpeg_entropy.h == emulator) and tests/test_gpu_jpeg_decode.py (salve_bev_jpeg_decode ==
Pillow).

`decode(scan, huffman, mh, mw)` is ITU-T T.81 Annex F.2.2 over one interleaved 4:2:0 scan without restart intervals: the 0x00 behind
every 0xFF dropped (B.1.1.5), Huffman decoding by the maxcode walk of F.2.2.3 straight from BITS / HUFFVAL, DC category plus value
bits with the EXTEND rule and a predictor per component across the whole scan, (run, size) symbols with ZRL and EOB in zigzag order.
It returns the quantised levels [MCU rows, MCUs across, 6, 64] in natural order (the layout of jpeg_coder_cases.quantised_mcus) and a
status word with the bits of include/salve_hip.h's SALVE_JPEG_*.  A failing scan keeps what it had decoded; the rest is zero.
`pixels` takes the levels through tests/jpeg_cases.py's inverse chain.  `mutant=` switches one rule to a plausible wrong variant; the
host test shows that the case table tells each from the real decoder.
"""

from __future__ import annotations

import io
from typing import List, Optional, Tuple

import numpy as np

import jpeg_cases as jc
from salve_amd import jpeg

MUTANTS = ("no_unstuffing", "dc_reset_per_mcu_row", "extend_off_by_one", "zrl_is_15", "eob_ignored")

BAD_CODE, COEF_OVERRUN, TRUNCATED, DC_RANGE, LEFTOVER, MARKER, BAD_SLOT = 1, 2, 4, 8, 16, 32, 64

STANDARD_HUFFMAN = np.zeros((4, jpeg.HUFFMAN_TABLE_BYTES), dtype=np.uint8)
for _t, (_bits, _vals) in enumerate(((jpeg.BITS_DC_LUMA, jpeg.HUFFVAL_DC_LUMA), (jpeg.BITS_AC_LUMA, jpeg.HUFFVAL_AC_LUMA),
                                     (jpeg.BITS_DC_CHROMA, jpeg.HUFFVAL_DC_CHROMA), (jpeg.BITS_AC_CHROMA, jpeg.HUFFVAL_AC_CHROMA))):
    STANDARD_HUFFMAN[_t, :16] = _bits
    STANDARD_HUFFMAN[_t, 16:16 + len(_vals)] = _vals


def _decoder_table(table: np.ndarray):
    """BITS / HUFFVAL -> {(length, code): symbol}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(table[length - 1])):
            out[(length, code)] = int(table[16 + k])
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, data: bytes):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8)).tolist() + [0] * 64   # bits beyond the end read as 0
        self.at, self.total = 0, 8 * len(data)                                                # `at`: the next bit

    def take(self, n: int) -> int:
        v = 0
        if self.at + n <= len(self.bits):
            for bit in self.bits[self.at:self.at + n]:
                v = (v << 1) | bit
        self.at += n
        return v

    def symbol(self, table) -> int:
        code, bits, at = 0, self.bits, self.at
        for length in range(1, 17):
            code = (code << 1) | (bits[at] if at < len(bits) else 0)
            at += 1
            if (length, code) in table:
                self.at = at
                return table[(length, code)]
        self.at = at
        return -1


def _unstuff(scan: bytes, keep_stuffing: bool) -> Tuple[bytes, int]:
    out, status, i = bytearray(), 0, 0
    while i < len(scan):
        b = scan[i]
        i += 1
        if b == 0xFF and not keep_stuffing:
            if i < len(scan) and scan[i] == 0:
                i += 1
            else:          # a marker (or a last byte 0xFF): the scan ends in front of it
                status |= MARKER
                break
        out.append(b)
    return bytes(out), status


def decode(scan: bytes, huffman: np.ndarray, mh: int, mw: int, mutant: Optional[str] = None) -> Tuple[np.ndarray, int]:
    assert mutant is None or mutant in MUTANTS
    tables = [_decoder_table(np.asarray(huffman[t])) for t in range(4)]
    data, status = _unstuff(bytes(scan), mutant == "no_unstuffing")
    bits = _Bits(data)
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    zigzag = jpeg.ZIGZAG.tolist()

    def value(size: int) -> int:
        v = bits.take(size)
        if size and v < (1 << (size - 1)):
            v += (-1 << size) + (0 if mutant == "extend_off_by_one" else 1)
        return v

    def block(dst: np.ndarray, comp: int, pred: List[int]) -> int:
        t = 0 if comp == 0 else 2
        size = bits.symbol(tables[t])
        if size < 0:
            return BAD_CODE
        if size > 11:
            return DC_RANGE
        dc = pred[comp] + value(size)
        if bits.at > bits.total:
            return TRUNCATED
        if not -2047 <= dc <= 2047:
            return DC_RANGE
        pred[comp] = dc
        dst[0] = dc
        k = 1
        while k < 64:
            rs = bits.symbol(tables[t + 1])
            if rs < 0:
                return BAD_CODE
            run, size = rs >> 4, rs & 15
            if size == 0:
                if bits.at > bits.total:
                    return TRUNCATED
                if run != 15:
                    if mutant == "eob_ignored":
                        k += 1
                        continue
                    break
                k += 15 if mutant == "zrl_is_15" else 16
                if k > 64:
                    return COEF_OVERRUN
                continue
            k += run
            if k > 63:
                return COEF_OVERRUN
            v = value(size)
            if bits.at > bits.total:
                return TRUNCATED
            dst[zigzag[k]] = v
            k += 1
        return 0

    pred = [0, 0, 0]
    for my in range(mh):
        if mutant == "dc_reset_per_mcu_row":
            pred = [0, 0, 0]
        for mx in range(mw):
            for b in range(6):
                if status & ~MARKER or (status and bits.at >= bits.total):
                    return out, status
                status |= block(out[my, mx, b], 0 if b < 4 else b - 3, pred)
    if not status:
        left = bits.total - bits.at
        if left > 7 or bits.take(left) != (1 << left) - 1:
            status |= LEFTOVER
    return out, status


def pixels(levels: np.ndarray, qtab: np.ndarray, h: int, w: int) -> np.ndarray:
    """Quantised levels [MCU rows, MCUs, 6, 64] -> uint8 [h, w, 3] through jpeg_cases' inverse chain (dequantise, jpeg_idct_islow,
    fancy upsampling, YCbCr -> RGB), as libjpeg's decoder orders it."""
    mh, mw = levels.shape[:2]
    q = np.asarray(qtab, dtype=np.int64)
    luma = np.zeros((2 * mh, 2 * mw, 8, 8), dtype=np.int64)
    for k in range(4):
        luma[k >> 1::2, k & 1::2] = jc.idct_islow((levels[:, :, k] * q[0]).reshape(mh, mw, 8, 8))
    y = jc._unblocks(luma)[:h, :w]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    planes = []
    for k in (4, 5):
        small = jc._unblocks(jc.idct_islow((levels[:, :, k] * q[1]).reshape(mh, mw, 8, 8)))[:ch, :cw]
        planes.append(jc.upsample_h2v2(small)[:h, :w])
    return jc.ycc_to_rgb(y, planes[0], planes[1])


def decode_file(data: bytes, mutant: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """A whole file -> (pixels uint8 [h, w, 3], levels, status) with the tables of its own header."""
    p = jpeg.parse_file(data)
    levels, status = decode(data[p.scan_offset:p.scan_offset + p.scan_bytes], p.huffman, -(-p.h // 16), -(-p.w // 16), mutant)
    return pixels(levels, p.qtab, p.h, p.w), levels, status


def pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


def pillow_file(rgb: np.ndarray, **save) -> bytes:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **save)
    return buf.getvalue()
