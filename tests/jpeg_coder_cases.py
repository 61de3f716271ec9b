"""The JPEG entropy coder's emulator and case table, shared by tests/test_jpeg_coder_host.py (emulator == Pillow's file) and
tests/test_gpu_jpeg_encode.py (salve_bev_jpeg_encode == emulator == Pillow's file).

`scan(rgb, quality)` is the entropy-coded segment of the baseline 4:2:0 file libjpeg writes with its defaults, written from ITU-T T.81
(Annex F.1.2: Huffman coding of DC differences and of AC coefficients in zigzag order with ZRL and EOB; Annex C: code generation;
B.1.1.5 / F.1.2.3: byte stuffing and 1-bit padding) over the quantised coefficients of tests/jpeg_cases.py's integer forward chain.
One thing is libjpeg's and not the standard's: blocks of an edge MCU that lie outside the image's own blocks are DUMMY blocks (jccoefct.c:
all AC zero; DC that of the block before them in the MCU at the right edge, of the block before their row of blocks at the bottom).
`mutant=` switches one rule to a plausible wrong variant; the host test shows that the case table tells each from the real coder.
The second value of `scan` counts what the symbol stream contained, so that the host test can assert that the table as a whole
exercises every rule of the coder.
"""

from __future__ import annotations

import io
from typing import Dict, List, Optional, Tuple

import numpy as np

import jpeg_cases as jc
from salve_amd import jpeg

MUTANTS = ("no_stuffing", "zero_padding", "dc_reset_per_mcu_row", "missing_zrl", "eob_always")


# ---------------------------------------------------------------------------------------------------- coefficients
def quantised_mcus(rgb: np.ndarray, qtab: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> int64 [MCU rows, MCUs across, 6, 64]: the quantised levels of every block in natural order, blocks in the
    MCU's order Y0 Y1 Y2 Y3 Cb Cr."""
    h, w = rgb.shape[:2]
    y, cb, cr = jc.rgb_to_ycc(rgb)
    hb, wb = -(-h // 8), -(-w // 8)           # the luma component's size in blocks
    ch, cw = (h + 1) // 2, (w + 1) // 2
    CH, CW = -(-ch // 8) * 8, -(-cw // 8) * 8
    mh, mw = CH // 8, CW // 8                 # MCUs: one chroma block each
    yq = jc.quantise(jc.fdct_islow(jc._blocks(jc._pad_edge(y, hb * 8, wb * 8)) - 128), qtab[0]).reshape(hb, wb, 64)
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    for k, c in enumerate((cb, cr)):
        small = jc._pad_edge(jc.downsample_h2v2(jc._pad_edge(c, 2 * ch, 2 * CW)), CH, CW)
        out[:, :, 4 + k] = jc.quantise(jc.fdct_islow(jc._blocks(small) - 128), qtab[1]).reshape(mh, mw, 64)
    for my in range(mh):
        for mx in range(mw):
            for by in range(2):
                for bx in range(2):
                    k = 2 * by + bx
                    if 2 * my + by < hb and 2 * mx + bx < wb:
                        out[my, mx, k] = yq[2 * my + by, 2 * mx + bx]
                    else:   # dummy block: zero AC, DC of the block before it (right edge) or before its row of blocks (bottom)
                        out[my, mx, k, 0] = out[my, mx, k - 1 if 2 * my + by < hb else 1, 0]
    return out


# ---------------------------------------------------------------------------------------------------- the coder
class _Bits:
    """Bits most significant first; whole bytes leave the accumulator as they fill."""

    def __init__(self):
        self.acc, self.pending, self.n, self.out = 0, 0, 0, bytearray()

    def put(self, code: int, length: int):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.pending += length
        self.n += length
        while self.pending >= 8:
            self.pending -= 8
            self.out.append(self.acc >> self.pending)
            self.acc &= (1 << self.pending) - 1


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def _value_bits(v: int, size: int) -> int:
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _new_stats() -> Dict[str, object]:
    return {"zrl": 0, "max_zrl_in_a_row": 0, "blocks_without_eob": 0, "zero_ac_blocks": 0, "dc_categories": set(), "dc_signs": set(),
            "ac_categories": set(), "stuffed": 0, "pad_bits": 0, "pad_byte": None}


def scan(rgb: np.ndarray, quality: int, mutant: Optional[str] = None) -> Tuple[bytes, Dict[str, object]]:
    """The entropy-coded segment (stuffed, padded; no header, no EOI) and the counts of what it contained."""
    assert mutant is None or mutant in MUTANTS
    mcus = quantised_mcus(rgb, jpeg.quality_tables(quality))[..., jpeg.ZIGZAG].tolist()   # zigzag order, plain ints
    dc_codes, ac_codes = jpeg.DC_CODES.tolist(), jpeg.AC_CODES.tolist()
    st = _new_stats()
    bits = _Bits()
    pred = [0, 0, 0]
    for my in range(len(mcus)):
        if mutant == "dc_reset_per_mcu_row":
            pred = [0, 0, 0]
        for mx in range(len(mcus[my])):
            for k in range(6):
                comp = 0 if k < 4 else k - 3
                t = 0 if comp == 0 else 1
                zz = mcus[my][mx][k]
                diff = zz[0] - pred[comp]
                pred[comp] = zz[0]
                size = _category(diff)
                st["dc_categories"].add(size)
                if diff:
                    st["dc_signs"].add(1 if diff > 0 else -1)
                e = dc_codes[t][size]
                assert e, "a DC category outside the baseline table"
                bits.put(e >> 5, e & 31)
                bits.put(_value_bits(diff, size), size)
                run, zrl_row = 0, 0
                nz = [p for p in range(1, 64) if zz[p]]
                if not nz:
                    st["zero_ac_blocks"] += 1
                last = 0
                for p in nz:
                    run = p - last - 1
                    last = p
                    zrl_row = 0
                    while run >= 16:
                        if mutant != "missing_zrl":
                            z = ac_codes[t][0xF0]
                            bits.put(z >> 5, z & 31)
                        st["zrl"] += 1
                        zrl_row += 1
                        run -= 16
                    st["max_zrl_in_a_row"] = max(st["max_zrl_in_a_row"], zrl_row)
                    v = zz[p]
                    size = _category(v)
                    st["ac_categories"].add(size)
                    e = ac_codes[t][(run << 4) | size]
                    assert e, "an AC symbol outside the baseline table"
                    bits.put(e >> 5, e & 31)
                    bits.put(_value_bits(v, size), size)
                if last < 63 or mutant == "eob_always":
                    e = ac_codes[t][0]
                    bits.put(e >> 5, e & 31)
                if last == 63:
                    st["blocks_without_eob"] += 1
    pad = (-bits.n) % 8
    st["pad_bits"] = pad
    bits.put(0 if mutant == "zero_padding" else (1 << pad) - 1, pad)
    assert bits.pending == 0
    raw = bytes(bits.out)
    st["pad_byte"] = raw[-1] if pad else None
    st["stuffed"] = raw.count(b"\xff")
    return (raw if mutant == "no_stuffing" else raw.replace(b"\xff", b"\xff\x00")), st


def file(rgb: np.ndarray, quality: int, mutant: Optional[str] = None) -> bytes:
    h, w = rgb.shape[:2]
    return jpeg.file_bytes(scan(rgb, quality, mutant)[0], h, w, quality)


def pillow_file(rgb: np.ndarray, quality: int) -> bytes:
    """The bytes `Image.fromarray(rgb).save(path, quality=quality)` writes."""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


# ---------------------------------------------------------------------------------------------------- cases
CRAFTED = ("zrl", "ffheavy", "checker", "halfstep", "padff")
PADFF_SEED = 21  # make_image("padff", 8, 8): the 8 x 8 noise image of this seed whose final, padded byte is 0xFF at quality 100 (found by search)


def _basis_blocks(h: int, w: int, pick) -> np.ndarray:
    """A grey image whose 8 x 8 block (i, j) is 128 + amp * the DCT basis function (u, v), (u, v, amp) = pick(i, j)."""
    yy, xx = np.mgrid[0:8, 0:8]
    img = np.zeros((-(-h // 8) * 8, -(-w // 8) * 8), dtype=np.float64)
    for i in range(img.shape[0] // 8):
        for j in range(img.shape[1] // 8):
            u, v, amp = pick(i, j)
            img[8 * i:8 * i + 8, 8 * j:8 * j + 8] = 128 + amp * np.cos((2 * xx + 1) * u * np.pi / 16) * np.cos((2 * yy + 1) * v * np.pi / 16)
    g = np.clip(np.rint(img[:h, :w]), 0, 255).astype(np.uint8)
    return np.stack([g, g, g], -1)


def make_image(content: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    if content not in CRAFTED:
        return jc.make_image(content, h, w, seed)
    if content == "zrl":       # one high-frequency coefficient per block: runs of 16 .. 62 zeros, (7, 7) is coefficient 63 (no EOB)
        spots = ((7, 7), (5, 3), (3, 6), (7, 4), (2, 5), (6, 6))
        return _basis_blocks(h, w, lambda i, j: spots[(i * 3 + j) % len(spots)] + (120,))
    if content == "ffheavy":   # mid-frequency coefficients of size >= 6 behind short runs: the 16-bit codes that begin with nine 1-bits
        return _basis_blocks(h, w, lambda i, j: (1 + (i + 2 * j) % 4, 2 + (2 * i + j) % 3, 127))
    if content == "checker":   # black and white blocks: DC differences of both signs and of category 11 at quality 100
        yy, xx = np.mgrid[0:h, 0:w]
        g = ((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)
        return np.stack([g, g, g], -1)
    if content == "halfstep":  # a black | white edge in the middle of every block: the largest AC coefficients there are
        xx = np.mgrid[0:h, 0:w][1]
        g = (((xx // 4) % 2) * 255).astype(np.uint8)
        return np.stack([g, g, g], -1)
    return jc.make_image("noise", h, w, PADFF_SEED)


def cases() -> List[Tuple[str, int, int, int]]:
    """(content, h, w, quality): the round trip's table, quality 100 on the three smallest shapes, and the crafted images."""
    out = list(jc.cases())
    out += [(c, h, w, 100) for (h, w) in jc.SMALL_SIZES[:3] for c in jc.CONTENTS]
    out += [("zrl", 33, 47, 75), ("ffheavy", 33, 47, 75), ("zrl", 16, 16, 100), ("checker", 16, 16, 100), ("halfstep", 16, 16, 100),
            ("checker", 33, 47, 30), ("padff", 8, 8, 100)]
    return out


_REF: Dict[Tuple[str, int, int, int], Tuple[bytes, bytes, Dict[str, object]]] = {}


def reference(case: Tuple[str, int, int, int]) -> Tuple[bytes, bytes, Dict[str, object]]:
    """(Pillow's file, the emulator's scan, the emulator's counts) of a case, computed once per process and shared."""
    if case not in _REF:
        c, h, w, q = case
        img = make_image(c, h, w)
        s, st = scan(img, q)
        _REF[case] = (pillow_file(img, q), s, st)
    return _REF[case]
