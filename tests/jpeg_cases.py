"""The JPEG round trip's integer emulator and case table, shared by tests/test_jpeg_host.py (emulator == Pillow) and
tests/test_gpu_jpeg.py (salve_bev_jpeg_roundtrip == emulator == Pillow).

`roundtrip(rgb, qtab)` is decode(encode(rgb)) of baseline 4:2:0 JPEG with libjpeg's defaults, stage by stage as libjpeg's sources
order them (jccolor.c, jcprepct.c, jcsample.c, jfdctint.c, jcdctmgr.c, jidctint.c, jdsample.c, jdcolor.c), in numpy with int64
intermediates.  No entropy coding: quantised coefficients of 8-bit baseline data always fit the code range, so the decoded pixels
depend on the coefficients alone.  `mutant=` switches one stage to a plausible wrong variant; the host test shows that the case
table tells each of them from the real chain.
"""

from __future__ import annotations

import io
from typing import Dict, List, Optional, Tuple

import numpy as np

MUTANTS = ("constant_bias", "replicate_upsample", "truncating_quantise", "no_edge_replication")

# jfdctint.c / jidctint.c: CONST_BITS = 13, PASS1_BITS = 2
CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def rgb_to_ycc(rgb: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """jccolor.c: rgb_ycc_convert, 16-bit fixed point."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    half, off = 1 << 15, 128 << 16
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """jdcolor.c: ycc_rgb_convert with its four tables and the range limit."""
    half = 1 << 15
    cbx, crx = cb - 128, cr - 128
    r = y + ((_fix(1.40200) * crx + half) >> 16)
    b = y + ((_fix(1.77200) * cbx + half) >> 16)
    g = y + ((-_fix(0.34414) * cbx + half - _fix(0.71414) * crx) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def _pad_edge(plane: np.ndarray, H: int, W: int, replicate: bool = True) -> np.ndarray:
    h, w = plane.shape
    return np.pad(plane, ((0, H - h), (0, W - w)), mode="edge" if replicate else "constant")


def downsample_h2v2(c: np.ndarray, constant_bias: bool = False) -> np.ndarray:
    """jcsample.c: h2v2_downsample -- the 2 x 2 box with the bias alternating 1, 2 along a row (it restarts at every row)."""
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = np.full(s.shape[1], 2, dtype=np.int64) if constant_bias else 1 + (np.arange(s.shape[1], dtype=np.int64) & 1)
    return (s + bias[None, :]) >> 2


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """jfdctint.c: jpeg_fdct_islow on [..., 8, 8] level-shifted samples; the outputs are scaled up by 8."""

    def one_d(d, second):
        t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
        t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
        t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
        t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = CONST_BITS + PASS1_BITS if second else CONST_BITS - PASS1_BITS
        o = [None] * 8
        o[0] = _descale(t10 + t11, PASS1_BITS) if second else (t10 + t11) << PASS1_BITS
        o[4] = _descale(t10 - t11, PASS1_BITS) if second else (t10 - t11) << PASS1_BITS
        z1 = (t12 + t13) * F_0_541196100
        o[2] = _descale(z1 + t13 * F_0_765366865, n)
        o[6] = _descale(z1 + t12 * (-F_1_847759065), n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * F_1_175875602
        t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
        z1, z2 = z1 * (-F_0_899976223), z2 * (-F_2_562915447)
        z3, z4 = z3 * (-F_1_961570560) + z5, z4 * (-F_0_390180644) + z5
        o[7] = _descale(t4 + z1 + z3, n)
        o[5] = _descale(t5 + z2 + z4, n)
        o[3] = _descale(t6 + z2 + z3, n)
        o[1] = _descale(t7 + z1 + z4, n)
        return np.stack(o, -1)

    rows = one_d(blocks.astype(np.int64), False)
    return np.swapaxes(one_d(np.swapaxes(rows, -1, -2), True), -1, -2)


def quantise(coef: np.ndarray, q: np.ndarray, truncate: bool = False) -> np.ndarray:
    """jcdctmgr.c: the divisor is q << 3 (the forward DCT's scaling), the magnitude is rounded half up, the sign restored."""
    qv = q.astype(np.int64).reshape(8, 8) << 3
    mag = np.abs(coef)
    mag = mag // qv if truncate else (mag + (qv >> 1)) // qv
    return np.where(coef < 0, -mag, mag)


def range_limit_idct(v: np.ndarray) -> np.ndarray:
    """jidctint.c: range_limit[v & RANGE_MASK] -- the table behind the level shift: 0..127 -> 128..255, 128..511 -> 255,
    512..895 -> 0, 896..1023 -> 0..127."""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def idct_islow(coef: np.ndarray) -> np.ndarray:
    """jidctint.c: jpeg_idct_islow on dequantised [..., 8, 8] coefficients -> samples 0..255.  (Its all-zero-AC short cuts give what
    the general formulas give.)"""

    def one_d(d, n):
        z2, z3 = d[..., 2], d[..., 6]
        z1 = (z2 + z3) * F_0_541196100
        t2, t3 = z1 + z3 * (-F_1_847759065), z1 + z2 * F_0_765366865
        t0, t1 = (d[..., 0] + d[..., 4]) << CONST_BITS, (d[..., 0] - d[..., 4]) << CONST_BITS
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * F_1_175875602
        t0, t1, t2, t3 = t0 * F_0_298631336, t1 * F_2_053119869, t2 * F_3_072711026, t3 * F_1_501321110
        z1, z2 = z1 * (-F_0_899976223), z2 * (-F_2_562915447)
        z3, z4 = z3 * (-F_1_961570560) + z5, z4 * (-F_0_390180644) + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        return np.stack([_descale(t10 + t3, n), _descale(t11 + t2, n), _descale(t12 + t1, n), _descale(t13 + t0, n),
                         _descale(t13 - t0, n), _descale(t12 - t1, n), _descale(t11 - t2, n), _descale(t10 - t3, n)], -1)

    cols = np.swapaxes(one_d(np.swapaxes(coef.astype(np.int64), -1, -2), CONST_BITS - PASS1_BITS), -1, -2)
    return range_limit_idct(one_d(cols, CONST_BITS + PASS1_BITS + 3))


def _blocks(plane: np.ndarray) -> np.ndarray:
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b: np.ndarray) -> np.ndarray:
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def code_plane(plane: np.ndarray, q: np.ndarray, truncate: bool = False) -> np.ndarray:
    """Samples 0..255 of a plane of whole blocks -> the decoder's samples: level shift, DCT, quantise, dequantise, inverse DCT."""
    coef = quantise(fdct_islow(_blocks(plane.astype(np.int64)) - 128), q, truncate)
    return _unblocks(idct_islow(coef * q.astype(np.int64).reshape(8, 8)))


def upsample_h2v2(c: np.ndarray, fancy: bool = True) -> np.ndarray:
    """jdsample.c: h2v2_fancy_upsample (the triangle filter: 3/4 nearer + 1/4 further sample in each direction, biases 8 and 7,
    the first / last column and the top / bottom row taking the nearer sample twice); libjpeg takes the replicating h2v2_upsample
    instead where the component is at most two samples wide."""
    ch, cw = c.shape
    if not fancy or cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    colsum = np.stack([3 * c + up, 3 * c + down], 1).reshape(2 * ch, cw)   # output rows 2 r (above) and 2 r + 1 (below)
    left = np.concatenate([colsum[:, :1], colsum[:, :-1]], 1)
    right = np.concatenate([colsum[:, 1:], colsum[:, -1:]], 1)
    return np.stack([(3 * colsum + left + 8) >> 4, (3 * colsum + right + 7) >> 4], -1).reshape(2 * ch, 2 * cw)


def roundtrip(rgb: np.ndarray, qtab: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [h, w, 3]: decode(encode(rgb)) with tables `qtab` ([2, 64], natural order: luma, chroma)."""
    assert mutant is None or mutant in MUTANTS
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    rep = mutant != "no_edge_replication"
    y, cb, cr = rgb_to_ycc(rgb)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    # jcprepct.c / jcsample.c: rows are replicated to a whole row group (2), columns to twice the chroma plane's block width, then the
    # DOWNSAMPLED rows are replicated to whole blocks; luma is replicated to whole blocks in both directions
    y_dec = code_plane(_pad_edge(y, -(-h // 8) * 8, -(-w // 8) * 8, rep), qtab[0], mutant == "truncating_quantise")[:h, :w]
    CH, CW = -(-ch // 8) * 8, -(-cw // 8) * 8
    planes = []
    for c in (cb, cr):
        small = downsample_h2v2(_pad_edge(c, 2 * ch, 2 * CW, rep), mutant == "constant_bias")
        dec = code_plane(_pad_edge(small, CH, CW, rep), qtab[1], mutant == "truncating_quantise")[:ch, :cw]
        planes.append(upsample_h2v2(dec, mutant != "replicate_upsample")[:h, :w])
    return ycc_to_rgb(y_dec, planes[0], planes[1])


def pillow_roundtrip(rgb: np.ndarray, quality: int) -> np.ndarray:
    """What the reference's file hop does to an image: Pillow's `save(quality=)` and `open`, in memory."""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=quality)
    buf.seek(0)
    with Image.open(buf) as im:
        return np.asarray(im.convert("RGB")).copy()


# ---------------------------------------------------------------------------------------------------- cases
SMALL_SIZES = ((1, 1), (8, 8), (16, 16), (15, 17), (17, 9), (33, 47))   # (h, w): see the table in the module docstring of the tests
PRODUCT_SIZE = (501, 501)
SMALL_QUALITIES = (75, 30, 95)
CONTENTS = ("noise", "constant", "hramp", "vramp", "stripes", "disc", "layout")
LAYOUT_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255))


def make_image(content: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    rng = np.random.RandomState(seed * 7919 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":   # saturates both range limits
        return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if content == "constant":
        return np.broadcast_to(np.array([37, 200, 119], dtype=np.uint8), (h, w, 3)).copy()
    if content == "hramp":
        v = (xx * 255 // max(1, w - 1)).astype(np.uint8)
        return np.stack([v, 255 - v, v // 2], -1)
    if content == "vramp":
        v = (yy * 255 // max(1, h - 1)).astype(np.uint8)
        return np.stack([v // 3, v, 255 - v], -1)
    if content == "stripes":   # the eight saturated corner colours in 3-pixel stripes: chroma extremes across upsampling borders
        k = (xx // 3 + (yy // 3) * 3) % 8
        return np.stack([(k & 1) * 255, ((k >> 1) & 1) * 255, ((k >> 2) & 1) * 255], -1).astype(np.uint8)
    if content == "disc":   # black background, a textured disc: what a BEV render looks like
        img = np.zeros((h, w, 3), dtype=np.uint8)
        inside = (yy - h * 0.45) ** 2 + (xx - w * 0.55) ** 2 <= (0.4 * min(h, w)) ** 2
        tex = rng.randint(0, 256, size=(h, w, 3)) // 2 + (((xx + 2 * yy) * 5) % 128)[..., None]
        img[inside] = tex[inside].astype(np.uint8)
        return img
    if content == "layout":   # flat colours with lines 1 to 5 pixels wide
        img = np.zeros((h, w, 3), dtype=np.uint8)
        img[:, : w // 2] = LAYOUT_COLOURS[0]
        at = 1
        for t in range(1, 6):
            img[:, at:at + t] = LAYOUT_COLOURS[t % len(LAYOUT_COLOURS)]
            img[at:at + t, :] = LAYOUT_COLOURS[(t + 2) % len(LAYOUT_COLOURS)]
            at += 2 * t + 1
        return img
    raise ValueError(content)


def cases() -> List[Tuple[str, int, int, int]]:
    """(content, h, w, quality) of every case: every content at every small size and quality, and at the product's size at 75."""
    out = [(c, h, w, q) for (h, w) in SMALL_SIZES for q in SMALL_QUALITIES for c in CONTENTS]
    return out + [(c, PRODUCT_SIZE[0], PRODUCT_SIZE[1], 75) for c in CONTENTS]


_PILLOW: Dict[Tuple[str, int, int, int], np.ndarray] = {}


def pillow_reference(case: Tuple[str, int, int, int]) -> np.ndarray:
    """Pillow's round trip of a case, computed once per process and shared (read only)."""
    if case not in _PILLOW:
        c, h, w, q = case
        ref = pillow_roundtrip(make_image(c, h, w), q)
        ref.setflags(write=False)
        _PILLOW[case] = ref
    return _PILLOW[case]


def pack_bgr(rgb: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint32 [...] holding 0x00BBGGRR, the BEV images' layout."""
    a = rgb.astype(np.uint32)
    return a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)


def unpack_bgr(packed: np.ndarray) -> np.ndarray:
    p = packed.astype(np.uint32)
    return np.stack([p & 255, (p >> 8) & 255, (p >> 16) & 255], -1).astype(np.uint8)
