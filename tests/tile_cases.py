"""The tile and resize family across its accepted contract (include/salve_hip.h: salve_bev_tiles, salve_bev_tiles_aug,
salve_bev_tile_pairs, salve_bev_train_tiles, salve_bev_densify_tiles' tile phase, salve_resize_rgb_u8, salve_bev_export_u8): the case
tables and an emulator of every entry's DOCUMENTED output that shares no code with the library or with oracle/bev_oracle.py.
tests/test_tile_cases_host.py pins the emulator to the oracle and shows that fifteen emulated wrong kernels fail the cases;
tests/test_gpu_tile_contract.py compares the kernels with it bit for bit.  numpy, struct, math, fractions -- nothing else.

The arithmetic.  OpenCV's uint8 INTER_LINEAR (imgproc resize.cpp).  Per destination index d of dst from src, scalar-wise as its set-up
loop: fx = (float)((d + 0.5) * (src / dst) - 0.5) evaluated in double and narrowed to float32 (struct), s = floor(fx), fx = fx - s in
float32, the two edge clamps (s < 0: s = 0, fx = 0; s >= src - 1: s = src - 1, fx = 0), taps round-half-even(float32(w) * 2048) for
w = 1 - fx and w = fx, second source index min(s + 1, src - 1).  Per pixel: S = a * w0 + b * w1 along the row (x 2048), then
(((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, clamped to 0 .. 255.  cv2 is not installed where this suite runs:
parity with OpenCV itself stays unpinned; what is pinned is that a second derivation from the published algorithm agrees with the
library's and the oracle's tables, and that the fixed-point result stays within FIXED_VS_EXACT of the bilinear value it stands for.

FIXED_VS_EXACT: |fixed-point pixel - exact rational bilinear value| for sources up to 1023 pixels, in grey levels, from the algorithm
alone (values a, b, ... in 0 .. 255; exact weights 1 - f, f per axis at the exact coordinate x = (d + 0.5) * src / dst - 0.5, clamped
to [0, src - 1]):
  1. the coordinate.  x < 1024 is narrowed to float32: half an ulp of [512, 1024) is 2^-15 (the double evaluation in front of it adds
     less than 2^-40).  fx - s is exact.  The bilinear value is continuous and piecewise linear in x with slope |b - a| <= 255, so a
     coordinate off by e moves it by at most 255 e -- also across an integer, where floor() changes: 255 (2^-15 + 2^-40) per axis,
     0.01556 for both.
  2. the taps.  w1 = rne(2048 f) is off by at most 1/2; w0 = rne(2048 float32(1 - f)) by at most 1/2 + 2^-14 (1 - f is rounded to
     float32 first when f < 1/2).  Nothing here assumes w0 + w1 = 2048.  Horizontal: |S / 2048 - (a (1 - f) + b f)| <=
     255 (1 + 2^-14) / 2048 = e_h = 0.12452 for either row.  Vertical: with b_i / 2048 = g_i + n_i, |n_i| <= (1/2 + 2^-14) / 2048,
     sum_i (g_i + n_i) (H_i + e_i) differs from the exact sum_i g_i H_i by at most e_h + 2 (1/2 + 2^-14) / 2048 * (255 + e_h) =
     0.12452 + 0.12458.
  3. the two floors of the vertical pass, both downwards.  S >> 4 drops at most 15/16 of a unit of 2^-7: (b0 + b1) * (15/16) / 2^16
     quarter levels, with b0 + b1 <= 2049: 0.00733 grey levels.  Each `>> 16` drops less than one quarter level: 0.5 for the two.
  4. the final `+ 2 >> 2`: at most 1/2, upwards at the tie.  The clamp to 0 .. 255 only moves the result towards the exact value.
Downwards the terms add to 0.01556 + 0.24910 + 0.00733 + 0.5 + 0.5 = 1.27199; upwards to 0.01556 + 0.24910 + 0.5 = 0.76466.
FIXED_VS_EXACT is the larger, as the expression below.  Where w0 + w1 = 2048 (every table of this module: asserted by the host file)
the tap errors of a pair cancel in part (e_h = 127.5 / 2048, the vertical term likewise) and the bound is 1.1475.  Measured over all
geometries, contents and resize sizes of this module: at most 0.8044 below and 0.5532 above (tests/test_tile_cases_host.py prints it).

The entries, from the header.  Centre crop at (resize - crop) / 2, truncated.  The aug / train draw: offsets clamped into
[0, resize - crop], crop, THEN the flips (output pixel (i, j) = crop pixel (crop - 1 - i if VFLIP, crop - 1 - j if HFLIP)).  The
normalisation table in float32; fp16 / bf16 by ONE rounding to nearest even; NCHW / NHWC placement; the pair entry's group of six
channels in either order, zero padding behind a sample's last group (the group behind which no further group fits: c0 + 12 > out_c;
out_c = 8 is one group and its two padding channels); the train entry writes EVERY channel; U8X4 is 0x00BBGGRR; salve_resize_rgb_u8
takes the box mean (a + b + c + d + 2) >> 2 only when BOTH ratios are exactly 2.  Whatever an entry does not name keeps the sentinel
(`blank`): NaN for the float formats, 0x5A bytes for the integer ones.
"""

import functools
import math
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np

FIXED_VS_EXACT = (2 * 255 * (2.0 ** -15 + 2.0 ** -40)                                          # 1. both coordinates
                  + 255 * (1 + 2.0 ** -14) / 2048                                              # 2. horizontal taps
                  + 2 * (0.5 + 2.0 ** -14) / 2048 * (255 + 255 * (1 + 2.0 ** -14) / 2048)      #    vertical taps
                  + 2049 * (15 / 16) / 2 ** 16 / 4 + 0.5                                       # 3. the floors
                  + 0.5)                                                                       # 4. the final rounding
MAX_SRC = 1023

# formats and flag bits as the header numbers them (restated: this module imports nothing of the library)
F32_NCHW, F16_NHWC, U8X4, F32_NHWC, BF16_NHWC = 0, 1, 2, 3, 4
HFLIP, VFLIP = 1, 2
SENTINEL_U32 = 0x5A5A5A5A

Geo = namedtuple("Geo", "h w resize crop")
Geo.id = property(lambda g: f"{g.h}x{g.w}-{g.resize}-{g.crop}")
GEOMETRIES = (Geo(41, 37, 30, 24), Geo(37, 41, 90, 64), Geo(64, 64, 32, 32), Geo(33, 33, 33, 17), Geo(101, 101, 47, 40),
              Geo(101, 101, 300, 290), Geo(41, 37, 30, 1), Geo(501, 501, 234, 224))
ANCHOR = GEOMETRIES[-1]
SMALL = tuple(g for g in GEOMETRIES if g is not ANCHOR)
BY_ID = {g.id: g for g in GEOMETRIES}
G_NARROW, G_ODD, G_WIDE = BY_ID["41x37-30-24"], BY_ID["101x101-47-40"], BY_ID["101x101-300-290"]
CONTENTS = ("noise", "checker", "columns", "rows", "white", "black", "ramp")

# ---- the emulated wrong kernels (tests/test_tile_cases_host.py: each is rejected by at least one case of every entry it applies to)
M_XROWS = "x taps used for rows"
M_CROP_UP = "crop offset rounded up"
M_FLIP_FIRST = "flips applied before the crop"
M_FLIP_BITS = "H and V flip bits swapped"
M_NO_CLAMP = "offsets not clamped"
M_BGR = "channels read as BGR"
M_HALVES = "the pair's two halves swapped"
M_PADDING = "padding channels left unwritten"
M_LAST_BLOCK = "last partial block of 256 pixels unwritten"
M_MINUS_8 = "sample k >= 8 written to k - 8"
M_COL_GROUP = "second column group (j >= 256) unwritten"
M_TIE = "the tie of + 2 >> 2 rounded down"   # (`+ 2 >> 2` IS round half up: the mutant is the kernel whose tie goes the other way, `+ 1 >> 2`)
M_ONE_ROUNDING = "one rounding at the end instead of the >> 4 / >> 16 truncations"
M_BOX = "box mean used when only one ratio is 2"
M_F16_AWAY = "fp16 ties away from zero"
ENTRIES = ("tiles", "aug", "pairs", "train", "phase_h", "resize_rgb", "export")
MUTANTS = {
    M_XROWS: ("tiles", "aug", "pairs", "train", "phase_h", "resize_rgb"),
    M_CROP_UP: ("tiles", "pairs", "phase_h"),
    M_FLIP_FIRST: ("aug", "train"),
    M_FLIP_BITS: ("aug", "train"),
    M_NO_CLAMP: ("aug", "train"),
    M_BGR: ENTRIES,
    M_HALVES: ("pairs", "phase_h"),
    M_PADDING: ("pairs", "train", "phase_h"),
    M_LAST_BLOCK: ("tiles", "aug", "pairs", "train", "resize_rgb", "export"),
    M_MINUS_8: ("pairs", "train"),
    M_COL_GROUP: ("phase_h",),
    M_TIE: ("tiles", "aug", "pairs", "train", "phase_h", "resize_rgb"),
    M_ONE_ROUNDING: ("tiles", "aug", "pairs", "train", "phase_h", "resize_rgb"),
    M_BOX: ("resize_rgb",),
    M_F16_AWAY: ("tiles", "pairs", "phase_h"),
}


# ------------------------------------------------------------------------------------------------ taps
def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


@functools.lru_cache(maxsize=None)
def taps(dst: int, src: int) -> np.ndarray:
    """int32 [dst, 4] = (s0, s1, w0, w1), one destination index at a time."""
    scale = float(src) / float(dst)
    rows = []
    for d in range(dst):
        fx = _f32((d + 0.5) * scale - 0.5)
        s = math.floor(fx)
        fx = _f32(fx - float(s))
        if s < 0:
            s, fx = 0, 0.0
        if s >= src - 1:
            s, fx = src - 1, 0.0
        w0 = round(_f32(_f32(1.0 - fx) * 2048.0))   # (Python's round: half to even, as cvRound)
        w1 = round(_f32(fx * 2048.0))
        rows.append((s, min(s + 1, src - 1), w0, w1))
    t = np.array(rows, dtype=np.int32).reshape(dst, 4)
    t.setflags(write=False)
    return t


def exact_coordinate(d: int, dst: int, src: int):
    """(s, f): floor and fraction of the exact source coordinate ((2 d + 1) src - dst) / (2 dst) clamped to [0, src - 1]."""
    x = min(max(Fraction((2 * d + 1) * src - dst, 2 * dst), Fraction(0)), Fraction(src - 1))
    s = min(math.floor(x), max(src - 2, 0))
    return s, x - s


# ------------------------------------------------------------------------------------------------ contents
@functools.lru_cache(maxsize=None)
def image(h: int, w: int, content: str) -> np.ndarray:
    """uint8 [h, w, 3], read-only."""
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        im = np.random.default_rng(1000 * h + w).integers(0, 256, size=(h, w, 3))
    elif content == "checker":
        im = np.repeat((((xx + yy) & 1) * 255)[..., None], 3, 2)
    elif content == "columns":
        im = np.repeat(((xx & 1) * 255)[..., None], 3, 2)
    elif content == "rows":
        im = np.repeat(((yy & 1) * 255)[..., None], 3, 2)
    elif content == "white":
        im = np.full((h, w, 3), 255)
    elif content == "black":
        im = np.zeros((h, w, 3))
    elif content == "ramp":       # distinct R, G and B: a channel swap shows
        im = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + yy + 64) % 256, (255 - (xx + 11 * yy)) % 256], -1)
    elif content == "cells":      # 2 x 2 cells of 255, 255, 255, 254: the box mean's + 2 decides (1019 + 2) >> 2 = 255
        im = np.repeat((255 - ((xx & 1) & (yy & 1)))[..., None], 3, 2)
    else:
        raise ValueError(content)
    im = np.ascontiguousarray(im, dtype=np.uint8)
    im.setflags(write=False)
    return im


def pack(img_u8: np.ndarray, top: int = 0) -> np.ndarray:
    """uint8 [..., 3] -> uint32 0x00BBGGRR (with `top` in the fourth byte)."""
    p = img_u8.astype(np.uint32)
    return p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16) | np.uint32(top << 24)


@functools.lru_cache(maxsize=None)
def lut(kind: str = "imagenet") -> np.ndarray:
    """float32 [3, 256].  "imagenet": (v - 255 m_c) / (255 s_c) in float32, the table ToTensor + Normalize amount to.  "ties": every entry
    exactly half-way between two fp16 values (1 + (2 v + 1) 2^-11, its negative, 2 + (2 v + 1) 2^-10) -- the imagenet table holds no
    such value, and the table is an argument of every entry."""
    v = np.arange(256, dtype=np.float32)
    if kind == "imagenet":
        rows = [(v - np.float32(m * 255)) / np.float32(s * 255) for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    elif kind == "ties":
        o = (2 * v + 1)
        rows = [1 + o * np.float32(2.0 ** -11), -(1 + o * np.float32(2.0 ** -11)), 2 + o * np.float32(2.0 ** -10)]
    else:
        raise ValueError(kind)
    t = np.stack(rows).astype(np.float32)
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------------------------------ roundings
def to_f16(x: np.ndarray, mutant=None) -> np.ndarray:
    """float32 -> float16, one rounding to nearest even (numpy's)."""
    h = x.astype(np.float16)
    if mutant == M_F16_AWAY:     # where x lies exactly half-way between two fp16 values, the one of larger magnitude
        hd, xd = h.astype(np.float64), x.astype(np.float64)
        other = np.nextafter(h, np.where(xd > hd, np.inf, -np.inf).astype(np.float16))   # the fp16 value on the other side of x
        tie = (hd != xd) & (np.abs(hd - xd) == np.abs(other.astype(np.float64) - xd))
        h = np.where(tie & (np.abs(other) > np.abs(h)), other, h)
    return h


def to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> uint16 bf16 bit patterns, one rounding to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def blank(shape, dtype) -> np.ndarray:
    """A sentinel-filled output buffer: NaN for float formats, 0x5A bytes for integer ones."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.full(shape, np.nan, dtype=dtype)
    return np.full(shape, SENTINEL_U32 & ((1 << (8 * dtype.itemsize)) - 1), dtype=dtype)


def bits(a: np.ndarray) -> np.ndarray:
    """The array as unsigned integers of its element size: the zero-tolerance comparator compares these."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got: np.ndarray, want: np.ndarray) -> bool:
    return got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------ the pixel
def resize_u8(img: np.ndarray, ty: np.ndarray, tx: np.ndarray, mutant=None) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [len(ty), len(tx), 3]: the horizontal pass into x 2048 integers, the vertical pass with its two floors."""
    H, W = img.shape[:2]
    ty, tx = np.asarray(ty, dtype=np.int64), np.asarray(tx, dtype=np.int64)
    if mutant == M_XROWS:   # (a wrong kernel would read outside a shorter table or image; the emulation stays defined by clamping)
        ty = tx[np.minimum(np.arange(len(ty)), len(tx) - 1)].copy()
        ty[:, :2] = np.minimum(ty[:, :2], H - 1)
    p = img.astype(np.int64)
    if mutant == M_BGR:
        p = p[..., ::-1]
    out = np.empty((len(ty), len(tx), 3), dtype=np.int64)
    a0, a1 = tx[:, 2][None, :, None], tx[:, 3][None, :, None]
    for i, (y0, y1, b0, b1) in enumerate(ty.tolist()):
        top = p[y0][tx[:, 0]][None] * a0 + p[y0][tx[:, 1]][None] * a1
        bot = p[y1][tx[:, 0]][None] * a0 + p[y1][tx[:, 1]][None] * a1
        if mutant == M_ONE_ROUNDING:
            out[i] = ((b0 * top + b1 * bot + (1 << 21)) >> 22)[0]
        else:
            out[i] = ((((b0 * (top >> 4)) >> 16) + ((b1 * (bot >> 4)) >> 16) + (1 if mutant == M_TIE else 2)) >> 2)[0]
    return np.clip(out, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=256)
def _resized(geo: Geo, content: str, mutant=None) -> np.ndarray:
    r = resize_u8(image(geo.h, geo.w, content), taps(geo.resize, geo.h), taps(geo.resize, geo.w), mutant)
    r.setflags(write=False)
    return r


_RESIZE_MUTANTS = (M_XROWS, M_BGR, M_TIE, M_ONE_ROUNDING)


def crop_u8(geo: Geo, content: str, draw=None, mutant=None) -> np.ndarray:
    """The Resize + Crop (+ flips) result, uint8 [crop, crop, 3].  draw = None: the centre crop; else (crop_y, crop_x, flags)."""
    r = _resized(geo, content, mutant if mutant in _RESIZE_MUTANTS else None)
    room = geo.resize - geo.crop
    if draw is None:
        oy = ox = (room + 1) // 2 if mutant == M_CROP_UP else room // 2
        return r[oy:oy + geo.crop, ox:ox + geo.crop]
    oy, ox, flags = draw
    if mutant == M_FLIP_BITS:
        flags = (HFLIP if flags & VFLIP else 0) | (VFLIP if flags & HFLIP else 0)
    if mutant != M_NO_CLAMP:
        oy, ox = min(max(oy, 0), room), min(max(ox, 0), room)
    if mutant == M_FLIP_FIRST:   # the resized image is mirrored, then cropped at the offsets
        r = r[::-1] if flags & VFLIP else r
        r = r[:, ::-1] if flags & HFLIP else r
        flags = 0
    iy = np.clip(np.arange(geo.crop) + oy, 0, geo.resize - 1)   # (unclamped offsets: a wrong kernel reads taps outside the table; clamped here)
    ix = np.clip(np.arange(geo.crop) + ox, 0, geo.resize - 1)
    c = r[iy][:, ix]
    c = c[::-1] if flags & VFLIP else c
    return c[:, ::-1] if flags & HFLIP else c


def normalised(u8: np.ndarray, table: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> float32 [h, w, 3] through the table."""
    return np.stack([table[c][u8[..., c]] for c in range(3)], -1)


def _written(crop: int, mutant=None) -> np.ndarray:
    """bool [crop, crop]: the pixels a kernel with a thread per pixel and blocks of 256 writes."""
    n = crop * crop
    w = np.ones(n, dtype=bool)
    if mutant == M_LAST_BLOCK and n % 256:
        w[n // 256 * 256:] = False
    return w.reshape(crop, crop)


# ------------------------------------------------------------------------------------------------ salve_bev_tiles
SLOT_PERM = (4, 0, 6, 2, 7, 1, 3)      # content k -> slot: a non-identity permutation; slots 5 and 8 of the 9 are named by no job
IMAGE_ORDER = (3, 6, 0, 5, 1, 4, 2)    # content k is image IMAGE_ORDER[k] of its array: named out of order, the array's last image included
N_SLOTS = 9


def tiles_cases():
    """(geometry id, format, table kind): every geometry x content in all three formats -- the seven contents are the seven jobs of ONE
    launch -- and the fp16 tie table once."""
    return [(g.id, fmt, "imagenet") for g in GEOMETRIES for fmt in (F32_NCHW, F16_NHWC, U8X4)] + [(G_NARROW.id, F16_NHWC, "ties")]


def tiles_jobs(fmt):
    """[(content, image index, slot, chan)]; chan 0 and 3 (one image per slot for U8X4, which ignores chan)."""
    return [(c, IMAGE_ORDER[k], SLOT_PERM[k], 3 * (k & 1)) for k, c in enumerate(CONTENTS)]


def image_array(geo: Geo, top: int = 0) -> np.ndarray:
    """uint32 [7, h, w]: the contents in IMAGE_ORDER."""
    a = np.empty((len(CONTENTS), geo.h, geo.w), dtype=np.uint32)
    for k, c in enumerate(CONTENTS):
        a[IMAGE_ORDER[k]] = pack(image(geo.h, geo.w, c), top)
    return a


def tiles_out_c(fmt):
    return {F32_NCHW: 6, F16_NHWC: 8, U8X4: 3}[fmt]


def tiles_expected(case, mutant=None) -> np.ndarray:
    gid, fmt, kind = case
    geo, out_c, c = BY_ID[gid], tiles_out_c(fmt), BY_ID[gid].crop
    w = _written(c, mutant)
    if fmt == U8X4:
        out = blank((N_SLOTS, c, c), np.uint32)
    elif fmt == F32_NCHW:
        out = blank((N_SLOTS, out_c, c, c), np.float32)
    else:
        out = blank((N_SLOTS, c, c, out_c), np.float16)   # three of a sample's eight channels per job: the others keep the sentinel
    for content, _, slot, chan in tiles_jobs(fmt):
        u8 = crop_u8(geo, content, None, mutant)
        if fmt == U8X4:
            out[slot][w] = pack(u8)[w]
            continue
        v = normalised(u8, lut(kind))
        if fmt == F32_NCHW:
            for ch in range(3):
                out[slot, chan + ch][w] = v[..., ch][w]
        else:
            out[slot][w, chan:chan + 3] = to_f16(v, mutant)[w]
    return out


# ------------------------------------------------------------------------------------------------ salve_bev_tiles_aug
def draws(geo: Geo):
    """[(crop_y, crop_x, flags)]: offsets 0, the maximum, interior, below 0 and above the maximum (clamped), each with all four flips."""
    m = geo.resize - geo.crop
    offs = [(0, 0), (m, m), (m // 2 + 1, 1), (-3, m - 1), (m + 4, -1), (1, m + 2)]
    return [(oy, ox, f) for oy, ox in offs for f in (0, HFLIP, VFLIP, HFLIP | VFLIP)]


AUG_GEOMETRIES = (G_NARROW.id, G_ODD.id)


def aug_cases():
    return list(AUG_GEOMETRIES)


def aug_jobs(geo: Geo):
    """[(content, image index, slot, chan, draw)]: job k draws draws[k]; two jobs per six-channel sample, the slots reversed."""
    d = draws(geo)
    n_slots = len(d) // 2
    return [(CONTENTS[(3 * k) % 7], IMAGE_ORDER[(3 * k) % 7], n_slots - 1 - k // 2, 3 * (1 - (k & 1)), d[k]) for k in range(len(d))]


def aug_expected(gid, mutant=None) -> np.ndarray:
    geo = BY_ID[gid]
    jobs, c = aug_jobs(geo), geo.crop
    w = _written(c, mutant)
    out = blank((len(jobs) // 2 + 1, 6, c, c), np.float32)     # the last slot is named by no job
    for content, _, slot, chan, draw in jobs:
        v = normalised(crop_u8(geo, content, draw, mutant), lut())
        for ch in range(3):
            out[slot, chan + ch][w] = v[..., ch][w]
    return out


# ------------------------------------------------------------------------------------------------ salve_bev_tile_pairs, phase H
PairCase = namedtuple("PairCase", "gid n out_c groups kind")   # n pairs, `groups` pairs per sample (the last sample may hold fewer)


def pairs_cases():
    """Counts 1 / 7 / 8 / 9 / 17; out_c 6 .. 16 with one and two groups; both channel orders inside every case (pairs_jobs)."""
    shapes = [(1, 6, 1), (7, 8, 1), (8, 10, 1), (9, 12, 2), (17, 14, 2), (9, 16, 2), (7, 16, 1), (17, 8, 1), (8, 12, 1)]
    return ([PairCase(g, n, oc, gr, "imagenet") for g in (G_NARROW.id, G_ODD.id) for n, oc, gr in shapes]
            + [PairCase(ANCHOR.id, 3, 16, 2, "imagenet"), PairCase(G_NARROW.id, 9, 16, 2, "ties")])


def _perm(n):
    """A non-identity permutation of range(n) for n > 1 (a rotation by n // 2 + 1 of the reversed order ...)."""
    return [(n - 1 - k + n // 2 + 1) % n for k in range(n)] if n > 1 else [0]


def pairs_jobs(case: PairCase):
    """[(content a, image a, chan a, content b, image b, chan b, slot)] and the number of slots (one more than the samples: named by none).
    Pair k is group k % groups of sample k // groups; the group's halves alternate (image a first for even k + k // 3); a one-group
    sample of a 16-channel buffer takes the SECOND group on odd samples (channels 6 .. 11, padding 12 .. 15 zero, 0 .. 5 untouched)."""
    samples = (case.n + case.groups - 1) // case.groups
    perm = _perm(samples)
    jobs = []
    for k in range(case.n):
        smp, grp = divmod(k, case.groups)
        if case.groups == 1 and case.out_c >= 12 and smp & 1:
            grp = 1
        a_first = (k + k // 3) % 2 == 0
        ca, cb = CONTENTS[(3 * k + 1) % 7], CONTENTS[(5 * k + 6) % 7]
        jobs.append((ca, IMAGE_ORDER[(3 * k + 1) % 7], 6 * grp + (0 if a_first else 3), cb, IMAGE_ORDER[(5 * k + 6) % 7], 6 * grp + (3 if a_first else 0), perm[smp]))
    return jobs, samples + 1


def _put_pair(sample, geo, c0, lo, hi, out_c, mutant, written):
    """One group of six fp16 channels (lo | hi, float32 [crop, crop, 3] each) at channel c0 of an NHWC sample, the padding behind a last group."""
    if mutant == M_HALVES:
        lo, hi = hi, lo
    sample[written, c0:c0 + 3] = to_f16(lo, mutant)[written]
    sample[written, c0 + 3:c0 + 6] = to_f16(hi, mutant)[written]
    if (out_c == 8 or c0 + 12 > out_c) and mutant != M_PADDING:
        sample[written, c0 + 6:] = 0


def pairs_expected(case: PairCase, mutant=None) -> np.ndarray:
    geo = BY_ID[case.gid]
    jobs, n_slots = pairs_jobs(case)
    out = blank((n_slots, geo.crop, geo.crop, case.out_c), np.float16)
    w = _written(geo.crop, mutant)
    for k, (ca, _, cha, cb, _, chb, slot) in enumerate(jobs):
        if mutant == M_MINUS_8 and k >= 8:
            slot = jobs[k - 8][6]
        va = normalised(crop_u8(geo, ca, None, mutant), lut(case.kind))
        vb = normalised(crop_u8(geo, cb, None, mutant), lut(case.kind))
        lo, hi = (va, vb) if cha < chb else (vb, va)
        _put_pair(out[slot], geo, min(cha, chb), lo, hi, case.out_c, mutant, w)
    return out


PhaseCase = namedtuple("PhaseCase", "gid content out_c a_first c0 kind")   # ONE render: its image, the pair's second image = the next content


def phase_h_cases():
    """The fused tile phase: extreme contents (and noise, ramp) on the crop > 256 geometry, the non-square one, the odd difference and the
    anchor, both channel orders, out_c 8 and 16 (16: the first group -- channels 6 .. 15 untouched -- and the last, its padding zero)."""
    combos = [(8, True, 0), (16, False, 6), (16, True, 0), (8, False, 0)]
    cases = [PhaseCase(g.id, content, oc, af, c0, "imagenet") for g in (G_WIDE, G_NARROW, G_ODD, ANCHOR) for content in CONTENTS for oc, af, c0 in combos]
    return cases + [PhaseCase(G_NARROW.id, "ramp", 16, True, 6, "ties")]


def phase_h_second(case: PhaseCase) -> str:
    return CONTENTS[(CONTENTS.index(case.content) + 3) % 7]


def phase_h_expected(case: PhaseCase, mutant=None) -> np.ndarray:
    """fp16 [3, crop, crop, out_c]: the render's sample is slot 1, slots 0 and 2 keep the sentinel."""
    geo = BY_ID[case.gid]
    out = blank((3, geo.crop, geo.crop, case.out_c), np.float16)
    va = normalised(crop_u8(geo, case.content, None, mutant), lut(case.kind))
    vb = normalised(crop_u8(geo, phase_h_second(case), None, None if mutant in (M_XROWS, M_CROP_UP, M_TIE, M_ONE_ROUNDING) else mutant), lut(case.kind))
    w = np.ones((geo.crop, geo.crop), dtype=bool)   # (a thread per column: no block of 256 pixels here)
    if mutant == M_COL_GROUP:
        w[:, 256:] = False
    lo, hi = (va, vb) if case.a_first else (vb, va)
    _put_pair(out[1], geo, case.c0, lo, hi, case.out_c, mutant, w)
    return out


# ------------------------------------------------------------------------------------------------ salve_bev_train_tiles
TrainCase = namedtuple("TrainCase", "gid batch per_sample out_c")


def train_cases():
    """Batches 1 / 7 / 8 / 9 / 17, per_sample 1 .. 3 with out_c 8 / 16 / 24 (and a buffer wider than the sample needs)."""
    shapes = [(1, 1, 8), (7, 2, 16), (8, 3, 24), (9, 3, 24), (17, 1, 8), (9, 1, 16), (17, 2, 16), (7, 2, 24)]
    return [TrainCase(g, b, ps, oc) for g in (G_NARROW.id, G_ODD.id) for b, ps, oc in shapes]


def train_jobs(case: TrainCase):
    """(jobs_a, jobs_b, draws): jobs [batch][per_sample] of (content, image index, chan); sample s draws draws[(5 s + 2) % 24]; image k of
    a sample takes the group 6 k, its halves alternate with s + k."""
    geo = BY_ID[case.gid]
    d = draws(geo)
    ja, jb, dr = [], [], []
    for s in range(case.batch):
        dr.append(d[(5 * s + 2) % len(d)])
        for k in range(case.per_sample):
            a_first = (s + k) % 2 == 0
            ia, ib = (2 * s + 3 * k) % 7, (4 * s + k + 6) % 7
            ja.append((CONTENTS[ia], IMAGE_ORDER[ia], 6 * k + (0 if a_first else 3)))
            jb.append((CONTENTS[ib], IMAGE_ORDER[ib], 6 * k + (3 if a_first else 0)))
    return ja, jb, dr


def train_expected(case: TrainCase, mutant=None) -> np.ndarray:
    """float32 [batch, crop, crop, out_c]: every channel written, the ones no job names zero (bf16: `to_bf16_bits` of it)."""
    geo = BY_ID[case.gid]
    ja, jb, dr = train_jobs(case)
    out = blank((case.batch, geo.crop, geo.crop, case.out_c), np.float32)
    w = _written(geo.crop, mutant)
    for s in range(case.batch):
        to = s - 8 if mutant == M_MINUS_8 and s >= 8 else s
        px = np.zeros((geo.crop, geo.crop, case.out_c), dtype=np.float32)
        named = np.zeros(case.out_c, dtype=bool)
        for content, _, chan in ja[s * case.per_sample:(s + 1) * case.per_sample] + jb[s * case.per_sample:(s + 1) * case.per_sample]:
            px[..., chan:chan + 3] = normalised(crop_u8(geo, content, dr[s], mutant), lut())
            named[chan:chan + 3] = True
        keep = named if mutant == M_PADDING else np.ones(case.out_c, dtype=bool)
        sel = w[..., None] & keep[None, None, :]
        out[to][sel] = px[sel]
    return out


# ------------------------------------------------------------------------------------------------ salve_resize_rgb_u8, salve_bev_export_u8
RESIZE_SIZES = (((6, 10), (3, 5)),      # both ratios exactly 2: the box mean
                ((6, 10), (3, 6)),      # one ratio only: the bilinear path
                ((5, 7), (11, 13)),     # up-scale
                ((1, 9), (4, 4)),       # one source row
                ((40, 24), (17, 31)),   # 2 x 17 x 31 = 1054 pixels: four full blocks of 256 and a partial one
                ((7, 9), (7, 9)),       # equal sizes: identity taps
                ((32, 32), (16, 16)))   # the box mean over exactly two blocks of 256
RESIZE_CONTENTS = (("cells", "checker"), ("noise", "ramp"), ("columns", "rows"), ("white", "black"))   # two images per call


def resize_cases():
    return [(src, dst, pair) for src, dst in RESIZE_SIZES for pair in RESIZE_CONTENTS]


def resize_expected(case, mutant=None) -> np.ndarray:
    """uint8 [2, dst_h, dst_w, 3]."""
    (H, W), (h, w), pair = case
    out = blank((2, h, w, 3), np.uint8)
    box = (H == 2 * h or W == 2 * w) if mutant == M_BOX else (H == 2 * h and W == 2 * w)
    for n, content in enumerate(pair):
        img = image(H, W, content)
        if box:
            p = (img[..., ::-1] if mutant == M_BGR else img).astype(np.int64)
            yy, xx = np.minimum(2 * np.arange(h), H - 2 if H > 1 else 0), np.minimum(2 * np.arange(w), W - 2)
            r = (p[yy][:, xx] + p[yy][:, xx + 1] + p[np.minimum(yy + 1, H - 1)][:, xx] + p[np.minimum(yy + 1, H - 1)][:, xx + 1] + (1 if mutant == M_TIE else 2)) >> 2
            out[n] = r.astype(np.uint8)
        else:
            out[n] = resize_u8(img, taps(h, H), taps(w, W), mutant)
    if mutant == M_LAST_BLOCK and (2 * h * w) % 256:
        out.reshape(-1, 3)[2 * h * w // 256 * 256:] = blank((1,), np.uint8)[0]
    return out


EXPORT_HW = (19, 23)   # 2 x 19 x 23 = 874 words: three full blocks and a partial one


def export_case():
    """uint32 [2, 19, 23] words of the ramp and the noise image with the top byte SET (0xA5, 0xFF)."""
    return np.stack([pack(image(*EXPORT_HW, "ramp"), 0xA5), pack(image(*EXPORT_HW, "noise"), 0xFF)])


def export_expected(mutant=None) -> np.ndarray:
    out = np.stack([image(*EXPORT_HW, "ramp"), image(*EXPORT_HW, "noise")]).copy()
    if mutant == M_BGR:
        out = out[..., ::-1].copy()
    if mutant == M_LAST_BLOCK:
        out.reshape(-1, 3)[out.size // 3 // 256 * 256:] = blank((1,), np.uint8)[0]
    return out


# ------------------------------------------------------------------------------------------------ every entry through one door
def entry_cases(entry: str):
    return {"tiles": tiles_cases, "aug": aug_cases, "pairs": pairs_cases, "train": train_cases, "phase_h": phase_h_cases,
            "resize_rgb": resize_cases, "export": lambda: [None]}[entry]()


def entry_expected(entry: str, case, mutant=None) -> np.ndarray:
    if entry == "export":
        return export_expected(mutant)
    return {"tiles": tiles_expected, "aug": aug_expected, "pairs": pairs_expected, "train": train_expected, "phase_h": phase_h_expected,
            "resize_rgb": resize_expected}[entry](case, mutant)
