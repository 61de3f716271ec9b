"""salve_bev_train_tiles_jitter (include/salve_hip.h): the case tables and an emulator of its DOCUMENTED output --
torchvision's tensor ColorJitter (functional_tensor.py of torchvision 0.11 / 0.12) on the uint8 resized image, between Resize and
Crop -- in numpy float32, elementwise, sharing no code with the library.  The resize, the normalisation table and the bf16 rounding
are tile_cases', by import.  tests/test_jitter_cases_host.py pins the emulator to a restatement of the torchvision functions in torch
operations (torchvision itself is not installed where this suite runs: parity with it stays unpinned) and shows that fourteen
emulated wrong kernels fail the cases; tests/test_gpu_jitter.py compares the kernels with it bit for bit.

The arithmetic: float32, one rounding per operation (numpy's elementwise ufuncs: no fused multiply-add).  trunc8(v): v clamped to
[0, 255], truncated.  grey = trunc8((0.2989f r + 0.587f g) + 0.114f b).  blend(x, y, f) = trunc8(f x + f_c y) with f_c =
float32(1.0 - (double) f).  brightness: blend(x, 0, b); saturation: blend(x, grey(pixel), s); contrast: blend(x, m, c) with m =
float32(S) / float32(N), S the integer sum of grey over the N = resize^2 pixels of the WHOLE resized image as the operations in front
of contrast left it; hue: x / 255 -> _rgb2hsv -> remainder(h + hue, 1) -> _hsv2rgb -> (byte)(c * 255).  Per image: the four operations
in the record's order, those whose mask bit is clear skipped.
"""

import functools
import itertools
from collections import namedtuple

import numpy as np

import tile_cases as tc

F = np.float32
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3      # torchvision's fn_id; the mask's bit numbers
FULL = 15
ORDERS = tuple(itertools.permutations(range(4)))         # all 24
Rec = namedtuple("Rec", "order mask b c s h")            # one image's draw
IDENTITY = Rec((0, 1, 2, 3), 7, 1.0, 1.0, 1.0, 0.0)      # factors 1, hue disabled: the image itself

# ---- the emulated wrong kernels (tests/test_jitter_cases_host.py: each fails at least one case)
M_MEAN_CROP = "mean over the crop"
M_MEAN_RECIP = "mean as sum times reciprocal"
M_MEAN_UNTOUCHED = "mean of the untouched image when contrast is not first"
M_COMPLEMENT_F32 = "complement formed in float32"
M_BLEND_FUSED = "blend with one rounding"
M_ROUND_NEAREST = "store rounded to nearest"
M_NO_CLAMP = "clamp missing"
M_GREY_FLOAT = "grey not truncated"
M_GREY_DOUBLE = "grey constants in double"
M_ONE_DRAW = "one draw per sample"
M_ORDER_REVERSED = "order reversed"
M_REM_NO_PLUS = "remainder without the + 1"
M_HUE_NEW_FORM = "hue stored with the 255 + 1 - 1e-3 form"
M_HUE_MASKS = "hue masks without the maxc != r terms"
MUTANTS = (M_MEAN_CROP, M_MEAN_RECIP, M_MEAN_UNTOUCHED, M_COMPLEMENT_F32, M_BLEND_FUSED, M_ROUND_NEAREST, M_NO_CLAMP, M_GREY_FLOAT,
           M_GREY_DOUBLE, M_ONE_DRAW, M_ORDER_REVERSED, M_REM_NO_PLUS, M_HUE_NEW_FORM, M_HUE_MASKS)


# ------------------------------------------------------------------------------------------------ the operations
def complement(f: float, mutant=None) -> np.float32:
    if mutant == M_COMPLEMENT_F32:
        return F(1.0) - F(f)
    return F(1.0 - float(f))     # (f: the Python float the caller holds; for a float32 draw both forms agree, for any other they need not)


def trunc8(v: np.ndarray, mutant=None) -> np.ndarray:
    """float32 -> uint8: clamp to [0, 255], truncate toward zero."""
    v = np.asarray(v, dtype=F)
    if mutant == M_ROUND_NEAREST:
        v = np.rint(v)
    if mutant == M_NO_CLAMP:    # the conversion wraps instead
        return (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)
    return np.minimum(np.maximum(v, F(0)), F(255)).astype(np.uint8)


def grey_f32(img: np.ndarray, mutant=None) -> np.ndarray:
    x = img.astype(F)
    if mutant == M_GREY_DOUBLE:
        x64 = img.astype(np.float64)
        return (0.2989 * x64[..., 0] + 0.587 * x64[..., 1] + 0.114 * x64[..., 2]).astype(F)
    return (F(0.2989) * x[..., 0] + F(0.587) * x[..., 1]) + F(0.114) * x[..., 2]


def grey(img: np.ndarray, mutant=None) -> np.ndarray:
    """uint8 [..., 3] -> the grey level, uint8 (float32 under M_GREY_FLOAT)."""
    g = grey_f32(img, mutant)
    return g if mutant == M_GREY_FLOAT else trunc8(g, mutant if mutant in (M_ROUND_NEAREST, M_NO_CLAMP) else None)


def blend(img: np.ndarray, other, f: float, mutant=None) -> np.ndarray:
    """uint8 [..., 3] and `other` (a float32 scalar, or an array [...] broadcast over the channels)."""
    x = img.astype(F)
    y = np.asarray(other, dtype=F)
    y = y[..., None] if y.ndim else y
    fc = complement(f, mutant)
    if mutant == M_BLEND_FUSED:   # products exact in double, the sum rounded once
        v = (np.float64(F(f)) * x.astype(np.float64) + np.float64(fc) * y.astype(np.float64)).astype(F)
    else:
        v = F(f) * x + fc * y
    return trunc8(v, mutant)


def mean_grey(img: np.ndarray, mutant=None) -> np.float32:
    g = grey(img, mutant)
    n = g.size
    if mutant == M_GREY_FLOAT:
        return F(F(g.astype(np.float64).sum()) / F(n))
    s = int(g.astype(np.int64).sum())
    assert 255 * n < 2 ** 24, "the contract: resize * resize * 255 < 2^24"
    if mutant == M_MEAN_RECIP:
        return F(s) * (F(1.0) / F(n))
    return F(s) / F(n)


def hue(img: np.ndarray, h: float, mutant=None) -> np.ndarray:
    x = img.astype(F) / F(255.0)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eqc, one, maxc)
    d = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    zero = np.zeros_like(maxc)
    if mutant == M_HUE_MASKS:
        hr = np.where(maxc == r, bc - gc, zero)
        hg = np.where(maxc == g, (F(2.0) + rc) - bc, zero)
        hb = np.where(maxc == b, (F(4.0) + gc) - rc, zero)
    else:
        hr = np.where(maxc == r, bc - gc, zero)
        hg = np.where((maxc == g) & (maxc != r), (F(2.0) + rc) - bc, zero)
        hb = np.where((maxc != g) & (maxc != r), (F(4.0) + gc) - rc, zero)
    hh = np.fmod(((hr + hg) + hb) / F(6.0) + F(1.0), F(1.0))
    m = np.fmod(hh + F(h), F(1.0))                       # torch's remainder: fmod, and + 1 where that is negative
    if mutant != M_REM_NO_PLUS:
        m = np.where((m != 0) & (m < 0), m + F(1.0), m)
    hh = m.astype(F)
    h6 = hh * F(6.0)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int32) % 6
    clamp01 = lambda v: np.minimum(np.maximum(v, F(0)), F(1))
    v = maxc
    p = clamp01(v * (F(1.0) - s))
    q = clamp01(v * (F(1.0) - s * f))
    t = clamp01(v * (F(1.0) - s * (F(1.0) - f)))
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], -1).astype(F)
    if mutant == M_HUE_NEW_FORM:
        return (out * F(255 + 1 - 1e-3)).astype(np.uint8)
    return (out * F(255.0)).astype(np.uint8)


def jitter_image(resized: np.ndarray, rec: Rec, crop_box=None, mutant=None) -> np.ndarray:
    """uint8 [R, R, 3] -> uint8 [R, R, 3]: the record's enabled operations in its order.  crop_box (oy, ox, crop): only M_MEAN_CROP reads it."""
    img = resized
    order = rec.order[::-1] if mutant == M_ORDER_REVERSED else rec.order
    for op in order:
        if not (rec.mask >> op) & 1:
            continue
        if op == BRIGHTNESS:
            img = blend(img, F(0), rec.b, mutant)
        elif op == CONTRAST:
            src = resized if mutant == M_MEAN_UNTOUCHED else img
            if mutant == M_MEAN_CROP and crop_box is not None:
                oy, ox, c = crop_box
                src = src[oy:oy + c, ox:ox + c]
            img = blend(img, mean_grey(src, mutant), rec.c, mutant)
        elif op == SATURATION:
            img = blend(img, grey(img, mutant), rec.s, mutant)
        else:
            img = hue(img, rec.h, mutant)
    return img


# ------------------------------------------------------------------------------------------------ contents and records
N_IMAGES = 7
BORDER = (255, 250, 240)


@functools.lru_cache(maxsize=None)
def images(geo) -> np.ndarray:
    """uint8 [7, h, w, 3]: noise, each with a bright border as wide as the resized rows and columns in front of the smallest offset
    `draws` takes: it lies outside every crop, so a mean taken over the crop differs from the image's."""
    rng = np.random.default_rng(77 * geo.h + geo.w)
    im = rng.integers(0, 256, size=(N_IMAGES, geo.h, geo.w, 3)).astype(np.uint8)
    im[3] //= 3            # a dark one and a bright one: blends that clamp at both ends
    im[5] = 255 - im[5] // 4
    lo = (geo.resize - geo.crop) // 3
    by, bx = max(lo * geo.h // geo.resize, 1), max(lo * geo.w // geo.resize, 1)
    for a in (im[:, :by], im[:, -by:], im[:, :, :bx], im[:, :, -bx:]):
        a[...] = BORDER
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def resized(geo) -> np.ndarray:
    r = np.stack([tc.resize_u8(im, tc.taps(geo.resize, geo.h), tc.taps(geo.resize, geo.w)) for im in images(geo)])
    r.setflags(write=False)
    return r


def draws(geo, batch):
    """(crop_y, crop_x, flags) per sample: offsets inside the middle third of their range, every flip."""
    m = geo.resize - geo.crop
    lo, hi = m // 3, m - m // 3
    return [(lo + (3 * s) % (hi - lo + 1), lo + (5 * s + 1) % (hi - lo + 1), (s + 1) % 4) for s in range(batch)]


MASKS = (FULL, 1, 2, 4, 8, 7, 11, 13, 14, 3, 5, 6, 9, 10, 12, 0)   # the full mask, every single operation, then every other subset
EDGE_FACTORS = (0.5, 1.0, 1.5)
EDGE_HUES = tuple(float(F(h)) for h in (-0.05, 0.0, 0.05))   # (the float32 ends, as uniform_ on a float32 tensor gives them)


def record(n: int) -> Rec:
    """Record n of a case: the orders and masks cycle with coprime strides (54 records of a batch of nine show all 24 orders and all 16
    masks); every third record takes its factors from the interval ends, the others uniform draws in double."""
    rng = np.random.default_rng(1234 + n)
    if n % 3 == 0:
        b, c, s = (EDGE_FACTORS[(n // 3 + k) % 3] for k in range(3))
        h = EDGE_HUES[(n // 3) % 3]
    else:
        b, c, s = (float(rng.uniform(0.5, 1.5)) for _ in range(3))   # doubles, as a caller of the adjust_* functions may pass them
        h = float(rng.uniform(-0.05, 0.05))
    return Rec(ORDERS[(5 * n + 3) % 24], MASKS[(3 * n) % 16], b, c, s, h)


JCase = namedtuple("JCase", "gid batch per_sample out_c narrow", defaults=(False,))
G_A, G_B = tc.BY_ID["41x37-30-24"], tc.BY_ID["33x33-33-17"]

# (geometry, image, contrast factor), found by search: contrast alone on that image gives another byte somewhere when the mean is formed
# as sum * (1 / N) -- the two means differ in the last bit on these images (N = 900, 1089), and this factor puts a pixel on the edge.
# The random records above do not show it (tests/test_jitter_cases_host.py checks that these do).
NARROW = (("41x37-30-24", 0, 1.4970102930724918), ("41x37-30-24", 2, 0.8417426502061353), ("41x37-30-24", 6, 1.2138786034477889),
          ("33x33-33-17", 5, 0.7132704314847419))


def cases():
    """Both geometries, batches 1 and 9 (9 straddles the kernel's group of eight samples), per_sample 1 .. 3; then the NARROW records,
    a sample each."""
    return ([JCase(g.id, b, ps, oc) for g in (G_A, G_B) for b in (1, 9) for ps, oc in ((1, 8), (2, 16), (3, 24))]
            + [JCase(g.id, sum(n[0] == g.id for n in NARROW), 1, 8, True) for g in (G_A, G_B)])


def jobs(case: JCase):
    """(jobs_a, jobs_b, records, draws): jobs [batch][per_sample] of (image index, chan); image k of a sample takes the group 6 k, its
    halves alternating with s + k; records [batch][2 * per_sample] by channel group."""
    geo = tc.BY_ID[case.gid]
    G = 2 * case.per_sample
    ja, jb = [], []
    if case.narrow:   # sample s: NARROW's image under contrast alone in group 0, another image under a common record in group 1
        mine = [n for n in NARROW if n[0] == case.gid]
        ja, jb = [(image, 0) for _, image, _ in mine], [((image + 3) % N_IMAGES, 3) for _, image, _ in mine]
        recs = [[Rec((1, 0, 2, 3), 1 << CONTRAST, 1.0, c, 1.0, 0.0), record(100 + s)] for s, (_, _, c) in enumerate(mine)]
        return ja, jb, recs, draws(geo, case.batch)
    for s in range(case.batch):
        for k in range(case.per_sample):
            a_first = (s + k) % 2 == 0
            ja.append(((2 * s + 3 * k) % N_IMAGES, 6 * k + (0 if a_first else 3)))
            jb.append(((4 * s + k + 6) % N_IMAGES, 6 * k + (3 if a_first else 0)))
    recs = [[record(s * G + g + 7 * case.per_sample) for g in range(G)] for s in range(case.batch)]
    return ja, jb, recs, draws(geo, case.batch)


def crop_flip(img: np.ndarray, geo, draw) -> np.ndarray:
    oy, ox, flags = draw
    c = img[oy:oy + geo.crop, ox:ox + geo.crop]
    c = c[::-1] if flags & tc.VFLIP else c
    return c[:, ::-1] if flags & tc.HFLIP else c


def expected(case: JCase, mutant=None, records=None) -> np.ndarray:
    """float32 [batch, crop, crop, out_c]: every channel written, the ones no job names zero (bf16: `tc.to_bf16_bits` of it).
    records: other records than `jobs`' (the identity test)."""
    geo = tc.BY_ID[case.gid]
    ja, jb, recs, dr = jobs(case)
    recs = recs if records is None else records
    rs = resized(geo)
    out = np.zeros((case.batch, geo.crop, geo.crop, case.out_c), dtype=F)
    for s in range(case.batch):
        for image, chan in ja[s * case.per_sample:(s + 1) * case.per_sample] + jb[s * case.per_sample:(s + 1) * case.per_sample]:
            rec = recs[s][0] if mutant == M_ONE_DRAW else recs[s][chan // 3]
            j = jitter_image(rs[image], rec, (dr[s][0], dr[s][1], geo.crop), mutant)
            out[s, ..., chan:chan + 3] = tc.normalised(crop_flip(j, geo, dr[s]), tc.lut())
    return out


# ------------------------------------------------------------------------------------------------ the colour lattice
LEVELS = np.concatenate([np.arange(0, 64), np.arange(192, 256)]).astype(np.uint8)   # 128 levels: the dark and the bright quarter
LATTICE_SIDE, LATTICE_IMAGES = 256, 32                                              # 128^3 colours = 32 images of 256 x 256


@functools.lru_cache(maxsize=None)
def lattice() -> np.ndarray:
    """uint8 [32, 256, 256, 3]: every triple of LEVELS once (every hue sector, every tie of maxc / minc, truncations at both ends)."""
    n = np.arange(128 ** 3)
    im = np.stack([LEVELS[n % 128], LEVELS[(n // 128) % 128], LEVELS[n // 16384]], -1).reshape(LATTICE_IMAGES, LATTICE_SIDE, LATTICE_SIDE, 3)
    im.setflags(write=False)
    return im


def lattice_record(i: int, run: str) -> Rec:
    """Image i's record.  "colour": saturation, hue and brightness at the interval ends, contrast disabled, six orders; "contrast":
    contrast first, then the three others in six orders, all enabled."""
    e = (0.5, 1.5)
    three = tuple(itertools.permutations((BRIGHTNESS, SATURATION, HUE)))[i % 6]
    if run == "colour":
        return Rec((CONTRAST,) + three, FULL & ~(1 << CONTRAST), e[i & 1], 1.0, e[(i >> 1) & 1], EDGE_HUES[i % 3])
    return Rec((CONTRAST,) + three, FULL, e[(i >> 2) & 1], e[i & 1], e[(i >> 1) & 1], EDGE_HUES[(i + 1) % 3])


def lattice_expected(run: str, first: int, count: int) -> np.ndarray:
    """uint8 [count, 256, 256, 3]: images first .. first + count - 1 of the lattice under their records."""
    return np.stack([jitter_image(lattice()[i], lattice_record(i, run)) for i in range(first, first + count)])
