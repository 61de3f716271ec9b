"""Cases for the densify stage -- `bev_densify_kernel` (salve_amd/csrc/bev_render.hip) behind `salve_bev_keys_from_pixels` and
`salve_bev_densify` -- across the configuration space `make_devcfg` and `bev_stage` accept, and what the oracle computes for each of
them (not a test module; numpy and the oracle only).

The contract, restated here from include/salve_hip.h and the constants of the source (`refusal`): 2 <= bev_h, bev_w < 2048; mask_k odd,
1 .. 17; no out_flags bit beyond 1 | 2 | 4; ceil(bev_h / 16) * ceil(bev_w / 32) <= 512 mask tasks; and the LDS block of the image at most
160 KB -- a bound that no image within the task bound reaches (`max_lds_bytes_within_the_task_bound`: 85 KB), so no named shape moves
to the refused list on its account.

A case is (H, W, site family, mask_k, out_flags).  `sites(family, H, W, mask_k)` gives the explicit pixels and colours; `expected(case)`
the sparse image, the exact interpolant, the mask (`box_dilate(nonempty_mask(sparse), mask_k)`, unflipped) and the final image: the
interpolant times the mask unless bit 2 is set, flipped unless bit 1 is set, all zero for a degenerate site set.

"Non-empty" is not "occupied": the mask grows from the pixels whose uint8 channel product is non-zero MODULO 256, the triangulation uses
every site, and occupied pixels outside the mask are zeroed.  The `wrap` family puts sites whose product wraps to zero -- (16, 16, 1),
(2, 128, 1), (64, 4, 3) -- or is zero -- (0, 9, 9) -- at distances p - 1, p, p + 1 (p = mask_k // 2) around lone non-empty sites; the `gap`
family puts pairs of 2 x 2 clusters whose facing sites are w = 1 .. 18 pixels apart, w = mask_k and mask_k + 1 first, so that the masks of
the two just meet (w <= mask_k) or just miss, anchored so that one cluster's mask ends ON the first pixel beyond a 32-bit word boundary
(31 | 32, 63 | 64: the carries `prev >> (32 - d)`, `next << (32 - d)` of the horizontal dilation at d = p) or a 16-row task boundary
(15 | 16, 31 | 32: the outermost halo row of the vertical dilation).

`emulate(case, mutant)` is the kernel's mask pass in numpy, word by word and task by task, with ONE mistake (`MUTANTS`); without one it
must equal the oracle (tests/test_densify_cases_host.py), and every mutant must change the image of some case: the table bites before
it is run on a device.
"""

import functools
from collections import namedtuple

import numpy as np

from oracle import bev_oracle as bo

# ---------------------------------------------------------------------------------------------------- the contract
SD_MAX_DIM = 2048            # star_delaunay.h: coordinates below 2048
MASK_ROWS_PER_TASK = 16      # bev_render.hip: a mask task = one 32-pixel column word x 16 rows ...
MASK_MAX_HALF = 8            # ... with a halo of 8 rows on either side: mask_k <= 17
DENSIFY_THREADS = 512        # one thread per mask task
N_SCAL, SD_CACHE_SIZE = 24, 1536
LDS_LIMIT = 160 * 1024
KNOWN_OUT_FLAGS = 7          # 1: no flip, 2: no mask, 4: given order
TRI_CACHE_MAX_DIM = 1024     # above it in either dimension the general walk runs without its triangle cache
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2

Refusal = namedtuple("Refusal", "code where reason")   # where: "config" (every entry, 0 workspace bytes) or "densify" (that call alone)


def mask_tasks(H, W):
    return -(-H // MASK_ROWS_PER_TASK) * -(-W // 32)


def lds_bytes(H, W):
    """`densify_lds_bytes`: two bitmaps, two int16 row extents, the scalars, the triangle cache."""
    wpr = (W + 31) // 32
    return 2 * H * wpr * 4 + 2 * ((H + 1) & ~1) * 2 + N_SCAL * 4 + 8 + SD_CACHE_SIZE * 8


def refusal(H, W, mask_k=11, out_flags=0):
    """None if the configuration is accepted, else how the library refuses it (`make_devcfg`'s order, then `bev_stage`'s LDS check)."""
    if H < 2 or W < 2 or H >= SD_MAX_DIM or W >= SD_MAX_DIM:
        return Refusal(ERR_BAD_ARG, "config", "bev size out of range")
    if mask_k < 1 or mask_k % 2 == 0 or mask_k // 2 > MASK_MAX_HALF:
        return Refusal(ERR_BAD_ARG, "config", "mask_k must be odd and <= 17")
    if out_flags & ~KNOWN_OUT_FLAGS:
        return Refusal(ERR_BAD_ARG, "config", "unknown bit in out_flags")
    if mask_tasks(H, W) > DENSIFY_THREADS:
        return Refusal(ERR_BAD_ARG, "config", f"{mask_tasks(H, W)} mask tasks, at most {DENSIFY_THREADS}")
    if lds_bytes(H, W) > LDS_LIMIT:
        return Refusal(ERR_UNSUPPORTED, "densify", f"{lds_bytes(H, W)} bytes of LDS, at most {LDS_LIMIT}")
    return None


def max_lds_bytes_within_the_task_bound():
    """The largest LDS block of any image the task bound lets through: for every count of row tasks, the tallest image and the widest
    row that still fit."""
    best = 0
    for row_tasks in range(1, -(-(SD_MAX_DIM - 1) // MASK_ROWS_PER_TASK) + 1):
        H = min(row_tasks * MASK_ROWS_PER_TASK, SD_MAX_DIM - 1)
        W = min((DENSIFY_THREADS // row_tasks) * 32, SD_MAX_DIM - 1)
        if W >= 2:
            assert mask_tasks(H, W) <= DENSIFY_THREADS
            best = max(best, lds_bytes(H, W))
    return best


# (H, W).  512 x 512, 1024 x 256, 2047 x 127 and 127 x 2047 have exactly 512 mask tasks; 1025 x 40 and 40 x 1025 and the 2047s run without
# the triangle cache; 33 x 32 is one full word per row, 17 x 33 and 64 x 65 one pixel more than full words, 3 x 2 and 2 x 2 the smallest.
SHAPES = ((2, 2), (3, 2), (17, 33), (33, 32), (64, 65), (48, 300), (300, 48), (512, 512), (1024, 256), (1025, 40), (40, 1025), (2047, 127),
          (127, 2047))
REFUSED_SHAPES = {
    (513, 512): "33 x 16 = 528 mask tasks",
    (1025, 255): "65 x 8 = 520 mask tasks",
    (2048, 16): "bev_h = 2048: coordinates must stay below 2048",
    (16, 2048): "bev_w = 2048",
    (1, 8): "bev_h = 1: an image has at least two rows",
}
REFUSED_MASK_K = (0, 2, 19)
REFUSED_OUT_FLAGS = (8,)
SWEEP_SHAPES = ((33, 32), (300, 48), (1025, 40))
SWEEP_MASK_K = (1, 3, 9, 15, 17)
SWEEP_OUT_FLAGS = (0, 1, 2, 3)
SHAPE_CLASSES = {"small": (33, 32), "wide": (48, 300), "tall": (300, 48), "above 1024": (1025, 40)}   # the poisoned-workspace reruns

SITE_BUDGET = 4500
FAMILIES = ("random2", "random25", "ring", "diagonal", "gap", "border", "wrap")
DEGENERATE = ("three", "column", "row", "four-in-row", "empty")
# the family (families) every shape runs with (mask_k, out_flags) = (11, 0)
SHAPE_FAMILIES = {
    (2, 2): ("border",), (3, 2): ("border", "random25"), (17, 33): ("random25", "ring"), (33, 32): ("ring", "border"), (64, 65): ("gap", "wrap"),
    (48, 300): ("random2", "diagonal"), (300, 48): ("wrap", "random25"), (512, 512): ("random25", "ring"), (1024, 256): ("diagonal", "gap"),
    (1025, 40): ("border", "random2"), (40, 1025): ("random2", "gap"), (2047, 127): ("diagonal", "random25"), (127, 2047): ("ring", "wrap"),
}
WRAP_COLOURS = ((16, 16, 1), (2, 128, 1), (0, 9, 9), (64, 4, 3))   # channel products 256, 256, 0, 768: "empty" to the mask, occupied to the rest

Case = namedtuple("Case", "id H W family mask_k out_flags want_mask")
Sites = namedtuple("Sites", "pts col gaps")   # pts int64 [n, 2] (x, y), distinct; col uint8 [n, 3]; gaps: the gap family's records
Gap = namedtuple("Gap", "axis w between")     # between: int64 [m, 2] (x, y), the pixels strictly between the facing sites (both lines)
Expected = namedtuple("Expected", "sparse interp mask final sites degenerate")


# ---------------------------------------------------------------------------------------------------- site sets
def odd_colours(pts):
    """Three odd channels: an odd product, non-empty whatever wraps."""
    x, y = pts[:, 0], pts[:, 1]
    return np.stack([(2 * (x * 7 + y * 3) + 1) % 256, (2 * (x * 5 + 11) + 1) % 256, (2 * (y * 13) + 1) % 256], 1).astype(np.uint8)


def _random(H, W, dens, seed):
    """White noise of density `dens` (random colours: a few are empty or wrap by themselves) over the whole image, or, where that
    would exceed the site budget, over a box in the far corner -- the largest coordinates -- plus one site at the origin."""
    bh, bw = H, W
    while bh * bw * dens > 0.8 * SITE_BUDGET:
        if bh >= bw:
            bh = max(2, bh * 3 // 4)
        else:
            bw = max(2, bw * 3 // 4)
    rng = np.random.default_rng(seed + 7919 * H + W)
    pts = np.argwhere(rng.random((bh, bw)) < dens)[:, ::-1] + np.array([W - bw, H - bh])
    if (bh, bw) != (H, W):
        pts = np.concatenate([pts, [[0, 0]]])
    return pts, rng.integers(0, 256, size=(len(pts), 3)).astype(np.uint8)


def _ring(H, W):
    th = np.linspace(0, 2 * np.pi, 2 * max(H, W), endpoint=False)
    pts = np.round(np.stack([(W - 1) / 2.0 + 0.45 * W * np.cos(th), (H - 1) / 2.0 + 0.45 * H * np.sin(th)], 1)).astype(np.int64)   # empty interior
    return pts, None


def _diagonal(H, W):
    """A band three pixels wide along the diagonal whose sites are 3 ... 200 pixels apart along the longer axis: the hull triangles are
    long and thin, and the spacings 126 .. 129 sit on either side of what the int8 relative-vertex field of a queue entry holds."""
    major, minor = max(H, W), min(H, W)
    steps, t, k, at = (3, 17, 64, 126, 127, 128, 129, 7, 200, 1), 0, 0, []
    while t < major:
        at.append((t, min(minor - 1, max(0, round(t * (minor - 1) / max(1, major - 1)) + k % 3 - 1))))
        t += steps[k % len(steps)]
        k += 1
    at.append((major - 1, minor - 1))
    pts = np.array(at, dtype=np.int64)
    return (pts if W >= H else pts[:, ::-1]), None


def _border(H, W):
    """All four borders (every pixel, or every step-th where the perimeter exceeds the budget), the four corners, the centre; random
    colours, so that some border sites are empty."""
    step = max(1, -(-2 * (H + W) // 3000))
    xs, ys = np.union1d(np.arange(0, W, step), [W - 1]), np.union1d(np.arange(0, H, step), [H - 1])
    pts = np.concatenate([np.stack([xs, np.zeros_like(xs)], 1), np.stack([xs, np.full_like(xs, H - 1)], 1), np.stack([np.zeros_like(ys), ys], 1),
                          np.stack([np.full_like(ys, W - 1), ys], 1), [[W // 2, H // 2]]])
    pts = np.unique(pts, axis=0)
    return pts, np.random.default_rng(11 + H * 4099 + W).integers(0, 256, size=(len(pts), 3)).astype(np.uint8)


def _gap(H, W, mask_k):
    """Pairs of 2 x 2 clusters whose facing sites are w pixels apart along x or along y, w = mask_k and mask_k + 1 first, then the rest of
    1 .. 18, as many as the image holds with more than p + 1 pixels between any two pairs (no pair's mask reaches another's gap).
    Side "lo": the first cluster's facing site lies max(p, 1) below a boundary B (column 32 or 64, row 16 or 32), so its mask ends ON
    pixel B; side "hi": the second cluster's lies max(p, 1) - 1 above it, so its mask ends on pixel B - 1.  Where the image is too small for
    an anchored pair it starts at pixel 1 instead."""
    p = mask_k // 2
    q = max(p, 1)
    jobs = [(w, axis, side) for side in ("lo", "hi") for axis in ("x", "y") for w in (mask_k, mask_k + 1)]   # a small image holds these first
    jobs += [(w, axis, side) for w in range(1, 19) if w not in (mask_k, mask_k + 1) for axis in ("x", "y") for side in ("lo", "hi")]
    placed, pts, gaps, turn = [], [], [], 0

    def free(r):
        return all(r[0] - (p + 1) > s[2] or s[0] - (p + 1) > r[2] or r[1] - (p + 1) > s[3] or s[1] - (p + 1) > r[3] for s in placed)

    def place(w, axis, a, b, m_from):
        """The pair whose facing sites are at a and b along `axis`, on the first two free lines across it; False if there are none."""
        L, M = (W, H) if axis == "x" else (H, W)
        if a - 1 < 0 or b + 1 > L - 1:
            return False
        for m in range(m_from, M - 1):
            r = (a - 1, m, b + 1, m + 1) if axis == "x" else (m, a - 1, m + 1, b + 1)
            if not free(r):
                continue
            placed.append(r)
            aa, mm = np.meshgrid(np.array([a - 1, a, b, b + 1]), [m, m + 1])
            ba, bm = np.meshgrid(np.arange(a + 1, b), [m, m + 1])
            cell, between = np.stack([aa.ravel(), mm.ravel()], 1), np.stack([ba.ravel(), bm.ravel()], 1)
            pts.append(cell if axis == "x" else cell[:, ::-1])
            gaps.append(Gap(axis, w, (between if axis == "x" else between[:, ::-1]).astype(np.int64)))
            return True
        return False

    for w, axis, side in jobs:
        turn += 1
        bounds = (32, 64) if axis == "x" else (16, 32)
        # the pairs along x live below row 64 of a tall image's pairs along y, the pairs along y right of column 96 of a wide image's pairs along x
        m_from = (64 if H >= 96 else 0) if axis == "x" else (96 if W >= 128 else 0)
        cands = [(B - q, B - q + w) if side == "lo" else (B - 1 + q - w, B - 1 + q) for B in (bounds if turn % 2 else bounds[::-1])]
        any(place(w, axis, a, b, m_from) for a, b in cands + [(1, 1 + w)])
    pts = np.concatenate(pts).astype(np.int64) if pts else np.zeros((0, 2), np.int64)
    return pts, None, tuple(gaps)


def _wrap(H, W, mask_k):
    """Lone non-empty sites, each inside a full block of radius p + 2 of sites whose colours are empty to the mask: the block's pixels
    within p of the centre (in both axes) keep their colours, the two rings beyond are occupied pixels the stage must zero.  The first
    centre is (31, 16) -- the block straddles the word boundary 31 | 32 and the task boundary 15 | 16 --, the second sits against the far
    corner where the image has room for both."""
    p = mask_k // 2
    R = p + 2
    centres = [(min(31, W - 2), min(16, H - 2))]
    far = (W - 2, H - 2)
    if max(far[0] - centres[0][0], far[1] - centres[0][1]) > 2 * R + p:
        centres.append(far)
    pts, col = [], []
    for cx, cy in centres:
        ys, xs = np.mgrid[max(0, cy - R):min(H, cy + R + 1), max(0, cx - R):min(W, cx + R + 1)]
        blk = np.stack([xs.ravel(), ys.ravel()], 1)
        c = np.array(WRAP_COLOURS, dtype=np.uint8)[(blk[:, 0] * 3 + blk[:, 1]) % len(WRAP_COLOURS)]
        centre = (blk[:, 0] == cx) & (blk[:, 1] == cy)
        c[centre] = (201, 77, 3)
        pts.append(blk)
        col.append(c)
    return np.concatenate(pts).astype(np.int64), np.concatenate(col)


def _degenerate(name, H, W):
    if name == "three":
        return np.array([[1, 0], [0, 1], [W - 1, H - 1]])
    if name == "column":
        ys = np.arange(0, H, 2)
        return np.stack([np.full_like(ys, W // 2), ys], 1)
    if name == "row":
        xs = np.arange(0, W, 3)
        return np.stack([xs, np.full_like(xs, H // 2)], 1)
    if name == "four-in-row":
        return np.array([[0, H // 2], [W // 3, H // 2], [2 * W // 3, H // 2], [W - 1, H // 2]])
    return np.zeros((0, 2), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def sites(family, H, W, mask_k=11):
    """The site set of a family at a shape (and, for `gap` and `wrap`, a mask size): distinct pixels inside the image, read-only arrays."""
    gaps = ()
    if family == "random2":
        pts, col = _random(H, W, 0.02, 101)
    elif family == "random25":
        pts, col = _random(H, W, 0.25, 102)
    elif family == "ring":
        pts, col = _ring(H, W)
    elif family == "diagonal":
        pts, col = _diagonal(H, W)
    elif family == "border":
        pts, col = _border(H, W)
    elif family == "gap":
        pts, col, gaps = _gap(H, W, mask_k)
    elif family == "wrap":
        pts, col = _wrap(H, W, mask_k)
    elif family in DEGENERATE:
        pts, col = _degenerate(family, H, W), None
    else:
        raise KeyError(family)
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    pts, first = np.unique(pts, axis=0, return_index=True)
    col = odd_colours(pts) if col is None else np.ascontiguousarray(col[first], dtype=np.uint8)
    assert pts.size == 0 or (pts.min() >= 0 and pts[:, 0].max() < W and pts[:, 1].max() < H), (family, H, W)
    pts.setflags(write=False)
    col.setflags(write=False)
    return Sites(pts, col, gaps)


# ---------------------------------------------------------------------------------------------------- the table
def _case(H, W, family, mask_k, out_flags, want_mask):
    return Case(f"{H}x{W}-{family}-k{mask_k}-f{out_flags}", H, W, family, mask_k, out_flags, want_mask)


@functools.lru_cache(maxsize=None)
def cases():
    """Every shape with its families at (11, 0); at the three sweep shapes mask_k x out_flags on `gap` and `wrap` (these also ask for the
    mask image), and every degenerate set at out_flags 0 and 3.  13 shapes with two families but one, 3 x 5 x 4 x 2 and 3 x 5 x 2 -- 175
    rows: the products named for the sweep alone come to 150, so the table keeps them whole rather than staying near 120; all but a
    dozen rows are images of 300 x 48 pixels or less."""
    table = [_case(H, W, f, 11, 0, False) for (H, W) in SHAPES for f in SHAPE_FAMILIES[(H, W)]]
    for H, W in SWEEP_SHAPES:
        table += [_case(H, W, f, k, fl, True) for f in ("gap", "wrap") for k in SWEEP_MASK_K for fl in SWEEP_OUT_FLAGS]
        table += [_case(H, W, f, 11, fl, False) for f in DEGENERATE for fl in (0, 3)]
    assert len({c.id for c in table}) == len(table)
    return tuple(table)


def case(case_id):
    return next(c for c in cases() if c.id == case_id)


def class_case(name):
    """The (11, 0) case a shape class reruns over a poisoned workspace."""
    H, W = SHAPE_CLASSES[name]
    return next(c for c in cases() if (c.H, c.W, c.mask_k, c.out_flags) == (H, W, 11, 0) and c.family not in DEGENERATE)


# ---------------------------------------------------------------------------------------------------- the oracle
def parts(pts, col, H, W):
    """(sparse image, exact interpolant) of explicit sites: what does not depend on mask_k and out_flags."""
    sparse = np.zeros((H, W, 3), dtype=np.uint8)
    sparse[pts[:, 1], pts[:, 0]] = col
    interp = np.zeros((H, W, 3), dtype=np.uint8) if bo._is_degenerate(pts) else bo.interp_exact(pts, col, H, W)[0]
    return sparse, interp


def compose(pts, sparse, interp, mask_k, out_flags):
    """The composition of `render_bev_image` (its lines 413-414) under a mask size and the two output flags."""
    mask = bo.box_dilate(bo.nonempty_mask(sparse), mask_k)
    degenerate = bo._is_degenerate(pts)
    if degenerate:
        final = np.zeros_like(sparse)
    else:
        final = interp if out_flags & 2 else bo.remove_hallucinated(sparse, interp, mask_k)
    if not out_flags & 1:
        final = np.flipud(final)
    return Expected(sparse, interp, mask, np.ascontiguousarray(final), len(pts), degenerate)


@functools.lru_cache(maxsize=None)
def _parts_of(family, H, W, mask_k):
    s = sites(family, H, W, mask_k)
    return parts(s.pts, s.col, H, W)


def case_sites(c):
    return sites(c.family, c.H, c.W, c.mask_k if c.family in ("gap", "wrap") else 11)


def expected(c):
    s = case_sites(c)
    sparse, interp = _parts_of(c.family, c.H, c.W, c.mask_k if c.family in ("gap", "wrap") else 11)
    return compose(s.pts, sparse, interp, c.mask_k, c.out_flags)


# ---------------------------------------------------------------------------------------------------- the kernel's mask pass, and three mistakes
MUTANTS = ("phase B drops prev >> (32 - d)", "phase C's lower halo stops at p - 1", "phase G keeps occupied pixels outside the mask")


def emulate_mask(nonempty, p, mutant=None):
    """Phases B and C of bev_densify_kernel: per row, bit x of a word takes the bits x - d and x + d (d = 1 .. p) of the same word or of its
    neighbour; then per task of 16 rows, row y takes the rows y - p .. y + p out of the task's register halo."""
    H, W = nonempty.shape
    xs, ys = np.arange(W), np.arange(H)
    hor = nonempty.copy()
    for d in range(1, min(p, W - 1) + 1):
        from_left = np.zeros_like(nonempty)
        from_left[:, d:] = nonempty[:, :W - d]
        if mutant == MUTANTS[0]:
            from_left[:, (xs // 32) != ((xs - d) // 32)] = False   # the source bit lies in the previous word
        hor[:, :W - d] |= nonempty[:, d:]
        hor |= from_left
    out = np.zeros_like(nonempty)
    for d in range(-p, p + 1):
        if abs(d) >= H:
            continue
        src = np.zeros_like(nonempty)
        lo, hi = max(0, -d), min(H, H - d)
        src[lo:hi] = hor[lo + d:hi + d]
        if mutant == MUTANTS[1] and d == -p:
            src[ys % MASK_ROWS_PER_TASK == 0] = False              # rows[MASK_MAX_HALF - p] is the task's first row's row y - p
        out |= src
    return out


def emulate(c, mutant=None):
    """(mask image, final image) as the kernel computes them: interpolated pixels where the mask has them, occupied pixels zeroed where
    it has not (phase G), everything zero for a degenerate set."""
    s = case_sites(c)
    e = expected(c)
    mask = emulate_mask(bo.nonempty_mask(e.sparse), c.mask_k // 2, mutant)
    occ = np.zeros((c.H, c.W), dtype=bool)
    occ[s.pts[:, 1], s.pts[:, 0]] = True
    if e.degenerate:
        final = np.zeros_like(e.sparse)
    else:
        applied = np.ones_like(mask) if c.out_flags & 2 else mask
        keep = applied | occ if mutant == MUTANTS[2] else applied
        final = e.interp * keep[:, :, None].astype(np.uint8)
    if not c.out_flags & 1:
        final = np.flipud(final)
    return mask, np.ascontiguousarray(final)
