"""Integer-pixel cases for `salve_layout_rasterise` across its accepted contract, the image the oracle draws for each of them, and
the image a kernel with ONE mistake would draw (not a test module).

A case is a batch of images of one size, rasterised in one launch through the C ABI: `salve_layout_t` records, `poly_xy` int32
[*, 2] and `segs` int32 [*, 8] = x1, y1, x2, y2, colour 0x00BBGGRR, thickness, 0, 0 (`Case.tables`).  `expected(case)` is built from
the oracle's integer-level pieces alone -- zeros, `lo.fill_poly` when the image has a polygon, `lo.cv_thick_line_aa` per segment in
table order, `np.flipud` -- so it does not depend on anything in front of the pixel coordinates.  The oracle writes pixels with loops
as OpenCV does; the kernel evaluates closed forms per pixel and per 16 x 16 tile: comparing the two is what tests the kernel's logic.

Groups (every group at 45 x 83 and 83 x 45: not square, no multiple of 16, a 13-pixel and a 3-pixel partial tile):
thickness_direction, short, borders, tiles, chunks, colours, polygons; `reduced` at 16 x 16, 17 x 33, 1 x 1 and 1 x 40; `workload`
at 501 x 501.  Left out on purpose: coordinates near the 2^24 limit (the scan of a thick segment walks every scanline from the
polygon's top: seconds in the oracle, tens of millions of iterations per tile in the kernel), thickness <= 0 (OpenCV refuses it)
and thickness >= 19 (tests/test_layout.py).  OpenCV itself is not installed: parity with cv2 stays unpinned.
"""

import contextlib
import functools
import math

import numpy as np

from oracle import layout_oracle as lo
from salve_amd import _lib

SIZES = ((45, 83), (83, 45))
REDUCED_SIZES = ((16, 16), (17, 33), (1, 1), (1, 40))
WORKLOAD_SIZE = (501, 501)
THICKNESSES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 17, 18)
SHORT_LENGTHS, SHORT_THICKNESSES = (0, 1, 2, 3, 7), (1, 2, 5, 8)
BORDER_THICKNESSES = (1, 2, 5, 8, 17)
TILE_THICKNESSES = (1, 2, 5, 8, 18)
CHUNK_COUNTS = (0, 1, 6, 7, 8, 13, 14, 15, 22)
PALETTE = (0x327BC8, 0x010203, 0xFEFDFC, 0x808080)          # channels that are neither 0 nor 255: the blend's rounding, both signs
COLOURS = PALETTE + (0x000000, 0xFFFFFF)
MIXED = (0x327BC8, 0xC87B32, 0x10E0A0, 0xFEFDFC, 0x808080, 0x2040FF, 0xE01070, 0x010203)
TILE, SEGC = 16, 7                                           # layout.hip: pixels per tile side, segments per LDS chunk

# mutant -> the group built to catch it
MUTANTS = {
    "clip_line_fixed with w and h exchanged": "borders",
    "_put_point blends once": "colours",
    "end caps at 30-degree steps at every radius": "thickness_direction",
    "no odd-thickness half pixel": "thickness_direction",
    "no flip": "borders",
    "segments in reverse order": "chunks",
    "segments beyond the seventh dropped": "chunks",
    "tile culling with reach = thickness / 2": "tiles",
    "R and B exchanged": "colours",
    "non-zero winding fill": "polygons",
}


class Case:
    """`images`: per image (polygon int [K, 2] or None, [(x1, y1, x2, y2, colour, thickness), ...]); `draws`: per image True (the
    oracle must draw something), False (nothing) or None (not claimed)."""

    def __init__(self, group, hw, images, draws=None):
        self.group, self.hw = group, (int(hw[0]), int(hw[1]))
        self.images = [(None if p is None else np.asarray(p, dtype=np.int64).reshape(-1, 2), [tuple(int(v) for v in s) for s in segs])
                       for p, segs in images]
        self.draws = list(draws) if draws is not None else [None] * len(self.images)
        assert len(self.draws) == len(self.images) > 0
        self.id = f"{group}-{self.hw[0]}x{self.hw[1]}"

    @property
    def n_segments(self):
        return sum(len(s) for _, s in self.images)

    def tables(self):
        """(salve_layout_t records [n], poly_xy int32 [*, 2], segs int32 [*, 8]) with absolute offsets, as `pack_layout_tables` lays
        them out (a table without a row is one row of zeros)."""
        rec = np.zeros(len(self.images), dtype=_lib.LAYOUT_DTYPE)
        polys, segs = [], []
        n_poly = 0
        for i, (poly, ss) in enumerate(self.images):
            rec[i]["poly_off"], rec[i]["seg_off"], rec[i]["n_seg"] = n_poly, len(segs), len(ss)
            if poly is not None and len(poly):
                rec[i]["n_poly"] = len(poly)
                polys.append(poly)
                n_poly += len(poly)
            segs.extend((*s, 0, 0) for s in ss)
        return (rec, np.concatenate(polys).astype(np.int32) if polys else np.zeros((1, 2), np.int32),
                np.array(segs, dtype=np.int64).astype(np.int32).reshape(-1, 8) if segs else np.zeros((1, 8), np.int32))


def _rgb(colour):
    return colour & 255, (colour >> 8) & 255, (colour >> 16) & 255


def _render(hw, poly, segs, flip=True):
    img = np.zeros((hw[0], hw[1], 3), dtype=np.uint8)
    if poly is not None and len(poly) > 0:
        lo.fill_poly(img, poly, lo.WHITE)
    for x1, y1, x2, y2, colour, thickness in segs:
        lo.cv_thick_line_aa(img, x1, y1, x2, y2, _rgb(colour), thickness)
    return np.flipud(img) if flip else img


# ---------------------------------------------------------------------------------------------------- mutants
@contextlib.contextmanager
def _swapped(name, fn):
    """One of the oracle's module-level functions replaced for the duration of a call (the oracle's file is not edited)."""
    orig = getattr(lo, name)
    setattr(lo, name, fn(orig))
    try:
        yield
    finally:
        setattr(lo, name, orig)


def _put_point_once(_orig):
    def put(img, x, y, colour, a):
        for ch in range(3):
            c = int(img[y, x, ch])
            c += ((int(colour[ch]) - c) * a + 127) >> 8
            img[y, x, ch] = c & 255
    return put


def _ellipse_poly_30(_orig):
    def poly(cx, cy, axis):
        out, prev = [], None
        for ang in range(0, 361, 30):
            x, y = float(axis) * float(np.float32(lo.SIN30[450 - ang])), float(axis) * float(np.float32(lo.SIN30[ang]))
            px, py = float(cx) + x, float(cy) + y
            qx, qy = lo.cv_round(px / lo.XY_ONE) << lo.XY_SHIFT, lo.cv_round(py / lo.XY_ONE) << lo.XY_SHIFT
            qx, qy = qx + lo.cv_round(px - qx), qy + lo.cv_round(py - qy)
            if (qx, qy) != prev:
                out.append((qx, qy))
                prev = (qx, qy)
        return out if len(out) > 1 else [(cx, cy), (cx, cy)]
    return poly


def _geometry_without_odd(_orig):
    def geometry(x1, y1, x2, y2, thickness):
        p0x, p0y, p1x, p1y = x1 << lo.XY_SHIFT, y1 << lo.XY_SHIFT, x2 << lo.XY_SHIFT, y2 << lo.XY_SHIFT
        dx, dy = (p0x - p1x) / lo.XY_ONE, (p1y - p0y) / lo.XY_ONE
        r = dx * dx + dy * dy
        th = thickness << (lo.XY_SHIFT - 1)
        quad = None
        if abs(r) > np.finfo(np.float64).eps:
            r = th / np.sqrt(r)
            dpx, dpy = lo.cv_round(dy * r), lo.cv_round(dx * r)
            quad = [(p0x + dpx, p0y + dpy), (p0x - dpx, p0y - dpy), (p1x - dpx, p1y - dpy), (p1x + dpx, p1y + dpy)]
        return quad, th, (p0x, p0y), (p1x, p1y)
    return geometry


def _fill_poly_nonzero(_orig):
    def fill(img, pts, colour):
        H, W = img.shape[:2]
        pts = np.asarray(pts, dtype=np.int64)
        K = len(pts)
        edges = [(int(pts[i][0]), int(pts[i][1]), int(pts[(i + 1) % K][0]), int(pts[(i + 1) % K][1])) for i in range(K)]
        xs = np.arange(W, dtype=np.int64)
        xf = xs << 16
        for y in range(H):
            wle, wlt = np.zeros(W, np.int64), np.zeros(W, np.int64)
            for x0, y0, x1, y1 in edges:
                if y0 == y1:
                    continue
                d = 1
                if y0 > y1:
                    x0, y0, x1, y1, d = x1, y1, x0, y0, -1
                if y0 <= y < y1:
                    num = (x1 - x0) << 16
                    c = (x0 << 16) + (y - y0) * (abs(num) // (y1 - y0) * (1 if num >= 0 else -1))
                    wle += d * (c <= xf)
                    wlt += d * (c < xf)
            inside = (wle != 0) | (wlt != 0)
            for e in edges:
                inside |= lo._on_line8_row(xs, y, e)
            img[y, inside] = colour
    return fill


def _render_tile_culled(hw, poly, segs):
    """A kernel whose tiles keep only the segments whose bounding box grown by thickness / 2 (not thickness / 2 + 3) meets them."""
    H, W = hw
    out = np.zeros((H, W, 3), dtype=np.uint8)
    cache = {}
    for ty0 in range(0, H, TILE):
        for tx0 in range(0, W, TILE):
            keep = tuple(k for k, (x1, y1, x2, y2, _, t) in enumerate(segs)
                         if not (max(x1, x2) + t // 2 < tx0 or min(x1, x2) - t // 2 > tx0 + TILE - 1 or
                                 max(y1, y2) + t // 2 < ty0 or min(y1, y2) - t // 2 > ty0 + TILE - 1))
            if keep not in cache:
                cache[keep] = _render(hw, poly, [segs[k] for k in keep], flip=False)
            out[ty0:ty0 + TILE, tx0:tx0 + TILE] = cache[keep][ty0:ty0 + TILE, tx0:tx0 + TILE]
    return np.flipud(out)


def _render_mutant(hw, poly, segs, mutant):
    swaps = {"clip_line_fixed with w and h exchanged": ("clip_line_fixed", lambda orig: lambda w, h, *p: orig(h, w, *p)),
             "_put_point blends once": ("_put_point", _put_point_once),
             "end caps at 30-degree steps at every radius": ("cv_ellipse_poly", _ellipse_poly_30),
             "no odd-thickness half pixel": ("thick_line_geometry", _geometry_without_odd),
             "non-zero winding fill": ("fill_poly", _fill_poly_nonzero)}
    if mutant in swaps:
        with _swapped(*swaps[mutant]):
            return _render(hw, poly, segs)
    if mutant == "no flip":
        return _render(hw, poly, segs, flip=False)
    if mutant == "segments in reverse order":
        return _render(hw, poly, segs[::-1])
    if mutant == "segments beyond the seventh dropped":
        return _render(hw, poly, segs[:SEGC])
    if mutant == "tile culling with reach = thickness / 2":
        return _render_tile_culled(hw, poly, segs)
    if mutant == "R and B exchanged":
        return _render(hw, poly, segs)[..., ::-1]
    raise KeyError(mutant)


_TRUE = {}


def expected(case, mutant=None):
    """uint8 [n, H, W, 3] (R, G, B): the oracle's images of the case -- computed once per case and read-only --, or the images of a
    kernel with the one mistake `mutant` names (a key of MUTANTS)."""
    if mutant is not None:
        return np.stack([_render_mutant(case.hw, p, s, mutant) for p, s in case.images])
    if case.id not in _TRUE:
        img = np.stack([_render(case.hw, p, s) for p, s in case.images])
        img.setflags(write=False)
        _TRUE[case.id] = img
    return _TRUE[case.id]


def words(images):
    """uint8 [..., 3] -> int32 [...] 0x00BBGGRR, the kernel's output format (top byte 0)."""
    u = images.astype(np.int32)
    return u[..., 0] | (u[..., 1] << 8) | (u[..., 2] << 16)


# ---------------------------------------------------------------------------------------------------- groups
DIRECTIONS = ((30, 0), (0, 30), (30, 1), (30, -1), (1, 30), (-1, 30),              # the axes and just off them, both signs
              (21, 21), (21, -21), (22, 20), (20, 22), (22, -20), (20, -22),      # the diagonals and just off them, both signs
              (26, 15), (15, 26), (26, -15), (15, -26))                           # 30 and 60 degrees


def _thickness_direction(hw):
    H, W = hw
    images = []
    for t in THICKNESSES:
        for k, (dx, dy) in enumerate(DIRECTIONS):
            x0, y0 = W // 2 - dx // 2, H // 2 - dy // 2
            col = MIXED[(k + t) % len(MIXED)]
            images.append((None, [(x0, y0, x0 + dx, y0 + dy, col, t)]))
            images.append((None, [(x0 + dx, y0 + dy, x0, y0, col, t)]))            # the other end-point order
    return Case("thickness_direction", hw, images, [True] * len(images))


def _short(hw):
    H, W = hw
    images = []
    for t in SHORT_THICKNESSES:
        for n in SHORT_LENGTHS:
            h = (n + 1) // 2
            for k, (dx, dy) in enumerate(((n, 0), (-n, 0), (0, n), (0, -n), (n, n), (n, -n), (n, h), (-h, n), (-n, -h))):
                x0, y0 = W // 2 - 3 + k, H // 2 + 1 - k
                images.append((None, [(x0, y0, x0 + dx, y0 + dy, MIXED[(k + n) % len(MIXED)], t)]))
    # (a zero-length LineAA is two faint steps: whether it leaves a mark depends on the colour -- not claimed)
    return Case("short", hw, images, [None if s[0][5] == 1 and s[0][:2] == s[0][2:4] else True for _, s in images])


def _borders(hw):
    H, W = hw
    mx, my = W // 2, H // 2
    items = []   # (segment without colour, draws)
    for t in BORDER_THICKNESSES:
        r = t // 2
        # across each border, through each corner, cutting each corner with both ends outside
        items += [((10, my, -10, my + 3, t), True), ((W - 11, my, W + 9, my - 3, t), True), ((mx, 10, mx + 3, -10, t), True),
                  ((mx, H - 11, mx - 3, H + 9, t), True)]
        for cx, sx in ((0, -1), (W - 1, 1)):
            for cy, sy in ((0, -1), (H - 1, 1)):
                items += [((cx - 6 * sx, cy - 6 * sy, cx + 6 * sx, cy + 6 * sy, t), True),
                          ((cx + 4 * sx, cy - 8 * sy, cx - 8 * sx, cy + 4 * sy, t), True)]
        # an end point exactly on row / column 0, H - 1 / W - 1, and one pixel beyond; segments along the border rows and columns
        for e in (0, 1):
            along = e == 0 or t > 1   # a single LineAA one pixel outside is clipped away whole: its tail row does not reach the image
            items += [((12, my, -e, my + 2, t), True), ((W - 13, my, W - 1 + e, my - 2, t), True), ((mx, 12, mx + 2, -e, t), True),
                      ((mx, H - 13, mx - 2, H - 1 + e, t), True),
                      ((5, -e, W - 6, -e, t), along), ((W - 6, H - 1 + e, 5, H - 1 + e, t), along), ((-e, 5, -e, H - 6, t), along),
                      ((W - 1 + e, H - 6, W - 1 + e, 5, t), along)]
        # wholly outside at distance d: the fill reaches the image up to d = thickness / 2, nothing does from thickness / 2 + 3 on
        for d in range(1, r + 5):
            draws = True if d <= r else (False if d >= r + 3 or t == 1 else None)   # (clipLine drops a LineAA that lies outside)
            items += [((-d, 5, -d, H - 6, t), draws), ((W - 1 + d, 5, W - 1 + d, H - 6, t), draws), ((5, -d, W - 6, -d, t), draws),
                      ((5, H - 1 + d, W - 6, H - 1 + d, t), draws),
                      ((-d, -d, -d, -d, t), False if d >= r + 3 else None), ((W - 1 + d, H - 1 + d, W - 1 + d, H - 1 + d, t), False if d >= r + 3 else None)]
    # end points up to +/- 20 000 pixels away, the segment crossing the image; one end inside
    for t in (1, 8, 17):
        for vx, vy in ((20, 9), (20, -9), (9, 20), (-1, 20), (20, 0), (0, 20), (20, 1)):
            items.append(((mx - 1000 * vx, my - 1000 * vy, mx + 1000 * vx, my + 1000 * vy, t), True))
        items += [((mx, my, mx + 20000, my - 7000, t), True), ((mx - 3, my + 2, mx - 6000, my + 20000, t), True)]
    images = [(None, [(*s[:4], MIXED[k % len(MIXED)], s[4])]) for k, (s, _) in enumerate(items)]
    return Case("borders", hw, images, [d for _, d in items])


def _tiles(hw):
    """The tile lines at 16 and 32 swept over every part of a segment: parallel to the line (the quadrilateral's edge and its
    anti-aliased tail row), ending on it (the cap's edge and tail), and oblique.  Offsets from -(thickness / 2 + 4) to
    thickness / 2 + 4 put the segment's axis on 15, 16, 31 and 32 and on every pixel around them that its reach covers -- among them
    segments lying entirely in one tile whose tail alone reaches the next."""
    images = []
    for t in TILE_THICKNESSES:
        for axis, b, kinds in (("x", 16, 3), ("y", 32, 3), ("x", 32, 1), ("y", 16, 1)):
            for o in range(-(t // 2 + 4), t // 2 + 5):
                c = b + o
                for kind in range(kinds):
                    s = ((c, 20, c, 27), (c - 6, 23, c, 23), (c - 4, 20, c, 26))[kind]
                    if axis == "y":
                        s = (s[1], s[0], s[3], s[2])
                    images.append((None, [(*s, MIXED[(o + kind) % len(MIXED)], t)]))
    return Case("tiles", hw, images, [True] * len(images))


def _star(n, cx, cy, r, phase, thicknesses=(2, 3, 5, 8, 1, 6, 4)):
    segs = []
    for j in range(n):
        a = phase + j * math.pi / max(n, 1)
        dx, dy = int(round(r * math.cos(a))), int(round(r * math.sin(a)))
        ox, oy = j % 3 - 1, (j // 3) % 3 - 1
        segs.append((cx + ox - dx, cy + oy - dy, cx + ox + dx, cy + oy + dy, MIXED[j % len(MIXED)], thicknesses[j % len(thicknesses)]))
    return segs


def _chunks(hw):
    H, W = hw
    counts = CHUNK_COUNTS + (7, 22, 0, 8)     # neighbours with different counts, in both directions
    images = [(None, _star(n, W // 2, H // 2, 0.45 * min(H, W), 0.1 + 0.37 * i)) for i, n in enumerate(counts)]
    return Case("chunks", hw, images, [n > 0 for n in counts])


def _colours(hw):
    H, W = hw
    my = H // 2
    room = [(3, 3), (W - 4, 3), (W - 4, H - 4), (3, H - 4)]
    images, draws = [], []
    for c in COLOURS:
        segs = [(5, 8, W - 8, H - 12, c, 8), (6, H - 8, W - 9, 5, c, 1), (W // 2 - 9, 4, W // 2 - 7, H - 6, c, 3)]
        images += [(None, segs), (room, segs)]
        draws += [c != 0, True]
    for a in COLOURS:
        for b in COLOURS:
            if a != b:   # b's anti-aliased pixels blend over a's fill and tails
                images.append((None, [(5, my - 3, W - 6, my + 4, a, 8), (5, my + 5, W - 6, my - 5, b, 2), (8, 4, W - 20, H - 5, b, 1)]))
                draws.append(True)
    return Case("colours", hw, images, draws)


def polygon_set(hw):
    """name -> (vertices, draws) of the polygon classes of the `polygons` group."""
    H, W = hw
    mx, my = W // 2, H // 2
    f = lambda pts: [(int(round(u * (W - 1))), int(round(v * (H - 1)))) for u, v in pts]
    ring = lambda k, order: [(mx + int(round(0.45 * W * math.cos(2 * math.pi * j / k + 0.3))), my + int(round(0.45 * H * math.sin(2 * math.pi * j / k + 0.3))))
                             for j in order]
    convex = f([(0.2, 0.1), (0.8, 0.2), (0.9, 0.7), (0.5, 0.9), (0.1, 0.6)])
    concave = f([(0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.5, 0.4), (0.1, 0.9)])
    spiral = [(mx + int(round((0.08 + 0.4 * k / 19) * W * math.cos(k * 2 * math.pi / 9))), my + int(round((0.08 + 0.4 * k / 19) * H * math.sin(k * 2 * math.pi / 9))))
              for k in range(20)]   # two turns and a bit: the outer turn overlaps the inner one
    rng = np.random.default_rng(W * 1000 + H)
    rand = lambda n: np.stack([rng.integers(-10, W + 10, n), rng.integers(-10, H + 10, n)], 1)
    return {
        "convex": (convex, True), "concave": (concave, True), "bow-tie": (f([(0.1, 0.1), (0.9, 0.9), (0.9, 0.1), (0.1, 0.9)]), True),
        "pentagram": (ring(5, (0, 2, 4, 1, 3)), True), "spiral": (spiral, True),
        "rectangle": ([(5, 5), (W - 6, 5), (W - 6, H - 6), (5, H - 6)], True),
        "staircase": ([(4, 4), (W - 5, 4), (W - 5, my), (mx, my), (mx, H - 5), (mx - 8, H - 5), (mx - 8, my + 6), (4, my + 6)], True),
        "vertices on the border": ([(0, my), (mx, 0), (W - 1, my), (mx, H - 1)], True),
        "the border itself": ([(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], True),
        "outside on one side": ([(-30, 5), (mx, my), (-30, H - 5)], True),
        "outside on all sides": ([(-20, my), (mx, -20), (W + 20, my), (mx, H + 20)], True),
        "far away": ([(-20000, -15000), (20000, 100), (-300, 20000)], True),
        "far away and thin": ([(-20000, my - 3), (20000, my + 2), (20000, my + 4), (-20000, my)], True),
        "covering the image": ([(-5, -5), (W + 5, -5), (W + 5, H + 5), (-5, H + 5)], True),
        "outside to the right": ([(W, 0), (W + 10, 0), (W + 10, H)], False),
        "outside above": ([(5, -20), (W - 5, -1), (mx, -30)], False),
        "outside and far": ([(-20000, -20000), (-3, -3), (-20000, 300)], False),
        "no vertex": (None, False), "one vertex": ([(mx, my)], True), "two vertices": ([(5, 5), (W - 6, H - 8)], True),
        "three vertices": ([(4, H - 5), (mx, 3), (W - 5, H - 9)], True),
        "consecutive duplicates": ([convex[0], convex[0], convex[1], convex[2], convex[2], convex[2], convex[3], convex[4], convex[4]], True),
        "closed ring": (concave + concave[:1], True),
        "100 random vertices": (rand(100), True), "150 random vertices": (rand(150), True),
    }


def _polygons(hw):
    H, W = hw
    on_top = [(4, H - 6, W - 5, 5, 0x327BC8, 8), (3, 3, W - 4, H - 9, 0x808080, 1), (W // 2, -4, W // 2 + 5, H + 3, 0x010203, 5)]
    images, draws = [], []
    for pts, d in polygon_set(hw).values():
        images += [(pts, []), (pts, on_top)]        # alone, and with segments on top
        draws += [d, True]
    return Case("polygons", hw, images, draws)


def _reduced(hw):
    """The smallest images: one full tile, one tile and a pixel, one pixel, one row."""
    H, W = hw
    mx, my = W // 2, H // 2
    images = []
    for t in (1, 2, 5, 8, 18):
        for s in ((0, 0, W - 1, H - 1), (mx, my, mx, my), (-3, my, W + 2, my + 1), (mx, -5, mx + 1, H + 4), (W - 1, 0, 0, H - 1)):
            images.append((None, [(*s, MIXED[t % len(MIXED)], t)]))
    rng = np.random.default_rng(H * 100 + W)
    polys = [[(-5, -5), (W + 5, -5), (W + 5, H + 5), (-5, H + 5)], [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], [(0, 0)],
             [(0, 0), (W - 1, 0), (0, H - 1)], np.stack([rng.integers(-4, W + 4, 20), rng.integers(-4, H + 4, 20)], 1)]
    images += [(p, []) for p in polys]
    images.append((polys[4], _star(8, mx, my, 0.6 * max(H, W), 0.2)))
    return Case("reduced", hw, images, [True] * len(images))


def _workload(hw):
    """The workload's size, kept small: many tiles per image, long edges, a room with its W/D/Os and its thin contour."""
    H, W = hw
    rng = np.random.default_rng(7)
    room = [(60, 70), (430, 60), (440, 300), (300, 310), (295, 440), (70, 430), (60, 70)]
    wdo = [(100, 69, 180, 67, 0x00FF00, 8), (432, 100, 435, 180, 0x0000FF, 8), (300, 330, 297, 400, 0xFF0000, 8), (150, 432, 230, 434, 0x00FF00, 8)]
    contour = [(*room[k], *room[k + 1], 0xFFFFFF, 2) for k in range(len(room) - 1)]
    images = [(np.stack([rng.integers(-50, 550, 100), rng.integers(-50, 550, 100)], 1), _star(15, 250, 250, 200, 0.05, (18, 17, 2, 8, 1, 9, 4))),
              (None, [(-100, 250, 600, 260, 0x327BC8, 8), (250, -50, 255, 560, 0x808080, 17), (-10, -10, 510, 510, 0xFEFDFC, 2),
                      (480, 20, 520, -20, 0x10E0A0, 12), (0, 500, 500, 500, 0xC87B32, 1)]),
              (None, []), (room, wdo), (None, contour + wdo)]
    return Case("workload", hw, images, [True, True, False, True, True])


GROUPS = {"thickness_direction": _thickness_direction, "short": _short, "borders": _borders, "tiles": _tiles, "chunks": _chunks,
          "colours": _colours, "polygons": _polygons}


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, built once: the seven groups at both non-square sizes, the reduced group at the four smallest, the workload's."""
    out = [build(hw) for build in GROUPS.values() for hw in SIZES]
    out += [_reduced(hw) for hw in REDUCED_SIZES]
    out.append(_workload(WORKLOAD_SIZE))
    return tuple(out)


def case(case_id):
    return next(c for c in cases() if c.id == case_id)
