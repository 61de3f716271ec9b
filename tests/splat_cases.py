"""Cases for the front end of the BEV rasteriser -- `bev_pano_index_kernel`, `bev_splat_kernel`, `emit_tile` (salve_amd/csrc/bev_splat.h)
-- across the contract `make_devcfg` accepts, what the oracle renders for each of them, and what a kernel with ONE mistake would
render (not a test module; numpy and the oracle only).

A case is one geometry: a panorama size `H x W` with its `crop_ratio`, and the `BEVParams` of the image.  It carries a stack of depth
and colour panoramas (one per depth family, `FAMILIES`) and a table of render rows `(pano, surface, R, t, apply_pose)` that one launch
renders.  `expected(case)` runs the oracle -- `xyzrgb_from_arrays` -> `pose_pair` -> `render_bev_image(mode="exact")` -- once per row
and keeps, per row: the in-window count, `img_xy` scattered to the cropped raster index, the winner index per pixel, the sparse image,
the mask, the final image and the site count.  `expected(case, mutant=...)` emulates one wrong kernel in numpy on the same points
(`MUTANTS`: mutant -> the cases built to catch it); `expected(case, mutant="none")` is the same emulator without a mistake, which the
host test requires to equal the oracle.

Panorama geometries (`PANOS`): `narrow` 42 x 20 (two block columns, the second 4 pixels wide; 30 rows: a partial last block row),
`wide` 70 x 1028 (65 block columns: a second group holding one block; 50 rows), `tall` 8800 x 4 and `tall-listed` 8400 x 4 without
crop (one block column, more than GLIST_CAP = 1024 groups between a surface's first and last point: the splat's un-listed branch; at
8400 the floor stays below the cap and the ceiling does not), `small` 64 x 128 (the golden small geometry).  Image geometries
(`BEVS`): 21 x 29 (smaller than a tile, not square, 0.25 m per pixel: heavy z-order contention), 129 x 257 (3 x 2 tiles whose last
column and row are ONE pixel, on which the window's edge lands), 128 x 128 (exactly one tile; 4 / 127 m per pixel so that the window
reaches pixel 127) and 101 x 101.  One more case, `narrow-21x29-zcut`, moves the z bounds of both surfaces onto points
(`z_cut_ranges`): the only way to see which side of lo < z <= hi is inclusive.
"""

import functools
from collections import namedtuple

import numpy as np

from oracle import bev_oracle as bo
from salve_amd import synthetic

GLIST_CAP, GROUP = 1024, 64         # bev_splat.h: groups a tile's pre-cull can list, blocks per group
BLK_W, BLK_H, TILE = 16, 4, 128     # panorama block (one wavefront), output tile
MARGIN, SLACK = np.float32(0.02), np.float32(1e-5)   # bev_splat_kernel's tile margin, splat_reaches' rounding slack
CROP = 80 / 512
SURFACES = ("floor", "ceiling")

PANOS = {"box-room": (512, 1024, CROP), "narrow": (42, 20, CROP), "wide": (70, 1028, CROP), "tall": (8800, 4, 0.0), "tall-listed": (8400, 4, 0.0), "small": (64, 128, CROP)}
BEVS = {"21x29": (20, 28, 0.25), "129x257": (128, 256, 0.0625), "128x128": (127, 127, 4 / 127), "101x101": (100, 100, 0.1), "501x501": (500, 500, 0.02)}
EXACT_SCALE = ("21x29", "129x257")  # 1 / meters_per_px is 4 and 16: pixel positions of the single-pixel rows are exact
CASES = (("narrow", "21x29"), ("narrow", "129x257"), ("narrow", "128x128"), ("wide", "21x29"), ("wide", "129x257"), ("wide", "128x128"),
         ("tall", "129x257"), ("tall-listed", "128x128"), ("small", "101x101"))
Z_CUT = "narrow-21x29-zcut"         # one more case: narrow, 21 x 29, with the z bounds of both surfaces ON points (`z_cut_ranges`)
Z_RANGES = ((-float("inf"), -1.0), (0.5, float("inf")))   # floor, ceiling: lo < z <= hi (the rasteriser's and the oracle's defaults)
FAMILIES = ("noise", "near-noise", "checker", "zero", "far", "flat", "one-pixel", "room")

Row = namedtuple("Row", "pano surface R t apply_pose pose")
Result = namedtuple("Result", "count img_xy winner sparse mask bev sites")
QUANTITIES = Result._fields

# mutant -> the cases built to catch it
_NARROW = ("narrow-21x29", "narrow-129x257", "narrow-128x128")
_WIDE = ("wide-21x29", "wide-129x257", "wide-128x128")
_MOST = _NARROW + ("wide-129x257",)
MUTANTS = {
    "first index wins within a slice": _MOST,
    "lower slice wins": _MOST,
    "round half away from zero": ("narrow-21x29", "narrow-129x257", "wide-21x29", "wide-129x257"),
    "window exclusive at its upper edges": ("narrow-21x29", "narrow-129x257", "wide-21x29", "wide-129x257"),
    "z filter lo <= z < hi": (Z_CUT,),   # (with the default bounds no uint16 depth puts z on one: test_splat_cases_host.py proves it)
    "t * 1.5 in double": _MOST,
    "count leaves out points beyond the slices": _MOST,
    "partial block column dropped": _MOST,
    "partial block row dropped": _MOST,
    "block columns >= 64 dropped": _WIDE,
    "groups beyond GLIST_CAP dropped": ("tall-129x257", "tall-listed-128x128"),
    "centre-only cull": _MOST,
    "cull ignores the rotation": _MOST,
    "colours without the crop offset": _MOST + ("small-101x101",),
    "non-empty from occupancy": _MOST,
}


# ---------------------------------------------------------------------------------------------------- panoramas
def one_pixel_at(H, W, crop_ratio):
    """(row, column) of the single non-zero pixel of the `one-pixel` family: four fifths down the cropped rows, 54 degrees or less
    below the horizon, where 1.8 m of depth is a floor point (z <= -1) at most 1.4 m from the camera."""
    crop = int(H * crop_ratio) if crop_ratio > 0 else 0
    return crop + int(0.8 * (H - 2 * crop)), W // 3


@functools.lru_cache(maxsize=None)
def pano_set(name):
    """(rgb uint8 [P, H, W, 3], depth uint16 [P, H, W]) of a panorama geometry, one panorama per family of FAMILIES, read-only."""
    H, W, cr = PANOS[name]
    if name == "box-room":
        panos = [synthetic.make_pano(i) for i in range(2)]
        return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    rng = np.random.default_rng(1000 * H + W)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.zeros((len(FAMILIES), H, W), dtype=np.uint16)
    depth[0] = rng.integers(0, 65536, (H, W))                       # most points outside the window and the slices
    depth[1] = rng.integers(500, 20000 if name.startswith("tall") else 6000, (H, W))
    depth[2] = np.where((v + u) % 2 == 0, 800, 9000)                # every block's box is metres wide
    depth[3], depth[4], depth[5] = 0, 65535, 1500
    depth[6][one_pixel_at(H, W, cr)] = 1800
    depth[7] = synthetic.make_pano(3, H, W)[1]
    rgb = rng.integers(0, 256, (len(FAMILIES), H, W, 3)).astype(np.uint8)
    kind = rng.random((len(FAMILIES), H, W))
    rgb[kind < 0.10] = (16, 16, 16)                                  # channel product 4096: wraps to 0
    rgb[(kind >= 0.10) & (kind < 0.15)] = (32, 8, 255)               # 65280: wraps to 0
    rgb[(kind >= 0.15) & (kind < 0.22)] = (0, 200, 90)               # a zero channel
    rgb[(kind >= 0.22) & (kind < 0.27)] = (7, 255, 0)
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


def box_room_case():
    """The scene the older bit-exact tests render (tests/test_gpu_rasteriser.py's fixture and first test): two 512 x 1024 box rooms, the first
    four rows of that test (two of `make_hypotheses(16, 2, seed=0)`, posed and identity), 501 x 501.  Not one of `cases()`: the host test measures the cull mutants on it."""
    hyp = synthetic.make_hypotheses(16, 2, seed=0)
    rows = []
    for hi in range(2):
        rows += [Row(int(hyp.i1[hi]), hi % 2, hyp.R[hi], hyp.t[hi], 1, "box room"), Row(int(hyp.i2[hi]), hi % 2, hyp.R[hi], hyp.t[hi], 0, "box room")]
    return Case("box-room", "501x501", rows)


def _crop_rows(name):
    H, _, cr = PANOS[name]
    return int(H * cr) if cr > 0 else 0


@functools.lru_cache(maxsize=None)
def _cloud(name, p):
    """Every pixel of the cropped panorama back-projected as `xyzrgb_from_arrays` does, BEFORE the z filter, with the rotmat2d(-90)
    product of `pose_pair` applied: (xy float64 [npts, 2], z float64 [npts])."""
    H, W, _ = PANOS[name]
    crop = _crop_rows(name)
    d = pano_set(name)[1][p][..., None].astype(np.float32) * np.float32(0.001)
    xyz = (d * bo.sphere_table(H, W))[crop:H - crop].reshape(-1, 3)
    return bo.rot2(xyz[:, :2], bo.rotmat2d(-90)), np.ascontiguousarray(xyz[:, 2])


@functools.lru_cache(maxsize=None)
def kept(name, p, surface, z_range=None):
    """The oracle's own point cloud of (panorama, surface): (xyzrgb float64 [M, 6], raster index in the cropped panorama int64 [M]).
    z_range: (lo, hi) of the surface's filter lo < z <= hi; default the reference's (`bo.floor_ceiling_z_range`)."""
    rgb, depth = pano_set(name)
    zr = bo.floor_ceiling_z_range(SURFACES[surface])
    assert tuple(zr) == Z_RANGES[surface]
    return bo.xyzrgb_from_arrays(depth[p], rgb[p], zr if z_range is None else list(z_range), crop_ratio=PANOS[name][2], return_index=True)


def z_cut_ranges(name):
    """z ranges whose finite bounds lie ON points: the floor's upper bound is the z of the highest row of the `flat` panorama (constant
    1500: one z per row) that the reference's floor filter keeps, the ceiling's lower bound the z of the lowest row its ceiling filter
    keeps.  Under lo < z <= hi the first row stays a floor row and the second is no ceiling row; under lo <= z < hi it is the other way
    round.  (z = float32(depth * 0.001f) * zdir(row) is never exactly -1.0 or 0.5, so the default bounds cannot tell the two apart.)"""
    z = _cloud(name, FAMILIES.index("flat"))[1].reshape(_rows_of(name), -1)[:, 0]
    return ((-float("inf"), float(z[z <= -1.0].max())), (float(z[z > 0.5].min()), float("inf")))


def group_of(name, idx):
    """Index group g = (row // 4) * gpr + (column // 16) // 64 of raster indices of the cropped panorama."""
    W = PANOS[name][1]
    gpr = ((W + BLK_W - 1) // BLK_W + GROUP - 1) // GROUP
    return (idx // W // BLK_H) * gpr + (idx % W) // BLK_W // GROUP


# ---------------------------------------------------------------------------------------------------- poses
def _rot(deg, s=1.0):
    a = np.deg2rad(deg)
    return (s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])).astype(np.float32)


def solve_t(q):
    """float32 t with float32(t * 1.5f) == q exactly (q a float32 value), or None."""
    q = np.float32(q)
    t = np.float32(np.float64(q) / 1.5)
    for cand in (t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))):
        if np.float32(cand * np.float32(1.5)) == q:
            return cand
    return None


def _axis_t(lo, scale, candidates):
    """(t, pixel position) for the first of the pixel positions `candidates` that a float32 t reaches exactly."""
    for v in candidates:
        q = v / scale + lo
        if float(np.float32(q)) == q and solve_t(q) is not None:
            return solve_t(q), v
    raise ValueError("no exact translation for any of the pixel positions")


def single_pixel_poses(bev):
    """name -> (t float32 [2], (pixel position x, y) before rounding or None): the translations of the zero-matrix rows, which put every
    point of a cloud on ONE posed position t * 1.5.  With an exact scale (EXACT_SCALE) the positions are exact: `tie-even` lies half way
    above an even pixel in x (np.round goes down, half-away-from-zero goes up) and above an odd one in y, `tie-odd` the other way round,
    `seam` on 127.5 where the image is wider / higher than a tile, `corner` on the inclusive window corner (xmax, ymax), `outside` one
    float32 step beyond it in x."""
    img_h, img_w, mpp = BEVS[bev]
    g = bo.BevGrid(img_h, img_w, mpp)
    xmin, xmax, ymin, ymax = g.lims
    s = g.scale
    even, odd = [m + 0.5 for m in range(4, 16, 2)], [m + 0.5 for m in range(3, 15, 2)]
    out = {}
    if bev in EXACT_SCALE:
        for name, cx, cy in (("tie-even", even, odd), ("tie-odd", odd, even)):
            (tx, vx), (ty, vy) = _axis_t(xmin, s, cx), _axis_t(ymin, s, cy)
            out[name] = (np.array([tx, ty], np.float32), (vx, vy))
        (tx, vx), (ty, vy) = _axis_t(xmin, s, [127.5] if g.W > TILE else even[2:]), _axis_t(ymin, s, [127.5] if g.H > TILE else odd[2:])
        out["seam"] = (np.array([tx, ty], np.float32), (vx, vy))
    else:   # the scale is not a power of two: near the same places, ties not claimed
        for name, vx, vy in (("tie-even", 4.5, 5.5), ("tie-odd", 5.5, 4.5), ("seam", g.W - 1.5, g.H // 2 + 0.5)):
            q = np.array([vx / s + xmin, vy / s + ymin], np.float32)
            out[name] = ((q.astype(np.float64) / 1.5).astype(np.float32), None)
    out["corner"] = (np.array([solve_t(xmax), solve_t(ymax)], np.float32), ((xmax - xmin) * s, (ymax - ymin) * s))
    q = np.float32(xmax)
    while True:   # (not every float32 is 1.5 times another: the first one beyond xmax that is)
        q = np.nextafter(q, np.float32(np.inf))
        if solve_t(q) is not None:
            break
    out["outside"] = (np.array([solve_t(q), solve_t(ymax)], np.float32), None)
    return out


def _table(pano, bev):
    """The render rows of a case.  Geometric poses over the five dense families, both surfaces alternating; the single-pixel poses over
    two; the three (nearly) empty families; a far, a NaN and an infinite translation.  69 rows: no multiple of 8, so the splat's last
    group of eight renders is partial."""
    img_h, img_w, mpp = BEVS[bev]
    xmin, xmax, ymin, ymax = bo.BevGrid(img_h, img_w, mpp).lims
    hx, hy = float(xmax), float(ymax)
    I = np.eye(2, dtype=np.float32)
    zero = np.zeros((2, 2), np.float32)
    a = np.deg2rad(64.0)
    reflection = np.array([[np.cos(a), np.sin(a)], [np.sin(a), -np.cos(a)]], np.float32)
    t = lambda fx, fy: np.array([fx * hx / 1.5, fy * hy / 1.5], np.float32)
    geometric = [("identity", I, t(0, 0), 0), ("rot0", I, t(0.1, -0.15), 1),
                 ("rot90", np.array([[0, -1], [1, 0]], np.float32), t(-0.2, 0.1), 1), ("rot180", np.array([[-1, 0], [0, -1]], np.float32), t(0.3, 0.25), 1),
                 ("rot270", np.array([[0, 1], [-1, 0]], np.float32), t(0.05, -0.3), 1), ("generic", _rot(37.0), t(-0.25, 0.2), 1),
                 ("reflection", reflection, t(0.15, 0.1), 1), ("scaled 0.3", _rot(205.0, 0.3), t(-0.5, -0.4), 1), ("scaled 3", _rot(118.0, 3.0), t(0.4, -0.2), 1)]
    rows = []
    for k, p in enumerate((0, 1, 2, 5, 7)):
        rows += [Row(p, (k + j) % 2, R, tt, ap, name) for j, (name, R, tt, ap) in enumerate(geometric)]
    for k, (name, (tt, _)) in enumerate(single_pixel_poses(bev).items()):
        rows += [Row(1, k % 2, zero, tt, 1, name), Row(5, (k + 1) % 2, zero, tt, 1, name)]
    for p in (3, 4, 6):
        rows += [Row(p, 0, I, t(0, 0), 0, "identity"), Row(p, 1, I, t(0, 0), 0, "identity"), Row(p, p % 2, _rot(37.0), t(-0.25, 0.2), 1, "generic")]
    corner = single_pixel_poses(bev)["corner"][0]
    rows += [Row(4, 0, zero, corner, 1, "corner"), Row(4, 1, zero, corner, 1, "corner")]   # 65 m: counted, mostly beyond the slices
    rows += [Row(1, 0, _rot(37.0), np.array([1e6, 1e6], np.float32), 1, "far"), Row(1, 1, _rot(37.0), np.array([np.nan, 0.5], np.float32), 1, "nan"),
             Row(2, 0, I, np.array([0.25, np.inf], np.float32), 1, "inf")]
    return tuple(rows)


class Case:
    def __init__(self, pano, bev, table=None, z_cut=False):
        self.pano, self.bev, self.id = pano, bev, f"{pano}-{bev}" + ("-zcut" if z_cut else "")
        self.z_ranges = z_cut_ranges(pano) if z_cut else Z_RANGES   # per surface (lo, hi): what the test sets in the rasteriser's configuration
        self.pano_hw, self.crop_ratio = PANOS[pano][:2], PANOS[pano][2]
        self.crop_rows = _crop_rows(pano)
        self.rows = self.pano_hw[0] - 2 * self.crop_rows
        self.npts = self.rows * self.pano_hw[1]
        self.bev_params = BEVS[bev]                      # BEVParams(*bev_params)
        self.grid = bo.BevGrid(*BEVS[bev])
        self.hw = (self.grid.H, self.grid.W)
        self.rgb, self.depth = pano_set(pano)
        self.table = _table(pano, bev) if table is None else tuple(table)

    def kept_range(self, surface):
        """The surface's z range as `kept` and `block_boxes` take it: None for the default."""
        return None if self.z_ranges is Z_RANGES else self.z_ranges[surface]


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(Case(p, b) for p, b in CASES) + (Case("narrow", "21x29", z_cut=True),)


def case(case_id):
    return next(c for c in cases() if c.id == case_id)


# ---------------------------------------------------------------------------------------------------- the oracle
def _empty(c):
    H, W = c.hw
    return Result(0, np.full((c.npts, 2), -1, np.int16), np.full((H, W), -1, np.int32), np.zeros((H, W, 3), np.uint8), np.zeros((H, W), bool),
                  np.zeros((H, W, 3), np.uint8), 0)


def posed_cloud(c, row):
    """The oracle's posed cloud of a row (what `render_bev_image` is given) and the raster index of its points."""
    xyzrgb, idx = kept(c.pano, row.pano, row.surface, c.kept_range(row.surface))
    if row.apply_pose:
        a, _ = bo.pose_pair(xyzrgb, xyzrgb[:1], row.R, row.t)
    else:
        _, a = bo.pose_pair(xyzrgb[:1], xyzrgb, row.R, row.t)
    return a, idx


def _oracle_row(c, row):
    a, idx = posed_cloud(c, row)
    res = bo.render_bev_image(a, c.grid, mode="exact")
    if res is None:
        return _empty(c)
    H, W = c.hw
    img_xy = np.full((c.npts, 2), -1, np.int16)
    img_xy[idx[res["kept"]]] = res["img_xy"].astype(np.int16)
    winner = np.full((H, W), -1, np.int32)
    wxy = res["img_xy"][res["valid"]]
    winner[wxy[:, 1], wxy[:, 0]] = idx[res["kept"]][res["valid"]]
    return Result(int(res["kept"].sum()), img_xy, winner, res["sparse"], res["mask"], np.ascontiguousarray(res["bev"]), int(res["valid"].sum()))


# ---------------------------------------------------------------------------------------------------- the emulator and its mutants
@functools.lru_cache(maxsize=None)
def block_boxes(name, p, surface, z_range=None):
    """float32 [blocks, 4] (xmin, ymin, xmax, ymax) in the pre-pose frame of the kept points of every 16 x 4 block, as
    `pano_index_entry` computes it (an empty block: xmin > xmax), and the same per group of 64 block columns."""
    W = PANOS[name][1]
    xy, _ = _cloud(name, p)
    idx = kept(name, p, surface, z_range)[1]
    bpr = (W + BLK_W - 1) // BLK_W
    nbr = (_rows_of(name) + BLK_H - 1) // BLK_H
    gpr = (bpr + GROUP - 1) // GROUP
    x, y = xy[idx, 0].astype(np.float32), xy[idx, 1].astype(np.float32)
    out = []
    for ids, n in (((idx // W // BLK_H) * bpr + (idx % W) // BLK_W, nbr * bpr), (group_of(name, idx), nbr * gpr)):
        box = np.empty((n, 4), np.float32)
        box[:, :2], box[:, 2:] = 1e30, -1e30
        np.minimum.at(box[:, 0], ids, x); np.minimum.at(box[:, 1], ids, y)
        np.maximum.at(box[:, 2], ids, x); np.maximum.at(box[:, 3], ids, y)
        out.append(box)
    return out[0], out[1]


def _rows_of(name):
    return PANOS[name][0] - 2 * _crop_rows(name)


def reaches(box, R, t15, rect, mode="true"):
    """`splat_reaches` in float32 numpy for boxes [n, 4] against tile rectangles [n, 4] = (wx0, wx1, wy0, wy1), margin included.
    mode "true": centre + |R| half-extents + slack; "no-rotation": the half-extents not mixed by |R|; "centre": the posed centre alone."""
    f = np.float32
    R = np.asarray(R, f)
    cx, cy = f(0.5) * (box[:, 0] + box[:, 2]), f(0.5) * (box[:, 1] + box[:, 3])
    hx, hy = f(0.5) * (box[:, 2] - box[:, 0]), f(0.5) * (box[:, 3] - box[:, 1])
    px, py = R[0, 0] * cx + R[0, 1] * cy + t15[0], R[1, 0] * cx + R[1, 1] * cy + t15[1]
    if mode == "true":
        qx, qy = np.abs(R[0, 0]) * hx + np.abs(R[0, 1]) * hy, np.abs(R[1, 0]) * hx + np.abs(R[1, 1]) * hy
    elif mode == "no-rotation":
        qx, qy = hx, hy
    else:
        qx = qy = f(0)
    slack = f(0) if mode == "centre" else SLACK * (np.abs(cx) + np.abs(cy) + hx + hy + np.abs(t15[0]) + np.abs(t15[1]))
    with np.errstate(invalid="ignore"):
        return (box[:, 0] <= box[:, 2]) & (px + qx + slack >= rect[:, 0]) & (px - qx - slack <= rect[:, 1]) & (py + qy + slack >= rect[:, 2]) & (py - qy - slack <= rect[:, 3])


def tile_rects(c, margin=MARGIN):
    """float32 [tiles_y, tiles_x, 4] (wx0, wx1, wy0, wy1): the tiles in the posed frame as `bev_splat_kernel` computes them."""
    g = c.grid
    xmin, xmax, ymin, ymax = g.lims
    H, W = c.hw
    out = np.zeros(((H + TILE - 1) // TILE, (W + TILE - 1) // TILE, 4), np.float32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            x0, y0 = tx * TILE, ty * TILE
            tw, th = min(TILE, W - x0), min(TILE, H - y0)
            out[ty, tx] = (np.float32(max(xmin if x0 == 0 else (x0 - 0.5) / g.scale + xmin, xmin)) - margin,
                           np.float32(min(xmax if x0 + tw == W else (x0 + tw - 0.5) / g.scale + xmin, xmax)) + margin,
                           np.float32(max(ymin if y0 == 0 else (y0 - 0.5) / g.scale + ymin, ymin)) - margin,
                           np.float32(min(ymax if y0 + th == H else (y0 + th - 0.5) / g.scale + ymin, ymax)) + margin)
    return out


def survives_cull(c, row, idx, pix, mode):
    """bool per in-window point (raster index `idx`, pixel `pix`): does the tile that owns the point visit the point's block under the
    two-level cull in `mode`?  ("centre": the block level alone, without margin.)"""
    W = c.pano_hw[1]
    bpr = (W + BLK_W - 1) // BLK_W
    boxes, gboxes = block_boxes(c.pano, row.pano, row.surface, c.kept_range(row.surface))
    R = row.R if row.apply_pose else np.eye(2, dtype=np.float32)
    t15 = (row.t * np.float32(1.5)) if row.apply_pose else np.zeros(2, np.float32)
    rect = tile_rects(c, np.float32(0) if mode == "centre" else MARGIN)[pix[:, 1] // TILE, pix[:, 0] // TILE]
    ok = reaches(boxes[(idx // W // BLK_H) * bpr + (idx % W) // BLK_W], R, t15, rect, mode)
    if mode != "centre":
        ok &= reaches(gboxes[group_of(c.pano, idx)], R, t15, rect, mode)
    return ok


def _emulate_row(c, row, mutant):
    H, W = c.hw
    Hp, Wp = c.pano_hw
    xy_all, z_all = _cloud(c.pano, row.pano)
    lo, hi = c.z_ranges[row.surface]
    keep = (z_all >= lo) & (z_all < hi) if mutant == "z filter lo <= z < hi" else (z_all > lo) & (z_all <= hi)
    p_all = np.arange(c.npts)
    if mutant == "partial block column dropped":
        keep &= p_all % Wp < Wp // BLK_W * BLK_W
    if mutant == "partial block row dropped":
        keep &= p_all // Wp < c.rows // BLK_H * BLK_H
    if mutant == "block columns >= 64 dropped":
        keep &= p_all % Wp // BLK_W < GROUP
    if mutant == "groups beyond GLIST_CAP dropped" and keep.any():
        g = group_of(c.pano, p_all)
        keep &= g < g[keep].min() + GLIST_CAP
    idx = np.nonzero(keep)[0]
    xy, z = xy_all[idx], z_all[idx]
    if row.apply_pose:
        t15 = row.t.astype(np.float64) * 1.5 if mutant == "t * 1.5 in double" else (row.t * np.float32(1.5)).astype(np.float64)
        xy = bo.rot2(xy, row.R.astype(np.float64), t15)
    xmin, xmax, ymin, ymax = c.grid.lims
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        if mutant == "window exclusive at its upper edges":
            inwin = (xmin <= x) & (x < xmax) & (ymin <= y) & (y < ymax)
        else:
            inwin = (xmin <= x) & (x <= xmax) & (ymin <= y) & (y <= ymax)
    idx, z = idx[inwin], z[inwin]
    v = (xy[inwin] + np.array([-xmin, -ymin], np.float64)) * c.grid.scale
    pix = (np.floor(v + 0.5) if mutant == "round half away from zero" else np.round(v)).astype(np.int64)
    if mutant in ("centre-only cull", "cull ignores the rotation", "emulated cull") and idx.size:
        ok = survives_cull(c, row, idx, pix, {"centre-only cull": "centre", "cull ignores the rotation": "no-rotation", "emulated cull": "true"}[mutant])
        idx, z, pix = idx[ok], z[ok], pix[ok]
    sl = np.floor(z) + 2
    cand = (sl >= 0) & (sl < 4)
    count = int(cand.sum()) if mutant == "count leaves out points beyond the slices" else int(idx.size)
    if idx.size == 0:
        return _empty(c)
    out = _empty(c)
    out.img_xy[idx] = pix.astype(np.int16)
    ci, cs, cp = idx[cand], sl[cand].astype(np.int64), pix[cand]
    if ci.size == 0:
        return out._replace(count=count)
    cell = cp[:, 1] * W + cp[:, 0]
    order = np.lexsort((-ci if mutant == "first index wins within a slice" else ci, -cs if mutant == "lower slice wins" else cs, cell))
    last = np.ones(order.size, bool)
    last[:-1] = cell[order][1:] != cell[order][:-1]
    win = order[last]
    widx, wpix = ci[win], cp[win]
    out.winner[wpix[:, 1], wpix[:, 0]] = widx
    colours = c.rgb[row.pano].reshape(-1, 3) if mutant == "colours without the crop offset" else c.rgb[row.pano][c.crop_rows:Hp - c.crop_rows].reshape(-1, 3)
    col = colours[widx]
    out.sparse[wpix[:, 1], wpix[:, 0]] = col
    seed = out.winner >= 0 if mutant == "non-empty from occupancy" else bo.nonempty_mask(out.sparse)
    mask = bo.box_dilate(seed, 11)
    interp = bo.interp_exact(wpix, col, H, W)[0]
    bev = np.ascontiguousarray(np.flipud((mask[:, :, None].astype(np.float32) * interp).astype(np.uint8)))
    return Result(count, out.img_xy, out.winner, out.sparse, mask, bev, int(widx.size))


_CACHE = {}


def expected(c, mutant=None):
    """Per row of the case a Result(count, img_xy int16 [npts, 2], winner int32 [H, W] (-1: none), sparse uint8 [H, W, 3], mask bool
    [H, W], bev uint8 [H, W, 3] (flipped, as the kernel writes it), sites).  mutant None: the ORACLE's, computed once per case and
    read-only; "none": the emulator without a mistake; "emulated cull": the emulator with the kernel's own two-level cull in float32;
    a key of MUTANTS: the emulator with that one mistake."""
    if mutant is not None:
        return [_emulate_row(c, row, mutant) for row in c.table]
    if c.id not in _CACHE:
        res = [_oracle_row(c, row) for row in c.table]
        for r in res:
            for a in r[1:6]:
                a.setflags(write=False)
        _CACHE[c.id] = res
    return _CACHE[c.id]


def differing(a, b):
    """The names of the compared quantities in which two Results differ."""
    return [q for q in QUANTITIES if not np.array_equal(getattr(a, q), getattr(b, q))]


def words(images):
    """uint8 [..., 3] -> int32 [...] 0x00BBGGRR, the kernel's image format."""
    u = images.astype(np.int32)
    return u[..., 0] | (u[..., 1] << 8) | (u[..., 2] << 16)
