"""The seeded layout fixtures the host and the GPU tests of device-side layout posing share -- the seeded set, the half-pixel set and
the strided set (rooms and W/D/O lists longer than the posing kernel's 64 threads, also in a non-square window) --, the comparator of
the integer tables, and an emulator of WRONG posing kernels the comparator must reject (not a test module)."""

import functools

import numpy as np

from salve_amd import layout, synthetic, synthetic_layouts
from salve_amd.common.bevparams import BEVParams
from salve_amd.common.sim2 import Sim2

P, N = 64, 512   # panoramas, posed images (the P identity images follow them)
VARIANTS = ("R transposed", "t after the scale", "no 1.5 factor", "round half away", "closing vertex dropped", "doors and windows swapped")


@functools.lru_cache(maxsize=None)
def seeded_set():
    """(PanoLayouts, pano [N + P], R, t, s, posed): 512 poses over the full circle whose translations push parts of rooms out of the
    window, scales 1 and not 1, then every panorama's own layout (garbage in R / t / s: an identity image must not read them).
    Panorama 1 has an empty room; panoramas 2, 5, 8, ... have no W/D/O."""
    pl = synthetic_layouts.make_layouts(P, seed=0)
    hyp = synthetic.make_hypotheses(N, P, seed=2)
    s = np.where(np.arange(N) % 3 == 0, 1.0, np.random.default_rng(1).uniform(0.8, 1.25, N))
    pano = np.concatenate([hyp.i1.astype(np.int64), np.arange(P)])
    pano[:3] = (1, 2, 5)   # the empty room and two rooms without W/D/Os are posed too
    R = np.concatenate([hyp.R, np.full((P, 2, 2), 3.0, np.float32)])
    t = np.concatenate([hyp.t, np.full((P, 2), -7.0, np.float32)])
    return pl, pano, R, t, np.concatenate([s, np.full(P, 9.0)]), np.arange(N + P) < N


def host_specs(pl, pano, R, t, s, posed):
    """The `layout_pair_specs`-style specs of the same images: the host chain `pack_layouts` takes."""
    return [pl.spec(int(p), Sim2(R[k], t[k], float(s[k])) if posed[k] else None) for k, p in enumerate(pano)]


@functools.lru_cache(maxsize=None)
def seeded_host_tables():
    """`pack_layouts`' rec / poly / seg of the seeded set (computed once, never changed)."""
    tabs = layout.pack_layout_tables(host_specs(*seeded_set()))
    for a in tabs:
        a.setflags(write=False)
    return tabs


def half_pixel_set():
    """Identity images whose coordinates land EXACTLY on half pixels: (x * 1.5 + 5) * 50 = 212.5, 362.5, 512.5, 287.5, 137.5 for
    x = -0.5, 1.5, 3.5, 0.5, -1.5 -- every step exact in fp64.  Half to even and half away from zero differ on the first three."""
    v = np.array([-0.5, 1.5, 3.5, 0.5, -1.5])
    assert ((v * 1.5 + 5.0) * 50.0 % 1.0 == 0.5).all()
    ring = np.array([[-0.5, -0.5], [1.5, -0.5], [3.5, 0.5], [1.5, 1.5], [-0.5, 1.5], [-1.5, 0.5]])
    room = np.vstack([ring, ring[:1]])
    pl = layout.PanoLayouts.from_specs([(room, [("doors", np.array([[-0.5, -0.5], [1.5, -0.5]])), ("windows", np.array([[1.5, 1.5], [-0.5, 1.5]]))]),
                                        (room[::-1].copy(), [("openings", np.array([[3.5, 0.5], [1.5, 1.5]]))])])
    return pl, np.array([0, 1]), None, None, None, np.array([False, False])


STRIDE_ROOMS, STRIDE_WDOS = (1, 63, 64, 65, 130, 200), (0, 31, 32, 33, 70)   # salve_layout_pose strides by 64 threads: vertex 64, W/D/O 32
STRIDE_PANOS = ((1, 0), (63, 31), (64, 32), (65, 33), (130, 70), (200, 31), (64, 70), (200, 0))   # (stored room vertices, W/D/Os) per panorama
WINDOWS = {"default": None, "44x82 at 0.1": dict(img_h=44, img_w=82, meters_per_px=0.1)}


def window_params(name):
    """The BEVParams of a WINDOWS entry (None: the default 500 x 500 at 0.02 m per pixel)."""
    kw = WINDOWS[name]
    return None if kw is None else BEVParams(**kw)


@functools.lru_cache(maxsize=None)
def strided_set():
    """(PanoLayouts, pano, R, t, s, posed) for the second pass of the posing kernel's loops: rooms of 1, 63, 64, 65, 130 and 200
    stored vertices (closed rings on a wobbling circle; the single vertex is a point), 0, 31, 32, 33 and 70 W/D/Os per panorama
    spread over all three types, every panorama under three poses like `seeded_set`'s -- rotations over the full circle,
    translations that push geometry out of the window, scales 1 and not 1 --, then every panorama's own layout."""
    rng = np.random.default_rng(5)
    specs = []
    for nv, nw in STRIDE_PANOS:
        if nv == 1:
            room = np.array([[0.3, -0.2]])
        else:
            a = 2 * np.pi * np.arange(nv - 1) / (nv - 1)
            rad = 2.0 + 0.5 * np.sin(5 * a) + rng.uniform(-0.1, 0.1, nv - 1)
            ring = np.stack([rad * np.cos(a), rad * np.sin(a)], 1)
            room = np.vstack([ring, ring[:1]])
        wdos = []
        for j in range(nw):
            a0 = 2 * np.pi * j / nw
            c = np.array([2.1 * np.cos(a0), 2.1 * np.sin(a0)])
            d = 0.3 * np.array([-np.sin(a0 + 0.2), np.cos(a0 + 0.2)])
            wdos.append((layout.WDO_TYPES[j % 3], np.stack([c - d, c + d])))
        specs.append((room, wdos))
    pl = layout.PanoLayouts.from_specs(specs)
    P_, per = len(STRIDE_PANOS), 3
    n = P_ * per
    ang = rng.uniform(0, 2 * np.pi, n) + 2 * np.pi * np.arange(n) / n
    R = np.stack([np.stack([np.cos(ang), -np.sin(ang)], 1), np.stack([np.sin(ang), np.cos(ang)], 1)], 1).astype(np.float32)
    t = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    s = np.where(np.arange(n) % 3 == 0, 1.0, rng.uniform(0.8, 1.25, n))
    pano = np.concatenate([np.repeat(np.arange(P_), per), np.arange(P_)])
    return (pl, pano, np.concatenate([R, np.full((P_, 2, 2), 3.0, np.float32)]), np.concatenate([t, np.full((P_, 2), -7.0, np.float32)]),
            np.concatenate([s, np.full(P_, 9.0)]), np.arange(n + P_) < n)


@functools.lru_cache(maxsize=None)
def strided_host_tables(window):
    """`pack_layout_tables`' rec / poly / seg of the strided set in a WINDOWS entry (computed once, never changed)."""
    tabs = layout.pack_layout_tables(host_specs(*strided_set()), window_params(window))
    for a in tabs:
        a.setflags(write=False)
    return tabs


def tables_equal(a, b) -> bool:
    """The comparator: three tables, equal in dtype, shape and every element."""
    return len(a) == len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def emulate(variant, pl, pano, R, t, s, posed):
    """The tables of a posing kernel with ONE mistake (`variant`; None: no mistake), written as a plain loop over the images."""
    n = len(pano)
    posed = np.ones(n, bool) if posed is None else np.asarray(posed, bool)
    rec = np.zeros(n, dtype=layout._lib.LAYOUT_DTYPE)
    polys, segs = [], []
    colour = {"windows": 0x0000ff, "doors": 0x00ff00, "openings": 0xff0000}
    if variant == "doors and windows swapped":
        colour["windows"], colour["doors"] = colour["doors"], colour["windows"]

    def px(xy, k):
        Rk = np.asarray(R[k], np.float64).reshape(2, 2) if posed[k] else np.eye(2)
        tk = np.asarray(t[k], np.float64) if posed[k] else np.zeros(2)
        sk = float(s[k]) if posed[k] else 1.0
        if variant == "R transposed":
            Rk = Rk.T
        x = xy[:, 0] * Rk[0, 0] + xy[:, 1] * Rk[0, 1]
        y = xy[:, 0] * Rk[1, 0] + xy[:, 1] * Rk[1, 1]
        q = np.stack([x, y], 1)
        q = q * sk + tk if variant == "t after the scale" else (q + tk) * sk
        q = ((q if variant == "no 1.5 factor" else q * 1.5) + 5.0) * 50.0
        return (np.sign(q) * np.floor(np.abs(q) + 0.5) if variant == "round half away" else np.round(q)).astype(np.int64)

    for k in range(n):
        p = int(pano[k])
        room = pl.room_xy[pl.room_off[p]:pl.room_off[p + 1]]
        if variant == "closing vertex dropped":
            room = room[:-1]
        rec[k] = (len(room), sum(len(a) for a in polys), int(pl.wdo_count[p]), len(segs))
        polys.append(px(room, k))
        for j in range(int(pl.wdo_off[p]), int(pl.wdo_off[p + 1])):
            e = px(pl.wdo_xy[j], k)
            segs.append((*e[0], *e[1], colour[layout.WDO_TYPES[int(pl.wdo_type[j])]], 8, 0, 0))
    return (rec, np.concatenate(polys).astype(np.int32) if n else np.zeros((1, 2), np.int32),
            np.array(segs, dtype=np.int64).astype(np.int32).reshape(-1, 8) if segs else np.zeros((1, 8), np.int32))
