"""The seeded layout fixtures the host and the GPU tests of device-side layout posing share, the comparator of the integer tables,
and an emulator of WRONG posing kernels the comparator must reject (not a test module)."""

import functools

import numpy as np

from salve_amd import layout, synthetic, synthetic_layouts
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
