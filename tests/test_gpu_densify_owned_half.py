"""bev_densify_kernel with the owned-half star walks (star_delaunay.h sd_walk, star_local.h): site sets where most sites have no right
neighbour -- the walks that used to go round the whole star --, through the C ABI with the work counters, bit for bit against the
oracle's exact interpolant.  G = 48: two bitmap words per row, the 31 / 32 boundary inside; G = 131: five words."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import bev_oracle as bo  # noqa: E402
from test_star_owned_half_host import border_set, two_clusters  # noqa: E402


def random_set(G, dens, seed):
    return np.argwhere(np.random.default_rng(seed).random((G, G)) < dens)[:, ::-1]


def columns_in_a_disc(G):
    yy, xx = np.mgrid[0:G, 0:G]
    c = (G - 1) / 2.0
    m = (xx % 2 == 0) & ((xx - c) ** 2 + (yy - c) ** 2 <= (0.47 * G) ** 2)   # no site has a right neighbour, the outline is round
    return np.stack([xx[m], yy[m]], 1)


def ring(G):
    th = np.linspace(0, 2 * np.pi, 6 * G, endpoint=False)
    c = (G - 1) / 2.0
    return np.unique(np.round(np.stack([c + 0.45 * G * np.cos(th), c + 0.45 * G * np.sin(th)], 1)).astype(int), axis=0)   # empty interior


def row_with_gaps(G):
    xs = np.array([x for x in range(1, G - 1) if x % 7 not in (3, 4) and x % 11 != 0])
    return np.concatenate([np.stack([xs, np.full(len(xs), G // 2)], 1), [[G // 3, G - 2], [2 * G // 3, 1]]])   # + one site above, one below


SETS = {
    "random 2 %": lambda G: random_set(G, 0.02, 101),
    "random 10 %": lambda G: random_set(G, 0.10, 102),
    "random 30 %": lambda G: random_set(G, 0.30, 103),
    "every other column in a disc": columns_in_a_disc,
    "ring": ring,
    "row with gaps": row_with_gaps,
    "two clusters": lambda G: two_clusters()[0],
    "image border and word boundaries": lambda G: border_set()[0],
}
CASES = [(G, name) for G in (48, 131) for name in SETS if G == 131 or name not in ("two clusters", "image border and word boundaries")]

_ras = {}


def rasteriser(G):
    from salve_amd.common.bevparams import BEVParams
    from salve_amd.rasteriser import BevRasteriser

    if G not in _ras:
        _ras[G] = BevRasteriser(torch.device("cuda:0"), bev_params=BEVParams(img_h=G - 1, img_w=G - 1, meters_per_px=1.0))
        _ras[G].cfg.out_flags = 3   # no flip, no mask: the plain interpolant
    return _ras[G]


@pytest.mark.parametrize("G,name", CASES)
def test_densify_is_the_oracle_interpolant(G, name):
    from salve_amd import status

    dev = torch.device("cuda:0")
    ras = rasteriser(G)
    pts = np.unique(np.asarray(SETS[name](G), dtype=np.int64), axis=0)
    assert len(pts) >= 4 and pts.min() >= 0 and pts.max() < G and not bo._is_degenerate(pts)
    col = np.stack([(pts[:, 0] * 7 + pts[:, 1] * 3) % 256, (pts[:, 0] * 5 + 11) % 256, (pts[:, 1] * 13) % 256], 1).astype(np.uint8)
    xy = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.int32)).to(dev)
    rgb = torch.from_numpy(col).to(dev)
    bev = torch.empty((1, G, G), dtype=torch.int32, device=dev)
    status.check(dev, "before")
    ras.keys_from_pixels(xy, rgb, bev)
    stats = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    ws = ras._workspace(1)
    st = ras.lib.salve_bev_densify(ctypes.byref(ras.cfg), 1, ctypes.c_void_p(bev.data_ptr()), None, ctypes.c_void_p(stats.data_ptr()),
                                   status.ptr(dev), ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert st == 0, ras.lib.salve_last_error()
    torch.cuda.synchronize()
    status.check(dev, name)      # raises on SALVE_STATUS_WALK_FAILED
    sv = stats.cpu().numpy()[0]
    print(f"G = {G}, {name}: {sv[0]} sites, {sv[4]} lean iterations, {sv[6]} hard sites, {sv[7]} queued triangles")
    assert sv[0] == len(pts) and sv[5] == 0
    got = ras.export_u8(bev)[0].cpu().numpy()
    assert np.array_equal(got, bo.interp_exact(pts, col, G, G)[0]), (G, name)
