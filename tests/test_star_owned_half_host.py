"""The owned-half stop rule of the star walks (salve_amd/csrc/star_delaunay.h sd_walk, star_local.h sdl_lean_step), compiled for
the HOST with g++ from the very same headers: a walk visits only the neighbours at angles [0, pi), in a first and at most one second
direction, and the lean walk hands its direction AND its phase over to the general walk.  Checked against the independent CPU oracle."""

import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import bev_oracle as bo
from salve_amd import synthetic

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("owned_half") / "star_owned_half_host.so"
    extra = os.environ.get("STAR_HOST_CXXFLAGS", "").split()   # e.g. sanitizer flags (CPU build only), as in test_star_host.py
    subprocess.run(["g++", "-O2", "-shared", "-fPIC"] + extra + ["-o", str(so), str(ROOT / "tests" / "host" / "star_owned_half_host.cpp")], check=True)
    return ctypes.CDLL(str(so))


def oracle_tri_xy(pts):
    order, tri = bo.delaunay_exact(pts[:, 0], pts[:, 1])
    return np.ascontiguousarray(pts[order][tri].reshape(-1, 6), dtype=np.int32)


def handover(lib, pts, H, W, table, cache, ref=None):
    """every site, every k: lean walk for k steps + general walk from there == the oracle's triangles the site owns, each once"""
    pts = np.unique(np.asarray(pts, dtype=np.int64), axis=0)
    ref = oracle_tri_xy(pts) if ref is None else ref
    xs = np.ascontiguousarray(pts[:, 0], dtype=np.int32)
    ys = np.ascontiguousarray(pts[:, 1], dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    fail = np.zeros(4, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bad = lib.owned_half_handover(p(xs), p(ys), len(xs), H, W, p(ref), len(ref), table, cache, p(stats), p(fail))
    assert bad == 0, f"{bad} hand-overs differ from the oracle; first: site ({fail[0]}, {fail[1]}) after {fail[2]} lean steps (table {table}, cache {cache})"
    return stats


def all_modes(lib, pts, H, W):
    pts = np.unique(np.asarray(pts, dtype=np.int64), axis=0)
    assert not bo._is_degenerate(pts)
    ref = oracle_tri_xy(pts)
    assert len(ref) > 0
    total = np.zeros(8, dtype=np.int64)
    for table in (1, 0):
        for cache in (0, 1):
            total += handover(lib, pts, H, W, table, cache, ref)
    return total


def test_handover_at_every_step_random_lattice_sets(lib):
    rng = np.random.default_rng(5)
    done = 0
    total = np.zeros(8, dtype=np.int64)
    for _ in range(250):
        G = int(rng.integers(3, 60))
        pts = np.unique(rng.integers(0, G, size=(int(rng.integers(3, 500)), 2)), axis=0)
        if bo._is_degenerate(pts):
            continue
        ref = oracle_tri_xy(pts)
        if not len(ref):
            continue
        for table in (1, 0):
            for cache in (0, 1):
                total += handover(lib, pts, G, G, table, cache, ref)
        done += 1
    assert done > 150
    print("hand-overs", total[0], "resumed", total[1], "with dir +1, -1, +2, -2, half:", total[2:7].tolist(), "lean walks finished", total[7])
    # every phase and direction the state word can carry was handed over (+2 without a right neighbour is the rare one: a clockwise
    # first direction that met the hull before it entered the owned half)
    assert total[1] == total[2:7].sum() and (total[[2, 3, 5, 6]] > 1000).all() and total[4] > 0


def test_handover_at_every_step_structured_degenerate_sets(lib):
    """Full lattices, lines with one off-point, rings, every other site: maximal co-circularity and collinear hulls."""
    yy, xx = np.mgrid[0:12, 0:17]
    full = np.stack([xx.ravel(), yy.ravel()], 1)
    line = np.array([[i, 3] for i in range(20)] + [[7, 9]])
    th = np.linspace(0, 2 * np.pi, 80, endpoint=False)
    ring = np.unique(np.round(np.stack([30 + 25 * np.cos(th), 30 + 25 * np.sin(th)], 1)).astype(int), axis=0)
    for pts, G in ((full, 17), (line, 20), (ring, 61), (full[::2], 17)):
        all_modes(lib, pts, G, G)


def blob(rng, cx, cy, r, n):
    p = rng.integers(-r, r + 1, size=(n, 2))
    p = p[(p ** 2).sum(1) <= r * r]
    return p + np.array([cx, cy])


def two_clusters():
    rng = np.random.default_rng(41)
    # 40 pixels apart: the edges between them are far beyond the candidate table; (33, 30) has no 8-neighbour -- a fresh walk with a far n0
    return np.concatenate([blob(rng, 12, 14, 7, 60), blob(rng, 52, 10, 7, 60), blob(rng, 14, 54, 6, 40), [[33, 30], [60, 62], [0, 40]]]), 64


def border_set():
    rng = np.random.default_rng(43)
    G = 70
    cols = np.array([0, 31, 32, 63, 64, G - 1])
    ys = np.arange(0, G, 3)
    grid = np.stack(np.meshgrid(cols, ys), -1).reshape(-1, 2)
    top = np.stack([np.arange(0, G, 2), np.zeros(G // 2, dtype=int)], 1)
    bottom = np.stack([np.arange(1, G, 4), np.full(len(range(1, G, 4)), G - 1)], 1)
    pairs = np.array([[30, 20], [31, 20], [32, 20], [33, 20], [62, 41], [63, 41], [64, 41], [65, 41], [31, 50], [32, 51], [63, 7], [64, 8]])
    return np.concatenate([grid, top, bottom, pairs, rng.integers(0, G, size=(60, 2))]), G


def test_crafted_stars(lib):
    rng = np.random.default_rng(37)
    G = 48
    # the raster-last site isolated (every neighbour precedes it: it owns nothing), the raster-first site isolated (it owns its whole star)
    body = blob(rng, 24, 20, 9, 120)
    all_modes(lib, np.concatenate([body, [[25, 40]]]), G, G)
    all_modes(lib, np.concatenate([body, [[22, 2]]]), G, G)
    all_modes(lib, np.concatenate([body, [[25, 40], [22, 2], [2, 21], [45, 19]]]), G, G)
    # n0 at each of the eight neighbour positions, with and without a right neighbour, in the interior, on the outline and as the whole star's first edge
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)):
        for right in (False, True):
            for where in ("inside", "below", "above", "left", "right"):
                far = rng.integers(0, G, size=(90, 2))
                far = far[(np.abs(far - 24).max(1) >= 3)]   # nothing else in the 5 x 5 around s = (24, 24)
                if where == "below":
                    far = far[far[:, 1] < 24]
                elif where == "above":
                    far = far[far[:, 1] > 24]
                elif where == "left":
                    far = far[far[:, 0] < 24]
                elif where == "right":
                    far = far[far[:, 0] > 24]
                pts = np.concatenate([far, [[24, 24], [24 + dx, 24 + dy]], [[25, 24]] if right else np.zeros((0, 2), dtype=int)])
                all_modes(lib, pts, G, G)
    # hull vertices whose gap covers the upper half from the 0 side (right of the cloud), from the pi side (left), entirely (top):
    # a sparse disc has hull vertices all round, the four extreme sites of a diamond and of a square added
    disc = blob(rng, 24, 24, 15, 110)
    all_modes(lib, np.concatenate([disc, [[24, 44], [24, 4], [3, 24], [45, 24]]]), G, G)
    all_modes(lib, np.concatenate([disc, [[2, 2], [46, 2], [2, 46], [46, 46]]]), G, G)
    all_modes(lib, np.concatenate([blob(rng, 24, 24, 15, 700), [[24, 44], [24, 4], [3, 24], [45, 24]]]), G, G)
    pts, Gc = two_clusters()
    total = all_modes(lib, pts, Gc, Gc)
    assert total[0] - total[1] > 0
    pts, Gb = border_set()
    all_modes(lib, pts, Gb, Gb)


# ---- work counters: tools/probe/host/walk_counters.cpp on the six site sets of tools/probe/host/walk_sites.py, schedule NW = 8, RUN = 8.
# The parent's figures (full-circle walks), measured with the same tool on the same sets: lean steps of the walked sites, E2 apex queries.
PARENT = {("box", 0): (111645, 2823), ("box", 5): (111409, 1833), ("cluttered", 0): (103054, 3280), ("cluttered", 5): (101433, 2954),
          ("noisy", 0): (106276, 3867), ("noisy", 5): (99758, 5639)}


def tool_hash(sp, tri):
    """walk_counters.cpp's hash of the sorted triangle list, from the oracle's triangles: (s, b, c), s raster-first, counter-clockwise"""
    v = sp[tri].astype(np.int64)                                   # [nt, 3, (x, y)]
    first = np.argmin(v[:, :, 1] * 4096 + v[:, :, 0], axis=1)
    idx = (first[:, None] + np.arange(3)[None]) % 3
    v = np.take_along_axis(v, idx[:, :, None], 1)
    orient = (v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1]) - (v[:, 1, 1] - v[:, 0, 1]) * (v[:, 2, 0] - v[:, 0, 0])
    assert (orient != 0).all()
    v[orient < 0] = v[orient < 0][:, [0, 2, 1]]
    rows = v.reshape(-1, 6)
    rows = rows[np.lexsort(rows.T[::-1])]
    q = rows.ravel().astype(np.uint64)
    with np.errstate(over="ignore"):
        pw = np.cumprod(np.concatenate([[np.uint64(1)], np.full(len(q) - 1, 1000003, dtype=np.uint64)]), dtype=np.uint64)[::-1]
        return int((q * pw).sum(dtype=np.uint64))


def test_work_counters_against_the_full_circle_walks(tmp_path):
    exe = tmp_path / "walk_counters"
    subprocess.run(["g++", "-O2", "-DNW=8", "-DRUN=8", "-o", str(exe), str(ROOT / "tools" / "probe" / "host" / "walk_counters.cpp")], check=True)
    hyp = synthetic.make_hypotheses(16, 2, seed=0)   # (the recipe of tools/probe/host/walk_sites.py, which keeps only the sites)
    files, want = [], {}
    for scene, j in PARENT:
        rgb, depth = synthetic.make_pano(j % 2, scene=scene)
        a = bo.xyzrgb_from_arrays(depth, rgb, bo.floor_ceiling_z_range("floor"))
        a, _ = bo.pose_pair(a, a[:1], hyp.R[j], hyp.t[j])
        res = bo.render_bev_image(a, mode="exact")
        f = tmp_path / f"sites_{scene}_{j}.bin"
        res["site_xy_sorted"].astype(np.int32).tofile(f)
        files.append(str(f))
        want[str(f)] = (scene, j, len(res["site_xy_sorted"]), len(res["tri"]), tool_hash(res["site_xy_sorted"], res["tri"]))
    out = subprocess.run([str(exe)] + files, check=True, capture_output=True, text=True).stdout
    lines = out.strip().splitlines()
    assert len(lines) == len(files)
    for line in lines:
        print(line)
        name = line.split(": sites ")[0]
        scene, j, nsites, ntri, h = want[name]
        m = re.search(r"sites (\d+) triangles (\d+) \(hash ([0-9a-f]+)\)", line)
        assert (int(m.group(1)), int(m.group(2))) == (nsites, ntri)
        assert int(m.group(3), 16) == h, "the tool's triangles are not the oracle's"
        lean = int(re.search(r"lean steps (\d+)", line).group(1))
        apex = int(re.search(r"apex queries (\d+) =", line).group(1))
        m = re.search(r"sweeping (\d+) \((\d+) of them for a triangle the site does not own\)", line)
        assert 0 <= int(m.group(2)) <= int(m.group(1))
        p_lean, p_apex = PARENT[(scene, j)]
        print(f"  {scene} {j}: lean steps {lean} = {lean / p_lean:.3f} of the parent's, E2 apex queries {apex} = {apex / p_apex:.3f}")
        assert lean <= 0.90 * p_lean
        assert apex <= 0.80 * p_apex
