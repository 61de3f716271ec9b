"""The case set of tests/layout_raster_cases.py on the CPU: the oracle draws every case, every group holds the variety it claims, and
every emulated wrong kernel (`expected(case, mutant=...)`) differs from the true image in the group built for it -- the proof that
the comparison of tests/test_gpu_layout_raster.py can fail.  No GPU.

Measured: the whole module takes 20 s on one CPU core (the oracle over all 19 cases 7 s -- 3 453 images, 3 928 segments, 134 of
the images with a polygon --, the ten mutants over their groups 12 s)."""

import math

import numpy as np
import pytest

import layout_raster_cases as rc
from oracle import layout_oracle as lo

BY_ID = {c.id: c for c in rc.cases()}
LIMIT = 20100   # the farthest coordinate a case uses: nothing near the 2^24 limit (the module's docstring says why)


def _group(name):
    return [c for c in rc.cases() if c.group == name]


def _first(c):
    """The first segment of every image of a one-segment-per-image case."""
    return [s[0] for _, s in c.images]


def test_the_case_list_is_the_groups_times_the_sizes():
    want = [f"{g}-{h}x{w}" for g in rc.GROUPS for h, w in rc.SIZES] + [f"reduced-{h}x{w}" for h, w in rc.REDUCED_SIZES] + ["workload-501x501"]
    assert [c.id for c in rc.cases()] == want and len(BY_ID) == len(want) == 19
    assert rc.SIZES == ((45, 83), (83, 45)) and rc.REDUCED_SIZES == ((16, 16), (17, 33), (1, 1), (1, 40))
    assert set(rc.MUTANTS.values()) <= set(rc.GROUPS) and len(rc.MUTANTS) == 10


@pytest.mark.parametrize("cid", list(BY_ID))
def test_the_oracle_draws_every_case_and_what_it_claims(cid):
    c = BY_ID[cid]
    H, W = c.hw
    rec, poly, segs = c.tables()
    # the tables: inside the kernel's accepted contract, offsets absolute and running
    assert rec.dtype.itemsize == 16 and poly.dtype == np.int32 and segs.dtype == np.int32 and poly.shape[1:] == (2,) and segs.shape[1:] == (8,)
    assert int(rec["n_seg"].sum()) == c.n_segments and (c.n_segments == 0 or len(segs) == c.n_segments)
    assert np.array_equal(rec["seg_off"], np.cumsum(rec["n_seg"]) - rec["n_seg"]) and np.array_equal(rec["poly_off"], np.cumsum(rec["n_poly"]) - rec["n_poly"])
    if c.n_segments:
        assert 1 <= int(segs[:, 5].min()) and int(segs[:, 5].max()) <= 18 and not segs[:, 6:].any()
        assert int(segs[:, 4].min()) >= 0 and int(segs[:, 4].max()) <= 0xFFFFFF
    assert max(int(np.abs(poly).max()), int(np.abs(segs[:, :4]).max())) <= LIMIT
    img = rc.expected(c)
    assert img.shape == (len(c.images), H, W, 3) and img.dtype == np.uint8 and not img.flags.writeable
    assert rc.expected(c) is img                                             # computed once, shared
    wrong = [(i, d) for i, d in enumerate(c.draws) if d is not None and bool(img[i].any()) != d]
    assert not wrong, f"{cid}: images that draw something / nothing against their claim: {wrong[:10]}"
    w = rc.words(img)
    assert w.dtype == np.int32 and int(w.min()) >= 0 and int(w.max()) <= 0xFFFFFF


def test_thickness_direction_group():
    for c in _group("thickness_direction"):
        H, W = c.hw
        segs = _first(c)
        assert all(len(s) == 1 and p is None for p, s in c.images)
        assert sorted({s[5] for s in segs}) == list(rc.THICKNESSES) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 17, 18]
        for t in rc.THICKNESSES:
            vec = [(s[2] - s[0], s[3] - s[1]) for s in segs if s[5] == t]
            undirected = {v if v > (-v[0], -v[1]) else (-v[0], -v[1]) for v in vec}
            assert len(undirected) >= 16 and all((-dx, -dy) in vec for dx, dy in vec)          # >= 16 directions, both end-point orders
            assert {(30, 0), (0, 30), (21, 21), (21, -21)} <= set(vec)                         # both axes, both diagonals
            assert {(30, 1), (30, -1), (1, 30), (-1, 30), (22, 20), (20, 22), (22, -20), (20, -22)} <= set(vec)   # just off them, both signs
            assert all(28 <= math.hypot(*v) <= 31 for v in vec)
        assert all(0 <= s[0] < W and 0 <= s[2] < W and 0 <= s[1] < H and 0 <= s[3] < H for s in segs)


def test_short_group():
    for c in _group("short"):
        segs = _first(c)
        for t in rc.SHORT_THICKNESSES:
            vec = {(s[2] - s[0], s[3] - s[1]) for s in segs if s[5] == t}
            assert {max(abs(dx), abs(dy)) for dx, dy in vec} == {0, 1, 2, 3, 7}
            for n in (1, 2, 3, 7):
                mine = {v for v in vec if max(abs(v[0]), abs(v[1])) == n}
                assert any(v[0] == 0 or v[1] == 0 for v in mine) and any(abs(v[0]) == abs(v[1]) for v in mine)   # axis-aligned, diagonal
            assert any(0 != abs(v[0]) != abs(v[1]) != 0 for v in vec)                                            # oblique
        assert sorted({s[5] for s in segs}) == [1, 2, 5, 8]


def test_borders_group():
    for c in _group("borders"):
        H, W = c.hw
        segs = _first(c)
        img = rc.expected(c)
        assert sorted({s[5] for s in segs}) == list(rc.BORDER_THICKNESSES)
        for t in rc.BORDER_THICKNESSES:
            mine = [s for s in segs if s[5] == t]
            ends = {(s[0], s[1]) for s in mine} | {(s[2], s[3]) for s in mine}
            assert {0, -1, W - 1, W} <= {x for x, _ in ends} and {0, -1, H - 1, H} <= {y for _, y in ends}   # on the border, one beyond
            for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):                                    # through and across each corner
                assert sum(1 for s in mine if min(s[0], s[2]) <= cx <= max(s[0], s[2]) and min(s[1], s[3]) <= cy <= max(s[1], s[3])
                           and abs(s[2] - s[0]) in (12,) and abs(s[3] - s[1]) == 12) >= 2
            for d in range(1, t // 2 + 5):   # wholly outside, at every distance up to thickness / 2 + 4, beyond each border
                assert {(-d, -d), (W - 1 + d, W - 1 + d)} <= {(s[0], s[2]) for s in mine if s[1] != s[3]}
                assert {(-d, -d), (H - 1 + d, H - 1 + d)} <= {(s[1], s[3]) for s in mine if s[0] != s[2]}
        outside = [i for i, s in enumerate(segs) if max(s[0], s[2]) < 0 or min(s[0], s[2]) >= W or max(s[1], s[3]) < 0 or min(s[1], s[3]) >= H]
        assert any(c.draws[i] is True for i in outside) and any(c.draws[i] is False for i in outside)
        assert all(c.draws[i] is False for i in outside if segs[i][5] == 1 and segs[i][:2] != segs[i][2:4]) # clipLine drops a LineAA that lies outside
        far = [i for i, s in enumerate(segs) if max(abs(v) for v in s[:4]) >= 19000]
        assert len(far) >= 20 and all(c.draws[i] is True and img[i].any() for i in far)                     # far end points, the image crossed
        assert any(max(abs(v) for v in segs[i][:2]) < 100 for i in far) and any(min(abs(segs[i][0]), abs(segs[i][1])) > 5000 for i in far)


def test_tiles_group():
    for c in _group("tiles"):
        H, W = c.hw
        segs = _first(c)
        img = rc.expected(c)[:, ::-1]                                                                        # (un-flipped: the kernel's rows)
        assert sorted({s[5] for s in segs}) == list(rc.TILE_THICKNESSES)
        for t in rc.TILE_THICKNESSES:
            mine = [(i, s) for i, s in enumerate(segs) if s[5] == t]
            for axis in (0, 1):   # the segment's axis, and one of its ends, on 15, 16, 31 and 32 and up to its reach + 1 on either side
                along = {s[axis] for _, s in mine if s[axis] == s[axis + 2]}
                ending = {s[axis + 2] for _, s in mine if s[axis] != s[axis + 2]}
                for b in (16, 32):
                    assert set(range(b - t // 2 - 4, b + t // 2 + 5)) <= along
                assert {15, 16, 31, 32} <= along and len(ending & {15, 16, 31, 32}) >= 2
            # a segment whose end points and filled body lie in one tile column while its anti-aliased tail lies in the next
            body = 0 if t == 1 else (t + 1) // 2
            reaching = [i for i, s in mine if s[0] == s[2] and 16 <= s[0] - body and s[0] + body <= 31 and 16 <= s[1] and s[3] <= 31
                        and (img[i][:, :16].any() or img[i][:, 32:].any())]
            assert reaching or 2 * body + 1 >= rc.TILE, t      # (an 18-pixel line is wider than a tile)


def test_chunks_group():
    for c in _group("chunks"):
        counts = [len(s) for _, s in c.images]
        assert set(rc.CHUNK_COUNTS) == {0, 1, 6, 7, 8, 13, 14, 15, 22} <= set(counts)
        assert all(a != b for a, b in zip(counts, counts[1:]))                                               # neighbours differ
        rec = c.tables()[0]
        assert rec["seg_off"].tolist() == (np.cumsum(counts) - counts).tolist() and len(set(rec["seg_off"].tolist())) > 8
        for _, s in c.images:
            if len(s) >= 7:
                assert len({q[4] for q in s}) >= 7 and len({q[5] for q in s}) >= 5                          # different colours and widths
                cx, cy = c.hw[1] // 2, c.hw[0] // 2   # mutually crossing: every segment passes within 2 pixels of the centre
                assert all(abs((q[2] - q[0]) * (cy - q[1]) - (q[3] - q[1]) * (cx - q[0])) <= 2.9 * math.hypot(q[2] - q[0], q[3] - q[1]) for q in s)


def test_colours_group():
    for c in _group("colours"):
        used = {q[4] for _, s in c.images for q in s}
        assert {0x327BC8, 0x010203, 0xFEFDFC, 0x808080} <= used
        assert any(p is not None for p, _ in c.images) and any(p is None for p, _ in c.images)               # over the white room, over black
        pairs = {(s[0][4], s[1][4]) for _, s in c.images if s[0][4] != s[1][4]}
        assert len(pairs) == 30                                                                              # over one another, both orders
        img = rc.expected(c).astype(int)
        assert ((img > 0) & (img < 255)).any()


def test_polygons_group():
    for c in _group("polygons"):
        H, W = c.hw
        named = rc.polygon_set(c.hw)
        assert {"convex", "concave", "bow-tie", "spiral", "pentagram"} <= set(named) and len(c.images) == 2 * len(named)
        n_poly = [0 if p is None else len(p) for p, _ in c.images]
        assert {0, 1, 2, 3, 100, 150} <= set(n_poly)
        assert all(len(a[1]) == 0 and len(b[1]) == 3 and (a[0] is b[0] or np.array_equal(a[0], b[0])) for a, b in zip(c.images[::2], c.images[1::2]))
        img = rc.expected(c)
        k = {name: 2 * i for i, name in enumerate(named)}
        assert (img[k["covering the image"]] == 255).all() and (img[k["the border itself"]] == 255).all()
        assert not img[k["outside to the right"]].any() and not img[k["outside above"]].any() and not img[k["no vertex"]].any()
        assert int(img[k["one vertex"]].any(-1).sum()) == 1 and img[k["one vertex"]][H - 1 - H // 2, W // 2].all()
        pts = lambda name: np.asarray(named[name][0])
        assert np.abs(pts("far away")).max() == 20000 and (pts("outside on one side")[:, 0] < 0).sum() == 2
        assert (pts("outside on all sides").min(0) < 0).all() and (pts("outside on all sides").max(0) > (W, H)).all()
        assert np.array_equal(pts("closed ring")[0], pts("closed ring")[-1]) and (np.diff(pts("consecutive duplicates"), axis=0) == 0).all(1).sum() == 4
        e = np.diff(np.vstack([pts("staircase"), pts("staircase")[:1]]), axis=0)
        assert ((e[:, 0] == 0) | (e[:, 1] == 0)).all() and (e[:, 0] == 0).any() and (e[:, 1] == 0).any()    # horizontal and vertical edges only
        on_border = pts("vertices on the border")
        assert {0, W - 1} <= set(on_border[:, 0].tolist()) and {0, H - 1} <= set(on_border[:, 1].tolist())
        # even-odd: the pentagram's centre (winding number 2) stays empty
        assert not img[k["pentagram"]][H - 1 - H // 2, W // 2].any() and img[k["convex"]][H - 1 - H // 2, W // 2].all()


def test_reduced_and_workload_groups():
    for c in _group("reduced"):
        t = {q[5] for _, s in c.images for q in s}
        assert {1, 2, 5, 8, 18} <= t and any(p is not None and len(s) == 8 for p, s in c.images)             # a polygon under two chunks
    c = BY_ID["workload-501x501"]
    assert len(c.images) <= 6 and c.n_segments <= 40 and {17, 18, 8, 2, 1} <= {q[5] for _, s in c.images for q in s}


@pytest.mark.parametrize("mutant", list(rc.MUTANTS))
def test_every_mutant_is_caught_by_the_group_built_for_it(mutant):
    target = _group(rc.MUTANTS[mutant])
    assert [c.hw for c in target] == list(rc.SIZES)
    for c in target:
        true, wrong = rc.expected(c), rc.expected(c, mutant=mutant)
        assert wrong.shape == true.shape and wrong.dtype == true.dtype
        differing = [i for i in range(len(true)) if not np.array_equal(true[i], wrong[i])]
        print(f"{mutant!r} on {c.id}: {len(differing)} of {len(true)} images differ")
        assert differing, f"{mutant!r} passes {c.id}"
    # the oracle is itself again: what it draws now is what it drew before
    c = target[0]
    k = next(i for i, d in enumerate(c.draws) if d)
    assert np.array_equal(rc._render(c.hw, *c.images[k]), rc.expected(c)[k])
    assert lo.clip_line_fixed.__module__ == lo.__name__ and lo.fill_poly.__module__ == lo.__name__ and lo._put_point.__module__ == lo.__name__
