"""The case set of tests/splat_cases.py on the CPU: every case lies inside `make_devcfg`'s contract, every geometry and row holds what
the module claims (the `tall` group spans from the oracle's own raster indices, rows without a point, rows with points and no site,
exact rounding ties, the window's corner, blocks whose posed box crosses a tile line), the module's numpy emulator equals the oracle
row for row, and every emulated wrong kernel (`expected(case, mutant=...)`) differs from the oracle in the cases built for it -- the
proof that the comparison of tests/test_gpu_splat_contract.py can fail.  No GPU.

One mutant needs a case with z bounds of its own: the surface filter with its bounds exchanged (`lo <= z < hi`) differs from
`lo < z <= hi` only for a point with z exactly on a bound, and z = float32(depth * 0.001f) * zdir(row) is never -1.0 or 0.5 for any
of the 65 536 depth words on any row of any geometry here (test_no_depth_word_puts_z_on_a_filter_bound).  `narrow-21x29-zcut`
therefore sets the bounds to the z of two rows of the constant-depth panorama.

Measured: the whole module takes 23 s on one CPU core (the oracle over the ten cases 6 s -- 690 renders --, the emulator without a
mistake and with the float32 cull 3 s, the fifteen mutants over their cases 9 s, the 512 x 1024 box-room scene 5 s)."""

import numpy as np
import pytest

import splat_cases as sc
from oracle import bev_oracle as bo

BY_ID = {c.id: c for c in sc.cases()}
MULTI_TILE = [cid for cid, c in BY_ID.items() if c.hw[0] > sc.TILE or c.hw[1] > sc.TILE]


def _rows(c, **want):
    return [k for k, r in enumerate(c.table) if all(getattr(r, a) == v for a, v in want.items())]


def test_the_case_list_is_what_the_module_declares():
    assert [c.id for c in sc.cases()] == [f"{p}-{b}" for p, b in sc.CASES] + [sc.Z_CUT] and len(BY_ID) == 10
    assert [c.id for c in sc.cases() if c.z_ranges is not sc.Z_RANGES] == [sc.Z_CUT] == ["narrow-21x29-zcut"]
    assert {p for p, _ in sc.CASES} == {"narrow", "wide", "tall", "tall-listed", "small"}
    for bev in ("21x29", "129x257", "128x128"):                              # each of them with at least narrow and wide
        assert {("narrow", bev), ("wide", bev)} <= set(sc.CASES)
    assert len(sc.MUTANTS) == 15 and all(set(ids) <= set(BY_ID) for ids in sc.MUTANTS.values())
    assert all(sc.MUTANTS.values()) and sc.MUTANTS["z filter lo <= z < hi"] == (sc.Z_CUT,)
    for c in sc.cases():
        assert len(c.table) == 69 and len(c.table) % 8 != 0                  # the last group of eight renders of a launch is partial
        assert len(sc.FAMILIES) == c.depth.shape[0] == c.rgb.shape[0] == 8
        assert {r.surface for r in c.table} == {0, 1} and {r.apply_pose for r in c.table} == {0, 1}
        assert {r.pano for r in c.table} == set(range(8))
        assert all(r.R.dtype == np.float32 and r.R.shape == (2, 2) and r.t.dtype == np.float32 and r.t.shape == (2,) for r in c.table)


@pytest.mark.parametrize("cid", list(BY_ID))
def test_every_case_is_inside_the_accepted_contract(cid):
    c = BY_ID[cid]
    (Hp, Wp), (H, W) = c.pano_hw, c.hw
    assert Wp > 0 and Wp % 4 == 0 and Hp > 0 and 0 <= c.crop_rows and 2 * c.crop_rows < Hp
    assert c.npts == (Hp - 2 * c.crop_rows) * Wp < 2 ** 21
    assert 2 <= H < 2048 and 2 <= W < 2048 and ((H + 15) // 16) * ((W + 31) // 32) <= 512
    assert c.depth.dtype == np.uint16 and c.depth.shape == (8, Hp, Wp) and c.rgb.dtype == np.uint8 and c.rgb.shape == (8, Hp, Wp, 3)
    assert not c.depth.flags.writeable and not c.rgb.flags.writeable
    # the oracle's grid is the rasteriser's: the same window and scale as BEVParams gives
    from salve_amd.common.bevparams import BEVParams

    bp = BEVParams(*c.bev_params)
    assert tuple(bp.xlims + bp.ylims) == c.grid.lims and float(bp.bevimg_Sim2_world.scale) == c.grid.scale
    assert (bp.img_h + 1, bp.img_w + 1) == c.hw
    exp = sc.expected(c)
    assert sc.expected(c) is exp and len(exp) == len(c.table)                # computed once, shared
    assert all(not r.img_xy.flags.writeable and not r.bev.flags.writeable for r in exp)
    for r in exp:
        assert r.img_xy.shape == (c.npts, 2) and r.img_xy.dtype == np.int16 and r.winner.shape == (H, W) and r.sparse.shape == (H, W, 3)
        assert r.mask.shape == (H, W) and r.bev.shape == (H, W, 3) and r.bev.dtype == np.uint8
        assert int((r.img_xy[:, 0] >= 0).sum()) == r.count and int((r.winner >= 0).sum()) == r.sites


def test_panorama_geometries_reach_what_they_claim():
    grid = lambda name: ((sc._rows_of(name) + 3) // 4, (sc.PANOS[name][1] + 15) // 16)
    H, W, _ = sc.PANOS["narrow"]
    assert (H, W) == (42, 20) and grid("narrow") == (8, 2) and W % 16 == 4 and sc._rows_of("narrow") == 30 and 30 % 4 == 2
    H, W, _ = sc.PANOS["wide"]
    assert (H, W) == (70, 1028) and grid("wide") == (13, 65) and (65 + 63) // 64 == 2 and 65 % 64 == 1 and sc._rows_of("wide") == 50 and 50 % 4 == 2
    assert 51000 < sc.case("wide-129x257").npts == 51400
    assert sc.PANOS["small"][:2] == (64, 128) and sc._rows_of("small") == 44
    # the `tall` geometries: the range of groups [min g, max g + 1) of the oracle's own kept raster indices
    span = {}
    for name in ("tall", "tall-listed"):
        assert sc.PANOS[name][1] == 4 and sc.PANOS[name][2] == 0.0 and grid(name)[1] == 1
        for p, fam in enumerate(sc.FAMILIES):
            for s in (0, 1):
                g = sc.group_of(name, sc.kept(name, p, s)[1])
                span[name, fam, s] = int(g.max() + 1 - g.min()) if g.size else 0
        print(name, {f: (span[name, f, 0], span[name, f, 1]) for f in sc.FAMILIES})
    for fam in ("noise", "near-noise", "far"):                               # both surfaces beyond the cap: the un-listed branch
        assert span["tall", fam, 0] > sc.GLIST_CAP and span["tall", fam, 1] > sc.GLIST_CAP
    assert span["tall-listed", "near-noise", 0] <= sc.GLIST_CAP < span["tall-listed", "near-noise", 1]
    assert span["tall-listed", "noise", 0] > sc.GLIST_CAP and span["tall-listed", "checker", 1] <= sc.GLIST_CAP
    for cid in ("tall-129x257", "tall-listed-128x128"):                      # ... and rows of the launch render those surfaces
        c = BY_ID[cid]
        kinds = {span[c.pano, sc.FAMILIES[r.pano], r.surface] > sc.GLIST_CAP for k, r in enumerate(c.table) if sc.expected(c)[k].sites > 3}
        assert kinds == {True, False}
    for name in sc.PANOS:
        if name != "box-room":
            _, depth = sc.pano_set(name)
            assert not depth[3].any() and (depth[4] == 65535).all() and (depth[5] == 1500).all() and int((depth[6] != 0).sum()) == 1
            assert set(np.unique(depth[2]).tolist()) == {800, 9000} and int(depth[0].max()) > 60000
            assert [len(sc.kept(name, 3, s)[1]) for s in (0, 1)] == [0, 0]                 # constant 0: no point passes either filter
            assert [len(sc.kept(name, 6, s)[1]) for s in (0, 1)] == [1, 0]
            rgb = sc.pano_set(name)[0].reshape(-1, 3).astype(np.uint32)
            prod = rgb[:, 0] * rgb[:, 1] * rgb[:, 2]
            assert ((prod > 0) & (prod & 255 == 0)).mean() > 0.1 and (prod == 0).mean() > 0.1   # wrapped to zero; a zero channel


def test_image_geometries_reach_what_they_claim():
    reach = {}
    for bev, (ih, iw, mpp) in sc.BEVS.items():
        g = bo.BevGrid(ih, iw, mpp)
        xmin, xmax, ymin, ymax = g.lims
        reach[bev] = ((xmax - xmin) * g.scale, (ymax - ymin) * g.scale, g.W, g.H)
    assert reach["21x29"] == (24.0, 16.0, 29, 21)        # limits truncated to 3 m and 2 m: columns 25 .. 28 and rows 17 .. 20 are unreachable
    assert reach["129x257"] == (256.0, 128.0, 257, 129)  # the window's edge lands on the one-pixel last tile column and row
    assert reach["128x128"] == (127.0, 127.0, 128, 128)  # one full tile whose last pixel is the window's edge
    assert reach["101x101"] == (100.0, 100.0, 101, 101)
    assert bo.BevGrid(*sc.BEVS["129x257"]).scale == 16.0 and bo.BevGrid(*sc.BEVS["21x29"]).scale == 4.0 and bo.BevGrid(*sc.BEVS["128x128"]).scale == 31.75
    assert MULTI_TILE == ["narrow-129x257", "wide-129x257", "tall-129x257"]


@pytest.mark.parametrize("cid", list(BY_ID))
def test_rows_hold_the_variety_they_claim(cid):
    c = BY_ID[cid]
    exp = sc.expected(c)
    H, W = c.hw
    xmin, xmax, ymin, ymax = c.grid.lims
    poses = {r.pose for r in c.table}
    assert {"identity", "rot0", "rot90", "rot180", "rot270", "generic", "reflection", "scaled 0.3", "scaled 3", "tie-even", "tie-odd", "seam",
            "corner", "outside", "far", "nan", "inf"} == poses
    for k, r in enumerate(c.table):
        if r.pose in ("rot0", "rot90", "rot180", "rot270"):
            assert set(np.abs(r.R).ravel().tolist()) == {0.0, 1.0} and abs(np.linalg.det(r.R.astype(np.float64))) == 1.0   # entries exactly 0 and +-1
        if r.pose in ("tie-even", "tie-odd", "seam", "corner", "outside"):
            assert not r.R.any() and r.apply_pose == 1
    assert np.linalg.det(next(r.R for r in c.table if r.pose == "reflection").astype(np.float64)) < -0.99
    assert abs(np.linalg.det(next(r.R for r in c.table if r.pose == "scaled 3").astype(np.float64)) - 9) < 1e-5
    assert abs(np.linalg.det(next(r.R for r in c.table if r.pose == "scaled 0.3").astype(np.float64)) - 0.09) < 1e-6
    # rows for which the oracle returns None: everything falls out, or there is no point at all
    none = [k for k in range(len(exp)) if exp[k].count == 0]
    assert set(_rows(c, pose="far") + _rows(c, pose="nan") + _rows(c, pose="inf") + _rows(c, pose="outside") + _rows(c, pano=3)) <= set(none)
    assert all(not exp[k].bev.any() and not exp[k].mask.any() and exp[k].sites == 0 and (exp[k].img_xy == -1).all() for k in none)
    assert np.isnan(c.table[_rows(c, pose="nan")[0]].t).any() and np.isinf(c.table[_rows(c, pose="inf")[0]].t).any()
    # the single pixel: one point, one site, a sparse image and no final image
    one = [k for k in _rows(c, pano=6, surface=0) if c.table[k].pose == "identity"]
    assert len(one) == 1 and exp[one[0]].count == 1 and exp[one[0]].sites == 1 and not exp[one[0]].bev.any() and exp[one[0]].winner.max() >= 0
    # the zero matrix: every point of the cloud on ONE pixel; the corner row on the inclusive window corner
    for k in [k for k, r in enumerate(c.table) if r.pose in ("tie-even", "tie-odd", "seam", "corner") and r.pano in (1, 5)]:
        assert exp[k].count == len(sc.kept(c.pano, c.table[k].pano, c.table[k].surface, c.kept_range(c.table[k].surface))[1]) > 4 and exp[k].sites == 1 and not exp[k].bev.any()
    last = (int(round((xmax - xmin) * c.grid.scale)), int(round((ymax - ymin) * c.grid.scale)))
    for k in _rows(c, pose="corner"):
        a, _ = sc.posed_cloud(c, c.table[k])
        assert (a[:, 0] == xmax).all() and (a[:, 1] == ymax).all()
        xy = exp[k].img_xy[exp[k].img_xy[:, 0] >= 0]
        assert len(xy) == exp[k].count and (xy == last).all()
    for k in _rows(c, pose="outside"):   # one float32 step (the first that is 1.5 times a float32) beyond the corner in x, on it in y
        a, _ = sc.posed_cloud(c, c.table[k])
        assert len(a) and (a[:, 0] > xmax).all() and (a[:, 0] - xmax < 1e-6 * max(1, xmax)).all() and (a[:, 1] == ymax).all()
    # rows that count points and have no site: all of them beyond the z slices
    dark = [k for k in range(len(exp)) if exp[k].count > 0 and exp[k].sites == 0]
    print(f"{cid}: {len(none)} rows without a point, {len(dark)} rows with points and no site, {sum(1 for r in exp if 0 < r.sites < 4)} with 1 to 3 sites")
    assert dark or c.pano in ("wide", "small"), cid   # (at 70 and 64 rows the 65 m cloud's rows next to the horizon stay inside the slices)
    if c.bev in sc.EXACT_SCALE:
        # exact rounding ties: the position before rounding is k + 0.5 on both axes, towards an even pixel on one and an odd one on the other
        spp = sc.single_pixel_poses(c.bev)
        for pose, want in (("tie-even", (0, 1)), ("tie-odd", (1, 0))):
            vx, vy = spp[pose][1]
            assert (int(vx - 0.5) % 2, int(vy - 0.5) % 2) == want and vx % 1 == 0.5 and vy % 1 == 0.5
            for k in _rows(c, pose=pose):
                a, _ = sc.posed_cloud(c, c.table[k])
                assert ((a[:, 0] - xmin) * c.grid.scale == vx).all() and ((a[:, 1] - ymin) * c.grid.scale == vy).all()
                xy = exp[k].img_xy[exp[k].img_xy[:, 0] >= 0]
                assert (xy == (np.round(vx), np.round(vy))).all() and np.round(vx) % 2 == 0 and np.round(vy) % 2 == 0
        if cid in MULTI_TILE:             # the tile seam: 127.5 rounds to 128, the first pixel of the next tile
            assert spp["seam"][1] == (127.5, 127.5)
            for k in _rows(c, pose="seam"):
                xy = exp[k].img_xy[exp[k].img_xy[:, 0] >= 0]
                assert len(xy) > 4 and (xy == (128, 128)).all()
    # pixels whose candidates come from two slices, and a winner that is not the last index of its pixel
    two = 0
    for k, r in enumerate(c.table):
        if exp[k].sites > 3 and r.pose not in ("tie-even", "tie-odd", "seam", "corner"):
            _, z = sc._cloud(c.pano, r.pano)
            at = np.nonzero(exp[k].img_xy[:, 0] >= 0)[0]
            sl = np.floor(z[at]) + 2
            at, sl = at[(sl >= 0) & (sl < 4)], sl[(sl >= 0) & (sl < 4)]
            cell = exp[k].img_xy[at, 1].astype(np.int64) * W + exp[k].img_xy[at, 0]
            lo, hi = np.full(H * W, 9.0), np.full(H * W, -1.0)
            np.minimum.at(lo, cell, sl); np.maximum.at(hi, cell, sl)
            last_idx = np.full(H * W, -1)
            np.maximum.at(last_idx, cell, at)
            two += int((hi > lo).sum() > 0 and (last_idx.reshape(H, W) != exp[k].winner)[exp[k].winner >= 0].any())
    assert two >= 5, f"{cid}: {two} rows with a two-slice pixel whose winner is not its last index"


@pytest.mark.parametrize("cid", MULTI_TILE + ["narrow-21x29", "wide-128x128"])
def test_posed_block_boxes_cross_tile_lines_and_the_window(cid):
    """Blocks whose posed box (centre + |R| half-extents, as the cull forms it) meets two or more tiles, or lies partly outside the window:
    where a cull that is too tight loses points.  Counted over the noise and checker rows; the box room's share is printed next to it by
    the mutant test."""
    c = BY_ID[cid]
    rects = sc.tile_rects(c, np.float32(0)).reshape(-1, 4)
    xmin, xmax, ymin, ymax = c.grid.lims
    crossing = straddling = total = 0
    for r in c.table:
        if r.pano in (0, 1, 2) and r.pose in ("identity", "rot90", "generic", "reflection", "scaled 3"):
            box = sc.block_boxes(c.pano, r.pano, r.surface, c.kept_range(r.surface))[0]
            box = box[box[:, 0] <= box[:, 2]].astype(np.float64)
            R = r.R.astype(np.float64) if r.apply_pose else np.eye(2)
            t = (r.t * np.float32(1.5)).astype(np.float64) if r.apply_pose else np.zeros(2)
            ctr, half = 0.5 * (box[:, :2] + box[:, 2:]), 0.5 * (box[:, 2:] - box[:, :2])
            p, q = ctr @ R.T + t, half @ np.abs(R).T
            meets = [(p[:, 0] + q[:, 0] >= w[0]) & (p[:, 0] - q[:, 0] <= w[1]) & (p[:, 1] + q[:, 1] >= w[2]) & (p[:, 1] - q[:, 1] <= w[3]) for w in rects]
            crossing += int((np.sum(meets, 0) >= 2).sum())
            inside = (p[:, 0] - q[:, 0] >= xmin) & (p[:, 0] + q[:, 0] <= xmax) & (p[:, 1] - q[:, 1] >= ymin) & (p[:, 1] + q[:, 1] <= ymax)
            straddling += int((np.any(meets, 0) & ~inside).sum())
            total += len(box)
    print(f"{cid}: of {total} posed block boxes {crossing} meet two or more tiles, {straddling} lie partly outside the window")
    assert straddling > 20 and (crossing > 20 or cid not in MULTI_TILE)


def test_no_depth_word_puts_z_on_a_filter_bound():
    """Why the mutant "z filter lo <= z < hi" needs a case with bounds of its own (`z_cut_ranges`): on a row, z = float32(dep * 0.001f) * zdir is monotone in the depth word, so the
    only words that could give z == -1.0 or z == 0.5 exactly are next to where z crosses the bound -- and none of them does, on any row
    of any geometry of the case set."""
    d32 = np.arange(65536, dtype=np.float32) * np.float32(0.001)
    assert (np.diff(d32) >= 0).all()
    d = d32.astype(np.float64)
    hits = tested = 0
    for name, (H, W, _) in sc.PANOS.items():
        crop = sc._crop_rows(name)
        for zv in bo.sphere_table(H, 1)[crop:H - crop, 0, 2]:
            for bound in (-1.0, 0.5):
                if bound / zv > 0:
                    i = int(np.searchsorted(d, bound / zv))
                    near = d[max(i - 3, 0):i + 4]
                    hits += int((near * zv == bound).sum())
                    tested += 1
    print(f"{tested} (row, bound) crossings tested: {hits} depth words give z on a bound")
    assert tested > 15000 and hits == 0
    for cid in ("narrow-21x29", "narrow-129x257", "small-101x101"):   # ... so with the default bounds the emulated mutant renders what the oracle renders
        c = BY_ID[cid]
        assert all(not sc.differing(a, b) for a, b in zip(sc.expected(c), sc.expected(c, mutant="z filter lo <= z < hi")))


def test_the_z_cut_case_puts_both_bounds_on_points():
    c = BY_ID[sc.Z_CUT]
    (flo, fhi), (clo, chi) = c.z_ranges
    assert flo == -np.inf and chi == np.inf and -1.3 < fhi < -1.0 and 0.5 < clo < 0.8
    flat = sc.FAMILIES.index("flat")
    z = sc._cloud(c.pano, flat)[1]
    on_floor, on_ceiling = np.nonzero(z == fhi)[0], np.nonzero(z == clo)[0]
    assert len(on_floor) == len(on_ceiling) == c.pano_hw[1]                       # one whole row of the flat panorama on each bound
    assert set(on_floor) <= set(sc.kept(c.pano, flat, 0, c.z_ranges[0])[1])       # z <= hi: kept
    assert not set(on_ceiling) & set(sc.kept(c.pano, flat, 1, c.z_ranges[1])[1])  # lo < z: dropped
    assert len(sc.kept(c.pano, flat, 0, c.z_ranges[0])[1]) == len(sc.kept(c.pano, flat, 0)[1])          # the floor rows the default keeps
    assert len(sc.kept(c.pano, flat, 1, c.z_ranges[1])[1]) == len(sc.kept(c.pano, flat, 1)[1]) - c.pano_hw[1]
    seen = [k for k, r in enumerate(c.table) if r.pano == flat and sc.expected(c)[k].count > 0]
    assert {c.table[k].surface for k in seen} == {0, 1}                           # rows of the launch render both


@pytest.mark.parametrize("cid", list(BY_ID))
def test_the_emulator_without_a_mistake_equals_the_oracle(cid):
    """The mutants are one-line changes of `splat_cases._emulate_row`; without one it reproduces the oracle in every compared quantity."""
    c = BY_ID[cid]
    for k, (a, b) in enumerate(zip(sc.expected(c), sc.expected(c, mutant="none"))):
        assert not sc.differing(a, b), (cid, k, c.table[k].pose, sc.differing(a, b))


@pytest.mark.parametrize("cid", ["narrow-21x29", "narrow-129x257", "wide-129x257", "tall-129x257", "tall-listed-128x128"])
def test_the_kernels_cull_emulated_in_float32_loses_no_point(cid):
    """`splat_reaches` on group and block boxes with the kernel's margin and slack, in numpy float32 (not the device's instruction
    sequence: a plausibility check of the constants, the GPU test is the proof): no point of any row is lost."""
    c = BY_ID[cid]
    for k, (a, b) in enumerate(zip(sc.expected(c), sc.expected(c, mutant="emulated cull"))):
        assert not sc.differing(a, b), (cid, k, c.table[k].pose, sc.differing(a, b))


@pytest.mark.parametrize("mutant", list(sc.MUTANTS))
def test_every_mutant_is_caught_in_the_cases_built_for_it(mutant):
    for cid in sc.MUTANTS[mutant]:
        c = BY_ID[cid]
        true, wrong = sc.expected(c), sc.expected(c, mutant=mutant)
        rows = [k for k in range(len(true)) if sc.differing(true[k], wrong[k])]
        what = sorted({q for k in rows for q in sc.differing(true[k], wrong[k])}, key=sc.QUANTITIES.index)
        print(f"{mutant!r} on {cid}: {len(rows)} of {len(true)} rows differ, in {what}")
        assert rows, f"{mutant!r} passes {cid}"


def test_cull_mutants_on_the_box_room_next_to_noise_and_checker():
    """How weak the older tests are against cull errors (reported, not bounded): the points the two cull mutants lose on the 512 x 1024
    box-room scene of tests/test_gpu_rasteriser.py's fixture, next to the noise and checker rows of `wide-129x257`."""
    box = sc.box_room_case()
    assert box.pano_hw == (512, 1024) and box.hw == (501, 501) and len(box.table) == 4
    wide = BY_ID["wide-129x257"]
    for mutant in ("centre-only cull", "cull ignores the rotation"):
        for name, c, pick in (("box room", box, lambda r: True), ("noise", wide, lambda r: r.pano in (0, 1)), ("checker", wide, lambda r: r.pano == 2)):
            true, wrong = sc.expected(c), sc.expected(c, mutant=mutant)
            ks = [k for k, r in enumerate(c.table) if pick(r)]
            total, lost = sum(true[k].count for k in ks), sum(true[k].count - wrong[k].count for k in ks)
            rows = sum(1 for k in ks if sc.differing(true[k], wrong[k]))
            print(f"{mutant!r}, {name}: {lost} of {total} in-window points lost ({100 * lost / max(total, 1):.2f} %), {rows} of {len(ks)} rows differ")
    lost = [a.count - b.count for a, b in zip(sc.expected(box), sc.expected(box, mutant="emulated cull"))]
    assert not any(lost)
