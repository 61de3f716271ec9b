"""tests/densify_cases.py against the oracle, on the host: the acceptance rule names every listed shape as listed, the site families do
what they were built for (wrap sites that are zeroed, gaps that just close and just stay open for every mask size, degenerate sets),
`expected` composes in the oracle's order, and the numpy restatement of the kernel's mask pass equals the oracle without a mistake and
differs from it with each of three."""

import numpy as np
import pytest

import densify_cases as dc
from oracle import bev_oracle as bo


def test_the_acceptance_rule_classifies_every_named_shape():
    for H, W in dc.SHAPES:
        assert dc.refusal(H, W) is None, (H, W)
        for k in range(1, 18, 2):
            for fl in range(8):
                assert dc.refusal(H, W, k, fl) is None
    for (H, W), why in dc.REFUSED_SHAPES.items():
        r = dc.refusal(H, W)
        assert r is not None and r.code == dc.ERR_BAD_ARG and r.where == "config", (H, W, why)
    assert [dc.mask_tasks(H, W) for H, W in ((512, 512), (1024, 256), (2047, 127), (127, 2047), (513, 512), (1025, 255))] == [512, 512, 512, 512, 528, 520]
    for k in dc.REFUSED_MASK_K + (-1, 18, 21):
        assert dc.refusal(33, 32, k, 0).code == dc.ERR_BAD_ARG
    for fl in dc.REFUSED_OUT_FLAGS + (16, 256, 512, -1):
        assert dc.refusal(33, 32, 11, fl).code == dc.ERR_BAD_ARG
    # the LDS bound excludes nothing the task bound lets through: no named shape moves to the refused list on its account
    assert max(dc.lds_bytes(H, W) for H, W in dc.SHAPES) <= dc.max_lds_bytes_within_the_task_bound() == 86088 < dc.LDS_LIMIT
    assert {(H, W) for H, W in dc.SHAPES if max(H, W) > dc.TRI_CACHE_MAX_DIM} == {(1025, 40), (40, 1025), (2047, 127), (127, 2047)}
    assert set(dc.SWEEP_SHAPES) <= set(dc.SHAPES) and set(dc.SHAPE_CLASSES.values()) <= set(dc.SHAPES)


def test_the_table_covers_what_it_names():
    table = dc.cases()
    assert {(c.H, c.W) for c in table if (c.mask_k, c.out_flags) == (11, 0)} == set(dc.SHAPES)
    assert {c.family for c in table if (c.mask_k, c.out_flags) == (11, 0)} >= set(dc.FAMILIES)
    for H, W in dc.SWEEP_SHAPES:
        for f in ("gap", "wrap"):
            assert {(c.mask_k, c.out_flags) for c in table if (c.H, c.W, c.family) == (H, W, f) and c.want_mask} == \
                {(k, fl) for k in dc.SWEEP_MASK_K for fl in dc.SWEEP_OUT_FLAGS}
        for f in dc.DEGENERATE:
            assert {c.out_flags for c in table if (c.H, c.W, c.family) == (H, W, f)} == {0, 3}
    assert all(dc.refusal(c.H, c.W, c.mask_k, c.out_flags) is None for c in table)
    for name in dc.SHAPE_CLASSES:
        assert not dc.expected(dc.class_case(name)).degenerate


def test_no_case_exceeds_its_site_budget():
    for c in dc.cases():
        s = dc.case_sites(c)
        assert len(s.pts) <= dc.SITE_BUDGET, (c.id, len(s.pts))
        assert len(np.unique(s.pts, axis=0)) == len(s.pts) == len(s.col)
        if c.family not in dc.DEGENERATE and min(c.H, c.W) >= 17:
            assert not bo._is_degenerate(s.pts), c.id


@pytest.mark.parametrize("H,W", dc.SWEEP_SHAPES + ((64, 65), (127, 2047)))
def test_the_wrap_set_holds_occupied_pixels_that_are_zeroed(H, W):
    for k in dc.SWEEP_MASK_K + (11,):
        s = dc.sites("wrap", H, W, k)
        e = dc.compose(s.pts, *dc.parts(s.pts, s.col, H, W), k, 1)
        occ = np.zeros((H, W), dtype=bool)
        occ[s.pts[:, 1], s.pts[:, 0]] = True
        ne = bo.nonempty_mask(e.sparse)
        assert 1 <= ne.sum() <= 2 and (occ & ~ne).sum() >= 20          # lone non-empty sites among sites that are empty to the mask
        zeroed = occ & ~e.mask & e.sparse.any(-1)
        assert zeroed.any() and not e.final[zeroed].any(), (H, W, k)      # occupied, coloured, outside the mask: zero in the result
        kept = occ & e.mask & ~ne
        assert np.array_equal(e.final[kept], e.sparse[kept])              # and inside it the wrap sites keep their colours
        if k > 1:
            assert kept.any()
        # the distances p - 1, p, p + 1 from a non-empty site, along both axes
        p = k // 2
        y0, x0 = np.argwhere(ne)[0]
        for d in (p - 1, p, p + 1):
            for x, y in ((x0 - d, y0), (x0, y0 + d), (x0 - d, y0 + d)):
                if d >= 1 and 0 <= x < W and 0 <= y < H:
                    assert occ[y, x] and e.mask[y, x] == (d <= p) and bool(e.final[y, x].any()) == (d <= p and bool(e.sparse[y, x].any()))


@pytest.mark.parametrize("H,W", dc.SWEEP_SHAPES)
def test_for_every_mask_size_one_gap_closes_and_one_does_not(H, W):
    for k in range(1, 18, 2):
        s = dc.sites("gap", H, W, k)
        e = dc.compose(s.pts, *dc.parts(s.pts, s.col, H, W), k, 1)
        assert bo.nonempty_mask(e.sparse).sum() == len(s.pts)               # every gap site is non-empty
        closed = []
        for g in s.gaps:
            b = g.between
            shut = bool(e.mask[b[:, 1], b[:, 0]].all())
            assert shut == (g.w <= k), (H, W, k, g.axis, g.w)                    # the pairs are isolated: a gap closes iff w <= mask_k
            if len(b):
                assert e.interp[b[:, 1], b[:, 0]].all()                          # the interpolant is there to be masked
                assert np.array_equal(e.final[b[:, 1], b[:, 0]].any(-1), e.mask[b[:, 1], b[:, 0]])
            closed.append(shut)
        assert any(closed) and not all(closed), (H, W, k)
        assert {g.w for g in s.gaps} >= {k, k + 1}
    # at the tall sweep shapes both directions hold a closing and an open pair, across a word and across a task boundary
    if H >= 300:
        for k in dc.SWEEP_MASK_K:
            gaps = dc.sites("gap", H, W, k).gaps
            assert {(g.axis, g.w) for g in gaps} >= {("x", k), ("x", k + 1), ("y", k), ("y", k + 1)}, (H, W, k)
            for axis, at, bounds in (("x", 0, (32,)), ("y", 1, (16, 32))):   # (facing sites: one pixel outside `between` on either end)
                spans = [(g.between[:, at].min() - 1, g.between[:, at].max() + 1) for g in gaps if g.axis == axis and g.w == k + 1]
                if axis == "x" and W < 48 and k > 9:
                    continue        # 40 columns: a pair 16 or 18 apart cannot end its mask on column 32 (300 x 48 holds those)
                assert any(lo < B <= hi for lo, hi in spans for B in bounds), (H, W, k, axis, spans)


def test_degenerate_sets_give_all_zero_images_under_every_flag():
    for H, W in dc.SWEEP_SHAPES:
        for f in dc.DEGENERATE:
            s = dc.sites(f, H, W)
            assert bo._is_degenerate(s.pts) and (f == "empty") == (len(s.pts) == 0)
            sparse, interp = dc.parts(s.pts, s.col, H, W)
            for fl in range(4):
                e = dc.compose(s.pts, sparse, interp, 11, fl)
                assert e.degenerate and not e.final.any() and e.sites == len(s.pts)
                assert e.mask.any() == (len(s.pts) > 0)
    assert [len(dc.sites(f, 33, 32).pts) for f in ("three", "four-in-row", "empty")] == [3, 4, 0]


def test_expected_composes_in_the_oracle_s_order():
    """mask_k = 11, out_flags = 0 on a small cloud: `render_bev_image`'s own sparse image, interpolant, mask and final image."""
    grid = bo.BevGrid(28, 36, 0.25)
    rng = np.random.default_rng(5)
    n = 400
    xyz = np.stack([rng.uniform(-5, 5, n), rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n)], 1)
    rgb = rng.integers(0, 256, size=(n, 3)) / 255.0
    rgb[::7] = np.array([16, 16, 1]) / 255.0      # wrap colours among them
    res = bo.render_bev_image(np.concatenate([xyz, rgb], 1), grid, mode="exact")
    pts = res["img_xy"][res["valid"]]
    col = res["sparse"][pts[:, 1], pts[:, 0]]
    assert len(pts) > 50 and not bo._is_degenerate(pts)
    e = dc.compose(pts, *dc.parts(pts, col, grid.H, grid.W), 11, 0)
    for got, want in ((e.sparse, res["sparse"]), (e.interp, res["interp"]), (e.mask, res["mask"]), (e.final, res["bev"])):
        assert np.array_equal(got, want)
    assert (res["sparse"].any(-1) & ~bo.nonempty_mask(res["sparse"])).any() and e.final.any() and not e.mask.all()
    # and the two flags do what they say
    assert np.array_equal(dc.compose(pts, e.sparse, e.interp, 11, 1).final, e.final[::-1])
    assert np.array_equal(dc.compose(pts, e.sparse, e.interp, 11, 3).final, res["interp"])
    assert np.array_equal(dc.compose(pts, e.sparse, e.interp, 11, 2).final, res["interp"][::-1])


def test_the_emulated_mask_pass_is_the_oracle_and_every_mutant_is_caught():
    """The kernel's word-and-task mask pass in numpy equals the oracle on every case; each one-line mistake changes some case's image."""
    caught = {m: [] for m in dc.MUTANTS}
    for c in dc.cases():
        e = dc.expected(c)
        mask, final = dc.emulate(c)
        assert np.array_equal(mask, e.mask) and np.array_equal(final, e.final), c.id
        for m in dc.MUTANTS:
            mm, mf = dc.emulate(c, m)
            if not np.array_equal(mf, e.final) or (c.want_mask and not np.array_equal(mm, e.mask)):
                caught[m].append(c.id)
    for m, ids in caught.items():
        print(f"{m}: caught by {len(ids)} cases, e.g. {ids[:6]}")
        assert ids, m
    for k in dc.SWEEP_MASK_K:   # every mask size of the sweep catches both mask mistakes at a tall sweep shape, through the FINAL image
        for m in dc.MUTANTS[:2]:
            if k == 1 and m == dc.MUTANTS[0]:
                continue            # p = 0: the horizontal dilation has no step to get wrong
            hit =[c.id for c in dc.cases() if c.mask_k == k and c.family == "gap" and c.out_flags == 0 and c.H >= 300
                   and not np.array_equal(dc.emulate(c, m)[1], dc.expected(c).final)]
            assert hit, (k, m)
    assert any("wrap" in i for i in caught[dc.MUTANTS[2]])
