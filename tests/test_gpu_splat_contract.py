"""The front end of the BEV rasteriser on the MI355X -- `bev_pano_index_kernel` with its update and group variants, `bev_splat_kernel`,
`emit_tile` -- against the oracle over the cases of tests/splat_cases.py: every case is ONE `render(debug=True)` launch plus one
`scatter` + `densify` into a sentinel-filled buffer, compared bit for bit and row by row (in-window counts, pixel indices, z-order
winners, sparse image, mask, final image, site counts, a clean status word).  Then: the index of an all-zero panorama, index updates
against fresh builds at the odd geometries, the explicit-cloud path against the splat, a bad row in the middle of a launch."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import splat_cases as sc  # noqa: E402
from salve_amd import _lib, status  # noqa: E402
from salve_amd.common.bevparams import BEVParams  # noqa: E402
from salve_amd.rasteriser import BevRasteriser, pack_hypotheses  # noqa: E402
from test_gpu_rasteriser import unpack_keys  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # no pixel: the kernels' words have a zero top byte
_RAS = {}


def _ras(c):
    """One rasteriser and one uploaded panorama stack per geometry, kept for the module."""
    if c.id not in _RAS:
        ras = BevRasteriser(DEV, pano_hw=c.pano_hw, bev_params=BEVParams(*c.bev_params), crop_ratio=c.crop_ratio)
        assert ras.npts == c.npts and ras.bev_hw == c.hw and ras.cfg.crop_rows == c.crop_rows
        assert tuple((ras.cfg.z_lo[s], ras.cfg.z_hi[s]) for s in (0, 1)) == sc.Z_RANGES
        for s, (lo, hi) in enumerate(c.z_ranges):   # (the z-cut case: bounds that lie on points; set before the index is first built)
            ras.cfg.z_lo[s], ras.cfg.z_hi[s] = lo, hi
        _RAS[c.id] = (ras,) + ras.upload_panos(c.rgb.copy(), c.depth.copy())   # (the case's arrays are read-only)
    return _RAS[c.id]


def _pack(rows):
    return pack_hypotheses([r.pano for r in rows], [r.surface for r in rows], np.stack([r.R for r in rows]), np.stack([r.t for r in rows]),
                           [r.apply_pose for r in rows])


def _same(got, want, what):
    if not np.array_equal(got, want):
        at = np.argwhere(np.asarray(got) != np.asarray(want))
        raise AssertionError(f"{what}: {len(at)} entries differ, first at {at[:4].tolist()}: got {[np.asarray(got)[tuple(a)].tolist() for a in at[:4]]}, "
                             f"want {[np.asarray(want)[tuple(a)].tolist() for a in at[:4]]}")


@pytest.mark.parametrize("cid", [c.id for c in sc.cases()])
def test_splat_equals_oracle_bit_for_bit(cid):
    c = sc.case(cid)
    exp = sc.expected(c)
    ras, d_rgb, d_depth = _ras(c)
    ras.check(f"before {cid}")
    H, W = c.hw
    n = len(c.table)
    hd = ras.upload_hypotheses(_pack(c.table))
    bev, dbg = ras.render(d_rgb, d_depth, hd, n, debug=True)
    buf = torch.full((n + 2, H, W), SENTINEL, dtype=torch.int32, device=DEV)   # one image in front and one behind
    counts = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ras.scatter(d_rgb, d_depth, hd, n, buf[1:], in_window=counts)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "scatter wrote outside its images"
    assert not bool((buf[1:-1] == SENTINEL).any()), "scatter left pixels unwritten"
    sparse = ras.export_u8(buf[1:-1].contiguous()).cpu().numpy()
    ras.densify(n, buf[1:])
    ras.check(cid)                                                              # a clean status word
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "densify wrote outside its images"
    final = ras.export_u8(bev).cpu().numpy()
    assert torch.equal(buf[1:-1], bev), "scatter + densify and render disagree"
    counts, dbg_counts = counts.cpu().numpy(), dbg.in_window.cpu().numpy()
    img_xy, keys, mask, stats = dbg.img_xy.cpu().numpy(), dbg.keys.cpu().numpy(), dbg.mask.cpu().numpy(), dbg.stats.cpu().numpy()
    _same(counts, [e.count for e in exp], f"{cid}: in-window counts")
    _same(dbg_counts, counts, f"{cid}: in-window counts of render")
    for k, (row, e) in enumerate(zip(c.table, exp)):
        what = f"{cid} row {k} ({sc.FAMILIES[row.pano]}, {sc.SURFACES[row.surface]}, {row.pose})"
        _same(img_xy[k], e.img_xy, what + ": pixel indices")
        occupied, rgb, point = unpack_keys(keys[k], H, W)
        _same(occupied, e.winner >= 0, what + ": occupancy")
        _same(np.where(occupied, point, -1), e.winner, what + ": z-order winners")
        _same(np.where(occupied[..., None], rgb, 0), e.sparse, what + ": sparse image of the keys")
        _same(sparse[k], e.sparse[::-1], what + ": sparse image after scatter")
        _same(mask[k].astype(bool), e.mask, what + ": mask")
        _same(final[k], e.bev, what + ": final image")
        assert stats[k, 0] == e.sites and stats[k, 5] == 0, (what, stats[k].tolist(), e.sites)


@pytest.mark.parametrize("cid", ["narrow-21x29", "wide-129x257", "tall-129x257"])
def test_an_all_zero_panorama_has_an_empty_group_range(cid):
    """Constant depth 0: no point passes either z filter, the range words of both surfaces stay empty (g_hi - g_lo == 0) and the splat
    visits nothing -- seen through the images and counts alone, under poses that would bring any point into the window."""
    c = sc.case(cid)
    ras, d_rgb, d_depth = _ras(c)
    zero = sc.FAMILIES.index("zero")
    rows = [sc.Row(zero, s, r.R, r.t, r.apply_pose, r.pose) for r in c.table if r.pose in ("identity", "generic", "scaled 0.3", "corner") and r.pano == 1
            for s in (0, 1)]
    assert len(rows) >= 6
    H, W = c.hw
    buf = torch.full((len(rows), H, W), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((len(rows),), -7, dtype=torch.int32, device=DEV)
    ras.scatter(d_rgb, d_depth, ras.upload_hypotheses(_pack(rows)), len(rows), buf, in_window=counts)
    assert not bool(buf.any()) and not bool(counts.any())
    ras.densify(len(rows), buf)
    ras.check(cid)
    assert not bool(buf.any())


def _build(ras, depth_dev):
    P = int(depth_dev.shape[0])
    buf = torch.empty(ras.pano_index_bytes(P), dtype=torch.uint8, device=DEV)
    st = ras.lib.salve_bev_pano_index_build(ctypes.byref(ras.cfg), ctypes.c_void_p(depth_dev.data_ptr()), P, ctypes.c_void_p(ras.sphere.data_ptr()),
                                            ctypes.c_void_p(buf.data_ptr()), buf.numel(), ras._stream())
    assert st == _lib.SALVE_OK, ras.lib.salve_last_error()
    return buf


def _update(ras, depth_dev, index, slots):
    slots_dev = torch.tensor(slots, dtype=torch.int32, device=DEV)
    st = ras.lib.salve_bev_pano_index_update(ctypes.byref(ras.cfg), ctypes.c_void_p(depth_dev.data_ptr()), int(depth_dev.shape[0]),
                                             ctypes.c_void_p(ras.sphere.data_ptr()), ctypes.c_void_p(index.data_ptr()), index.numel(),
                                             ctypes.c_void_p(slots_dev.data_ptr()), len(slots), status.ptr(DEV), ras._stream())
    assert st == _lib.SALVE_OK, ras.lib.salve_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("cid", ["narrow-21x29", "wide-129x257", "tall-129x257"])
def test_index_update_of_every_slot_equals_a_fresh_build(cid):
    """The partial block column and row, the one-block second group and 2200 groups of one block: the updated index -- block boxes,
    range words and group boxes of both surfaces -- is a fresh build's byte for byte, slot by slot and for all slots at once."""
    c = sc.case(cid)
    ras, _, d_depth = _ras(c)
    P = int(d_depth.shape[0])
    old = d_depth.clone()
    new = old.roll(3, 0).contiguous()            # every slot gets another family's depth map: empty ranges become full ones and back
    first = _build(ras, old)
    target = _build(ras, new)
    assert not torch.equal(first, target)
    work, index = old.clone(), first.clone()
    for s in range(P):                           # slot by slot: after each step a fresh build of the mixed stack
        work[s] = new[s]
        _update(ras, work, index, [s])
        assert torch.equal(index, _build(ras, work)), f"{cid}: slot {s}"
    assert torch.equal(index, target)
    _update(ras, old, index, list(range(P))[::-1])   # all slots in one call, back to the first stack
    assert torch.equal(index, first)
    ras.check(cid)


@pytest.mark.parametrize("cid", [c.id for c in sc.cases()])
def test_explicit_cloud_path_equals_the_splat_path(cid):
    """`render_points` of the oracle's posed cloud (bev_scatter_points_kernel -> bev_emit_keys_kernel -> densify) against the splat's final
    image of the same row, for a noise row and a checker (or room) row of every geometry."""
    c = sc.case(cid)
    exp = sc.expected(c)
    ras, d_rgb, d_depth = _ras(c)
    picks = [next(k for k, r in enumerate(c.table) if r.pano == 1 and r.pose == "generic"),
             next(k for k, r in enumerate(c.table) if r.pano in (2, 7) and r.apply_pose and exp[k].sites > 3)]   # the first posed checker (or room) row that densifies
    rows = [c.table[k] for k in picks]
    bev, _ = ras.render(d_rgb, d_depth, ras.upload_hypotheses(_pack(rows)), len(rows))
    splat = ras.export_u8(bev).cpu().numpy()
    for j, (k, row) in enumerate(zip(picks, rows)):
        a, idx = sc.posed_cloud(c, row)
        colours = c.rgb[row.pano][c.crop_rows:c.pano_hw[0] - c.crop_rows].reshape(-1, 3)[idx]
        got, n_in = ras.render_points(a[:, :3], colours)
        assert n_in == exp[k].count > 0 and exp[k].sites > 3
        got = ras.export_u8(got).cpu().numpy()[0]
        _same(got, splat[j], f"{cid} row {k}: explicit cloud against the splat")
        _same(got, exp[k].bev, f"{cid} row {k}: explicit cloud against the oracle")
    ras.check(cid)


@pytest.mark.parametrize("cid", ["narrow-129x257", "wide-21x29", "tall-listed-128x128"])
def test_a_bad_row_in_the_middle_of_a_launch(cid):
    """pano_idx = P and surface = 2 in one row between good ones: an empty image, count 0, SALVE_STATUS_BAD_HYPOTHESIS, and the rows on
    either side exact."""
    c = sc.case(cid)
    exp = sc.expected(c)
    ras, d_rgb, d_depth = _ras(c)
    ras.check("before the bad row")
    picks = [k for k, r in enumerate(c.table) if r.pano in (0, 1, 2) and r.pose in ("identity", "rot180", "generic", "scaled 3")][:10]
    assert len(picks) == 10
    h = _pack([c.table[k] for k in picks])
    bad = h[:1].copy()
    bad["pano_idx"], bad["surface"] = int(d_rgb.shape[0]), 2
    h = np.concatenate([h[:5], bad, h[5:]])
    n = len(h)
    H, W = c.hw
    buf = torch.full((n, H, W), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ras.scatter(d_rgb, d_depth, ras.upload_hypotheses(h), n, buf, in_window=counts)
    ras.densify(n, buf)
    torch.cuda.synchronize()
    with pytest.raises(_lib.SalveHipError, match="panorama outside"):
        ras.check(cid)
    ras.check("after the bad row")   # the word was reset
    got, counts = ras.export_u8(buf).cpu().numpy(), counts.cpu().numpy()
    assert not got[5].any() and counts[5] == 0
    for j, k in enumerate(picks):
        at = j if j < 5 else j + 1
        assert counts[at] == exp[k].count, (cid, k)
        _same(got[at], exp[k].bev, f"{cid} row {k} next to the bad row")
    assert sum(exp[k].sites > 3 for k in picks) >= 5
