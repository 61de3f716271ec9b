"""The densify stage on the MI355X -- `bev_densify_kernel` behind `salve_bev_keys_from_pixels` + `salve_bev_densify`, through the C ABI --
against the oracle over the cases of tests/densify_cases.py: every shape class the configuration accepts (2 x 2 up to 2047 x 127 and
127 x 2047, with and without the triangle cache, at and around the 512 mask tasks), every mask size at its ends, the two output flags
on their own, site sets whose "empty" sites are occupied.  Every comparison is bit for bit.  Then: the single-render path over a
poisoned workspace, the batch path (n > 1) under mask sizes 1 and 17, every refusal before any launch, and the two stand-alone
utilities (`salve_remove_hallucinated`, `salve_zorder_winners`) at their edges."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import densify_cases as dc  # noqa: E402
from oracle import bev_oracle as bo  # noqa: E402
from salve_amd import _lib, status  # noqa: E402
from salve_amd.common.bevparams import BEVParams  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # no pixel: the kernels' words have a zero top byte
_RAS = {}


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _ras(H, W):
    """One rasteriser (tables, workspace) per image shape, kept for the module; the panorama side of its configuration is not used."""
    if (H, W) not in _RAS:
        _RAS[(H, W)] = BevRasteriser(DEV, pano_hw=(64, 128), bev_params=BEVParams(img_h=H - 1, img_w=W - 1, meters_per_px=1.0))
        assert _RAS[(H, W)].bev_hw == (H, W)
    return _RAS[(H, W)]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(at)} entries differ, first at {at[:4].tolist()}: got {[got[tuple(a)].tolist() for a in at[:4]]}, "
                             f"want {[want[tuple(a)].tolist() for a in at[:4]]}")


def _densify(H, W, pts, col, mask_k, out_flags, want_mask=False, poison=None, what=""):
    """keys_from_pixels + densify of one site set through the C ABI, into the middle image of three sentinel-filled ones.  Returns
    (final uint8 [H, W, 3], mask uint8 [H, W] or None, stats int32 [8])."""
    ras = _ras(H, W)
    cfg = ras.cfg
    cfg.mask_k, cfg.out_flags = mask_k, out_flags
    ws = ras._workspace(1)
    if poison is not None:
        ws.fill_(poison)
    buf = torch.full((3, H, W), SENTINEL, dtype=torch.int32, device=DEV)      # one image in front and one behind
    xy = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.int32)).to(DEV)
    rgb = torch.from_numpy(np.array(col, dtype=np.uint8)).to(DEV)              # (a copy: the case's arrays are read-only)
    mask = torch.full((1, H, W), 0xA5, dtype=torch.uint8, device=DEV) if want_mask else None
    stats = torch.full((1, 8), -7, dtype=torch.int32, device=DEV)
    status.check(DEV, f"before {what}")                                        # a clean status word before ...
    with torch.cuda.device(DEV):
        st = ras.lib.salve_bev_keys_from_pixels(ctypes.byref(cfg), _p(xy), _p(rgb), len(pts), _p(buf[1]), _p(ws), ws.numel(), ras._stream())
        assert st == _lib.SALVE_OK, (what, ras.lib.salve_last_error())
        st = ras.lib.salve_bev_densify(ctypes.byref(cfg), 1, _p(buf[1]), _p(mask), _p(stats), status.ptr(DEV), _p(ws), ws.numel(), ras._stream())
        assert st == _lib.SALVE_OK, (what, ras.lib.salve_last_error())
    torch.cuda.synchronize()
    status.check(DEV, what)                                                    # ... and after
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all()), f"{what}: wrote outside its image"
    assert not bool((buf[1] == SENTINEL).any()), f"{what}: left pixels unwritten"
    final = ras.export_u8(buf[1:2])[0].cpu().numpy()
    return final, (None if mask is None else mask[0].cpu().numpy()), stats[0].cpu().numpy()


def _check_case(c, poison=None):
    s, e = dc.case_sites(c), dc.expected(c)
    final, mask, stats = _densify(c.H, c.W, s.pts, s.col, c.mask_k, c.out_flags, c.want_mask, poison, c.id)
    _same(final, e.final, f"{c.id}: final image")
    if c.want_mask:
        _same(mask.astype(bool), e.mask, f"{c.id}: mask")
        assert set(np.unique(mask).tolist()) <= {0, 1}
    assert stats[0] == e.sites and stats[5] == 0, (c.id, stats.tolist(), e.sites)
    return final


@pytest.mark.parametrize("cid", [c.id for c in dc.cases()])
def test_densify_equals_the_oracle_bit_for_bit(cid):
    c = dc.case(cid)
    assert dc.refusal(c.H, c.W, c.mask_k, c.out_flags) is None
    _check_case(c)


@pytest.mark.parametrize("name", list(dc.SHAPE_CLASSES))
def test_a_poisoned_workspace_changes_nothing(name):
    """The workspace needs no initialisation: all ones and all zeroes in every byte of it before `keys_from_pixels`, the same images."""
    c = dc.class_case(name)
    clean = _check_case(c)
    for byte in (0xFF, 0x00):
        _same(_check_case(c, poison=byte), clean, f"{c.id} over a workspace of {byte:#04x} bytes")


_BATCH = {}


def _batch_setup():
    """The splat contract's `wide-129x257` geometry: its rasteriser, its panoramas on the device, its table of render rows."""
    if not _BATCH:
        import splat_cases as sc
        from salve_amd.rasteriser import pack_hypotheses

        c = sc.case("wide-129x257")
        ras = BevRasteriser(DEV, pano_hw=c.pano_hw, bev_params=BEVParams(*c.bev_params), crop_ratio=c.crop_ratio)
        assert ras.bev_hw == c.hw == (129, 257) and len(c.table) > 1
        d_rgb, d_depth = ras.upload_panos(c.rgb.copy(), c.depth.copy())
        rows = c.table
        hyps = pack_hypotheses([r.pano for r in rows], [r.surface for r in rows], np.stack([r.R for r in rows]), np.stack([r.t for r in rows]),
                               [r.apply_pose for r in rows])
        _BATCH.update(ras=ras, rgb=d_rgb, depth=d_depth, hyps=ras.upload_hypotheses(hyps), n=len(rows), parts=None, keys=None)
    return _BATCH


@pytest.mark.parametrize("mask_k,out_flags", [(1, 0), (1, 1), (17, 0), (17, 1)])
def test_the_batch_path_under_a_non_default_mask(mask_k, out_flags):
    """n > 1 renders in one launch -- the `rid` addressing of bitmaps, lists and images -- under mask sizes 1 and 17, with and without
    the flip: sites and colours of every row from the returned keys (tests/test_gpu_splat_contract.py proves those exact), final image
    and mask against `expected` built from them."""
    from test_gpu_rasteriser import unpack_keys

    b = _batch_setup()
    ras, n = b["ras"], b["n"]
    H, W = ras.bev_hw
    ras.cfg.mask_k, ras.cfg.out_flags = mask_k, out_flags
    try:
        ras.check("before the batch")
        bev, dbg = ras.render(b["rgb"], b["depth"], b["hyps"], n, debug=True)
        ras.check(f"batch mask_k {mask_k} out_flags {out_flags}")
    finally:
        ras.cfg.mask_k, ras.cfg.out_flags = 11, 0
    final, mask, stats = ras.export_u8(bev).cpu().numpy(), dbg.mask.cpu().numpy(), dbg.stats.cpu().numpy()
    if b["parts"] is None:       # the rows' sites and interpolants: once, they depend on neither the mask size nor the flags
        b["keys"] = dbg.keys.clone()
        b["parts"] = []
        for key_img in dbg.keys.cpu().numpy():
            occupied, rgb, _ = unpack_keys(key_img, H, W)
            pts = np.argwhere(occupied)[:, ::-1].astype(np.int64)
            b["parts"].append((pts,) + dc.parts(pts, rgb[occupied], H, W))
        assert sum(not bo._is_degenerate(p[0]) for p in b["parts"]) >= 10
    assert torch.equal(dbg.keys, b["keys"])
    for k, (pts, sparse, interp) in enumerate(b["parts"]):
        e = dc.compose(pts, sparse, interp, mask_k, out_flags)
        _same(final[k], e.final, f"row {k}: final image")
        _same(mask[k].astype(bool), e.mask, f"row {k}: mask")
        assert stats[k, 0] == e.sites and stats[k, 5] == 0, (k, stats[k].tolist(), e.sites)


_REFUSED = [(f"{H}x{W}", H, W, 11, 0, ("size", "large")) for (H, W) in dc.REFUSED_SHAPES] + \
           [(f"mask_k {k}", 33, 32, k, 0, ("mask_k",)) for k in dc.REFUSED_MASK_K] + \
           [(f"out_flags {fl}", 33, 32, 11, fl, ("out_flags",)) for fl in dc.REFUSED_OUT_FLAGS]


@pytest.mark.parametrize("what,H,W,mask_k,out_flags,words", _REFUSED, ids=[r[0] for r in _REFUSED])
def test_refusals_come_from_the_host_before_any_launch(what, H, W, mask_k, out_flags, words):
    """0 workspace bytes, the documented error code with a message from both calls, the output buffer and the status word untouched."""
    r = dc.refusal(H, W, mask_k, out_flags)
    assert r is not None and r.where == "config" and r.code == dc.ERR_BAD_ARG == -1   # SALVE_ERR_BAD_ARG
    ras = _ras(33, 32)
    ras.cfg.mask_k, ras.cfg.out_flags = 11, 0
    assert ras.lib.salve_bev_workspace_bytes(ctypes.byref(ras.cfg), 1) > 0
    cfg = type(ras.cfg).from_buffer_copy(ras.cfg)
    cfg.bev_h, cfg.bev_w, cfg.mask_k, cfg.out_flags = H, W, mask_k, out_flags
    assert ras.lib.salve_bev_workspace_bytes(ctypes.byref(cfg), 1) == 0
    out = torch.full((H * W,), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=DEV)
    xy = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=torch.int32, device=DEV)[: 2 if H < 2 else 4]
    rgb = torch.full((4, 3), 201, dtype=torch.uint8, device=DEV)
    status.check(DEV, f"before {what}")
    with torch.cuda.device(DEV):
        st = ras.lib.salve_bev_keys_from_pixels(ctypes.byref(cfg), _p(xy), _p(rgb), int(xy.shape[0]), _p(out), _p(ws), ws.numel(), ras._stream())
        msg = ras.lib.salve_last_error().decode()
        assert st == r.code and any(w in msg for w in words), (what, st, msg)
        st = ras.lib.salve_bev_densify(ctypes.byref(cfg), 1, _p(out), None, None, status.ptr(DEV), _p(ws), ws.numel(), ras._stream())
        msg = ras.lib.salve_last_error().decode()
        assert st == r.code and any(w in msg for w in words), (what, st, msg)
    torch.cuda.synchronize()
    status.check(DEV, what)
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all()), f"{what}: a refused call wrote"


# ---------------------------------------------------------------------------------------------------- the stand-alone utilities
@pytest.mark.parametrize("H,W", [(7, 5), (33, 64), (64, 33)])
def test_remove_hallucinated_for_every_kernel_size(H, W):
    """`salve_remove_hallucinated` against the oracle on images that hold wrap colours; an even K is accepted and asymmetric, exactly as
    `box_dilate` documents (window rows i - K // 2 .. i - K // 2 + K - 1)."""
    lib = _lib.load()
    rng = np.random.default_rng(H * 100 + W)
    sparse = np.zeros((H, W, 3), dtype=np.uint8)
    at = rng.random((H, W)) < 0.04
    sparse[at] = rng.integers(0, 256, size=(int(at.sum()), 3))
    wrap = rng.random((H, W)) < 0.08
    sparse[wrap] = np.array(dc.WRAP_COLOURS, dtype=np.uint8)[rng.integers(0, len(dc.WRAP_COLOURS), int(wrap.sum()))]
    sparse[H // 2, W // 2] = (3, 5, 7)
    assert (sparse.any(-1) & ~bo.nonempty_mask(sparse)).any() and bo.nonempty_mask(sparse).any()
    interp = rng.integers(1, 256, size=(H, W, 3)).astype(np.uint8)
    sp, it = torch.from_numpy(sparse).to(DEV), torch.from_numpy(interp).to(DEV)
    seen = set()
    for K in (1, 2, 3, 4, 11, 17, 2 * max(H, W) + 1):
        scratch = torch.full((H * W,), 0xA5, dtype=torch.uint8, device=DEV)
        buf = torch.full((3, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
        st = lib.salve_remove_hallucinated(_p(sp), _p(it), H, W, K, _p(scratch), _p(buf[1]), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert st == _lib.SALVE_OK, lib.salve_last_error()
        got = buf.cpu().numpy()
        assert (got[0] == 0x5A).all() and (got[2] == 0x5A).all()
        want = bo.remove_hallucinated(sparse, interp, K)
        _same(got[1], want, f"{H} x {W}, K = {K}")
        seen.add(int(want.any(-1).sum()))
    assert len(seen) >= 5 and H * W in seen      # the sizes differ, the largest passes everything


@pytest.mark.parametrize("n", [1, 256, 257, 2000])
def test_zorder_winners_at_the_edges(n):
    """`salve_zorder_winners` on a 9 x 7 image: heavy pixel collisions, z exactly on the slice planes (zmin and zmax included) and
    outside the range, x and y outside the image -- those never win, the rest as `choose_elevated` of the points inside the image."""
    lib = _lib.load()
    w, h, zmin, zmax, slices = 9, 7, -2.0, 2.0, 4
    rng = np.random.default_rng(n)
    x = rng.integers(-2, w + 2, n).astype(np.int32)
    y = rng.integers(-2, h + 2, n).astype(np.int32)
    planes = np.linspace(zmin, zmax, slices + 1)
    z = rng.uniform(zmin - 1, zmax + 1, n)
    on_plane = rng.random(n) < 0.4
    z[on_plane] = planes[rng.integers(0, slices + 1, int(on_plane.sum()))]
    if n == 1:
        x[0], y[0], z[0] = 8, 6, zmin
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    want = np.zeros(n, dtype=bool)
    want[inside] = bo.choose_elevated(x[inside], y[inside], z[inside], zmin, zmax, slices)
    if n >= 256:
        assert (~inside).any() and (z == zmax).any() and (z == zmin).any() and (z > zmax).any() and (z < zmin).any()
        assert 0 < want.sum() <= w * h < inside.sum()
    xd, yd, zd, pd = (torch.from_numpy(a).to(DEV) for a in (x, y, z, planes))
    scratch = torch.full((w * h,), -1, dtype=torch.int64, device=DEV)
    valid = torch.full((n + 2,), 0x5A, dtype=torch.uint8, device=DEV)
    st = lib.salve_zorder_winners(_p(xd), _p(yd), _p(zd), n, _p(pd), slices, w, h, _p(scratch), _p(valid[1:]), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == _lib.SALVE_OK, lib.salve_last_error()
    got = valid.cpu().numpy()
    assert got[0] == 0x5A and got[-1] == 0x5A
    _same(got[1:-1].astype(bool), want, f"n = {n}")
    assert set(np.unique(got[1:-1]).tolist()) <= {0, 1}
