"""The tile and resize kernels on the MI355X -- `bev_tile_kernel` in its three formats, `bev_tile_aug_kernel`, `bev_tile_pair_kernel` plain and
pretiled, `bev_train_tile_kernel<8|16|24, fp32|bf16>`, phase H of `bev_densify_kernel`, `resize_rgb_kernel`, `bev_export_kernel` -- against the
emulator of tests/tile_cases.py over its case tables, through the C ABI.  Every comparison is on bits; every output buffer starts as the
sentinel (`tile_cases.blank`: NaN / 0x5A bytes) with samples no job names, and what the contract does not name must still hold it afterwards.
Then the refusals the header lists (documented code, output untouched) and the train entry's device-side job check.  The entries that do not
check their device-side tables are only ever given tables inside their arrays."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import tile_cases as tc  # noqa: E402
from salve_amd import _lib, status, synthetic  # noqa: E402
from salve_amd.common.bevparams import BEVParams  # noqa: E402
from salve_amd.rasteriser import BevRasteriser, linear_resize_taps, pack_hypotheses  # noqa: E402

DEV = torch.device("cuda:0")
_RAS = {}
P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())


def _ras(geo, kind="imagenet"):
    """One rasteriser per geometry and table, kept for the module: the library's own taps for (resize, h) and (resize, w)."""
    key = (geo, kind)
    if key not in _RAS:
        ras = BevRasteriser(DEV, bev_params=BEVParams(geo.h - 1, geo.w - 1, 1.0), resize=geo.resize, crop=geo.crop)
        assert ras.bev_hw == (geo.h, geo.w)
        if kind != "imagenet":
            ras.lut = _dev(tc.lut(kind))
        _RAS[key] = ras
    return _RAS[key]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if not tc.same(got, want):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        g, w = tc.bits(got), tc.bits(want)
        at = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(at)} of {g.size} elements differ, first at {at[:4].tolist()}: got {[hex(int(g[tuple(a)])) for a in at[:4]]}, "
                             f"want {[hex(int(w[tuple(a)])) for a in at[:4]]}")


def _aug(draws):
    a = np.zeros(len(draws), dtype=_lib.TILE_AUG_DTYPE)
    for k, (cy, cx, flags) in enumerate(draws):
        a[k] = (cy, cx, flags, 0)
    return torch.from_numpy(a.view(np.uint8)).to(DEV)


def _ok(st, ras):
    assert st == _lib.SALVE_OK, ras.lib.salve_last_error()


def _tiles(ras, bev, jobs, n, out, fmt, out_c, **kw):
    g = dict(resize=ras.resize, crop=ras.crop, lut=ras.lut)
    g.update(kw)
    return ras.lib.salve_bev_tiles(P(bev), *ras.bev_hw, P(jobs), n, P(ras.coef_y), P(ras.coef_x), g["resize"], g["crop"], P(g["lut"]), P(out), fmt, out_c, ras._stream())


def _tiles_aug(ras, bev, jobs, aug, n, out, out_c, **kw):
    g = dict(resize=ras.resize, crop=ras.crop)
    g.update(kw)
    return ras.lib.salve_bev_tiles_aug(P(bev), *ras.bev_hw, P(jobs), P(aug), n, P(ras.coef_y), P(ras.coef_x), g["resize"], g["crop"], P(ras.lut), P(out), out_c, ras._stream())


def _pairs(ras, bev_a, bev_b, ja, jb, n, out, out_c, pretiled, **kw):
    g = dict(resize=ras.resize, crop=ras.crop)
    g.update(kw)
    return ras.lib.salve_bev_tile_pairs(P(bev_a), P(bev_b), *ras.bev_hw, P(ja), P(jb), n, P(ras.coef_y), P(ras.coef_x), g["resize"], g["crop"], P(ras.lut), P(out), out_c,
                                        1 if pretiled else 0, ras._stream())


def _train(ras, bev_a, bev_b, ja, jb, per_sample, aug, batch, out, fmt, out_c, **kw):
    g = dict(resize=ras.resize, crop=ras.crop, out=out if isinstance(out, ctypes.c_void_p) else P(out))   # (a raw pointer: the misaligned one)
    g.update(kw)
    hw = ras.bev_hw[0] * ras.bev_hw[1]
    return ras.lib.salve_bev_train_tiles(P(bev_a), bev_a.numel() // hw, P(bev_b), bev_b.numel() // hw, *ras.bev_hw, P(ja), P(jb), per_sample, P(aug), batch,
                                         P(ras.coef_y), P(ras.coef_x), g["resize"], g["crop"], P(ras.lut), g["out"], fmt, out_c, status.ptr(DEV), ras._stream())


def _densify_tiles(ras, n, bev, ja, jb, tiles_b, out, out_c, **kw):
    g = dict(resize=ras.resize, crop=ras.crop, coef_y=ras.coef_y, coef_x=ras.coef_x)
    g.update(kw)
    ws = ras._workspace(g.get("ws_renders", max(n, 1)))
    return ras.lib.salve_bev_densify_tiles(ctypes.byref(ras.cfg), n, P(bev), P(ja), P(jb), P(tiles_b), P(g["coef_y"]), P(g["coef_x"]), g["resize"], g["crop"], P(ras.lut),
                                           P(out), out_c, status.ptr(DEV), P(ws), ws.numel(), ras._stream())


def _resize(lib, src, dst, cy, cx, n=None):
    _, H, W, _ = src.shape
    return lib.salve_resize_rgb_u8(P(src), src.shape[0] if n is None else n, H, W, P(dst), dst.shape[1], dst.shape[2], P(cy), P(cx),
                                   ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


# ---------------------------------------------------------------------------------------------------- salve_bev_tiles
@pytest.mark.parametrize("case", tc.tiles_cases(), ids=lambda c: f"{c[0]}-fmt{c[1]}-{c[2]}")
def test_tiles_equal_the_emulator(case):
    gid, fmt, kind = case
    geo = tc.BY_ID[gid]
    ras = _ras(geo, kind)
    want = tc.tiles_expected(case)
    jobs = tc.tiles_jobs(fmt)
    out = _dev(tc.blank(want.shape, want.dtype))
    j = ras.upload_tile_jobs([i for _, i, _, _ in jobs], [s for _, _, s, _ in jobs], [c for _, _, _, c in jobs])
    _ok(_tiles(ras, _dev(tc.image_array(geo)), j, len(jobs), out, fmt, tc.tiles_out_c(fmt)), ras)
    _same(out, want, f"salve_bev_tiles {case}")
    ras.check(str(case))


def test_tiles_ignore_the_top_byte_of_the_image_words():
    geo = tc.G_NARROW
    ras = _ras(geo)
    jobs = tc.tiles_jobs(tc.U8X4)
    j = ras.upload_tile_jobs([i for _, i, _, _ in jobs], [s for _, _, s, _ in jobs], [c for _, _, _, c in jobs])
    for fmt in (tc.F32_NCHW, tc.F16_NHWC, tc.U8X4):
        want = tc.tiles_expected((geo.id, fmt, "imagenet"))
        out = _dev(tc.blank(want.shape, want.dtype))
        _ok(_tiles(ras, _dev(tc.image_array(geo, top=0xC3)), j, len(jobs), out, fmt, tc.tiles_out_c(fmt)), ras)
        _same(out, want, f"top byte set, format {fmt}")


# ---------------------------------------------------------------------------------------------------- salve_bev_tiles_aug
@pytest.mark.parametrize("gid", tc.aug_cases())
def test_aug_tiles_equal_the_emulator(gid):
    geo = tc.BY_ID[gid]
    ras = _ras(geo)
    jobs = tc.aug_jobs(geo)
    want = tc.aug_expected(gid)
    bev = _dev(tc.image_array(geo))
    out = _dev(tc.blank(want.shape, want.dtype))
    j = ras.upload_tile_jobs([x[1] for x in jobs], [x[2] for x in jobs], [x[3] for x in jobs])
    _ok(_tiles_aug(ras, bev, j, _aug([x[4] for x in jobs]), len(jobs), out, 6), ras)
    _same(out, want, f"salve_bev_tiles_aug {gid}")
    # the centre draw without flips is salve_bev_tiles' F32_NCHW output, bit for bit
    tj = tc.tiles_jobs(tc.F32_NCHW)
    j = ras.upload_tile_jobs([i for _, i, _, _ in tj], [s for _, _, s, _ in tj], [c for _, _, _, c in tj])
    centre = (geo.resize - geo.crop) // 2
    a = _dev(tc.blank((tc.N_SLOTS, 6, geo.crop, geo.crop), np.float32))
    b = a.clone()
    _ok(_tiles_aug(ras, bev, j, _aug([(centre, centre, 0)] * len(tj)), len(tj), a, 6), ras)
    _ok(_tiles(ras, bev, j, len(tj), b, tc.F32_NCHW, 6), ras)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _same(a, tc.tiles_expected((gid, tc.F32_NCHW, "imagenet")), "centre draw")
    ras.check(gid)


# ---------------------------------------------------------------------------------------------------- salve_bev_tile_pairs
@pytest.mark.parametrize("case", tc.pairs_cases(), ids=lambda c: f"{c.gid}-n{c.n}-c{c.out_c}-g{c.groups}-{c.kind}")
def test_tile_pairs_equal_the_emulator_plain_pretiled_and_as_two_tile_calls(case):
    geo = tc.BY_ID[case.gid]
    ras = _ras(geo, case.kind)
    jobs, n_slots = tc.pairs_jobs(case)
    want = tc.pairs_expected(case)
    bev_a = _dev(tc.image_array(geo))
    bev_b = bev_a.clone()
    slots = [x[6] for x in jobs]
    ja = ras.upload_tile_jobs([x[1] for x in jobs], slots, [x[2] for x in jobs])
    jb = ras.upload_tile_jobs([x[4] for x in jobs], slots, [x[5] for x in jobs])
    out = _dev(tc.blank(want.shape, want.dtype))
    _ok(_pairs(ras, bev_a, bev_b, ja, jb, case.n, out, case.out_c, False), ras)
    _same(out, want, f"salve_bev_tile_pairs {case}")
    pre = ras.pretile(bev_b)                                     # SALVE_TILE_U8X4 images, as the pipeline makes them
    jbp = ras.upload_tile_jobs([x[4] for x in jobs], slots, [x[5] for x in jobs], pretiled=True)
    out2 = _dev(tc.blank(want.shape, want.dtype))
    _ok(_pairs(ras, bev_a, pre, ja, jbp, case.n, out2, case.out_c, True), ras)
    _same(out2, want, f"salve_bev_tile_pairs, b_pretiled {case}")
    two = _dev(tc.blank(want.shape, want.dtype))                 # two salve_bev_tiles calls write the same six channels (and no padding)
    _ok(_tiles(ras, bev_a, ja, case.n, two, tc.F16_NHWC, case.out_c), ras)
    _ok(_tiles(ras, bev_b, jb, case.n, two, tc.F16_NHWC, case.out_c), ras)
    two = two.cpu().numpy()
    named = ~np.isnan(two)
    assert named.sum() == case.n * 6 * geo.crop * geo.crop
    assert np.array_equal(tc.bits(two)[named], tc.bits(want)[named])
    pad = ~named & ~np.isnan(want)
    assert not want[pad].any()                                   # what the pair entry writes beyond them is the zero padding
    ras.check(str(case))


# ---------------------------------------------------------------------------------------------------- salve_bev_train_tiles
def _train_tables(ras, case):
    ja, jb, dr = tc.train_jobs(case)
    smp = np.repeat(np.arange(case.batch), case.per_sample)
    return (ras.upload_tile_jobs([x[1] for x in ja], smp, [x[2] for x in ja]), ras.upload_tile_jobs([x[1] for x in jb], smp, [x[2] for x in jb]), _aug(dr), ja, jb, dr)


@pytest.mark.parametrize("case", tc.train_cases(), ids=lambda c: f"{c.gid}-b{c.batch}-s{c.per_sample}-c{c.out_c}")
def test_train_tiles_equal_the_emulator_in_fp32_and_bf16(case):
    geo = tc.BY_ID[case.gid]
    ras = _ras(geo)
    ja, jb, aug, la, lb, dr = _train_tables(ras, case)
    want = np.concatenate([tc.train_expected(case), tc.blank((1, geo.crop, geo.crop, case.out_c), np.float32)])   # one sample behind the batch
    bev_a = _dev(tc.image_array(geo))
    bev_b = bev_a.clone()
    out = _dev(tc.blank(want.shape, np.float32))
    _ok(_train(ras, bev_a, bev_b, ja, jb, case.per_sample, aug, case.batch, out, _lib.TILE_F32_NHWC, case.out_c), ras)
    _same(out, want, f"salve_bev_train_tiles fp32 {case}")
    assert not bool(out[:case.batch, ..., 6 * case.per_sample:].any())                                      # the padding channels: exactly zero
    want16 = np.concatenate([tc.to_bf16_bits(want[:-1]), tc.blank((1, geo.crop, geo.crop, case.out_c), np.uint16)])
    out16 = _dev(tc.blank(want.shape, np.uint16))
    _ok(_train(ras, bev_a, bev_b, ja, jb, case.per_sample, aug, case.batch, out16, _lib.TILE_BF16_NHWC, case.out_c), ras)
    _same(out16, want16, f"salve_bev_train_tiles bf16 {case}")
    same_array = _dev(tc.blank(want.shape, np.float32))                                                      # bev_a and bev_b as the same array
    _ok(_train(ras, bev_a, bev_a, ja, jb, case.per_sample, aug, case.batch, same_array, _lib.TILE_F32_NHWC, case.out_c), ras)
    assert torch.equal(same_array.view(torch.int32), out.view(torch.int32))
    if case.batch in (9, 17):   # the fp32 bits are the aug entry's: every image of the batch as one aug job with its sample's draw
        C = 6 * case.per_sample
        smp = np.repeat(np.arange(case.batch), case.per_sample)
        nchw = _dev(tc.blank((case.batch, C, geo.crop, geo.crop), np.float32))
        for tab, bev in ((la, bev_a), (lb, bev_b)):
            j = ras.upload_tile_jobs([x[1] for x in tab], smp, [x[2] for x in tab])
            _ok(_tiles_aug(ras, bev, j, _aug([dr[s] for s in smp]), len(tab), nchw, C), ras)
        assert torch.equal(nchw.permute(0, 2, 3, 1).contiguous().view(torch.int32), out[:case.batch, ..., :C].contiguous().view(torch.int32))
    ras.check(str(case))


@pytest.mark.parametrize("field,value", [("chan", None), ("chan", -3), ("slot", 0), ("bev_offset", None), ("flags", 4)])
def test_train_tiles_bad_job_in_the_second_group_of_eight(field, value):
    """Sample 8 of 9 -- the first of the second group of the `id & 7` mapping -- names channels outside the sample, another sample, an image
    outside its array, an unknown flag: SALVE_STATUS_BAD_TILE_JOB, that sample keeps the sentinel, the other eight are written."""
    case = tc.TrainCase(tc.G_NARROW.id, 9, 2, 16)
    geo = tc.G_NARROW
    ras = _ras(geo)
    ras.check("before")
    ja, jb, aug, *_ = _train_tables(ras, case)
    bev = _dev(tc.image_array(geo))
    want = tc.train_expected(case)
    if field == "flags":
        a = aug.cpu().numpy().view(_lib.TILE_AUG_DTYPE).copy()
        a["flags"][8] |= value
        aug = torch.from_numpy(a.view(np.uint8)).to(DEV)
    else:
        j = jb.cpu().numpy().view(_lib.TILE_JOB_DTYPE).copy()
        j[field][8 * 2 + 1] = {"chan": case.out_c, "bev_offset": len(tc.CONTENTS) * geo.h * geo.w}[field] if value is None else value
        jb = torch.from_numpy(j.view(np.uint8)).to(DEV)
    out = _dev(tc.blank(want.shape, np.float32))
    _ok(_train(ras, bev, bev, ja, jb, 2, aug, 9, out, _lib.TILE_F32_NHWC, 16), ras)
    torch.cuda.synchronize()
    assert int(status.word(DEV).item()) == _lib.STATUS_BAD_TILE_JOB
    want[8] = tc.blank(want[8].shape, np.float32)
    _same(out, want, f"bad {field}")
    with pytest.raises(_lib.SalveHipError, match="train-tile job"):
        ras.check("bad job")
    ras.check("after")


# ---------------------------------------------------------------------------------------------------- phase H
def _inject(ras, geo, content):
    """The image as the sparse image of ONE render with EVERY pixel a site (salve_bev_keys_from_pixels), ready for a densify with out_flags = 3."""
    yy, xx = np.mgrid[0:geo.h, 0:geo.w]
    xy = _dev(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32))
    rgb = _dev(tc.image(geo.h, geo.w, content).reshape(-1, 3))
    bev = _dev(tc.blank((1, geo.h, geo.w), np.uint32))
    ras.keys_from_pixels(xy, rgb, bev)
    return bev


@pytest.mark.parametrize("gid", sorted({c.gid for c in tc.phase_h_cases()}))
def test_fused_tile_phase_equals_the_emulator_and_the_pair_kernel(gid):
    geo = tc.BY_ID[gid]
    for case in [c for c in tc.phase_h_cases() if c.gid == gid]:
        ras = _ras(geo, case.kind)
        ras.cfg.out_flags = 3                                         # no flip, no mask: the plain interpolant of a full lattice is the image
        img = tc.image(geo.h, geo.w, case.content)
        bev = _inject(ras, geo, case.content)
        pre = ras.pretile(_dev(tc.pack(tc.image(geo.h, geo.w, tc.phase_h_second(case)))[None]))
        ja = ras.upload_tile_jobs([0], [1], [case.c0 + (0 if case.a_first else 3)])
        jb = ras.upload_tile_jobs([0], [1], [case.c0 + (3 if case.a_first else 0)], pretiled=True)
        want = tc.phase_h_expected(case)
        out = _dev(tc.blank(want.shape, want.dtype))
        _ok(_densify_tiles(ras, 1, bev, ja, jb, pre, out, case.out_c), ras)
        ras.check(str(case))
        _same(ras.export_u8(bev)[0], img, f"{case}: the completed image against the injected one")
        assert not bool((bev >> 24).any())
        _same(out, want, f"phase H {case}")
        pair = _dev(tc.blank(want.shape, want.dtype))
        _ok(_pairs(ras, bev, pre, ja, jb, 1, pair, case.out_c, True), ras)
        assert torch.equal(pair.view(torch.int16), out.view(torch.int16)), case


def test_fused_tile_phase_of_a_launch_whose_renders_partly_name_no_sample():
    """Nine renders of synthetic panoramas in one launch, jobs_a.slot < 0 for three of them: those write no tile (their samples keep the
    sentinel), the others equal scatter + densify + salve_bev_tile_pairs(b_pretiled = 1); the images equal in both forms."""
    ras = BevRasteriser(DEV)
    panos = [synthetic.make_pano(i, scene="cluttered" if i % 2 else "box") for i in range(2)]
    d_rgb, d_depth = ras.upload_panos(np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos]))
    hyp = synthetic.make_hypotheses(9, 2, seed=11)
    ident, _ = ras.render(d_rgb, d_depth, ras.upload_hypotheses(pack_hypotheses([0, 1], [0, 0], hyp.R[:2], hyp.t[:2], [0, 0])), 2)
    pre = ras.pretile(ident)
    n = 9
    hd = ras.upload_hypotheses(pack_hypotheses(hyp.i1, np.zeros(n, dtype=int), hyp.R, hyp.t, np.ones(n, dtype=int)))
    slot = np.array([3, -1, 0, 5, -1, 1, 4, -5, 2])
    swap = np.arange(n) % 2
    ja = ras.upload_tile_jobs(np.arange(n), slot, 3 * swap)
    jb = ras.upload_tile_jobs(np.asarray(hyp.i2), np.maximum(slot, 0), 3 * (1 - swap), pretiled=True)
    shape = (7, 224, 224, 8)                                          # samples 0 .. 5 are named, 6 by none
    fused_bev, plain_bev = (torch.empty((n, 501, 501), dtype=torch.int32, device=DEV) for _ in range(2))
    fused = _dev(tc.blank(shape, np.float16))
    ras.scatter(d_rgb, d_depth, hd, n, fused_bev)
    _ok(_densify_tiles(ras, n, fused_bev, ja, jb, pre, fused, 8), ras)
    ras.scatter(d_rgb, d_depth, hd, n, plain_bev)
    ras.densify(n, plain_bev)
    ras.check("multi-render")
    assert torch.equal(fused_bev, plain_bev)
    keep = np.nonzero(slot >= 0)[0]
    plain = _dev(tc.blank(shape, np.float16))
    _ok(_pairs(ras, plain_bev, pre, ras.upload_tile_jobs(keep, slot[keep], 3 * swap[keep]),
               ras.upload_tile_jobs(np.asarray(hyp.i2)[keep], slot[keep], 3 * (1 - swap[keep]), pretiled=True), len(keep), plain, 8, True), ras)
    assert torch.equal(fused.view(torch.int16), plain.view(torch.int16))
    got = fused.cpu().numpy()
    assert np.isnan(got[6]).all() and np.isfinite(got[:6].astype(np.float32)).all() and not got[:6, ..., 6:].any()


# ---------------------------------------------------------------------------------------------------- salve_resize_rgb_u8, salve_bev_export_u8
@pytest.mark.parametrize("case", tc.resize_cases(), ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}-{c[2][0]}")
def test_resize_rgb_equals_the_emulator(case):
    (H, W), (h, w), pair = case
    lib = _lib.load()
    want = np.concatenate([tc.resize_expected(case), tc.blank((1, h, w, 3), np.uint8)])      # one image behind the two
    src = _dev(np.stack([tc.image(H, W, c) for c in pair]))
    out = _dev(tc.blank(want.shape, np.uint8))
    box = (H, W) == (2 * h, 2 * w)
    cy, cx = (None, None) if box else (_dev(linear_resize_taps(h, H)), _dev(linear_resize_taps(w, W)))
    assert _resize(lib, src, out, cy, cx) == _lib.SALVE_OK, lib.salve_last_error()
    _same(out, want, f"salve_resize_rgb_u8 {case}")
    if (H, W) != (h, w):                                                                      # the shipped wrapper (it returns equal sizes unchanged)
        from salve_amd.ingest import resize_rgb_on_device

        _same(resize_rgb_on_device(src, (h, w)), want[:2], f"resize_rgb_on_device {case}")


def test_export_drops_the_top_byte():
    lib = _lib.load()
    words = tc.export_case()
    want = np.concatenate([tc.export_expected(), tc.blank((1,) + tc.EXPORT_HW + (3,), np.uint8)])
    out = _dev(tc.blank(want.shape, np.uint8))
    st = lib.salve_bev_export_u8(P(_dev(words)), 2, *tc.EXPORT_HW, P(out), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == _lib.SALVE_OK and (words >> 24).all()
    _same(out, want, "salve_bev_export_u8")


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_their_documented_code_and_write_nothing():
    geo = tc.G_NARROW
    ras = _ras(geo)
    ras.cfg.out_flags = 3
    ras.check("before the refusals")
    lib, BAD, UNS, OK = ras.lib, _lib.SALVE_ERR_BAD_ARG, _lib.SALVE_ERR_UNSUPPORTED, _lib.SALVE_OK
    bev = _dev(tc.image_array(geo))
    j = ras.upload_tile_jobs([0, 1], [0, 1], [0, 3])
    jp = ras.upload_tile_jobs([0, 1], [0, 1], [3, 0], pretiled=True)
    aug = _aug([(0, 0, 0), (1, 1, 3)])
    pre = ras.pretile(bev)
    out = _dev(tc.blank((2 * geo.crop * geo.crop * 16,), np.float32))       # room for every format below
    clean = out.clone()
    seen = []

    def refused(st, code, what):
        assert st == code, (what, st, lib.salve_last_error())
        assert code == OK or lib.salve_last_error().decode() != "", what
        seen.append(what)

    refused(_tiles(ras, bev, j, 2, out, tc.F32_NCHW, 6, crop=0), BAD, "tiles crop 0")
    refused(_tiles(ras, bev, j, 2, out, tc.F32_NCHW, 6, crop=-4), BAD, "tiles crop < 0")
    refused(_tiles(ras, bev, j, 2, out, tc.F32_NCHW, 6, resize=geo.crop - 1), BAD, "tiles resize < crop")
    refused(_tiles(ras, bev, j, 2, out, tc.F32_NCHW, 2), BAD, "tiles out_c 2")
    refused(_tiles(ras, bev, j, 2, out, 7, 6), UNS, "tiles format 7")
    refused(_tiles(ras, bev, j, 2, out, tc.F32_NHWC, 8), UNS, "tiles with a train format")
    refused(_tiles(ras, bev, j, 65536, out, tc.F32_NCHW, 6), BAD, "tiles 65536 jobs")
    refused(_tiles(ras, bev, j, 0, out, tc.F32_NCHW, 6), OK, "tiles 0 jobs")
    refused(_tiles_aug(ras, bev, j, aug, 2, out, 6, crop=0), BAD, "aug crop 0")
    refused(_tiles_aug(ras, bev, j, aug, 2, out, 6, resize=geo.crop - 1), BAD, "aug resize < crop")
    refused(_tiles_aug(ras, bev, j, aug, 2, out, 2), BAD, "aug out_c 2")
    refused(_tiles_aug(ras, bev, j, aug, 65536, out, 6), BAD, "aug 65536 jobs")
    refused(_tiles_aug(ras, bev, j, aug, 0, out, 6), OK, "aug 0 jobs")
    for pretiled, b, jb in ((False, bev, j), (True, pre, jp)):
        refused(_pairs(ras, bev, b, j, jb, 2, out, 8, pretiled, crop=0), BAD, "pairs crop 0")
        refused(_pairs(ras, bev, b, j, jb, 2, out, 8, pretiled, resize=geo.crop - 1), BAD, "pairs resize < crop")
        refused(_pairs(ras, bev, b, j, jb, 2, out, 4, pretiled), BAD, "pairs out_c 4")
        refused(_pairs(ras, bev, b, j, jb, 2, out, 7, pretiled), BAD, "pairs out_c 7")
        refused(_pairs(ras, bev, b, j, jb, 65536, out, 8, pretiled), BAD, "pairs 65536")
        refused(_pairs(ras, bev, b, j, jb, 0, out, 8, pretiled), OK, "pairs 0")
    tj = ras.upload_tile_jobs([0, 1], [0, 1], [0, 0])
    tk = ras.upload_tile_jobs([2, 3], [0, 1], [3, 3])
    t = lambda **kw: _train(ras, bev, bev, tj, tk, kw.pop("per_sample", 1), aug, kw.pop("batch", 2), kw.pop("out", out), kw.pop("fmt", _lib.TILE_F32_NHWC), kw.pop("out_c", 8), **kw)
    refused(t(crop=0), BAD, "train crop 0")
    refused(t(resize=geo.crop - 1), BAD, "train resize < crop")
    refused(t(per_sample=0), BAD, "train per_sample 0")
    refused(t(per_sample=4, out_c=24), BAD, "train per_sample 4")
    refused(t(out_c=12), BAD, "train out_c 12")
    refused(t(out_c=6), BAD, "train out_c 6")
    refused(t(out_c=32), BAD, "train out_c 32")
    refused(t(per_sample=2, out_c=8), BAD, "train out_c too small for two images")
    refused(t(fmt=7), BAD, "train format 7")
    refused(t(fmt=tc.F16_NHWC), BAD, "train with a tile format")
    refused(t(out=ctypes.c_void_p(out.data_ptr() + 4)), BAD, "train misaligned out")
    refused(t(batch=65536), BAD, "train 65536 samples")
    refused(t(batch=0), OK, "train 0 samples")
    one = _inject(ras, geo, "ramp")
    dj = ras.upload_tile_jobs([0], [0], [0])
    djb = ras.upload_tile_jobs([0], [0], [3], pretiled=True)
    big = 420                                                        # 420 * 32 + 3072 bytes of tables against the 13.2 KB LDS block of a 41 x 37 image
    big_y, big_x = _dev(linear_resize_taps(big, geo.h)), _dev(linear_resize_taps(big, geo.w))
    refused(_densify_tiles(ras, 1, one, dj, djb, pre, out, 8, resize=big, coef_y=big_y, coef_x=big_x), UNS, "fused phase: resize too large")
    refused(_densify_tiles(ras, 1, one, dj, djb, pre, out, 8, crop=0), BAD, "fused phase crop 0")
    refused(_densify_tiles(ras, 1, one, dj, djb, pre, out, 8, resize=geo.crop - 1), BAD, "fused phase resize < crop")
    refused(_densify_tiles(ras, 1, one, dj, djb, pre, out, 4), BAD, "fused phase out_c 4")
    refused(_densify_tiles(ras, 1, one, dj, djb, pre, out, 9), BAD, "fused phase out_c 9")
    refused(_densify_tiles(ras, 65536, one, dj, djb, pre, out, 8, ws_renders=1), BAD, "fused phase 65536 renders")
    refused(_densify_tiles(ras, 0, one, dj, djb, pre, out, 8), OK, "fused phase 0 renders")
    src = _dev(np.stack([tc.image(6, 10, "ramp")] * 2))
    dst = out.view(torch.uint8)[:2 * 3 * 6 * 3].view(2, 3, 6, 3)
    refused(_resize(lib, src, dst, None, None), BAD, "resize_rgb without tap tables at a ratio that is not 2 x 2")
    refused(_resize(lib, src, dst[:, :0], None, None), BAD, "resize_rgb dst_h 0")
    refused(_resize(lib, src, dst, None, None, n=0), OK, "resize_rgb 0 images")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), clean.view(torch.int32)), "a refused call wrote"
    _same(ras.export_u8(one)[0], tc.image(geo.h, geo.w, "ramp"), "the sparse image of the refused fused launches")
    ras.check("refusals")
    assert len(seen) == 48
