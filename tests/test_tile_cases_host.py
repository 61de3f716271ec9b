"""The case set of tests/tile_cases.py on the CPU: the module's scalar tap derivation equals `oracle.bev_oracle._linear_coeffs` and
`salve_amd.rasteriser.linear_resize_taps` (two copies of one text, pinned here to a second derivation), its pixel emulator equals the
oracle's `resize_linear_u8` / `resize_pano_u8` / `tile_from_bev` on every geometry and content, the fixed-point result stays within the
derived FIXED_VS_EXACT of the exact `fractions.Fraction` bilinear value on the small geometries, the tables hold what they claim, and
each of fifteen emulated wrong kernels is rejected by the zero-tolerance comparator on at least one case of EVERY entry it applies to --
the proof that the comparisons of tests/test_gpu_tile_contract.py can fail.  No GPU.  Parity with OpenCV itself stays unpinned.

Measured: the whole module takes 26 s on one CPU core (the fifteen mutants over the cases of their entries 14 s, the table of who
carries the narrow ones 8 s); the fixed-point result lies at most 0.8044 below and 0.5532 above the exact value, against the
derived 1.2720."""

from fractions import Fraction

import numpy as np
import pytest

import tile_cases as tc
from oracle import bev_oracle as bo
from salve_amd.rasteriser import linear_resize_taps, normalisation_lut

TAP_PAIRS = sorted({(g.resize, s) for g in tc.GEOMETRIES for s in (g.h, g.w)} | {(d, s) for src, dst in tc.RESIZE_SIZES for d, s in zip(dst, src)}
                   | {(234, 501), (1002, 501), (2000, 501), (37, 41), (41, 37), (1, 5), (5, 1), (512, 1024), (1024, 2048), (512, 500), (1023, 1023),
                      (7, 1023), (1023, 7)})


def test_the_tables_are_what_the_module_declares():
    assert [g.id for g in tc.GEOMETRIES] == ["41x37-30-24", "37x41-90-64", "64x64-32-32", "33x33-33-17", "101x101-47-40", "101x101-300-290",
                                             "41x37-30-1", "501x501-234-224"]
    g = tc.BY_ID
    assert g["37x41-90-64"].resize > 41 and g["64x64-32-32"].resize == g["64x64-32-32"].crop and 64 == 2 * 32              # up-scale; ratio 2, crop == resize
    assert (g["101x101-47-40"].resize - g["101x101-47-40"].crop) % 2 == 1 and g["101x101-300-290"].crop > 256             # odd difference; second column group
    assert [x.id for x in tc.GEOMETRIES if (x.crop * x.crop) % 256 == 0] == ["37x41-90-64", "64x64-32-32", "501x501-234-224"]   # the others end in a partial block
    assert all(x.h <= tc.MAX_SRC and x.w <= tc.MAX_SRC for x in tc.GEOMETRIES)
    assert sorted(tc.SLOT_PERM) == [0, 1, 2, 3, 4, 6, 7] and list(tc.SLOT_PERM) != sorted(tc.SLOT_PERM)
    assert sorted(tc.IMAGE_ORDER) == list(range(7)) and list(tc.IMAGE_ORDER) != sorted(tc.IMAGE_ORDER) and 6 in tc.IMAGE_ORDER
    assert len(tc.MUTANTS) == 15 and all(set(e) <= set(tc.ENTRIES) and e for e in tc.MUTANTS.values())
    assert {c.n for c in tc.pairs_cases()} >= {1, 7, 8, 9, 17} and {c.out_c for c in tc.pairs_cases()} == {6, 8, 10, 12, 14, 16}
    assert {(c.out_c, c.groups) for c in tc.pairs_cases()} >= {(12, 1), (12, 2), (16, 1), (16, 2)}
    assert {c.batch for c in tc.train_cases()} == {1, 7, 8, 9, 17} and {(c.per_sample, c.out_c) for c in tc.train_cases()} >= {(1, 8), (2, 16), (3, 24)}
    for c in tc.pairs_cases():
        jobs, n_slots = tc.pairs_jobs(c)
        slots = [j[6] for j in jobs]
        assert len(jobs) == c.n and max(slots) == n_slots - 2 and all(abs(j[2] - j[5]) == 3 and min(j[2], j[5]) % 6 == 0 and max(j[2], j[5]) + 3 <= c.out_c for j in jobs)
        assert len({(j[6], min(j[2], j[5])) for j in jobs}) == c.n                                  # no two pairs write one group
        if c.n > 2:
            assert {j[2] < j[5] for j in jobs} == {True, False}                                     # both channel orders
            assert [j[6] for j in jobs[::c.groups]] != sorted(j[6] for j in jobs[::c.groups])        # a non-identity slot permutation
    for c in tc.train_cases():
        ja, jb, dr = tc.train_jobs(c)
        assert len(ja) == len(jb) == c.batch * c.per_sample and len(dr) == c.batch
        for s in range(c.batch):
            mine = ja[s * c.per_sample:(s + 1) * c.per_sample] + jb[s * c.per_sample:(s + 1) * c.per_sample]
            assert sorted(j[2] for j in mine) == list(range(0, 6 * c.per_sample, 3))            # every group of three named once, the rest padding
        assert c.batch < 3 or {ja[s * c.per_sample][2] for s in range(c.batch)} == {0, 3}        # both channel orders
    for gid in tc.AUG_GEOMETRIES:
        geo = tc.BY_ID[gid]
        d, m = tc.draws(geo), geo.resize - geo.crop
        assert {f for _, _, f in d} == {0, 1, 2, 3} and (0, 0, 0) in d and (m, m, 3) in d
        assert any(oy < 0 for oy, _, _ in d) and any(ox < 0 for _, ox, _ in d) and any(oy > m for oy, _, _ in d) and any(ox > m for _, ox, _ in d)
        assert any(0 < oy < m and 0 < ox < m for oy, ox, _ in d)
    assert {(c.out_c, c.a_first) for c in tc.phase_h_cases()} == {(8, True), (8, False), (16, True), (16, False)}
    assert {c.gid for c in tc.phase_h_cases()} == {"101x101-300-290", "41x37-30-24", "101x101-47-40", "501x501-234-224"}
    assert any((2 * h * w) % 256 for _, (h, w) in tc.RESIZE_SIZES) and ((7, 9), (7, 9)) in tc.RESIZE_SIZES


@pytest.mark.parametrize("dst,src", TAP_PAIRS)
def test_scalar_taps_equal_the_two_array_derivations(dst, src):
    t = tc.taps(dst, src)
    s0, s1, a0, a1 = bo._linear_coeffs(dst, src)
    assert np.array_equal(t, np.stack([s0, s1, a0, a1], -1)) and np.array_equal(t, linear_resize_taps(dst, src))
    assert t.dtype == np.int32 and t.shape == (dst, 4) and not t.flags.writeable
    assert np.array_equal(t[:, 2] + t[:, 3], np.full(dst, 2048))             # complementary on every table of this suite (not assumed by FIXED_VS_EXACT)
    assert t[:, :2].min() >= 0 and t[:, :2].max() <= src - 1 and (t[:, 1] - t[:, 0]).max() <= 1


def test_identity_and_ratio_two_taps():
    assert np.array_equal(tc.taps(33, 33), np.stack([np.arange(33), np.minimum(np.arange(33) + 1, 32), np.full(33, 2048), np.zeros(33, int)], -1))
    t = tc.taps(32, 64)
    assert np.array_equal(t[:, 0], 2 * np.arange(32)) and np.array_equal(t[:, 2:], np.full((32, 2), 1024))


def test_the_tables_of_float_values_equal_the_librarys():
    assert tc.same(tc.lut(), normalisation_lut())
    mean, std = bo.imagenet_mean_std()
    v = np.arange(256, dtype=np.float32)
    assert all(tc.same(tc.lut()[c], (v - np.float32(mean[c])) / np.float32(std[c])) for c in range(3))
    ties = tc.lut("ties")
    assert (tc.to_f16(ties).astype(np.float64) != ties).all()                                  # no entry is an fp16 value ...
    up = np.nextafter(tc.to_f16(ties), np.where(ties > tc.to_f16(ties), np.inf, -np.inf).astype(np.float16)).astype(np.float64)
    assert np.array_equal(np.abs(up - ties), np.abs(tc.to_f16(ties).astype(np.float64) - ties))   # ... every entry is a tie
    away = tc.to_f16(ties, tc.M_F16_AWAY)
    assert (np.abs(away.astype(np.float64)) > np.abs(ties)).all() and not (np.abs(tc.to_f16(ties).astype(np.float64)) > np.abs(ties)).all()
    assert tc.same(tc.to_f16(tc.lut(), tc.M_F16_AWAY), tc.to_f16(tc.lut()))                   # the imagenet table holds no tie: hence the second table


def test_bf16_rounding_is_torchs():
    torch = pytest.importorskip("torch")
    x = np.concatenate([tc.lut().ravel(), np.array([0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5], dtype=np.float32)])   # incl. exact ties
    assert np.array_equal(tc.to_bf16_bits(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(tc.bits(tc.to_f16(x)), torch.from_numpy(x).half().view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize("gid", list(tc.BY_ID))
def test_pixel_emulator_equals_the_oracle(gid):
    geo = tc.BY_ID[gid]
    mean, std = bo.imagenet_mean_std()
    for content in tc.CONTENTS:
        img = tc.image(geo.h, geo.w, content)
        assert img.dtype == np.uint8 and img.shape == (geo.h, geo.w, 3) and not img.flags.writeable
        r = tc.resize_u8(img, tc.taps(geo.resize, geo.h), tc.taps(geo.resize, geo.w))
        assert np.array_equal(r, bo.resize_linear_u8(img, (geo.resize, geo.resize))), content
        want = bo.tile_from_bev(img, (geo.resize, geo.resize), (geo.crop, geo.crop))
        assert tc.same(tc.normalised(tc.crop_u8(geo, content), tc.lut()).transpose(2, 0, 1), want), content
    assert len({tc.image(geo.h, geo.w, "ramp")[..., c].tobytes() for c in range(3)}) == 3


@pytest.mark.parametrize("case", tc.resize_cases(), ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}-{c[2][0]}")
def test_resize_emulator_equals_the_oracle(case):
    (H, W), dst, pair = case
    want = np.stack([bo.resize_pano_u8(tc.image(H, W, c), dst) for c in pair])
    assert np.array_equal(tc.resize_expected(case), want)
    if (H, W) == dst:
        assert np.array_equal(want, np.stack([tc.image(H, W, c) for c in pair]))
    if pair[0] == "cells" and (H, W) == (2 * dst[0], 2 * dst[1]):
        assert (want[0] == 255).all()                                          # (255 + 255 + 255 + 254 + 2) >> 2: truncation would give 254


def exact_error(img, dst_h, dst_w, fixed):
    """max over pixels and channels of |fixed - exact bilinear value| as a Fraction.  Integer arithmetic over the common denominator
    (2 dst_h)(2 dst_w) -- the exact weights are `exact_coordinate`'s Fractions -- so that 24 000 pixels take no minute."""
    H, W = img.shape[:2]
    ys = [tc.exact_coordinate(d, dst_h, H) for d in range(dst_h)]
    xs = [tc.exact_coordinate(d, dst_w, W) for d in range(dst_w)]
    Dy, Dx = 2 * dst_h, 2 * dst_w
    assert all((f * Dy).denominator == 1 for _, f in ys) and all((f * Dx).denominator == 1 for _, f in xs)
    y0 = np.array([s for s, _ in ys]); gy = np.array([int(f * Dy) for _, f in ys], dtype=np.int64)
    x0 = np.array([s for s, _ in xs]); gx = np.array([int(f * Dx) for _, f in xs], dtype=np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    p = img.astype(np.int64)
    top = p[y0][:, x0] * (Dx - gx)[None, :, None] + p[y0][:, x1] * gx[None, :, None]
    bot = p[y1][:, x0] * (Dx - gx)[None, :, None] + p[y1][:, x1] * gx[None, :, None]
    num = top * (Dy - gy)[:, None, None] + bot * gy[:, None, None]           # exact value x Dx Dy
    diff = fixed.astype(np.int64) * (Dx * Dy) - num
    return Fraction(int(diff.max()), Dx * Dy), Fraction(int(-diff.min()), Dx * Dy)


def test_exact_coordinate_is_the_bilinear_coordinate():
    assert tc.exact_coordinate(0, 2, 4) == (0, Fraction(1, 2)) and tc.exact_coordinate(0, 8, 4) == (0, 0) and tc.exact_coordinate(7, 8, 4) == (2, 1)
    assert tc.exact_coordinate(3, 5, 5) == (3, 0) and tc.exact_coordinate(1, 3, 7) == (3, 0) and tc.exact_coordinate(0, 1, 1) == (0, 0)
    # one pixel through plain Fractions, against the integer form above
    img = tc.image(41, 37, "noise")
    fixed = tc.resize_u8(img, tc.taps(30, 41), tc.taps(30, 37))
    (sy, fy), (sx, fx) = tc.exact_coordinate(11, 30, 41), tc.exact_coordinate(17, 30, 37)
    v = [(1 - fy) * ((1 - fx) * int(img[sy, sx, c]) + fx * int(img[sy, sx + 1, c])) + fy * ((1 - fx) * int(img[sy + 1, sx, c]) + fx * int(img[sy + 1, sx + 1, c]))
         for c in range(3)]
    up, down = exact_error(img, 30, 30, fixed)
    assert all(abs(int(fixed[11, 17, c]) - v[c]) <= max(up, down) <= Fraction(tc.FIXED_VS_EXACT) for c in range(3))


def test_fixed_point_stays_within_the_derived_bound_of_the_exact_bilinear_value():
    """Every pixel of every small geometry and content, against the exact rational value (the anchor too: the integer form is cheap)."""
    assert 1.2719 < tc.FIXED_VS_EXACT < 1.2721
    worst_up = worst_down = Fraction(0)
    for geo in tc.GEOMETRIES:
        for content in tc.CONTENTS:
            img = tc.image(geo.h, geo.w, content)
            fixed = tc.resize_u8(img, tc.taps(geo.resize, geo.h), tc.taps(geo.resize, geo.w))
            up, down = exact_error(img, geo.resize, geo.resize, fixed)
            assert max(up, down) <= Fraction(tc.FIXED_VS_EXACT), (geo.id, content, float(up), float(down))
            worst_up, worst_down = max(worst_up, up), max(worst_down, down)
    for (H, W), (h, w) in tc.RESIZE_SIZES:
        if (H, W) != (2 * h, 2 * w):
            for content in ("noise", "checker", "columns", "rows", "ramp", "cells"):
                img = tc.image(H, W, content)
                up, down = exact_error(img, h, w, tc.resize_u8(img, tc.taps(h, H), tc.taps(w, W)))
                assert max(up, down) <= Fraction(tc.FIXED_VS_EXACT), ((H, W), (h, w), content)
                worst_up, worst_down = max(worst_up, up), max(worst_down, down)
    print(f"fixed point against exact bilinear: at most {float(worst_up):.4f} above, {float(worst_down):.4f} below; bound {tc.FIXED_VS_EXACT:.4f}")
    assert worst_down > Fraction(1, 2) and worst_up > Fraction(1, 4)           # the comparison is not vacuous: the floors and the rounding show


def test_sentinels_and_the_comparator():
    for dt in (np.float32, np.float16):
        assert np.isnan(tc.blank((2, 3), dt)).all()
    assert (tc.blank((3,), np.uint32) == 0x5A5A5A5A).all() and (tc.blank((3,), np.uint8) == 0x5A).all()
    a = tc.blank((4,), np.float32)
    assert tc.same(a, a.copy()) and not tc.same(a, np.zeros(4, np.float32)) and not tc.same(np.float32([0.0]), np.float32([-0.0]))
    # what the contract does not name keeps the sentinel
    t = tc.tiles_expected((tc.G_NARROW.id, tc.F16_NHWC, "imagenet"))
    named = np.zeros(t.shape, dtype=bool)
    for _, _, slot, chan in tc.tiles_jobs(tc.F16_NHWC):
        named[slot, :, :, chan:chan + 3] = True
    assert np.isnan(t[~named]).all() and np.isfinite(t[named].astype(np.float32)).all() and named.mean() < 0.4
    for case in tc.train_cases()[:3]:
        assert np.isfinite(tc.train_expected(case)).all()                     # the train entry writes every channel
    p = tc.pairs_expected(tc.PairCase(tc.G_NARROW.id, 9, 14, 2, "imagenet"))
    jobs, n_slots = tc.pairs_jobs(tc.PairCase(tc.G_NARROW.id, 9, 14, 2, "imagenet"))
    last = jobs[8][6]                                                          # the sample of the ninth pair holds ONE group of its two
    assert np.isfinite(p[last][..., :6].astype(np.float32)).all() and np.isnan(p[last][..., 6:]).all() and np.isnan(p[n_slots - 1]).all()
    full = jobs[0][6]
    assert (p[full][..., 12:] == 0).all() and np.isfinite(p[full][..., :12].astype(np.float32)).all()


@pytest.mark.parametrize("mutant", list(tc.MUTANTS))
def test_every_emulated_wrong_kernel_is_rejected_wherever_it_applies(mutant):
    for entry in tc.MUTANTS[mutant]:
        seen = [case for case in tc.entry_cases(entry) if not tc.same(tc.entry_expected(entry, case, mutant), tc.entry_expected(entry, case))]
        assert seen, f"{mutant!r} passes every case of {entry}"
    for entry in set(tc.ENTRIES) - set(tc.MUTANTS[mutant]):                    # and where it does not apply it is the identity
        case = tc.entry_cases(entry)[0]
        assert tc.same(tc.entry_expected(entry, case, mutant), tc.entry_expected(entry, case)), (mutant, entry)


def test_which_cases_carry_the_narrow_mutants():
    """The cases built for one mutant are the ones that see it."""
    see = lambda entry, m: {str(c) for c in tc.entry_cases(entry) if not tc.same(tc.entry_expected(entry, c, m), tc.entry_expected(entry, c))}
    odd = [g.id for g in tc.GEOMETRIES if (g.resize - g.crop) % 2]
    assert odd == ["101x101-47-40", "41x37-30-1"] and all(any(i in c for i in odd) for c in see("tiles", tc.M_CROP_UP))   # the odd differences alone
    assert all("101x101-47-40" in c for e in ("pairs", "phase_h") for c in see(e, tc.M_CROP_UP))
    assert all("'ties'" in c for e in ("tiles", "pairs", "phase_h") for c in see(e, tc.M_F16_AWAY))              # the tie table alone
    assert all("101x101-300-290" in c for c in see("phase_h", tc.M_COL_GROUP))                                   # crop > 256 alone
    assert not any("64x64" in c or "33x33" in c or "101x101" in c or "501x501" in c for c in see("tiles", tc.M_XROWS))   # non-square alone
    assert see("resize_rgb", tc.M_BOX) == {str(c) for c in tc.resize_cases() if (c[0], c[1]) == ((6, 10), (3, 6)) and c[2] != ("white", "black")}
    assert all(c.n > 8 for c in tc.pairs_cases() if str(c) in see("pairs", tc.M_MINUS_8)) and all(c.batch > 8 for c in tc.train_cases() if str(c) in see("train", tc.M_MINUS_8))
    assert any("64x64-32-32" in c for c in see("tiles", tc.M_TIE))            # 0 / 255 at ratio 2: (255 + 255 + 2) >> 2 = 128, the tie itself
