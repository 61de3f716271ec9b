"""The emulator of tests/jitter_cases.py on the CPU.  torchvision is not installed where this suite runs, so parity with torchvision
itself stays unpinned; what is pinned is every torch operation underneath: `TV` below restates the tensor ColorJitter functions of
torchvision 0.11 / 0.12 (functional_tensor.py: _blend, rgb_to_grayscale, adjust_brightness / _contrast / _saturation / _hue, _rgb2hsv,
_hsv2rgb) in torch operations on CHW uint8 tensors -- torch.mean(dim=(-3, -2, -1)), `%`, torch.fmod and the einsum select included --
and the numpy emulator must equal it bit for bit: all 24 orders, every enable subset, the factors' interval ends, random draws, noise
and the colour lattice.  Then: `TrainTransform.draw_jitter` makes ColorJitter.get_params' calls; factors 1 with hue disabled are the
identity; the record table holds the double-rounded complements; the opt-in keyword; and each of fourteen emulated wrong kernels
fails the cases tests/test_gpu_jitter.py runs -- the proof that its comparisons can fail.  No GPU."""

import itertools
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import jitter_cases as jc  # noqa: E402
import tile_cases as tc  # noqa: E402
from salve_amd import _lib, train_feed, training  # noqa: E402
from salve_amd.transforms import TrainTransform  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402


def config(**kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
             train_w=224, apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="t", num_epochs=2,
             workers=0, batch_size=2, data_root="", layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


# ---------------------------------------------------------------------------------------------------- torchvision, restated in torch ops
class TV:
    @staticmethod
    def blend(img1, img2, ratio):
        ratio = float(ratio)
        return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255.0).to(img1.dtype)

    @staticmethod
    def grayscale(img):
        r, g, b = img.unbind(dim=-3)
        return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)

    @staticmethod
    def brightness(img, f):
        return TV.blend(img, torch.zeros_like(img), f)

    @staticmethod
    def contrast(img, f):
        mean = torch.mean(TV.grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
        return TV.blend(img, mean, f)

    @staticmethod
    def saturation(img, f):
        return TV.blend(img, TV.grayscale(img), f)

    @staticmethod
    def rgb2hsv(img):
        r, g, b = img.unbind(dim=-3)
        maxc = torch.max(img, dim=-3).values
        minc = torch.min(img, dim=-3).values
        eqc = maxc == minc
        cr = maxc - minc
        ones = torch.ones_like(maxc)
        s = cr / torch.where(eqc, ones, maxc)
        cr_divisor = torch.where(eqc, ones, cr)
        rc = (maxc - r) / cr_divisor
        gc = (maxc - g) / cr_divisor
        bc = (maxc - b) / cr_divisor
        hr = (maxc == r) * (bc - gc)
        hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
        hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
        h = hr + hg + hb
        h = torch.fmod((h / 6.0 + 1.0), 1.0)
        return torch.stack((h, s, maxc), dim=-3)

    @staticmethod
    def hsv2rgb(img):
        h, s, v = img.unbind(dim=-3)
        i = torch.floor(h * 6.0)
        f = (h * 6.0) - i
        i = i.to(dtype=torch.int32)
        p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
        q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
        t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
        i = i % 6
        mask = i.unsqueeze(dim=-3) == torch.arange(6).view(-1, 1, 1)
        a1 = torch.stack((v, q, p, p, t, v), dim=-3)
        a2 = torch.stack((t, v, v, q, p, p), dim=-3)
        a3 = torch.stack((p, p, t, v, v, q), dim=-3)
        a4 = torch.stack((a1, a2, a3), dim=-4)
        return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)

    @staticmethod
    def hue(img, f):
        x = img.to(dtype=torch.float32) / 255.0
        x = TV.rgb2hsv(x)
        h, s, v = x.unbind(dim=-3)
        h = (h + f) % 1.0
        x = TV.hsv2rgb(torch.stack((h, s, v), dim=-3))
        return (x * 255.0).to(dtype=torch.uint8)

    @staticmethod
    def color_jitter(img_hwc: np.ndarray, rec: jc.Rec) -> np.ndarray:
        """ColorJitter.forward with get_params' results given: fn_idx = rec.order, a factor None where its mask bit is clear."""
        img = torch.from_numpy(np.array(img_hwc)).permute(2, 0, 1)
        for fn_id in rec.order:
            if not (rec.mask >> fn_id) & 1:
                continue
            img = (TV.brightness, TV.contrast, TV.saturation, TV.hue)[fn_id](img, (rec.b, rec.c, rec.s, rec.h)[fn_id])
        return img.permute(1, 2, 0).contiguous().numpy()


def _noise(seed, h=19, w=23):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3)).astype(np.uint8)


def _assert_equal(img, rec):
    got, want = jc.jitter_image(img, rec), TV.color_jitter(img, rec)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (rec, np.argwhere(got != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------- emulator == torch
@pytest.mark.parametrize("mask", range(16))
def test_emulator_equals_the_torch_restatement_for_all_orders_of_every_enable_subset(mask):
    for k, order in enumerate(jc.ORDERS):
        n = 24 * mask + k
        if k % 2:
            rec = jc.Rec(order, mask, jc.EDGE_FACTORS[n % 3], jc.EDGE_FACTORS[(n // 3) % 3], jc.EDGE_FACTORS[(n // 9) % 3], jc.EDGE_HUES[(n // 2) % 3])
        else:
            rec = jc.record(n)._replace(order=order, mask=mask)
        _assert_equal(_noise(n), rec)


def test_emulator_equals_the_torch_restatement_on_the_case_images_and_records():
    for geo in (jc.G_A, jc.G_B):
        for n in range(54):
            _assert_equal(jc.resized(geo)[n % jc.N_IMAGES], jc.record(n))


@pytest.mark.parametrize("run", ["colour", "contrast"])
def test_emulator_equals_the_torch_restatement_on_the_colour_lattice(run):
    lat = jc.lattice()
    assert lat.shape == (32, 256, 256, 3) and len(np.unique(tc.pack(lat))) == 128 ** 3
    for i in range(0, jc.LATTICE_IMAGES, 5):   # (seven of the 32 images here, all six orders of the three; the GPU test takes them all)
        _assert_equal(lat[i], jc.lattice_record(i, run))
    recs = [jc.lattice_record(i, run) for i in range(jc.LATTICE_IMAGES)]
    assert all(r.order[0] == jc.CONTRAST for r in recs) and len({r.order for r in recs}) == 6
    assert all(((r.mask >> jc.CONTRAST) & 1) == (run == "contrast") for r in recs)
    assert {r.s for r in recs} == {0.5, 1.5} and {r.b for r in recs} == {0.5, 1.5} and {r.h for r in recs} == set(jc.EDGE_HUES)


def test_hue_alone_at_zero_is_not_the_identity_and_equals_torch_on_every_lattice_colour_of_one_image():
    img = jc.lattice()[13]
    rec = jc.Rec((3, 0, 1, 2), 8, 1.0, 1.0, 1.0, 0.0)
    _assert_equal(img, rec)
    assert not np.array_equal(jc.jitter_image(img, rec), img)


def test_factors_one_with_hue_disabled_are_the_identity():
    for order in jc.ORDERS:
        for img in (_noise(5), jc.resized(jc.G_A)[2], jc.lattice()[7]):
            assert np.array_equal(jc.jitter_image(img, jc.IDENTITY._replace(order=order)), img)
    case = jc.cases()[4]
    G = 2 * case.per_sample
    ident = jc.expected(case, records=[[jc.IDENTITY] * G] * case.batch)
    ja, jb, _, dr = jc.jobs(case)
    geo = tc.BY_ID[case.gid]
    for s in range(case.batch):   # == the unjittered train transform
        for image, chan in ja[s * case.per_sample:(s + 1) * case.per_sample] + jb[s * case.per_sample:(s + 1) * case.per_sample]:
            want = tc.normalised(jc.crop_flip(jc.resized(geo)[image], geo, dr[s]), tc.lut())
            assert np.array_equal(ident[s, ..., chan:chan + 3], want)


def test_the_mean_is_one_division_of_an_exact_sum():
    """The issue's example: on a 30 x 30 image torch.mean and sum * (1 / N) differ; the emulator sides with torch.mean."""
    differ = 0
    for seed in range(40):
        img = _noise(seed, 30, 30)
        m = jc.mean_grey(img)
        t = torch.mean(TV.grayscale(torch.from_numpy(img.copy()).permute(2, 0, 1)).to(torch.float32), dim=(-3, -2, -1))
        assert np.float32(t.item()) == m
        differ += int(jc.mean_grey(img, jc.M_MEAN_RECIP) != m)
    assert differ > 0
    assert 256 * 256 * 255 < 2 ** 24 <= 257 * 257 * 255     # the contract's bound: resize <= 256


# ---------------------------------------------------------------------------------------------------- the cases hold what they claim
def test_the_case_tables_hold_what_they_claim():
    cases = [c for c in jc.cases() if not c.narrow]
    assert {c.gid for c in cases} == {"41x37-30-24", "33x33-33-17"} and {c.batch for c in cases} == {1, 9}
    assert [(c.gid, c.batch, c.per_sample, c.out_c) for c in jc.cases() if c.narrow] == [("41x37-30-24", 3, 1, 8), ("33x33-33-17", 1, 1, 8)]
    assert {(c.per_sample, c.out_c) for c in cases} == {(1, 8), (2, 16), (3, 24)}
    orders, masks, flips = set(), set(), set()
    for c in cases:
        geo = tc.BY_ID[c.gid]
        ja, jb, recs, dr = jc.jobs(c)
        assert len(recs) == c.batch and all(len(r) == 2 * c.per_sample for r in recs)
        for s in range(c.batch):
            assert len(set(recs[s])) == len(recs[s])                                  # the records of a sample's images differ
            chans = sorted(ch for _, ch in ja[s * c.per_sample:(s + 1) * c.per_sample] + jb[s * c.per_sample:(s + 1) * c.per_sample])
            assert chans == list(range(0, 6 * c.per_sample, 3))
            oy, ox, fl = dr[s]
            lo = (geo.resize - geo.crop) // 3
            assert lo <= oy <= geo.resize - geo.crop - lo and lo <= ox <= geo.resize - geo.crop - lo
            flips.add(fl)
        for r in itertools.chain(*recs):
            assert 0.5 <= r.b <= 1.5 and 0.5 <= r.c <= 1.5 and 0.5 <= r.s <= 1.5 and jc.EDGE_HUES[0] <= r.h <= jc.EDGE_HUES[2]
            orders.add(r.order)
            masks.add(r.mask)
    assert orders == set(jc.ORDERS) and masks == set(range(16)) and flips == {0, 1, 2, 3}
    for geo in (jc.G_A, jc.G_B):   # the border is bright in the resized image and outside every crop
        lo = (geo.resize - geo.crop) // 3
        r = jc.resized(geo)
        assert (r[:, 0] == jc.BORDER).all() and (r[:, :, -1] == jc.BORDER).all()
        inner = r[:, lo:geo.resize - lo, lo:geo.resize - lo]
        assert all(jc.mean_grey(inner[k]) != jc.mean_grey(r[k]) for k in range(jc.N_IMAGES))


# ---------------------------------------------------------------------------------------------------- the draws, the table, the keyword
def _get_params(jitter_types, generator=None):
    """ColorJitter.get_params of ColorJitter(0.5, 0.5, 0.5, 0.05) restricted to `jitter_types` (an operation left out has range None)."""
    rng = {"brightness": (0.5, 1.5), "contrast": (0.5, 1.5), "saturation": (0.5, 1.5), "hue": (-0.05, 0.05)}
    fn_idx = torch.randperm(4, generator=generator)
    f = [None if n not in jitter_types else float(torch.empty(1).uniform_(*rng[n], generator=generator)) for n in rng]
    return fn_idx, f


@pytest.mark.parametrize("types", [train_feed.JITTER_TYPES, ("contrast", "hue"), ("saturation",), ()])
def test_draw_jitter_makes_the_calls_of_get_params(types):
    tf = TrainTransform((234, 234), (224, 224), jitter_types=types)
    torch.manual_seed(11)
    got = [tf.draw_jitter() for _ in range(6)]
    torch.manual_seed(11)
    for order, mask, *factors in got:
        fn_idx, f = _get_params(types)
        assert list(order) == fn_idx.tolist()
        assert mask == sum(1 << k for k in range(4) if f[k] is not None)
        assert factors == [(0.0 if k == 3 else 1.0) if f[k] is None else f[k] for k in range(4)]
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    before = torch.get_rng_state()
    assert tf.draw_jitter(g1)[0] == tuple(_get_params(types, g2)[0].tolist())
    assert torch.equal(torch.get_rng_state(), before)                              # a given generator leaves the global one alone
    torch.manual_seed(3)
    flat = train_feed.jitter_draws(tf, 2, 4)
    torch.manual_seed(3)
    assert flat == [tf.draw_jitter() for _ in range(8)]


def test_draw_jitter_and_the_transform_refuse_what_they_cannot_do():
    with pytest.raises(RuntimeError, match="jitter_types"):
        TrainTransform((234, 234), (224, 224)).draw_jitter()
    with pytest.raises(ValueError, match="sharpness"):
        TrainTransform((234, 234), (224, 224), jitter_types=("sharpness",))
    with pytest.raises(RuntimeError, match="resize <= 256"):
        TrainTransform((257, 257), (224, 224), jitter_types=train_feed.JITTER_TYPES)
    TrainTransform((256, 256), (224, 224), jitter_types=train_feed.JITTER_TYPES)
    TrainTransform((300, 300), (224, 224))                                         # no jitter: no bound


def test_the_record_table_holds_the_complements_rounded_once_from_double():
    draws = [(r.order, r.mask, r.b, r.c, r.s, r.h) for r in (jc.record(n) for n in range(40))]
    t = train_feed.jitter_table(draws)
    assert t.dtype == _lib.TILE_JITTER_DTYPE and t.dtype.itemsize == 40 and t.shape == (40,)
    once_differs = 0
    for row, r in zip(t, (jc.record(n) for n in range(40))):
        assert tuple(row["order"]) == r.order and row["mask"] == r.mask and row["reserved"] == 0
        assert (row["brightness"], row["contrast"], row["saturation"], row["hue"]) == tuple(np.float32(v) for v in (r.b, r.c, r.s, r.h))
        for name, f in (("brightness_c", r.b), ("contrast_c", r.c), ("saturation_c", r.s)):
            assert row[name] == jc.complement(f) == np.float32(1.0 - f)
            once_differs += int(jc.complement(f) != jc.complement(f, jc.M_COMPLEMENT_F32))
    assert once_differs > 0
    assert train_feed.jitter_table([]).shape == (0,)


def test_the_entries_are_declared_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in ("salve_bev_train_tiles_jitter", "salve_bev_train_tiles_jitter_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and f"{name}(" in header and hasattr(lib, name), name
    assert "salve_tile_jitter_t" in header
    assert lib.salve_bev_train_tiles_jitter_workspace_bytes(9, 3) == 9 * 6 * 4
    assert [lib.salve_bev_train_tiles_jitter_workspace_bytes(b, k) for b, k in ((0, 1), (-1, 1), (65536, 1), (4, 0), (4, 4))] == [0] * 5


def test_the_keyword_permits_and_the_config_decides():
    on, off = config(apply_photometric_augmentation=True), config()
    with pytest.raises(RuntimeError, match=r"photometric=\"device\""):   # today's refusal, now naming the keyword
        training.get_train_transform(on)
    assert training.get_train_transform(on, photometric="device").jitter_types == train_feed.JITTER_TYPES
    assert training.get_train_transform(off, photometric="device").jitter_types is None
    assert training.get_train_transform(off).jitter_types is None
    with pytest.raises(ValueError, match="photometric"):
        training.get_train_transform(on, photometric="host")
    with pytest.raises(RuntimeError, match="padding|pads"):                 # out of scope, as before
        training.get_train_transform(config(apply_photometric_augmentation=True, train_h=300, train_w=300), photometric="device")
    for fn in (training.get_tile_file_source, training.get_dataloader, training.train, training.train_rendered):
        assert "photometric" in fn.__code__.co_varnames[:fn.__code__.co_argcount], fn.__name__
    from salve_amd import train
    with pytest.raises(SystemExit):
        train.main(["--config", "x.yaml", "--photometric", "host"])


# ---------------------------------------------------------------------------------------------------- the comparisons can fail
@pytest.fixture(scope="module")
def truth():
    return {c: jc.expected(c) for c in jc.cases()}


def _lattice_fails(mutant):
    """The first (run, image) of the colour lattice on which the wrong kernel's bytes differ, or None."""
    for run in ("colour", "contrast"):
        for i in range(jc.LATTICE_IMAGES):
            rec = jc.lattice_record(i, run)
            if not np.array_equal(jc.jitter_image(jc.lattice()[i], rec, mutant=mutant), jc.jitter_image(jc.lattice()[i], rec)):
                return run, i
    return None


@pytest.mark.parametrize("mutant", jc.MUTANTS)
def test_every_emulated_wrong_kernel_fails_a_case(mutant, truth):
    assert len(jc.MUTANTS) == 14
    failed = [c for c in jc.cases() if not tc.same(jc.expected(c, mutant), truth[c])]
    if mutant == jc.M_GREY_DOUBLE:   # three of the 128^3 colours have another grey level: only the lattice holds one of them
        assert not failed and _lattice_fails(mutant) is not None
        return
    assert failed, f"{mutant}: no case of tests/test_gpu_jitter.py fails"
    if mutant == jc.M_MEAN_RECIP:    # carried by the NARROW records alone
        assert all(c.narrow for c in failed) and {c.gid for c in failed} == {jc.G_A.id, jc.G_B.id}
    if mutant in (jc.M_REM_NO_PLUS, jc.M_HUE_NEW_FORM, jc.M_HUE_MASKS):   # the hue mutants show on the lattice too
        assert _lattice_fails(mutant) is not None
