"""salve_bev_train_tiles_jitter on the MI355X -- `bev_jitter_grey_sum_kernel` and `bev_train_tile_kernel<8|16|24, fp32|bf16, JITTER>` --
against the emulator of tests/jitter_cases.py, through the C ABI, into sentinel-filled buffers.  Every comparison is on bits; there is no
tolerance.  The cases: both geometries, batches 1 and 9, per_sample 1 .. 3, fp32 and bf16, flips on, records that differ within a sample
(all 24 orders, all 16 masks), the searched NARROW records, and the colour lattice (128^3 colours, 32 images of 256 x 256 at the largest
accepted resize) twice.  Then the identity, determinism, the host refusals, the device-side record check, `TrainTransform.apply(jitter=)`,
one jittered train batch of each feed, and the opt-in keyword."""

import ctypes
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import jitter_cases as jc  # noqa: E402
import tile_cases as tc  # noqa: E402
from salve_amd import _lib, status, synthetic, train_feed, train_render, training  # noqa: E402
from salve_amd.common.bevparams import BEVParams  # noqa: E402
from salve_amd.dataset.zind_data import ZindData  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402
from salve_amd.train_files import TileFileLoader, TileFileSource  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from salve_amd.transforms import TrainTransform  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")
RENDERINGS = Path(__file__).resolve().parent / "golden" / "renderings"
P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
_RAS = {}


def _ras(h, w, resize, crop):
    key = (h, w, resize, crop)
    if key not in _RAS:
        _RAS[key] = BevRasteriser(DEV, bev_params=BEVParams(h - 1, w - 1, 1.0), resize=resize, crop=crop)
        assert _RAS[key].bev_hw == (h, w)
    return _RAS[key]


def _dev(a):
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype, a.dtype))
    return torch.from_numpy(a.copy()).to(DEV)


def _bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


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
    return _bytes(a)


def _records(recs):
    """jc.Rec rows [batch][G] -> the device table, through the library's own `jitter_table`."""
    return _bytes(train_feed.jitter_table([tuple(r) for row in recs for r in row]))


def _workspace(ras, batch, per_sample):
    n = ras.lib.salve_bev_train_tiles_jitter_workspace_bytes(batch, per_sample)
    assert n == batch * 2 * per_sample * 4
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)     # (not zeroed: the entry zeroes what it sums into)


def _jitter(ras, bev_a, bev_b, ja, jb, per_sample, aug, batch, out, fmt, out_c, table, space, **kw):
    g = dict(resize=ras.resize, crop=ras.crop, jit=P(table), ws=P(space), ws_bytes=0 if space is None else space.numel())   # (kw: raw overrides)
    g.update(kw)
    hw = ras.bev_hw[0] * ras.bev_hw[1]
    return ras.lib.salve_bev_train_tiles_jitter(P(bev_a), bev_a.numel() // hw, P(bev_b), bev_b.numel() // hw, *ras.bev_hw, P(ja), P(jb), per_sample, P(aug), batch,
                                                P(ras.coef_y), P(ras.coef_x), g["resize"], g["crop"], P(ras.lut), P(out), fmt, out_c, g["jit"], g["ws"], g["ws_bytes"],
                                                status.ptr(DEV), ras._stream())


def _plain(ras, bev_a, bev_b, ja, jb, per_sample, aug, batch, out, fmt, out_c):
    hw = ras.bev_hw[0] * ras.bev_hw[1]
    return ras.lib.salve_bev_train_tiles(P(bev_a), bev_a.numel() // hw, P(bev_b), bev_b.numel() // hw, *ras.bev_hw, P(ja), P(jb), per_sample, P(aug), batch,
                                         P(ras.coef_y), P(ras.coef_x), ras.resize, ras.crop, P(ras.lut), P(out), fmt, out_c, status.ptr(DEV), ras._stream())


def _ok(st, ras):
    assert st == _lib.SALVE_OK, ras.lib.salve_last_error()


def _tables(ras, case):
    ja, jb, recs, dr = jc.jobs(case)
    smp = np.repeat(np.arange(case.batch), case.per_sample)
    return (ras.upload_tile_jobs([x[0] for x in ja], smp, [x[1] for x in ja]), ras.upload_tile_jobs([x[0] for x in jb], smp, [x[1] for x in jb]), _aug(dr), recs)


@pytest.fixture(scope="module")
def expected():
    """The emulator's fp32 result of every case, computed once and shared (read-only)."""
    out = {}
    for c in jc.cases():
        out[c] = jc.expected(c)
        out[c].setflags(write=False)
    return out


def _case_run(case):
    geo = tc.BY_ID[case.gid]
    ras = _ras(geo.h, geo.w, geo.resize, geo.crop)
    ja, jb, aug, recs = _tables(ras, case)
    return geo, ras, ja, jb, aug, recs, _dev(tc.pack(jc.images(geo)))


# ---------------------------------------------------------------------------------------------------- the emulator, bit for bit
@pytest.mark.parametrize("case", jc.cases(), ids=lambda c: f"{c.gid}-b{c.batch}-s{c.per_sample}-c{c.out_c}{'-narrow' if c.narrow else ''}")
def test_jitter_tiles_equal_the_emulator_in_fp32_and_bf16_and_twice(case, expected):
    geo, ras, ja, jb, aug, recs, bev = _case_run(case)
    ras.check("before")
    shape = (case.batch + 1, geo.crop, geo.crop, case.out_c)                                  # one sample behind the batch keeps the sentinel
    want = np.concatenate([expected[case], tc.blank((1,) + shape[1:], np.float32)])
    jit, ws = _records(recs), _workspace(ras, case.batch, case.per_sample)
    out = _dev(tc.blank(shape, np.float32))
    _ok(_jitter(ras, bev, bev.clone(), ja, jb, case.per_sample, aug, case.batch, out, _lib.TILE_F32_NHWC, case.out_c, jit, ws), ras)
    _same(out, want, f"salve_bev_train_tiles_jitter fp32 {case}")
    assert not bool(out[:case.batch, ..., 6 * case.per_sample:].any())                       # the padding channels: exactly zero
    out16 = _dev(tc.blank(shape, np.uint16))
    _ok(_jitter(ras, bev, bev, ja, jb, case.per_sample, aug, case.batch, out16, _lib.TILE_BF16_NHWC, case.out_c, jit, ws), ras)
    _same(out16, np.concatenate([tc.to_bf16_bits(want[:-1]), tc.blank((1,) + shape[1:], np.uint16)]), f"salve_bev_train_tiles_jitter bf16 {case}")
    again = _dev(tc.blank(shape, np.float32))                                                  # the same bytes on a second run, in a used workspace
    _ok(_jitter(ras, bev, bev, ja, jb, case.per_sample, aug, case.batch, again, _lib.TILE_F32_NHWC, case.out_c, jit, ws), ras)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    ras.check(str(case))


@pytest.mark.parametrize("case", [c for c in jc.cases() if c.batch == 9], ids=lambda c: f"{c.gid}-s{c.per_sample}")
def test_factors_one_with_hue_off_equal_the_plain_train_tiles(case):
    geo, ras, ja, jb, aug, recs, bev = _case_run(case)
    ident = [[jc.IDENTITY._replace(order=r.order) for r in row] for row in recs]
    shape = (case.batch, geo.crop, geo.crop, case.out_c)
    for fmt, dt in ((_lib.TILE_F32_NHWC, np.float32), (_lib.TILE_BF16_NHWC, np.uint16)):
        got, plain = _dev(tc.blank(shape, dt)), _dev(tc.blank(shape, dt))
        _ok(_jitter(ras, bev, bev, ja, jb, case.per_sample, aug, case.batch, got, fmt, case.out_c, _records(ident), _workspace(ras, case.batch, case.per_sample)), ras)
        _ok(_plain(ras, bev, bev, ja, jb, case.per_sample, aug, case.batch, plain, fmt, case.out_c), ras)
        _same(got, plain.cpu().numpy(), f"identity {case} fmt {fmt}")
    ras.check(str(case))


@pytest.mark.parametrize("run", ["colour", "contrast"])
def test_the_colour_lattice_equals_the_emulator(run):
    """Every triple of the levels 0..63 and 192..255 at identity resize, crop = resize = 256 (the largest accepted): 16 samples of two
    images.  "colour": saturation, hue and brightness at the interval ends; "contrast": contrast first, over the whole 65536-pixel image."""
    side, n = jc.LATTICE_SIDE, jc.LATTICE_IMAGES
    ras = _ras(side, side, side, side)
    bev = _dev(tc.pack(jc.lattice()))
    B = n // 2
    smp = np.arange(B)
    ja, jb = ras.upload_tile_jobs(2 * smp, smp, np.zeros(B, dtype=np.int64)), ras.upload_tile_jobs(2 * smp + 1, smp, np.full(B, 3))
    recs = [[jc.lattice_record(2 * s, run), jc.lattice_record(2 * s + 1, run)] for s in range(B)]
    out = _dev(tc.blank((B, side, side, 8), np.float32))
    _ok(_jitter(ras, bev, bev, ja, jb, 1, _aug([(0, 0, 0)] * B), B, out, _lib.TILE_F32_NHWC, 8, _records(recs), _workspace(ras, B, 1)), ras)
    got = out.cpu().numpy()
    ras.check(run)
    assert not got[..., 6:].any()
    table = tc.lut()
    for lo in range(0, n, 8):   # (eight images at a time: the emulator's temporaries stay small)
        want = tc.normalised(jc.lattice_expected(run, lo, 8), table)
        for i in range(lo, lo + 8):
            _same(got[i // 2, ..., 3 * (i % 2):3 * (i % 2) + 3], want[i - lo], f"lattice {run}, image {i}, record {jc.lattice_record(i, run)}")


# ---------------------------------------------------------------------------------------------------- refusals and the device-side check
def test_host_refusals_return_their_code_and_write_nothing():
    case = jc.JCase(jc.G_A.id, 9, 2, 16)
    geo, ras, ja, jb, aug, recs, bev = _case_run(case)
    jit, ws = _records(recs), _workspace(ras, 9, 2)
    out = _dev(tc.blank((9, geo.crop, geo.crop, 16), np.float32))
    call = lambda **kw: _jitter(ras, bev, bev, ja, jb, 2, aug, 9, out, _lib.TILE_F32_NHWC, 16, jit, ws, **kw)
    assert call(resize=257, crop=geo.crop) == -2 and "2^24" in ras.lib.salve_last_error().decode()          # SALVE_ERR_UNSUPPORTED
    assert call(ws=P(None)) == -1 and call(jit=P(None)) == -1                                                # SALVE_ERR_BAD_ARG
    assert call(ws_bytes=9 * 4 * 4 - 1) == -4                                                                # SALVE_ERR_WORKSPACE
    assert call(crop=geo.resize + 1) == -1                                                                   # salve_bev_train_tiles' own
    assert _jitter(ras, bev, bev, ja, jb, 4, aug, 9, out, _lib.TILE_F32_NHWC, 24, jit, ws) == -1
    assert _jitter(ras, bev, bev, ja, jb, 2, aug, 9, out, 1, 16, jit, ws) == -1
    assert _jitter(ras, bev, bev, ja, jb, 2, aug, 0, out, _lib.TILE_F32_NHWC, 16, None, None) == _lib.SALVE_OK   # an empty batch: nothing to do
    torch.cuda.synchronize()
    _same(out, tc.blank((9, geo.crop, geo.crop, 16), np.float32), "a refused call wrote")
    assert bool((ws == 0x5A).all())
    ras.check("refusals")


@pytest.mark.parametrize("what", ["order", "order-range", "mask", "nan", "inf-complement", "chan"])
def test_a_bad_record_in_the_second_group_of_eight_sets_the_status_bit_and_leaves_the_sentinel(what, expected):
    case = jc.JCase(jc.G_A.id, 9, 2, 16)
    geo, ras, ja, jb, aug, recs, bev = _case_run(case)
    ras.check("before")
    t = train_feed.jitter_table([tuple(r) for row in recs for r in row])
    row = 8 * 4 + 2                                                          # sample 8 -- the first of the second group of eight -- image 2
    if what == "order":
        t["order"][row] = (0, 1, 1, 3)
    elif what == "order-range":
        t["order"][row] = (0, 1, 2, 4)
    elif what == "mask":
        t["mask"][row] |= 16
    elif what == "nan":
        t["saturation"][row] = np.nan
    elif what == "inf-complement":
        t["contrast_c"][row] = -np.inf
    else:   # this entry's own rule: a job's channels lie inside the sample's 6 * per_sample, not only inside out_c
        j = jb.cpu().numpy().view(_lib.TILE_JOB_DTYPE).copy()
        j["chan"][8 * 2 + 1] = 12
        jb = _bytes(j)
    want = np.array(expected[case])
    want[8] = tc.blank(want[8].shape, np.float32)
    out = _dev(tc.blank(want.shape, np.float32))
    _ok(_jitter(ras, bev, bev, ja, jb, 2, aug, 9, out, _lib.TILE_F32_NHWC, 16, _bytes(t), _workspace(ras, 9, 2)), ras)
    torch.cuda.synchronize()
    assert int(status.word(DEV).item()) == _lib.STATUS_BAD_TILE_JOB
    _same(out, want, f"bad {what}")
    with pytest.raises(_lib.SalveHipError, match="train-tile job"):
        ras.check("bad record")
    ras.check("after")


# ---------------------------------------------------------------------------------------------------- the public interface
def _draw(rec):
    return tuple(rec)


def _unpacked(words: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).astype(np.uint8)


def _emulated(images_u8, jitter, draw, resize, crop):
    """float32 [crop, crop, 3 len(images)]: the emulator on one example's HWC images with one jitter draw each and the example's draw."""
    h, w = images_u8[0].shape[:2]
    geo = tc.Geo(h, w, resize, crop)
    cy, cx, hflip, vflip = draw
    flags = (tc.HFLIP if hflip else 0) | (tc.VFLIP if vflip else 0)
    tiles = []
    for im, jd in zip(images_u8, jitter):
        r = tc.resize_u8(im, tc.taps(resize, h), tc.taps(resize, w))
        tiles.append(tc.normalised(jc.crop_flip(jc.jitter_image(r, jc.Rec(*jd)), geo, (cy, cx, flags)), tc.lut()))
    return np.concatenate(tiles, -1)


@pytest.mark.parametrize("k", [2, 4, 6])
def test_transform_apply_with_jitter_equals_the_batch_entry_and_the_emulator(k):
    geo = jc.G_A
    tf = TrainTransform((geo.resize, geo.resize), (geo.crop, geo.crop), device=DEV, jitter_types=train_feed.JITTER_TYPES)
    images = [np.array(jc.images(geo)[(2 * i + 1) % jc.N_IMAGES]) for i in range(k)]
    jitter = [_draw(jc.record(40 + i)) for i in range(k)]
    tiles = tf.apply(images, 3, 2, True, False, jitter=jitter)
    status.check(DEV, "apply")
    assert len(tiles) == k and all(t.shape == (3, geo.crop, geo.crop) and t.dtype == torch.float32 for t in tiles)
    want = _emulated(images, jitter, (3, 2, True, False), geo.resize, geo.crop)
    _same(torch.cat(tiles, 0).permute(1, 2, 0).contiguous(), want, f"apply(jitter=) with {k} images")
    ras = _ras(geo.h, geo.w, geo.resize, geo.crop)                                       # the batch entry on the same example
    bev = _dev(tc.pack(np.stack(images)))
    K = k // 2
    ja = ras.upload_tile_jobs(np.arange(0, k, 2), np.zeros(K, dtype=np.int64), 3 * np.arange(0, k, 2))
    jb = ras.upload_tile_jobs(np.arange(1, k, 2), np.zeros(K, dtype=np.int64), 3 * np.arange(1, k, 2))
    out = torch.empty((1, geo.crop, geo.crop, (3 * k + 7) // 8 * 8), dtype=torch.float32, device=DEV)
    ras.train_tiles(bev, bev, ja, jb, K, _aug([(3, 2, tc.HFLIP)]), 1, out, jitter=_bytes(train_feed.jitter_table(jitter)))
    assert torch.equal(out[0, ..., :3 * k].permute(2, 0, 1), torch.cat(tiles, 0))
    torch.manual_seed(5)
    random.seed(5)
    called = tf(*images[:2])                                                              # __call__ draws both kinds itself
    torch.manual_seed(5)
    random.seed(5)
    d = tf.draw()
    again = tf.apply(images[:2], *d, jitter=[tf.draw_jitter() for _ in range(2)])
    assert all(torch.equal(a, b) for a, b in zip(called, again))
    with pytest.raises(RuntimeError, match="one jitter draw per image"):
        tf.apply(images, 0, 0, False, False, jitter=jitter[:-1])


def test_a_rendered_train_batch_equals_the_emulator_on_its_unjittered_images_and_val_never_jitters():
    N, Pn, B, seed = 8, 8, 4, 3
    panos = synthetic.make_panos(Pn, scene="box")
    rgb, depth = np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    hyp = synthetic.make_hypotheses(N, Pn)
    mods = ("floor_rgb_texture",)
    src = train_render.RenderedTrainSource(DEV, mods, batch_size=B, split="train", seed=seed, photometric="device")
    src.load_panos(rgb, depth)
    src.set_examples(hyp, np.arange(N, dtype=np.int64))
    random.seed(11)
    torch.manual_seed(12)
    x, y = next(iter(src))
    x = x.cpu().numpy()
    gen = torch.Generator()
    gen.manual_seed(seed)
    idx = train_render.plan_epoch(N, B, "train", gen)[0]
    random.seed(11)
    torch.manual_seed(12)
    draws, jitter = src.draws(B), src.jitter_draws(B)
    assert y[:, 0].cpu().tolist() == idx.tolist() and len(jitter) == 2 * B and len({j[2] for j in jitter}) == 2 * B
    jobs = src.batch_tables(idx, draws)[0]                                               # [2][B][1]: where each image lies, and its channels
    H, W = src.ras.bev_hw
    arrays = (src.bev.cpu().numpy().reshape(-1), src.ref_bev.cpu().numpy().reshape(-1))
    for k in range(B):
        images = [None, None]
        for half in range(2):
            off, chan = int(jobs["bev_offset"][half, k, 0]), int(jobs["chan"][half, k, 0])
            images[chan // 3] = _unpacked(arrays[half][off:off + H * W].reshape(H, W))
        want = _emulated(images, jitter[2 * k:2 * k + 2], draws[k], 234, 224)
        _same(x[k, ..., :6], want, f"rendered example {int(idx[k])}")
        assert not x[k, ..., 6:].any()
    status.check(DEV, "rendered")
    val = train_render.RenderedTrainSource(DEV, mods, batch_size=B, split="val", photometric="device")
    plain = train_render.RenderedTrainSource(DEV, mods, batch_size=B, split="val")
    for s in (val, plain):
        s.share_panos(src)
        s.set_examples(hyp, np.arange(N, dtype=np.int64))
    assert val.photometric is None and val.jitter_draws(B) is None
    before = torch.get_rng_state()
    assert torch.equal(next(iter(val))[0], next(iter(plain))[0]) and torch.equal(torch.get_rng_state(), before)
    with pytest.raises(ValueError, match="photometric"):
        train_render.RenderedTrainSource(DEV, mods, batch_size=B, photometric="host")
    with pytest.raises(ValueError, match="jitter draws"):
        src.batch(idx, draws, jitter=jitter[:-1])


def _config(data_root, **kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=False, resize_h=234, resize_w=234, train_h=224,
             train_w=224, apply_photometric_augmentation=True, modalities=("ceiling_rgb_texture", "floor_rgb_texture"), cfg_stem="t", num_epochs=1,
             workers=0, batch_size=2, data_root=str(data_root), layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    """tests/test_gpu_train_files.py's data set: the fixture pair as the positive example, two pairs written from it as negatives."""
    root = tmp_path_factory.mktemp("jitter_tiles") / "bev"
    src = RENDERINGS / "gt_alignment_approx" / "1208"
    for building in ("1208", "0340"):
        pos, neg = root / "gt_alignment_approx" / building, root / "incorrect_alignment" / building
        pos.mkdir(parents=True)
        neg.mkdir(parents=True)
        for f in src.glob("*.jpg"):
            shutil.copy(f, pos / f.name)
            rgb = image_io.read_rgb(str(f))
            image_io.write_jpeg(str(neg / f.name.replace("pair_58", "pair_3")), rgb[::-1].copy())
            image_io.write_jpeg(str(neg / f.name.replace("pair_58", "pair_7")), rgb[:, ::-1].copy())
    return root


def test_a_tile_file_train_batch_equals_the_emulator_and_the_dataloader_path(data_root):
    args = _config(data_root)
    with pytest.raises(RuntimeError, match="photometric"):
        training.get_tile_file_source(args, "train")
    idx = np.array([2, 0])
    draws = [(0, 10, False, True), (7, 3, True, False)]
    with training.get_tile_file_source(args, "train", photometric="device") as src, \
            training.get_tile_file_source(args, "train", photometric="device", read_ahead=True) as ahead, \
            training.get_tile_file_source(args, "val", photometric="device") as val:
        assert src.photometric == "device" and val.photometric is None and val.jitter_draws(2) is None and src.images_per_example == 4
        torch.manual_seed(21)
        jitter = src.jitter_draws(2)
        x, y = src.batch(idx, draws, jitter)
        images, position = src._load(src._paths(idx))                                     # the decoded, unjittered images of the batch
        decoded = images.cpu().numpy()
        for k in range(2):
            ims = [_unpacked(decoded[int(position[4 * k + j])]) for j in range(4)]
            _same(x[k, ..., :12].contiguous(), _emulated(ims, jitter[4 * k:4 * k + 4], draws[k], 234, 224), f"tile-file example {int(idx[k])}")
        assert not bool(x[..., 12:].any()) and y[:, 0].cpu().tolist() == [int(src.data_list[int(i)][-1]) for i in idx]
        tf = training.get_train_transform(args, photometric="device")                     # the DataLoader path's transform on the same files
        assert isinstance(tf, TrainTransform) and tf.jitter_types == train_feed.JITTER_TYPES
        for k, i in enumerate(idx):
            *paths, _ = src.data_list[int(i)]
            tiles = tf.apply(tuple(image_io.read_rgb(p) for p in paths), *draws[k], jitter=jitter[4 * k:4 * k + 4])
            assert torch.equal(torch.cat(tiles, 0).permute(1, 2, 0), x[k, ..., :12]), int(i)
        epochs = []                                                                       # a whole epoch, read ahead or not: the same batches
        for source in (src, ahead):
            random.seed(4)
            torch.manual_seed(4)
            source.gen.manual_seed(9)
            epochs.append([b[0].clone() for b in source])
        assert len(epochs[0]) == len(epochs[1]) == 1 and torch.equal(epochs[0][0], epochs[1][0])
        torch.manual_seed(5)                                                              # ... and other jitter draws give another batch
        src.gen.manual_seed(9)
        random.seed(4)
        assert not torch.equal(list(src)[0][0], epochs[0][0])
    off = _config(data_root, apply_photometric_augmentation=False)                        # the keyword only permits: the field decides
    with training.get_tile_file_source(off, "train", photometric="device") as plain:
        assert plain.photometric is None and plain.tf.jitter_types is None
    data = ZindData(split="val", transform=None, args=args)
    with TileFileLoader(DEV, data.data_list, 2, (234, 234), (224, 224), photometric="device") as ev, \
            TileFileLoader(DEV, data.data_list, 2, (234, 234), (224, 224)) as ev0:
        assert all(torch.equal(a[0], b[0]) for a, b in zip(ev, ev0))
    status.check(DEV, "tile files")


def test_one_tiny_epoch_trains_with_the_keyword_from_the_dataloader_and_from_device_decoded_files(data_root, tmp_path):
    args = _config(data_root, batch_size=3)   # one train batch (building 1208) and one val batch (0340) of three examples
    with pytest.raises(RuntimeError, match="photometric"):
        training.train(args, str(tmp_path / "refused"))
    for decode in ("host", "device"):
        res = training.train(args, str(tmp_path / decode), decode=decode, photometric="device")
        assert len(res["train_avg_loss"]) == 1 and np.isfinite(res["train_avg_loss"][0])
