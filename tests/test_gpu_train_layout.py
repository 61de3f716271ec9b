"""The layout modality of the rendered training feed on the MI355X: salve_layout_pose against `pack_layouts`' tables and the images
drawn from them, its bad-record handling and refusals, RenderedTrainSource (layout alone and ceiling + floor + layout) against
rasterise / render -> export -> TrainTransform, the identity modes and the resident pool, forward_packed on 24 channels, a model that
learns from layout batches, and `python -m salve_amd.train --render-from` end to end.  Every comparison is torch.equal."""

import ctypes
import functools
import json
import os
import random
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import layout_cases as lc  # noqa: E402
from salve_amd import _lib, layout, status, synthetic, synthetic_layouts, train_render, training  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet, _nhwc, _pad8  # noqa: E402
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from salve_amd.transforms import TrainTransform, ValTestTransform  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")
LAYOUT, ALL3 = ["layout"], ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]
RESIZE, CROP = 234, 224


def _device_tables(dl: layout.DeviceLayouts, n: int):
    """The tables salve_layout_pose left on the device, cut to what the records name (in `pack_layouts`' conventions)."""
    rec = dl.rec.cpu().numpy().view(_lib.LAYOUT_DTYPE)[:n].copy()
    n_poly, n_seg = int(rec["n_poly"].sum()), int(rec["n_seg"].sum())
    poly, seg = dl.poly.cpu().numpy()[:n_poly], dl.seg.cpu().numpy()[:n_seg]
    return rec, poly if n else np.zeros((1, 2), np.int32), seg if n_seg else np.zeros((1, 8), np.int32)


# ---------------------------------------------------------------------------------------------------- 1. the kernel
def test_layout_pose_tables_and_images_equal_the_host_path():
    status.check(DEV, "before the layout tests")
    case = lc.seeded_set()
    pl, n = case[0], len(case[1])
    dl = layout.DeviceLayouts(pl, DEV, n)
    recs = layout.pose_records(*case)
    out = torch.full((n, 501, 501), -1, dtype=torch.int32, device=DEV)
    dl.draw(recs, out)
    status.check(DEV, "layout pose + rasterise")
    got = _device_tables(dl, n)
    want = lc.seeded_host_tables()
    for name, a, b in zip(("records", "poly_xy", "segs"), want, got):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if not np.array_equal(a, b):   # a half-pixel tie of a fused multiply-add would show here: name the coordinate, do not loosen
            at = np.argwhere(a.view(np.int32).reshape(len(a), -1) != b.view(np.int32).reshape(len(b), -1))[:5]
            raise AssertionError(f"{name} differ at {at.tolist()}")
    assert lc.tables_equal(want, got)
    images = layout.rasterise_layouts(lc.host_specs(*case), DEV)
    assert torch.equal(out, images)
    assert bool((out[0] == 0).all()) and bool((out[lc.N + 1] == 0).all()) and bool((out[1] == 0x00ffffff).any())   # the empty room, posed and own


@pytest.mark.parametrize("window", list(lc.WINDOWS))
def test_strided_pose_tables_equal_the_host_paths(window):
    """Rooms of up to 200 vertices and 70 W/D/Os: the second and later passes of the kernel's 64-thread loops."""
    case = lc.strided_set()
    pl, n = case[0], len(case[1])
    bp = lc.window_params(window)
    dl = layout.DeviceLayouts(pl, DEV, n, bev_params=bp)
    dl.pose(torch.from_numpy(layout.pose_records(*case).view(np.uint8)).to(DEV), n)
    status.check(DEV, "strided layout pose")
    got = _device_tables(dl, n)
    for name, want in (("pose_layouts_numpy", layout.pose_layouts_numpy(*case, bev_params=bp)), ("pack_layout_tables", lc.strided_host_tables(window))):
        for tab, a, b in zip(("records", "poly_xy", "segs"), want, got):
            assert a.dtype == b.dtype and a.shape == b.shape, (name, tab)
            if not np.array_equal(a, b):
                at = np.argwhere(a.view(np.int32).reshape(len(a), -1) != b.view(np.int32).reshape(len(b), -1))[:5]
                raise AssertionError(f"{tab} differ from {name} at {at.tolist()}")
        assert lc.tables_equal(want, got), name


@pytest.mark.parametrize("window", list(lc.WINDOWS))
def test_strided_pose_images_equal_the_host_path(window):
    """The same set drawn: 70 segments are ten chunks of the rasteriser, in a square and a non-square window."""
    case = lc.strided_set()
    pl, n = case[0], len(case[1])
    bp = lc.window_params(window)
    dl = layout.DeviceLayouts(pl, DEV, n, bev_params=bp)
    out = torch.full((n, *dl.hw), -1, dtype=torch.int32, device=DEV)
    dl.draw(layout.pose_records(*case), out)
    status.check(DEV, "strided layout pose + rasterise")
    images = layout.rasterise_layouts(lc.host_specs(*case), DEV, bev_params=bp)
    status.check(DEV, "strided layouts through the host path")
    assert tuple(images.shape) == (n, *dl.hw) == ((n, 501, 501) if bp is None else (n, 45, 83))
    assert torch.equal(out, images)
    assert all(bool((out[k] != 0).any()) for k in range(n) if int(pl.wdo_count[case[1][k]]) > 0)


def test_layout_pose_half_pixel_ties_round_to_even():
    case = lc.half_pixel_set()
    dl = layout.DeviceLayouts(case[0], DEV, 2)
    dl.pose(torch.from_numpy(layout.pose_records(*case).view(np.uint8)).to(DEV), 2)
    status.check(DEV, "half-pixel ties")
    got = _device_tables(dl, 2)
    assert lc.tables_equal(layout.pack_layout_tables(lc.host_specs(case[0], case[1], None, None, None, case[5])), got)
    assert not lc.tables_equal(lc.emulate("round half away", *case), got)


def test_bad_layout_record_sets_the_status_bit_and_empties_only_that_image():
    pl, pano, R, t, s, posed = lc.seeded_set()
    n = 6
    good = layout.pose_records(pl, pano[10:10 + n], R[10:10 + n], t[10:10 + n], s[10:10 + n], posed[10:10 + n])
    dl = layout.DeviceLayouts(pl, DEV, n)
    ref = dl.draw(good, torch.zeros((n, 501, 501), dtype=torch.int32, device=DEV)).clone()
    ref_tabs = _device_tables(dl, n)
    status.check(DEV, "good records")
    assert all(bool((ref[k] != 0).any()) for k in range(n))
    far = np.float32(4.0e6)   # metres: x 1.5 x 50 lies beyond 2^24 pixels
    for field, value in (("pano", pl.P), ("pano", -1), ("poly_off", dl.poly_cap - 1), ("seg_off", -1), ("seg_off", dl.seg_cap + 1), ("t", far), ("s", np.nan)):
        recs = good.copy()
        recs[field][3] = value
        out = dl.draw(recs, torch.full((n, 501, 501), 7, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert int(status.word(DEV).item()) == _lib.STATUS_BAD_LAYOUT, (field, value)
        rec = dl.rec.cpu().numpy().view(_lib.LAYOUT_DTYPE)[:n]
        assert rec["n_poly"][3] == 0 and rec["n_seg"][3] == 0, (field, value)
        assert bool((out[3] == 0).all())                                                   # that image: empty
        keep = [k for k in range(n) if k != 3]
        assert torch.equal(out[keep], ref[keep]), (field, value)                           # the neighbours: as they were
        assert np.array_equal(rec[keep], ref_tabs[0][keep])
        with pytest.raises(_lib.SalveHipError, match="layout image"):
            status.check(DEV, "bad record")
        assert int(status.word(DEV).item()) == 0                                           # (check() reset the word)


def test_layout_pose_host_refusals():
    pl = lc.seeded_set()[0]
    dl = layout.DeviceLayouts(pl, DEV, 4)
    recs = torch.from_numpy(layout.pose_records(pl, [0, 3, 4, 6]).view(np.uint8)).to(DEV)
    lib = _lib.load()
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(**kw):
        a = dict(room_xy=p(dl.room_xy), room_off=p(dl.room_off), wdo_xy=p(dl.wdo_xy), wdo_type=p(dl.wdo_type), wdo_off=p(dl.wdo_off), recs=p(recs), n=4,
                 n_panos=pl.P, tx=5.0, ty=5.0, scale=50.0, rec=p(dl.rec), poly=p(dl.poly), poly_cap=dl.poly_cap, seg=p(dl.seg), seg_cap=dl.seg_cap)
        a.update(kw)
        return lib.salve_layout_pose(a["room_xy"], a["room_off"], len(pl.room_xy), a["wdo_xy"], a["wdo_type"], a["wdo_off"], len(pl.wdo_xy), a["n_panos"],
                                     a["recs"], a["n"], a["tx"], a["ty"], a["scale"], 8, a["rec"], a["poly"], a["poly_cap"], a["seg"], a["seg_cap"],
                                     status.ptr(DEV), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))

    for kw in (dict(room_xy=None), dict(room_off=None), dict(wdo_xy=None), dict(wdo_type=None), dict(wdo_off=None), dict(recs=None), dict(rec=None),
               dict(poly=None), dict(seg=None), dict(n=-1), dict(n=65536), dict(poly_cap=0), dict(seg_cap=-3), dict(tx=float("nan")),
               dict(ty=float("inf")), dict(scale=float("-inf")), dict(n_panos=0), dict(poly=ctypes.c_void_p(dl.poly.data_ptr() + 4))):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    assert call() == _lib.SALVE_OK and call(n=0) == _lib.SALVE_OK
    status.check(DEV, "refusals")
    assert int(status.word(DEV).item()) == 0


# ---------------------------------------------------------------------------------------------------- 2. the source
@functools.lru_cache(maxsize=None)
def _all_panos():
    panos = synthetic.make_panos(24, scene="box")
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])


def _panos(n: int):
    rgb, depth = _all_panos()   # (generated once: panorama k does not depend on how many there are)
    return rgb[:n], depth[:n]


def _table(n, P, seed):
    hyp = synthetic.make_hypotheses(n, P, seed=seed)
    hyp.swap = np.random.default_rng(seed).integers(0, 2, size=n).astype(bool)
    return hyp, np.arange(n, dtype=np.int64)   # (the label IS the example's index: the order shows in the labels)


@functools.lru_cache(maxsize=None)
def _reference(P: int, n: int, seed: int, textures: bool):
    """Per example its images in the MODEL's channel order as HWC uint8 arrays, composed from the shipped pieces: BevRasteriser.render
    -> export_u8 for the texture maps, layout.rasterise_layouts of `layout_pair_specs`-style specs for the layouts; the pair of a
    modality in (i1, i2) order, or (i2, i1) where the table swaps."""
    hyp, _ = _table(n, P, seed)
    pl = synthetic_layouts.make_layouts(P, seed=9)
    ras = BevRasteriser(DEV)
    specs = [pl.spec(int(hyp.i1[j]), Sim2(hyp.R[j], hyp.t[j], 1.0)) for j in range(n)] + [pl.spec(p) for p in range(P)]
    lay = ras.export_u8(layout.rasterise_layouts(specs, DEV)).cpu().numpy()
    groups = [(lay[:n, None], lay[n:, None])]
    if textures:
        rgb, depth = _panos(P)
        surf = [SURFACES[s] for s in ("ceiling", "floor")]
        rows = np.concatenate([
            pack_hypotheses(np.repeat(hyp.i1, 2), np.tile(surf, n), np.repeat(hyp.R, 2, axis=0), np.repeat(hyp.t, 2, axis=0), np.ones(n * 2)),
            pack_hypotheses(np.repeat(np.arange(P), 2), np.tile(surf, P), np.tile(np.eye(2, dtype=np.float32), (P * 2, 1, 1)),
                            np.zeros((P * 2, 2), np.float32), np.zeros(P * 2))])
        bev, _ = ras.render(*ras.upload_panos(rgb, depth), ras.upload_hypotheses(rows), (n + P) * 2)
        u8 = ras.export_u8(bev).cpu().numpy()
        groups.insert(0, (u8[:n * 2].reshape(n, 2, *u8.shape[1:]), u8[n * 2:].reshape(P, 2, *u8.shape[1:])))
    ras.check("reference images")
    out = []
    for j in range(n):
        imgs = []
        for posed, ident in groups:
            for k in range(posed.shape[1]):
                pair = (posed[j, k], ident[int(hyp.i2[j]), k])
                imgs.extend(pair[::-1] if hyp.swap[j] else pair)
        out.append(imgs)
    return out


def _source(mods, precision, split, B, seed, P, **kw):
    src = train_render.RenderedTrainSource(DEV, mods, batch_size=B, precision=precision, split=split, seed=seed,
                                           layouts=synthetic_layouts.make_layouts(P, seed=9), **kw)
    return src


def _loaded(mods, precision, split, B, seed, P, hyp, labels, **kw):
    src = _source(mods, precision, split, B, seed, P, **kw)
    rgb, depth = _panos(P) if len(mods) > 1 else (np.zeros((P, 1, 1, 3), np.uint8), np.zeros((P, 1, 1), np.uint16))   # layout alone reads no panorama
    src.load_panos(rgb, depth)
    src.set_examples(hyp, labels)
    return src


@pytest.mark.parametrize("mods", [LAYOUT, ALL3], ids=["layout", "ceiling+floor+layout"])
def test_layout_source_equals_rasterise_then_transform(mods):
    N, P, B, seed = 40, 8, 16, 3
    hyp, labels = _table(N, P, seed=5)
    assert hyp.swap.any() and not hyp.swap.all()
    images = _reference(P, N, 5, len(mods) > 1)
    C, Cp = 6 * len(mods), _pad8(6 * len(mods))
    assert Cp == (8 if mods == LAYOUT else 24)
    tf = TrainTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    src = _loaded(mods, "fp32", "train", B, seed, P, hyp, labels)
    if mods == LAYOUT:
        assert src.pano_rgb is None and src.pano_depth is None   # layout alone: no panorama on the device, no scatter / densify
    random.seed(11)
    got = [(x.clone(), y.clone()) for x, y in src]
    gen = torch.Generator()
    gen.manual_seed(seed)
    random.seed(11)
    plan = train_render.plan_epoch(N, B, "train", gen)
    assert len(got) == len(plan) == 2
    for (x, y), idx in zip(got, plan):
        draws = [tf.draw() for _ in idx]
        assert x.shape == (B, CROP, CROP, Cp) and x.dtype == torch.float32 and y[:, 0].cpu().tolist() == labels[idx].tolist()
        for k, (j, draw) in enumerate(zip(idx, draws)):
            want = torch.cat(tf.apply(images[int(j)], *draw), 0).permute(1, 2, 0)
            assert torch.equal(x[k][..., :C], want), (int(j), draw)
            assert bool((x[k][..., C:] == 0.0).all())                    # the padding channels: exactly zero
    assert any(bool((x[..., C - 6:C] != x[0, 0, 0, C - 6:C]).any()) for x, _ in got)   # (the layout channels are not blank)

    # the val split in bf16: table order, nothing dropped, ValTestTransform's tiles rounded once; the panoramas are shared
    val = _source(mods, "bf16", "val", B, seed, P)
    half = _loaded(mods, "bf16", "train", B, seed, P, hyp, labels)
    val.share_panos(half)
    val.set_examples(hyp, labels)
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    batches = list(val)
    assert [int(x.shape[0]) for x, _ in batches] == [16, 16, 8] and torch.cat([y for _, y in batches])[:, 0].cpu().tolist() == labels.tolist()
    xs = torch.cat([x for x, _ in batches])
    for j in range(N):
        want = torch.zeros((CROP, CROP, Cp), dtype=torch.float32, device=DEV)
        want[..., :C] = torch.cat(vt(*images[j]), 0).permute(1, 2, 0)
        assert torch.equal(xs[j].view(torch.int16), want.to(torch.bfloat16).view(torch.int16)), j


def _epoch(src, py_seed):
    random.seed(py_seed)
    return [(x.clone(), y.clone()) for x, y in src]


def _same(got, want):
    assert len(got) == len(want) > 0
    for k, ((x, y), (xw, yw)) in enumerate(zip(got, want)):
        assert x.dtype == xw.dtype and x.shape == xw.shape, k
        bits = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.view(bits), xw.view(bits)) and torch.equal(y, yw), k


@pytest.mark.parametrize("mods,precision", [(LAYOUT, "fp32"), (ALL3, "bf16")], ids=["layout-fp32", "ceiling+floor+layout-bf16"])
def test_identity_batch_and_resident_pool_equal_identity_kept(mods, precision):
    """24 panoramas, batches of 8: the identity layouts drawn with the batch, and a pool of 16 panorama slots (the layout tables stay
    fully resident, indexed by panorama), give the batches of the default source -- train, val on the shared buffers, train again."""
    P, pool, N, B, seed = 24, 16, 24, 8, 3
    hyp, labels = _table(N, P, seed=6)
    vhyp, vlabels = _table(11, P, seed=7)
    pairs = {}
    for name, kw in (("kept", {}), ("batch", dict(identity="batch")), ("pool", dict(identity="batch", resident_panos=pool))):
        tr = _loaded(mods, precision, "train", B, seed, P, hyp, labels, **kw)
        va = _source(mods, precision, "val", B, seed, P, **kw)
        va.share_panos(tr)
        va.set_examples(vhyp, vlabels)
        pairs[name] = (tr, va)
    assert pairs["kept"][0].ref_bev is not None and pairs["batch"][0].ref_bev is None
    for which, py_seed in ((0, 11), (1, 12), (0, 13)):
        want = _epoch(pairs["kept"][which], py_seed)
        assert len(want) == (3 if which == 0 else 2)
        _same(_epoch(pairs["batch"][which], py_seed), want)
        _same(_epoch(pairs["pool"][which], py_seed), want)
    if len(mods) > 1:
        assert pairs["pool"][0].uploads > pool and tuple(pairs["pool"][0].pano_rgb.shape[:1]) == (pool,)   # a pool that evicted
    else:
        assert pairs["pool"][0].uploads == 0 and pairs["pool"][0].pano_rgb is None                          # layout alone: nothing to hold


# ---------------------------------------------------------------------------------------------------- 3. the model
@pytest.mark.parametrize("precision,norm", [("fp32", "torch"), ("bf16", "hip")])
def test_forward_packed_on_24_channels_equals_forward(precision, norm):
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=ALL3)).to(DEV).train()
    model.set_train_precision(precision).set_train_norm(norm)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(4, 3, 96, 96, generator=g).to(DEV) for _ in range(6)]
    y = torch.tensor([0, 1, 1, 0], device=DEV)
    x = torch.cat(xs, 1)
    packed = _nhwc(x.to(torch.bfloat16) if precision == "bf16" else x, _pad8(x.shape[1]))
    assert packed.shape[3] == 24

    def run(fn):
        model.zero_grad(set_to_none=True)
        logits = fn()
        torch.nn.functional.cross_entropy(logits, y).backward()
        return logits.detach().clone(), {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}

    l1, g1 = run(lambda: model(*xs))
    l2, g2 = run(lambda: model.forward_packed(packed))
    assert torch.equal(l1, l2), (l1, l2)
    assert sum(g is not None for g in g1.values()) >= len(g1) - 4
    diff = [n for n in g1 if (g1[n] is None) != (g2[n] is None) or (g1[n] is not None and not torch.equal(g1[n], g2[n]))]
    assert not diff, diff


@pytest.mark.parametrize("precision,norm", [("bf16", "hip"), ("fp32", "torch")])
def test_resnet18_learns_a_fixed_layout_batch(precision, norm):
    """The procedure and criterion of test_resnet18_learns_a_fixed_rendered_batch (8 examples, Adam lr 1e-3, 40 steps, then loss < 0.1
    and accuracy 1.0), on ONE layout-only batch served by the source through forward_packed -- and the same 8 examples composed from
    rasterise_layouts -> ValTestTransform through the shipped `forward` from the same initial weights reach the same final loss: as
    closely as the composed path reaches its own when it is run twice (the spread is measured here, not assumed; the training path has
    been deterministic for equal batches on the MI355X, so this has meant equality)."""
    P = 8
    hyp, _ = _table(8, P, seed=1)
    labels = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int64)
    (x_packed, y), = list(_loaded(LAYOUT, precision, "val", 8, 0, P, hyp, labels))
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    pairs = [vt(*imgs) for imgs in _reference(P, 8, 1, False)]
    x1, x2 = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    def fit(step):
        torch.manual_seed(0)
        model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=LAYOUT)).to(DEV).train()
        model.set_train_precision(precision).set_train_norm(norm)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        for _ in range(40):
            probs, loss = step(model)
            opt.zero_grad()
            loss.backward()
            opt.step()
        with torch.no_grad():
            probs, loss = step(model)
        return float(loss.item()), float((probs.argmax(1) == y.squeeze()).float().mean())

    loss_p, acc_p = fit(lambda m: training.cross_entropy_forward_packed(m, "train", x_packed, y))
    composed = lambda m: training.cross_entropy_forward(m, "train", x1, x2, None, None, None, None, y)
    loss_s, acc_s = fit(composed)
    loss_again, _ = fit(composed)
    spread = abs(loss_s - loss_again)
    print(f"{precision} / {norm} after 40 steps: layout feed loss {loss_p!r} accuracy {acc_p}; composed path loss {loss_s!r} / {loss_again!r} "
          f"(spread {spread!r}) accuracy {acc_s}")
    assert loss_s < 0.1 and acc_s == 1.0
    assert loss_p < 0.1 and acc_p == 1.0
    assert abs(loss_p - loss_s) <= spread


# ---------------------------------------------------------------------------------------------------- 4. CLI
def test_train_cli_render_from_with_the_layout_modality(tmp_path):
    data = tmp_path / "panos"
    data.mkdir()
    P = 4
    np.save(data / "panos_rgb.npy", np.zeros((P, 512, 1024, 3), dtype=np.uint8))   # layout alone: the panoramas are not read
    np.save(data / "panos_depth.npy", np.zeros((P, 512, 1024), dtype=np.uint16))
    synthetic_layouts.make_layouts(P, seed=2).save(data / "layouts.npz")
    for split, n, seed in (("train", 9, 0), ("val", 4, 1)):
        h = synthetic.make_hypotheses(n, P, seed=seed)
        d = {"i1": h.i1.tolist(), "i2": h.i2.tolist(), "R": h.R.tolist(), "t": h.t.tolist(), "is_match": [k % 2 for k in range(n)]}
        if split == "train":
            d["swap"] = [bool(k % 3 == 0) for k in range(n)]
        (data / f"{split}.json").write_text(json.dumps(d))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    _target_: salve.training_config.TrainingConfig\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n"
                   "    weight_decay: 0.0001\n    num_ce_classes: 2\n    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n"
                   "    num_layers: 18\n    pretrained: False\n    dataparallel: True\n    resize_h: 234\n    resize_w: 234\n    train_h: 224\n"
                   "    train_w: 224\n    apply_photometric_augmentation: False\n    modalities: [\"layout\"]\n"
                   "    cfg_stem: lay\n    num_epochs: 50\n    workers: 15\n    batch_size: 4\n    data_root: /nonexistent\n    layout_data_root:\n"
                   f"    model_save_dirpath: {tmp_path / 'models'}\n    gpu_ids:\n")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--render-from", str(data), "--epochs", "1",
                        "--precision", "bf16", "--norm", "hip", "--out", str(out)], cwd=str(ROOT), capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"} and ck["max_epochs"] == 1
    res = json.loads((out / "results-lay.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 1 for v in res.values())
    args = TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=tuple(LAYOUT), cfg_stem="lay", num_epochs=1, workers=0,
                          batch_size=4, data_root="", layout_data_root="", model_save_dirpath="")
    inf = EarlyFusionCEResnet(18, False, 2, args)
    inf.load_state_dict(ck["state_dict"], strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in ck["state_dict"].values() if v.is_floating_point())
    # without layouts.npz the same command ends with one line
    (data / "layouts.npz").unlink()
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--render-from", str(data), "--epochs", "1", "--out", str(out)],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and "Traceback" not in r.stderr and "layouts.npz is missing" in lines[-1]
