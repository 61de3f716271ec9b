"""The rendered training feed on the MI355X: salve_bev_train_tiles against the shipped train transform (and numpy), its bad-job
handling, RenderedTrainSource against render -> export -> TrainTransform, forward_packed against forward, a model that learns from
rendered batches, and `python -m salve_amd.train --render-from` end to end.  Every comparison is bit-exact."""

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

from oracle import bev_oracle as bo  # noqa: E402
from salve_amd import _lib, status, synthetic, train_render, train_utils, training  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet, _nhwc, _pad8  # noqa: E402
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from salve_amd.transforms import TrainTransform, ValTestTransform  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
RENDERINGS = ROOT / "tests" / "golden" / "renderings"
DEV = torch.device("cuda:0")
FLOOR, BOTH = ["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"]
RESIZE, CROP = 234, 224
# all four flip combinations; crop offsets 0, the maximum (resize - crop = 10) and interior
DRAWS = [(0, 0, False, False), (10, 10, True, False), (3, 7, False, True), (5, 5, True, True), (10, 0, False, False), (0, 10, True, True),
         (7, 2, True, False), (1, 9, False, True)]


def _fixture_images():
    """ceiling pano 5, ceiling pano 8, floor pano 5, floor pano 8 (501 x 501, the BEV size)."""
    return [image_io.read_rgb(str(f)) for f in sorted((RENDERINGS / "gt_alignment_approx" / "1208").glob("*.jpg"))]


def _pack(imgs) -> torch.Tensor:
    s = np.stack(imgs).astype(np.uint32)
    return torch.from_numpy((s[..., 0] | (s[..., 1] << 8) | (s[..., 2] << 16)).astype(np.int32)).to(DEV)   # 0x00BBGGRR


def _aug(draws) -> torch.Tensor:
    a = np.zeros(len(draws), dtype=_lib.TILE_AUG_DTYPE)
    for k, (cy, cx, hf, vf) in enumerate(draws):
        a[k] = (cy, cx, (_lib.TILE_HFLIP if hf else 0) | (_lib.TILE_VFLIP if vf else 0), 0)
    return torch.from_numpy(a.view(np.uint8)).to(DEV)


def _kernel_case(n_surf: int, swaps):
    """The fixture pair as `batch` samples: (bev_a, bev_b, jobs_a, jobs_b, images of every sample in the model's channel order)."""
    imgs = _fixture_images()
    a_imgs, b_imgs = ([imgs[2]], [imgs[3]]) if n_surf == 1 else ([imgs[0], imgs[2]], [imgs[1], imgs[3]])   # posed pano 5 | identity pano 8
    B = len(swaps)
    si = np.tile(np.arange(n_surf), B)
    smp = np.repeat(np.arange(B), n_surf)
    sw = np.repeat(np.asarray(swaps), n_surf)
    ras = BevRasteriser(DEV)
    assert ras.bev_hw == imgs[0].shape[:2]
    jobs_a = ras.upload_tile_jobs(si, smp, 6 * si + 3 * sw)
    jobs_b = ras.upload_tile_jobs(si, smp, 6 * si + 3 * (1 - sw))
    order = []
    for s in swaps:
        order.append([im for k in range(n_surf) for im in ((b_imgs[k], a_imgs[k]) if s else (a_imgs[k], b_imgs[k]))])
    return ras, _pack(a_imgs), _pack(b_imgs), jobs_a, jobs_b, order


def _launch(ras, bev_a, bev_b, jobs_a, jobs_b, n_surf, draws, dtype, fill=float("nan")):
    out = torch.full((len(draws), CROP, CROP, _pad8(6 * n_surf)), fill, dtype=dtype, device=DEV)
    return ras.train_tiles(bev_a, bev_b, jobs_a, jobs_b, n_surf, _aug(draws), len(draws), out)


# ---------------------------------------------------------------------------------------------------- 5. kernel vs shipped transform
@pytest.mark.parametrize("swaps", [[0] * 8, [1] * 8, [0, 1, 1, 0, 1, 0, 0, 1]], ids=["i1-first", "i2-first", "mixed"])
@pytest.mark.parametrize("n_surf", [1, 2], ids=["6ch", "12ch"])
def test_train_tiles_equal_the_shipped_transform(n_surf, swaps):
    ras, bev_a, bev_b, jobs_a, jobs_b, order = _kernel_case(n_surf, swaps)
    C, Cp = 6 * n_surf, _pad8(6 * n_surf)
    f32 = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, n_surf, DRAWS, torch.float32)    # ONE launch, eight samples with different draws
    b16 = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, n_surf, DRAWS, torch.bfloat16)
    ras.check("train tiles")
    tf = TrainTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    mean, std = bo.imagenet_mean_std()
    for k, draw in enumerate(DRAWS):
        want = torch.zeros((CROP, CROP, Cp), dtype=torch.float32, device=DEV)
        want[..., :C] = torch.cat(tf.apply(order[k], *draw), 0).permute(1, 2, 0)
        assert torch.equal(f32[k], want), (k, draw)
        assert bool((f32[k][..., C:] == 0.0).all())                         # the padding channels: written, and exactly zero
        assert torch.equal(b16[k].view(torch.int16), want.to(torch.bfloat16).view(torch.int16)), (k, draw)
        # the numpy restatement of tests/test_gpu_train.py (resize_linear_u8, crop, flips, mean / std), written out again
        cy, cx, hflip, vflip = draw
        got = f32[k].cpu().numpy()
        for m, im in enumerate(order[k]):
            c = bo.resize_linear_u8(im, (RESIZE, RESIZE))[cy:cy + CROP, cx:cx + CROP]
            if hflip:
                c = c[:, ::-1]
            if vflip:
                c = c[::-1]
            e = c.astype(np.float32)
            for ch in range(3):
                e[..., ch] = (e[..., ch] - np.float32(mean[ch])) / np.float32(std[ch])
            assert np.array_equal(got[..., 3 * m:3 * m + 3], e), (k, m, draw)


def test_train_tiles_centre_draw_equals_the_val_transform():
    ras, bev_a, bev_b, jobs_a, jobs_b, order = _kernel_case(2, [0])
    out = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, 2, [(5, 5, False, False)], torch.float32)
    val = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)(*order[0])
    assert torch.equal(out[0][..., :12], torch.cat(val, 0).permute(1, 2, 0))


# ---------------------------------------------------------------------------------------------------- 6. determinism, bad jobs, refusals
def test_train_tiles_are_deterministic():
    ras, bev_a, bev_b, jobs_a, jobs_b, _ = _kernel_case(2, [0, 1, 1, 0, 1, 0, 0, 1])
    for dtype in (torch.float32, torch.bfloat16):
        one = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, 2, DRAWS, dtype)
        two = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, 2, DRAWS, dtype)
        assert torch.equal(one.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), two.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("field,value", [("chan", 16), ("chan", 15), ("chan", -3), ("slot", 0), ("bev_offset", 2 * 501 * 501), ("flags", 4)])
def test_bad_job_sets_the_status_bit_and_writes_nothing(field, value):
    """A handled argument error: the kernel range-checks the job before it forms an address, raises SALVE_STATUS_BAD_TILE_JOB and leaves
    that sample unwritten; every other sample is written as usual."""
    ras, bev_a, bev_b, jobs_a, jobs_b, _ = _kernel_case(2, [0, 1, 0, 1])
    draws = DRAWS[:4]
    good = _launch(ras, bev_a, bev_b, jobs_a, jobs_b, 2, draws, torch.float32)
    ras.check("good launch")
    aug = _aug(draws)
    if field == "flags":
        a = aug.cpu().numpy().view(_lib.TILE_AUG_DTYPE).copy()
        a["flags"][2] |= value
        aug = torch.from_numpy(a.view(np.uint8)).to(DEV)
    else:
        j = jobs_a.cpu().numpy().view(_lib.TILE_JOB_DTYPE).copy()
        j[field][2 * 2 + 1] = value   # sample 2's second job
        jobs_a = torch.from_numpy(j.view(np.uint8)).to(DEV)
    SENTINEL = 123.0
    out = torch.full((4, CROP, CROP, 16), SENTINEL, dtype=torch.float32, device=DEV)
    ras.train_tiles(bev_a, bev_b, jobs_a, jobs_b, 2, aug, 4, out)
    torch.cuda.synchronize()
    assert int(status.word(DEV).item()) == _lib.STATUS_BAD_TILE_JOB
    assert bool((out[2] == SENTINEL).all())                                    # the bad sample's slot: untouched
    assert all(torch.equal(out[k], good[k]) for k in (0, 1, 3))               # nothing outside it differs from the good launch
    with pytest.raises(_lib.SalveHipError, match="train-tile job"):
        ras.check("bad job")
    assert int(status.word(DEV).item()) == 0                                   # (check() reset the word)


def test_train_tiles_host_refusals():
    ras, bev_a, bev_b, jobs_a, jobs_b, _ = _kernel_case(2, [0])
    lib, aug = ras.lib, _aug(DRAWS[:1])
    out = torch.zeros((1, CROP, CROP, 16), dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(**kw):
        a = dict(bev_a=p(bev_a), bev_b=p(bev_b), jobs_a=p(jobs_a), aug=p(aug), out=p(out), per_sample=2, resize=RESIZE, crop=CROP,
                 fmt=_lib.TILE_F32_NHWC, out_c=16, batch=1)
        a.update(kw)
        return lib.salve_bev_train_tiles(a["bev_a"], 2, a["bev_b"], 2, 501, 501, a["jobs_a"], p(jobs_b), a["per_sample"], a["aug"], a["batch"],
                                         p(ras.coef_y), p(ras.coef_x), a["resize"], a["crop"], p(ras.lut), a["out"], a["fmt"], a["out_c"],
                                         status.ptr(DEV), ras._stream())

    for kw in (dict(bev_a=None), dict(jobs_a=None), dict(aug=None), dict(out=None), dict(crop=0), dict(resize=CROP - 1), dict(out_c=12),
               dict(out_c=8), dict(out_c=32), dict(fmt=_lib.TILE_F16_NHWC), dict(fmt=7), dict(per_sample=0), dict(per_sample=4), dict(batch=65536),
               dict(out=ctypes.c_void_p(out.data_ptr() + 4))):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    assert call() == _lib.SALVE_OK and call(batch=0) == _lib.SALVE_OK
    ras.check("refusals")


# ---------------------------------------------------------------------------------------------------- 7. source vs render-then-transform
@functools.lru_cache(maxsize=None)
def _panos(scene: str, n: int = 8):
    panos = synthetic.make_panos(n, scene=scene)
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])


def _reference_images(rgb, depth, hyp, surfaces):
    """BevRasteriser.render -> export_u8 -> host: (posed [N][S] images, identity [P][S] images) as HWC uint8 arrays."""
    ras = BevRasteriser(DEV)
    N, P, S = len(hyp), len(rgb), len(surfaces)
    surf = [SURFACES[s] for s in surfaces]
    rows = np.concatenate([
        pack_hypotheses(np.repeat(hyp.i1, S), np.tile(surf, N), np.repeat(hyp.R, S, axis=0), np.repeat(hyp.t, S, axis=0), np.ones(N * S)),
        pack_hypotheses(np.repeat(np.arange(P), S), np.tile(surf, P), np.tile(np.eye(2, dtype=np.float32), (P * S, 1, 1)),
                        np.zeros((P * S, 2), np.float32), np.zeros(P * S))])
    rgb_d, depth_d = ras.upload_panos(rgb, depth)
    bev, _ = ras.render(rgb_d, depth_d, ras.upload_hypotheses(rows), (N + P) * S)
    ras.check("reference renders")
    u8 = ras.export_u8(bev).cpu().numpy()
    return u8[:N * S].reshape(N, S, *u8.shape[1:]), u8[N * S:].reshape(P, S, *u8.shape[1:])


def _example_images(posed, ident, hyp, j, S):
    """The 2 S images of example j in the model's channel order (surface-major; (i1, i2) inside a surface: synthetic tables have no swap)."""
    return [im for k in range(S) for im in (posed[j, k], ident[int(hyp.i2[j]), k])]


@pytest.mark.parametrize("mods", [FLOOR, BOTH], ids=["floor", "ceiling+floor"])
@pytest.mark.parametrize("scene", ["box", "cluttered"])
def test_source_equals_render_then_transform(scene, mods):
    N, P, B, seed = 40, 8, 16, 3
    rgb, depth = _panos(scene)
    hyp = synthetic.make_hypotheses(N, P)
    labels = np.arange(N, dtype=np.int64)   # (the label IS the example's index: the order shows in the labels)
    S, C = len(mods), 6 * len(mods)
    posed, ident = _reference_images(rgb, depth, hyp, train_render.train_surfaces(mods))
    tf = TrainTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)

    def epoch(src_seed, py_seed):
        src = train_render.RenderedTrainSource(DEV, mods, batch_size=B, precision="fp32", split="train", seed=src_seed)
        src.load_panos(rgb, depth)
        src.set_examples(hyp, labels)
        assert len(src) == N // B
        random.seed(py_seed)
        return [(x.clone(), y.clone()) for x, y in src]

    got = epoch(seed, 11)
    gen = torch.Generator()
    gen.manual_seed(seed)
    random.seed(11)
    plan = train_render.plan_epoch(N, B, "train", gen)
    assert len(got) == len(plan) == 2
    for (x, y), idx in zip(got, plan):
        draws = [tf.draw() for _ in idx]   # one draw per example, in batch order
        assert x.shape == (B, CROP, CROP, _pad8(C)) and x.dtype == torch.float32 and y.shape == (B, 1) and y.dtype == torch.int64
        assert y[:, 0].cpu().tolist() == labels[idx].tolist()
        for k, (j, draw) in enumerate(zip(idx, draws)):
            want = torch.cat(tf.apply(_example_images(posed, ident, hyp, int(j), S), *draw), 0).permute(1, 2, 0)
            assert torch.equal(x[k][..., :C], want), (int(j), draw)
            assert bool((x[k][..., C:] == 0.0).all())
    again = epoch(seed, 11)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, again))
    other = epoch(seed + 1, 11)
    assert [y[:, 0].cpu().tolist() for _, y in other] != [y[:, 0].cpu().tolist() for _, y in got]

    # the val split: table order, nothing dropped, ValTestTransform's tiles -- in bf16: the fp32 tiles rounded once
    val = train_render.RenderedTrainSource(DEV, mods, batch_size=B, precision="bf16", split="val")
    val.load_panos(rgb, depth)
    val.set_examples(hyp, labels)
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    batches = list(val)
    assert len(val) == 3 and [int(x.shape[0]) for x, _ in batches] == [16, 16, 8]
    assert torch.cat([y for _, y in batches])[:, 0].cpu().tolist() == labels.tolist()
    xs = torch.cat([x for x, _ in batches])
    for j in range(N):
        want = torch.zeros((CROP, CROP, _pad8(C)), dtype=torch.float32, device=DEV)
        want[..., :C] = torch.cat(vt(*_example_images(posed, ident, hyp, j, S)), 0).permute(1, 2, 0)
        assert torch.equal(xs[j].view(torch.int16), want.to(torch.bfloat16).view(torch.int16)), j


def test_source_honours_swap():
    rgb, depth = _panos("box")
    hyp = synthetic.make_hypotheses(6, 8)
    hyp.swap = np.array([0, 1, 1, 0, 1, 0], dtype=bool)
    posed, ident = _reference_images(rgb, depth, hyp, ["floor"])
    src = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=6, split="val")
    src.load_panos(rgb, depth)
    src.set_examples(hyp, np.zeros(6, dtype=np.int64))
    (x, _), = list(src)
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    for j in range(6):
        a, b = vt(posed[j, 0], ident[int(hyp.i2[j]), 0])
        want = torch.cat((b, a) if hyp.swap[j] else (a, b), 0).permute(1, 2, 0)   # file-name order: RenderVerifyPipeline.prepare's rule
        assert torch.equal(x[j][..., :6], want), j


# ---------------------------------------------------------------------------------------------------- 8. model
@pytest.mark.parametrize("norm", ["torch", "hip"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layers,mods", [(18, FLOOR), (50, BOTH)], ids=["resnet18-6ch", "resnet50-12ch"])
def test_forward_packed_equals_forward(layers, mods, precision, norm):
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=mods)).to(DEV).train()
    model.set_train_precision(precision).set_train_norm(norm)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(4, 3, 96, 96, generator=g).to(DEV) for _ in range(2 * len(mods))]
    y = torch.tensor([0, 1, 1, 0], device=DEV)
    x = torch.cat(xs, 1)
    packed = _nhwc(x.to(torch.bfloat16) if precision == "bf16" else x, _pad8(x.shape[1]))   # the tensor `forward` hands its stem

    def run(fn):
        model.zero_grad(set_to_none=True)
        logits = fn()
        torch.nn.functional.cross_entropy(logits, y).backward()
        # (parameters the graph does not use -- the torchvision trunk's own stem and fc -- have no gradient on either path)
        return logits.detach().clone(), {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}

    l1, g1 = run(lambda: model(*xs))
    l2, g2 = run(lambda: model.forward_packed(packed))
    assert torch.equal(l1, l2), (l1, l2)
    assert sum(g is not None for g in g1.values()) >= len(g1) - 4
    diff = [n for n in g1 if (g1[n] is None) != (g2[n] is None) or (g1[n] is not None and not torch.equal(g1[n], g2[n]))]
    assert not diff, diff
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(*xs), model.forward_packed(packed))


# ---------------------------------------------------------------------------------------------------- 9. it learns
@pytest.mark.parametrize("precision,norm", [("bf16", "hip"), ("fp32", "torch")])
def test_resnet18_learns_a_fixed_rendered_batch(precision, norm):
    """As test_resnet18_learns_a_fixed_batch (8 examples, Adam lr 1e-3, 40 steps, then loss < 0.1 and accuracy 1.0), on ONE batch of 8
    rendered synthetic examples served by the source (split "val": no augmentation) through forward_packed -- and, as the yardstick,
    the same 8 examples as NCHW tensors (render -> ValTestTransform) through the shipped `forward` from the same initial weights."""
    rgb, depth = _panos("box")
    hyp = synthetic.make_hypotheses(8, 8, seed=1)
    labels = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int64)
    src = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=8, precision=precision, split="val")
    src.load_panos(rgb, depth)
    src.set_examples(hyp, labels)
    (x_packed, y), = list(src)
    posed, ident = _reference_images(rgb, depth, hyp, ["floor"])
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    pairs = [vt(posed[j, 0], ident[int(hyp.i2[j]), 0]) for j in range(8)]
    x1, x2 = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    def fit(step):
        torch.manual_seed(0)
        model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=FLOOR)).to(DEV).train()
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
    loss_s, acc_s = fit(lambda m: training.cross_entropy_forward(m, "train", x1, x2, None, None, None, None, y))
    print(f"{precision} / {norm} after 40 steps: forward_packed loss {loss_p:.6f} accuracy {acc_p}; shipped forward loss {loss_s:.6f} accuracy {acc_s}")
    assert loss_s < 0.1 and acc_s == 1.0
    assert loss_p < 0.1 and acc_p == 1.0


# ---------------------------------------------------------------------------------------------------- 10. CLI
def test_train_cli_render_from(tmp_path):
    data = tmp_path / "panos"
    data.mkdir()
    rgb, depth = _panos("box")
    np.save(data / "panos_rgb.npy", rgb[:4])
    np.save(data / "panos_depth.npy", depth[:4])
    for split, n, seed in (("train", 9, 0), ("val", 4, 1)):
        h = synthetic.make_hypotheses(n, 4, seed=seed)
        d = {"i1": h.i1.tolist(), "i2": h.i2.tolist(), "R": h.R.tolist(), "t": h.t.tolist(), "is_match": [k % 2 for k in range(n)]}
        if split == "train":
            d["swap"] = [bool(k % 3 == 0) for k in range(n)]
        (data / f"{split}.json").write_text(json.dumps(d))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    _target_: salve.training_config.TrainingConfig\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n"
                   "    weight_decay: 0.0001\n    num_ce_classes: 2\n    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n"
                   "    num_layers: 18\n    pretrained: False\n    dataparallel: True\n    resize_h: 234\n    resize_w: 234\n    train_h: 224\n"
                   "    train_w: 224\n    apply_photometric_augmentation: False\n    modalities: [\"ceiling_rgb_texture\", \"floor_rgb_texture\"]\n"
                   "    cfg_stem: rf\n    num_epochs: 50\n    workers: 15\n    batch_size: 4\n    data_root: /nonexistent\n    layout_data_root:\n"
                   f"    model_save_dirpath: {tmp_path / 'models'}\n    gpu_ids:\n")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--render-from", str(data), "--epochs", "1",
                        "--precision", "bf16", "--norm", "hip", "--out", str(out)], cwd=str(ROOT), capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"} and ck["max_epochs"] == 1
    res = json.loads((out / "results-rf.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 1 for v in res.values())
    args = TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=tuple(BOTH), cfg_stem="rf", num_epochs=1, workers=0,
                          batch_size=4, data_root="", layout_data_root="", model_save_dirpath="")
    inf = EarlyFusionCEResnet(18, False, 2, args)
    inf.load_state_dict(ck["state_dict"], strict=True)
    train_utils.load_model_checkpoint(str(out / "train_ckpt.pth"), inf, args)
    assert all(bool(torch.isfinite(v).all()) for v in ck["state_dict"].values() if v.is_floating_point())
