"""Training on the MI355X: the fp32 training convolutions against torch CPU float64, their determinism, a whole training step
against a float64 autograd restatement, a model that learns, the train transform and `python -m salve_amd.train` end to end."""

import json
import os
import random
import shutil
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from oracle import bev_oracle as bo  # noqa: E402
from salve_amd import training, train_utils  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.resnet_factory import RESNET_SPECS  # noqa: E402
from salve_amd.models.trainable import Conv2dF32Function, TrainableEarlyFusionCEResnet  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
RENDERINGS = ROOT / "tests" / "golden" / "renderings"
DEV = torch.device("cuda:0")


def rel(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def conv_shapes(layers: int, hw: int = 224):
    """(Cin, Cout, k, stride, H_in) of every convolution of the trunk (v1.5), the stem excluded."""
    kind, blocks = RESNET_SPECS[layers]
    exp = 4 if kind == "bottleneck" else 1
    out, h, inpl = set(), hw // 4, 64
    for si, (planes, n) in enumerate(zip([64, 128, 256, 512], blocks)):
        for bi in range(n):
            s = 2 if (bi == 0 and si > 0) else 1
            if kind == "bottleneck":
                out |= {(inpl, planes, 1, 1, h), (planes, planes, 3, s, h), (planes, planes * 4, 1, 1, h // s)}
            else:
                out |= {(inpl, planes, 3, s, h), (planes, planes, 3, 1, h // s)}
            if bi == 0 and (s != 1 or inpl != planes * exp):
                out.add((inpl, planes * exp, 1, s, h))
            inpl, h = planes * exp, h // s
    return out


SHAPES = sorted(conv_shapes(18) | conv_shapes(50) | conv_shapes(152)) + [(c, 64, 7, 2, 224) for c in (6, 12, 18)]


@pytest.mark.parametrize("cin,cout,k,s,h", SHAPES, ids=[f"{c}-{o}-k{k}s{s}-{h}" for c, o, k, s, h in SHAPES])
def test_conv_parity_against_float64(cin, cout, k, s, h):
    g = torch.Generator().manual_seed(cin * 7 + cout + k * 13 + s + h)
    x = torch.randn(2, cin, h, h, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5
    pad = k // 2
    y64 = F.conv2d(x, w, stride=s, padding=pad)
    gy = torch.randn(y64.shape, generator=g, dtype=torch.float64)
    x32, w32, gy32 = x.float(), w.float(), gy.float()
    ref = {"fwd": y64, "wgrad": torch.nn.grad.conv2d_weight(x, w.shape, gy, stride=s, padding=pad)}
    cpu32 = {"fwd": F.conv2d(x32, w32, stride=s, padding=pad), "wgrad": torch.nn.grad.conv2d_weight(x32, w.shape, gy32, stride=s, padding=pad)}
    stem = k == 7
    if not stem:
        ref["dgrad"] = torch.nn.grad.conv2d_input(x.shape, w, gy, stride=s, padding=pad)
        cpu32["dgrad"] = torch.nn.grad.conv2d_input(x.shape, w32, gy32, stride=s, padding=pad)
    xg = x32.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(not stem)
    wg = w32.to(DEV).requires_grad_(True)
    y = Conv2dF32Function.apply(xg, wg, s, pad)
    y.backward(gy32.to(DEV).contiguous(memory_format=torch.channels_last))
    got = {"fwd": y, "wgrad": wg.grad}
    if not stem:
        got["dgrad"] = xg.grad
    for name, r in ref.items():
        e, e32 = rel(got[name], r), rel(cpu32[name], r)
        bound = 3e-5 if name == "wgrad" else 1e-5
        print(f"{cin}->{cout} k{k}/s{s} @{h} {name}: HIP {e:.2e}  torch-CPU-fp32 {e32:.2e}")
        assert got[name].shape == r.shape and e <= bound, (name, e, e32)


def test_wgrad_and_dgrad_are_deterministic():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 64, 56, 56, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(DEV)
    gy = torch.randn(8, 128, 28, 28, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        Conv2dF32Function.apply(xr, wr, 2, 1).backward(gy)
        outs.append((xr.grad.clone(), wr.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------- whole training step
def ref_forward(p, bufs, layers, x, eps=1e-5, momentum=0.1):
    """Float64 (or fp32) CPU autograd restatement of salve/models/early_fusion.py:41-83 in train mode, torchvision's blocks."""
    def bn(t, name):
        return F.batch_norm(t, bufs[name + ".running_mean"], bufs[name + ".running_var"], p[name + ".weight"], p[name + ".bias"],
                            True, momentum, eps)

    kind, blocks = RESNET_SPECS[layers]
    t = F.relu(bn(F.conv2d(x, p["conv1.weight"], stride=2, padding=3), "resnet.bn1"))
    t = F.max_pool2d(t, 3, 2, 1)
    for si, n in enumerate(blocks):
        for bi in range(n):
            pre = f"resnet.layer{si + 1}.{bi}"
            s = 2 if (bi == 0 and si > 0) else 1
            if kind == "bottleneck":
                o = F.relu(bn(F.conv2d(t, p[pre + ".conv1.weight"]), pre + ".bn1"))
                o = F.relu(bn(F.conv2d(o, p[pre + ".conv2.weight"], stride=s, padding=1), pre + ".bn2"))
                o = bn(F.conv2d(o, p[pre + ".conv3.weight"]), pre + ".bn3")
            else:
                o = F.relu(bn(F.conv2d(t, p[pre + ".conv1.weight"], stride=s, padding=1), pre + ".bn1"))
                o = bn(F.conv2d(o, p[pre + ".conv2.weight"], padding=1), pre + ".bn2")
            idt = t
            if pre + ".downsample.0.weight" in p:
                idt = bn(F.conv2d(t, p[pre + ".downsample.0.weight"], stride=s), pre + ".downsample.1")
            t = F.relu(o + idt)
    return F.linear(torch.flatten(F.adaptive_avg_pool2d(t, 1), 1), p["fc.weight"], p["fc.bias"])


MODS = {1: ["floor_rgb_texture"], 2: ["ceiling_rgb_texture", "floor_rgb_texture"]}


@pytest.mark.parametrize("layers,n_mod", [(18, 1), (50, 2)])
def test_training_step_against_float64(layers, n_mod):
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[n_mod]))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(4, 3, 112, 112, generator=g) for _ in range(2 * n_mod)]
    y = torch.tensor([0, 1, 1, 0])
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    logits = model(*[x.to(DEV) for x in xs])
    loss = F.cross_entropy(logits, y.to(DEV))
    loss.backward()

    names = [k for k, _ in model.named_parameters()]
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: sd0[k].to(dt).clone().requires_grad_(True) for k in names}
        bufs = {k: v.to(dt).clone() for k, v in sd0.items() if k not in p}
        lg = ref_forward(p, bufs, layers, torch.cat(xs, 1).to(dt))
        ls = F.cross_entropy(lg, y)
        ls.backward()
        res[dt] = (lg.detach(), ls.detach(), {k: p[k].grad for k in names}, bufs, None)
    opt.step()
    # One Adam step from the GPU's own gradients (checked above) on CPU, in float64 and in fp32.  Adam's first step is about
    # -lr * sign(g): fed with the float64 gradients it would flip with the sign of every gradient component near zero, which says
    # nothing about the optimiser step.
    params = dict(model.named_parameters())
    for dt in (torch.float64, torch.float32):
        p = {k: sd0[k].to(dt).clone().requires_grad_(True) for k in names}
        for k in names:
            p[k].grad = None if params[k].grad is None else params[k].grad.detach().cpu().to(dt)
        torch.optim.Adam([p[k] for k in names], lr=1e-3, weight_decay=1e-4).step()
        res[dt] = res[dt][:4] + ({k: p[k].detach() for k in names},)
    (lg64, ls64, g64, b64, p64), (lg32, ls32, g32, b32, p32) = res[torch.float64], res[torch.float32]

    def check(what, got, r64, r32):
        e, e32 = rel(got, r64), rel(r32, r64)
        assert e <= max(10 * e32, 1e-5), (what, e, e32)

    check("logits", logits.detach(), lg64, lg32)
    check("loss", loss.detach().reshape(1), ls64.reshape(1), ls32.reshape(1))
    for k in names:
        if g64[k] is None:   # the trunk's own conv1 / fc: in the state dict, unused by the forward (early_fusion.py:66-81)
            assert params[k].grad is None, k
        else:
            check(f"grad {k}", params[k].grad, g64[k], g32[k])
        check(f"adam {k}", params[k].detach(), p64[k], p32[k])
    sd = model.state_dict()
    for k in b64:
        if "running" in k:
            check(k, sd[k], b64[k], b32[k])


def test_resnet18_learns_a_fixed_batch():
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(8, 3, 112, 112, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1, 0, 1, 1, 0, 0, 1]).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(40):
        probs, loss = training.cross_entropy_forward(model, "train", xs[0], xs[1], None, None, None, None, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        probs, loss = training.cross_entropy_forward(model, "train", xs[0], xs[1], None, None, None, None, y)
    acc = float((probs.argmax(1) == y).float().mean())
    print(f"loss after 40 steps {loss.item():.4f}, accuracy {acc}")
    assert loss.item() < 0.1 and acc == 1.0


# ---------------------------------------------------------------------------------------------------- train transform
def config(data_root="", modalities=("ceiling_rgb_texture", "floor_rgb_texture"), **kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
             train_w=224, apply_photometric_augmentation=False, modalities=tuple(modalities), cfg_stem="t", num_epochs=2,
             workers=0, batch_size=2, data_root=data_root, layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


def _fixture_images():
    files = sorted((RENDERINGS / "gt_alignment_approx" / "1208").glob("*.jpg"))
    return [image_io.read_rgb(str(f)) for f in files]


def test_train_transform_bit_exact_against_numpy():
    imgs = _fixture_images()
    tf = training.get_train_transform(config())
    mean, std = bo.imagenet_mean_std()
    resized = [bo.resize_linear_u8(im, (234, 234)) for im in imgs]
    for seed in range(6):
        random.seed(seed)
        out = tf(*imgs)
        random.seed(seed)
        h_off, w_off = random.randint(0, 10), random.randint(0, 10)
        hflip, vflip = random.random() < 0.5, random.random() < 0.5
        for r, t in zip(resized, out):
            c = r[h_off:h_off + 224, w_off:w_off + 224]
            if hflip:
                c = c[:, ::-1]
            if vflip:
                c = c[::-1]
            e = c.transpose(2, 0, 1).astype(np.float32)
            for ch in range(3):
                e[ch] = (e[ch] - np.float32(mean[ch])) / np.float32(std[ch])
            assert np.array_equal(t.cpu().numpy(), e), (seed, h_off, w_off, hflip, vflip)
    centre = tf.apply(imgs, 5, 5, False, False)
    val = train_utils.get_val_test_transform(config())(*imgs)
    assert all(torch.equal(a, b) for a, b in zip(centre, val))


# ---------------------------------------------------------------------------------------------------- end to end
def test_train_cli_end_to_end(tmp_path):
    root = tmp_path / "bev"
    src = RENDERINGS / "gt_alignment_approx" / "1208"
    for building in ("1208", "0340"):   # 1208: train split; 0340: val split
        pos, neg = root / "gt_alignment_approx" / building, root / "incorrect_alignment" / building
        pos.mkdir(parents=True)
        neg.mkdir(parents=True)
        for f in src.glob("*.jpg"):
            shutil.copy(f, pos / f.name)
            image_io.write_jpeg(str(neg / f.name.replace("pair_58", "pair_3")), image_io.read_rgb(str(f))[::-1].copy())
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    _target_: salve.training_config.TrainingConfig\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n"
                   "    weight_decay: 0.0001\n    num_ce_classes: 2\n    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n"
                   "    num_layers: 18\n    pretrained: False\n    dataparallel: True\n    resize_h: 234\n    resize_w: 234\n    train_h: 224\n"
                   "    train_w: 224\n    apply_photometric_augmentation: False\n    modalities: [\"ceiling_rgb_texture\", \"floor_rgb_texture\"]\n"
                   "    cfg_stem: e2e\n    num_epochs: 50\n    workers: 15\n    batch_size: 256\n    data_root: /nonexistent\n    layout_data_root:\n"
                   f"    model_save_dirpath: {tmp_path / 'models'}\n    gpu_ids:\n")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--epochs", "2", "--batch-size", "2",
                        "--data-root", str(root), "--seed", "0", "--out", str(out)], cwd=str(ROOT), capture_output=True, text=True,
                       timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"}
    assert ck["max_epochs"] == 2
    res = json.loads((out / "results-e2e.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 2 for v in res.values())

    args = config(str(root))
    inf = EarlyFusionCEResnet(18, False, 2, args)
    train_utils.load_model_checkpoint(str(out / "train_ckpt.pth"), inf, args)
    inf = inf.to(DEV).eval().set_precision("fp32")
    tr = TrainableEarlyFusionCEResnet(18, False, 2, args)
    tr.load_state_dict(ck["state_dict"], strict=True)
    tr = tr.to(DEV).eval()
    xs = list(train_utils.get_val_test_transform(args)(*_fixture_images()))
    xs = [torch.stack([x, x.flip(1)]) for x in xs]
    with torch.no_grad():
        a = inf(*xs, None, None)
        b = tr(*xs, None, None)
    bound = 1e-4 * max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= bound, (a, b)
