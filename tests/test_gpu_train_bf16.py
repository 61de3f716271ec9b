"""bf16 mixed-precision training on the MI355X: the bf16 training convolutions against float64 on bf16-rounded operands, their
determinism, a whole step against the fp32 step, a model that learns, and `python -m salve_amd.train --precision bf16` end to end."""

import copy
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from salve_amd import training, train_utils  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import Conv2dBF16Function, TrainableEarlyFusionCEResnet  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402
from tests.test_gpu_train import MODS, RENDERINGS, SHAPES, _fixture_images, config  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")


def bf16_round(t):
    return t.to(torch.bfloat16).double()


def rel(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def check_rounded(name, got, r, a):
    """A bf16 output rounded once from an fp32 accumulation: |got - r| <= 2^-8 |r| + 2^-20 A elementwise (A: the same
    convolution of the absolute operands), relative Frobenius error <= 3e-3."""
    got = got.detach().double().cpu()
    excess = float(((got - r).abs() - (2.0 ** -8 * r.abs() + 2.0 ** -20 * a)).max())
    e = rel(got, r)
    print(f"  {name}: rel {e:.2e}, worst elementwise margin {excess:.2e}")
    assert got.shape == r.shape
    assert excess <= 0, (name, excess)
    assert e <= 3e-3, (name, e)


@pytest.mark.parametrize("cin,cout,k,s,h", SHAPES, ids=[f"{c}-{o}-k{k}s{s}-{h}" for c, o, k, s, h in SHAPES])
def test_bf16_conv_parity_against_float64(cin, cout, k, s, h):
    g = torch.Generator().manual_seed(cin * 7 + cout + k * 13 + s + h)
    pad = k // 2
    x = bf16_round(torch.randn(2, cin, h, h, generator=g, dtype=torch.float64))
    w = bf16_round(torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5)
    ho = (h + 2 * pad - k) // s + 1
    gy = bf16_round(torch.randn(2, cout, ho, ho, generator=g, dtype=torch.float64))
    stem = k == 7
    xg = x.to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(not stem)
    wg = w.float().to(DEV).requires_grad_(True)   # the fp32 master weight holds bf16 values: its bf16 copy is exact
    y = Conv2dBF16Function.apply(xg, wg, s, pad)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(gy.to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last))
    print(f"{cin}->{cout} k{k}/s{s} @{h}")
    check_rounded("fwd", y, F.conv2d(x, w, stride=s, padding=pad), F.conv2d(x.abs(), w.abs(), stride=s, padding=pad))
    if not stem:
        assert xg.grad.dtype == torch.bfloat16
        check_rounded("dgrad", xg.grad, torch.nn.grad.conv2d_input(x.shape, w, gy, stride=s, padding=pad),
                      torch.nn.grad.conv2d_input(x.shape, w.abs(), gy.abs(), stride=s, padding=pad))
    assert wg.grad.dtype == torch.float32
    e = rel(wg.grad, torch.nn.grad.conv2d_weight(x, w.shape, gy, stride=s, padding=pad))
    print(f"  wgrad: rel {e:.2e}")
    assert wg.grad.shape == w.shape and e <= 3e-5, e


def test_bf16_passes_are_deterministic():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 64, 56, 56, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(DEV)
    gy = torch.randn(8, 128, 28, 28, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = Conv2dBF16Function.apply(xr, wr, 2, 1)
        y.backward(gy)
        outs.append((y.detach().clone(), xr.grad.clone(), wr.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


# An untrained ResNet-50's gradients are chaotic at batch 8: in fp32 alone, rounding only the INPUT to bf16 moves the flattened
# gradient to cosine 0.52 against the unrounded step, rounding only the weights to 0.39.  No bf16 step can
# meet a cosine bound there; ResNet-50 is checked for the mixed-precision contract and a loose loss bound, ResNet-18 (input
# rounding alone: cosine 0.98) for the gradient direction.
@pytest.mark.parametrize("layers,loss_bound,cos_bound", [(18, 2e-2, 0.9), (50, 5e-2, None)])
def test_bf16_step_against_fp32_step(layers, loss_bound, cos_bound):
    torch.manual_seed(0)
    m32 = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[1])).to(DEV).train()
    m16 = copy.deepcopy(m32).set_train_precision("bf16")
    stats0 = {k: v.clone() for k, v in m16.state_dict().items() if "running" in k}
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(8, 3, 224, 224, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=DEV)
    losses, grads = [], []
    for m in (m32, m16):
        logits = m(*xs)
        assert logits.dtype == torch.float32
        loss = F.cross_entropy(logits, y)
        loss.backward()
        losses.append(float(loss))
        grads.append(torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]))
    d_loss = abs(losses[1] - losses[0]) / abs(losses[0])
    cos = float(F.cosine_similarity(grads[0].double(), grads[1].double(), dim=0))
    print(f"resnet{layers}: loss fp32 {losses[0]:.6f} bf16 {losses[1]:.6f}: relative difference {d_loss:.2e}; gradient cosine {cos:.6f}")
    assert d_loss <= loss_bound, d_loss
    assert bool(torch.isfinite(grads[1]).all())
    if cos_bound is not None:
        assert cos >= cos_bound, cos
    assert all(p.dtype == torch.float32 for p in m16.parameters())
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in m16.parameters())
    sd = m16.state_dict()
    assert all(v.dtype == torch.float32 for k, v in sd.items() if "num_batches" not in k)
    assert all(not torch.equal(sd[k], v) for k, v in stats0.items()), "running statistics not updated"


def test_resnet18_learns_a_fixed_batch_in_bf16():
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).set_train_precision("bf16").to(DEV).train()
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
    print(f"bf16: loss after 40 steps {loss.item():.4f}, accuracy {acc}")
    assert loss.item() < 0.1 and acc == 1.0


def test_train_cli_bf16_end_to_end(tmp_path):
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
                        "--data-root", str(root), "--seed", "0", "--out", str(out), "--precision", "bf16"], cwd=str(ROOT),
                       capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"}
    assert all(v.dtype == torch.float32 for k, v in ck["state_dict"].items() if "num_batches" not in k)
    res = json.loads((out / "results-e2e.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 2 for v in res.values())

    args = config(str(root))
    inf = EarlyFusionCEResnet(18, False, 2, args)
    inf.load_state_dict(ck["state_dict"], strict=True)
    inf = inf.to(DEV).eval().set_precision("fp32")
    tr = TrainableEarlyFusionCEResnet(18, False, 2, args)
    tr.load_state_dict(ck["state_dict"], strict=True)
    tr = tr.to(DEV).eval()
    assert tr.train_precision == "fp32"
    xs = list(train_utils.get_val_test_transform(args)(*_fixture_images()))
    xs = [torch.stack([x, x.flip(1)]) for x in xs]
    with torch.no_grad():
        a = inf(*xs, None, None)
        b = tr(*xs, None, None)
        c = tr.set_train_precision("bf16")(*xs, None, None)
    bound = 1e-4 * max(1.0, float(b.abs().max()))
    print(f"fp32 engine vs trainable fp32 eval: {float((a - b).abs().max()):.2e} (bound {bound:.2e}); bf16 eval logits {c.tolist()}")
    assert float((a - b).abs().max()) <= bound, (a, b)
    assert c.dtype == torch.float32 and bool(torch.isfinite(c).all())
