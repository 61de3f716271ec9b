"""Training on the host (CPU): the training ABI symbols, the trainable model's parameter names, the train transform's draws,
the poly schedule's update order and the optimiser / CPU refusals."""

import random
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from salve_amd import _lib, training
from salve_amd.models.early_fusion import EarlyFusionCEResnet
from salve_amd.models.trainable import Conv2dF32Function, TrainableEarlyFusionCEResnet
from salve_amd.training_config import TrainingConfig
from salve_amd.transforms import TrainTransform

ROOT = Path(__file__).resolve().parents[1]
TRAIN_SYMBOLS = ("salve_conv_f32_workspace_bytes", "salve_conv_f32_forward", "salve_conv_f32_backward_data",
                 "salve_conv_f32_backward_weight", "salve_bev_tiles_aug")
MODALITIES = {2: ["floor_rgb_texture"], 4: ["ceiling_rgb_texture", "floor_rgb_texture"],
              6: ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]}


def config(**kw) -> TrainingConfig:
    d = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
             optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
             train_w=224, apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="t", num_epochs=2,
             workers=0, batch_size=2, data_root="", layout_data_root="", model_save_dirpath="")
    d.update(kw)
    return TrainingConfig(**d)


def test_training_symbols_are_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in TRAIN_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7
    assert "#define SALVE_HIP_ABI_VERSION 7" in header


def _ws(lib, desc, p):
    return int(lib.salve_conv_f32_workspace_bytes(desc, p))


def test_conv_descriptor_refusals():
    """The workspace query is host-only: it accepts the ResNet shapes and refuses the others (and the stem's dgrad)."""
    import ctypes

    lib = _lib.load()
    ok = [(2, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1), (2, 56, 56, 128, 28, 28, 128, 3, 3, 2, 1), (2, 14, 14, 1024, 7, 7, 2048, 1, 1, 2, 0),
          (2, 7, 7, 512, 7, 7, 2048, 1, 1, 1, 0), (2, 224, 224, 16, 112, 112, 64, 7, 7, 2, 3)]
    for t in ok:
        d = ctypes.byref(_lib.ConvDesc(*t))
        assert _ws(lib, d, _lib.CONV_FWD) > 0 and _ws(lib, d, _lib.CONV_WGRAD) > 0, t
        assert (_ws(lib, d, _lib.CONV_DGRAD) > 0) == (t[7] != 7), t
    bad = [(2, 56, 56, 64, 56, 56, 64, 3, 3, 1, 0),      # 3x3 without padding
           (2, 56, 56, 64, 56, 56, 64, 5, 5, 1, 2),      # 5x5
           (2, 56, 56, 32, 56, 56, 64, 3, 3, 1, 1),      # Cin not a multiple of 64
           (2, 56, 56, 64, 56, 56, 96, 3, 3, 1, 1),      # Cout not a multiple of 64
           (2, 56, 56, 64, 55, 56, 64, 3, 3, 1, 1),      # wrong Ho
           (2, 224, 224, 12, 112, 112, 64, 7, 7, 2, 3),  # stem channels not padded to 8
           (0, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1)]      # empty batch
    for t in bad:
        d = ctypes.byref(_lib.ConvDesc(*t))
        assert _ws(lib, d, _lib.CONV_FWD) == 0 and _ws(lib, d, _lib.CONV_WGRAD) == 0, t
    assert _ws(lib, ctypes.byref(_lib.ConvDesc(*ok[0])), 3) == 0


@pytest.mark.parametrize("layers", [18, 50, 152])
@pytest.mark.parametrize("n_images", [2, 4, 6])
def test_trainable_state_dict_equals_inference_state_dict(layers, n_images):
    args = SimpleNamespace(modalities=MODALITIES[n_images])
    torch.manual_seed(0)
    inf = EarlyFusionCEResnet(layers, False, 2, args)
    tr = TrainableEarlyFusionCEResnet(layers, False, 2, args)
    assert list(inf.state_dict().keys()) == list(tr.state_dict().keys())
    assert all(a.shape == b.shape for a, b in zip(inf.state_dict().values(), tr.state_dict().values()))
    tr.load_state_dict(inf.state_dict(), strict=True)
    inf.load_state_dict(tr.state_dict(), strict=True)


def _reference_draws(rng, resize, crop):
    """A restatement of the reference's train Compose for the draws it makes: CropBase crop_type "rand" (transform.py:372-374),
    then RandomHorizontalFlip and RandomVerticalFlip (p = 0.5 each, `random.random() < self.p`)."""
    h_off = rng.randint(0, resize - crop)
    w_off = rng.randint(0, resize - crop)
    hflip = rng.random() < 0.5
    vflip = rng.random() < 0.5
    return h_off, w_off, hflip, vflip


def test_train_transform_draws_follow_the_reference_order():
    tf = training.get_train_transform(config())
    assert isinstance(tf, TrainTransform) and (tf.resize, tf.crop) == (234, 224)
    a, b = random.Random(7), random.Random(7)
    seq = [tf.draw(a) for _ in range(200)]
    assert seq == [_reference_draws(b, 234, 224) for _ in range(200)]
    assert {s[2] for s in seq} == {True, False} and {s[3] for s in seq} == {True, False}
    random.seed(3)
    x = [tf.draw() for _ in range(5)]
    random.seed(3)
    assert x == [_reference_draws(random, 234, 224) for _ in range(5)]


def test_train_transform_refusals():
    with pytest.raises(RuntimeError, match="photometric"):
        training.get_train_transform(config(apply_photometric_augmentation=True))
    with pytest.raises(RuntimeError, match="crop larger"):
        training.get_train_transform(config(train_h=240, train_w=240))


class _TinyModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))

    def forward(self, x1, *rest):
        return x1[:, :2] * 0 + self.w


def test_poly_learning_rate_sequence_matches_the_reference_order(monkeypatch):
    """run_epoch's schedule: the lr of step i is poly(current_iter of the step BEFORE it), set after optimizer.step()
    (scripts/train.py:226-243: current_iter = epoch * len + iter + 1)."""
    args = config(num_epochs=3, base_lr=0.01, poly_lr_power=0.9)
    loader = [(torch.zeros(2, 3), torch.zeros(2, 3), torch.tensor([0, 1]), ["a", "b"], ["c", "d"]) for _ in range(4)]
    model = _TinyModel()
    opt = training.get_optimizer(args, model)
    seen = []
    step = opt.step

    def spy(*a, **k):
        seen.append(opt.param_groups[0]["lr"])
        return step(*a, **k)

    monkeypatch.setattr(opt, "step", spy)
    for epoch in range(args.num_epochs):
        training.run_epoch(args, epoch, model, loader, opt, "train")
    max_iter = args.num_epochs * len(loader)
    expected = [args.base_lr] + [args.base_lr * (1 - float(i) / max_iter) ** 0.9 for i in range(1, max_iter)]
    assert seen == pytest.approx(expected, rel=0, abs=0)
    assert opt.param_groups[0]["lr"] == 0.0
    assert training.poly_learning_rate(1.0, 5, 10, 0.9) == (1 - 0.5) ** 0.9


def test_get_optimizer_is_adam_and_refuses_others():
    model = _TinyModel()
    opt = training.get_optimizer(config(base_lr=0.002, weight_decay=1e-4), model)
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 0.002 and opt.defaults["weight_decay"] == 1e-4
    with pytest.raises(RuntimeError, match="Unknown optimizer"):
        training.get_optimizer(config(optimizer_algo="sgd"), model)


def test_trainable_model_and_convolution_refuse_cpu_tensors():
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).train()
    x = torch.randn(1, 3, 224, 224)
    with pytest.raises(RuntimeError, match="HIP device"):
        model(x, x, None, None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Conv2dF32Function.apply(torch.randn(1, 64, 8, 8), torch.randn(64, 64, 3, 3), 1, 1)


def test_inference_refusals_stay():
    from salve_amd import train_utils

    with pytest.raises(RuntimeError):
        train_utils.get_img_transform_list(config(), "train")
    with pytest.raises(RuntimeError):
        train_utils.cross_entropy_forward(None, "train", None, None, None, None, None, None, None)
