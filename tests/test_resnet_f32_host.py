"""The fp32 verifier engine's host side (CPU): ABI symbols, the fp32 op program and its weight blob, the finiteness rules."""

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from salve_amd import _lib, synthetic
from salve_amd.models import hip_resnet
from salve_amd.models.early_fusion import EarlyFusionCEResnet

ROOT = Path(__file__).resolve().parents[1]
F32_SYMBOLS = ("salve_resnet_f32_create", "salve_resnet_f32_destroy", "salve_resnet_f32_workspace_bytes", "salve_resnet_f32_forward")


def test_f32_symbols_are_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in F32_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7


def _model(layers, modalities, seed=0):
    torch.manual_seed(seed)
    model = EarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=modalities)).eval()
    synthetic.trained_looking_batchnorm(model, seed)
    return model


@pytest.mark.parametrize("layers,modalities", [
    (18, ["floor_rgb_texture"]),
    (50, ["ceiling_rgb_texture", "floor_rgb_texture"]),
    (34, ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]),
])
def test_fp32_program_is_the_fp16_program_with_fp32_weights(layers, modalities):
    """Same op rows and ktab; the weight blob is the fp32 BatchNorm fold itself, and its fp16 rounding is the fp16 blob."""
    sd = _model(layers, modalities).state_dict()
    ops16, w16, p16, k16, c16 = hip_resnet.build_program(sd, layers)
    ops32, w32, p32, k32, c32 = hip_resnet.build_program(sd, layers, precision="fp32")
    assert w16.dtype == np.int16 and w32.dtype == np.float32
    assert ops16.tobytes() == ops32.tobytes()
    assert np.array_equal(k16, k32) and np.array_equal(p16, p32) and c16 == c32
    assert w32.size == w16.size
    assert np.array_equal(w32.astype(np.float16).view(np.int16), w16)
    # the stem's weights in the fp32 blob ARE the fold (no rounding): conv1 (x) bn1, packed [Cout][kh][kw 8][Cin pad] / group-major
    wf, _ = hip_resnet.fold_bn(sd["conv1.weight"], {k: sd[f"resnet.bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")})
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(wf, torch.zeros(64), hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, 224, 224, 2, 3, True, kw_pad=8)
    n = bld.weights[0].size
    assert bld.weights[0].dtype == np.float32 and np.array_equal(w32[:n], bld.weights[0])
    assert set(np.unique(np.abs(w32[:n]))) - {0.0} <= set(np.abs(wf.numpy().reshape(-1)).tolist())


def test_default_builder_still_packs_fp16_bits():
    bld = hip_resnet._Builder()
    w = torch.randn(64, 64, 1, 1)
    bld.conv(w, torch.zeros(64), 0, 1, hip_resnet.NO_BUF, 8, 8, 1, 0, True)
    assert bld.weights[0].dtype == np.int16
    with pytest.raises(ValueError, match="precision"):
        hip_resnet._Builder(precision="bf16")


def test_large_weight_accepted_in_fp32_refused_in_fp16_nan_refused_in_both():
    model = _model(18, ["floor_rgb_texture"])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["resnet.layer1.0.conv1.weight"][0, 0, 0, 0] = 1e6
    with pytest.raises(ValueError, match="fp16 range"):
        hip_resnet.build_program(sd, 18)
    ops, w, p, k, c = hip_resnet.build_program(sd, 18, precision="fp32")
    assert np.abs(w).max() >= 1e5
    sd["resnet.layer2.0.conv2.weight"][1, 2, 0, 0] = float("nan")
    for precision in ("fp16", "fp32"):
        with pytest.raises(ValueError, match="non-finite"):
            hip_resnet.build_program(sd, 18, precision=precision)


def test_model_precision_setting():
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    assert model.precision == "fp16"
    assert model.set_precision("fp32") is model and model.precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        model.set_precision("fp64")
    assert model.precision == "fp32"
    assert model.set_precision("fp16").precision == "fp16"
