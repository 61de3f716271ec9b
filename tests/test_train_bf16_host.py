"""bf16 mixed-precision training on the host (CPU): the salve_conv_bf16_* symbols, their shape contract against the fp32
entries', and the precision switches' refusals."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from salve_amd import _lib, training
from salve_amd.models.trainable import Conv2dBF16Function, TrainableEarlyFusionCEResnet
from tests.test_gpu_train import SHAPES
from tests.test_train_host import config

ROOT = Path(__file__).resolve().parents[1]
BF16_SYMBOLS = ("salve_conv_bf16_workspace_bytes", "salve_conv_bf16_forward", "salve_conv_bf16_backward_data",
                "salve_conv_bf16_backward_weight")


def test_bf16_symbols_are_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in BF16_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7
    assert "#define SALVE_HIP_ABI_VERSION 7" in header


def _descs():
    """Every distinct ResNet-18/50/152 convolution and the three stems at batch 2, plus descriptors both entries must refuse."""
    ok = []
    for cin, cout, k, s, h in SHAPES:
        pad = k // 2
        ho = (h + 2 * pad - k) // s + 1
        ok.append((2, h, h, (cin + 7) // 8 * 8, ho, ho, cout, k, k, s, pad))
    bad = [(2, 56, 56, 64, 56, 56, 64, 3, 3, 1, 0),       # 3x3 without padding
           (2, 56, 56, 64, 56, 56, 64, 5, 5, 1, 2),       # 5x5
           (2, 56, 56, 64, 28, 28, 64, 3, 3, 3, 1),       # stride 3
           (2, 224, 224, 16, 224, 224, 64, 7, 7, 1, 3),   # stem with stride 1
           (2, 56, 56, 32, 56, 56, 64, 3, 3, 1, 1),       # Cin not a multiple of 64
           (2, 56, 56, 4096, 56, 56, 64, 1, 1, 1, 0),     # Cin too large
           (2, 56, 56, 64, 56, 56, 96, 3, 3, 1, 1),       # Cout not a multiple of 64
           (2, 56, 56, 64, 56, 56, 0, 1, 1, 1, 0),        # no output channels
           (2, 56, 56, 64, 55, 56, 64, 3, 3, 1, 1),       # wrong Ho
           (2, 56, 56, 64, 56, 57, 64, 3, 3, 1, 1),       # wrong Wo
           (2, 224, 224, 12, 112, 112, 64, 7, 7, 2, 3),   # stem channels not padded to 8
           (2, 224, 224, 64, 112, 112, 64, 7, 7, 2, 3),   # stem with 64 input channels
           (0, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1),       # empty batch
           (2, 5000, 5000, 64, 5000, 5000, 64, 1, 1, 1, 0),   # image too large
           (100000, 224, 224, 64, 224, 224, 64, 1, 1, 1, 0)]  # batch too large
    return ok, bad


def test_bf16_workspace_accepts_exactly_what_the_fp32_entries_accept():
    lib = _lib.load()
    ok, bad = _descs()
    assert len(ok) == len(SHAPES) >= 31
    for t in ok + bad:
        d = ctypes.byref(_lib.ConvDesc(*t))
        for p in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD, 3, -1):
            f32 = int(lib.salve_conv_f32_workspace_bytes(d, p))
            bf16 = int(lib.salve_conv_bf16_workspace_bytes(d, p))
            assert (bf16 > 0) == (f32 > 0), (t, p, f32, bf16)
    for t in ok:
        d = ctypes.byref(_lib.ConvDesc(*t))
        assert lib.salve_conv_bf16_workspace_bytes(d, _lib.CONV_FWD) > 0 and lib.salve_conv_bf16_workspace_bytes(d, _lib.CONV_WGRAD) > 0, t
        assert (lib.salve_conv_bf16_workspace_bytes(d, _lib.CONV_DGRAD) > 0) == (t[7] != 7), t
    for t in bad:
        d = ctypes.byref(_lib.ConvDesc(*t))
        assert all(lib.salve_conv_bf16_workspace_bytes(d, p) == 0 for p in (0, 1, 2)), t
    assert lib.salve_conv_bf16_workspace_bytes(None, _lib.CONV_FWD) == 0


def test_bf16_entries_refuse_bad_descriptors_and_the_stem_dgrad_without_a_device():
    """Refusals are decided on the host before any launch: null descriptor / bad shape -> SALVE_ERR_BAD_ARG, stem dgrad ->
    SALVE_ERR_UNSUPPORTED."""
    lib = _lib.load()
    ok, bad = _descs()
    null = ctypes.c_void_p(0)
    for fn in ("salve_conv_bf16_forward", "salve_conv_bf16_backward_data", "salve_conv_bf16_backward_weight"):
        assert getattr(lib, fn)(None, null, null, null, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, fn
        for t in bad:
            assert getattr(lib, fn)(ctypes.byref(_lib.ConvDesc(*t)), null, null, null, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, (fn, t)
    stem = next(t for t in ok if t[7] == 7)
    assert lib.salve_conv_bf16_backward_data(ctypes.byref(_lib.ConvDesc(*stem)), null, null, null, null, 0, null) == _lib.SALVE_ERR_UNSUPPORTED


def test_train_precision_switches_refuse_other_values():
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    assert model.train_precision == "fp32"
    assert model.set_train_precision("bf16") is model and model.train_precision == "bf16"
    assert model.set_train_precision("fp32").train_precision == "fp32"
    with pytest.raises(ValueError, match="fp16"):
        model.set_train_precision("fp16")
    assert model.train_precision == "fp32"
    with pytest.raises(ValueError, match="'x'"):
        training.train(config(), "/nonexistent/never-written", precision="x")
    with pytest.raises(ValueError):
        training.get_model(config(), precision="fp16")


def test_train_cli_help_lists_precision():
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--help"], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--precision" in r.stdout and "bf16" in r.stdout and "fp32" in r.stdout


def test_bf16_convolution_refuses_cpu_tensors_and_wrong_dtypes():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Conv2dBF16Function.apply(torch.randn(1, 64, 8, 8).bfloat16(), torch.randn(64, 64, 3, 3), 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Conv2dBF16Function.apply(torch.randn(1, 64, 8, 8), torch.randn(64, 64, 3, 3), 1, 1)
