"""The opt-in HIP BatchNorm on the host (CPU): the salve_bn_* symbols, the shape contract of the workspace query and the entries'
refusals (decided before any launch), the norm switches' refusals and the unchanged state dict."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from salve_amd import _lib, training
from salve_amd.models.early_fusion import EarlyFusionCEResnet
from salve_amd.models.resnet_factory import RESNET_SPECS
from salve_amd.models.trainable import BatchNormHipFunction, TrainableEarlyFusionCEResnet
from tests.test_train_host import config

ROOT = Path(__file__).resolve().parents[1]
BN_SYMBOLS = ("salve_bn_workspace_bytes", "salve_bn_f32_forward", "salve_bn_f32_backward", "salve_bn_bf16_forward", "salve_bn_bf16_backward")
RELU, ADD, EVAL = _lib.BN_RELU, _lib.BN_ADD, _lib.BN_EVAL


def bn_shapes(layers: int, hw: int = 224):
    """(C, H, flags) of every BatchNorm of the trunk (v1.5) with what the model fuses into it: bn + relu after the stem, conv1 and
    conv2, bn + add + relu at the end of a block, plain bn on the downsample branch."""
    kind, blocks = RESNET_SPECS[layers]
    exp = 4 if kind == "bottleneck" else 1
    out, h, inpl = {(64, hw // 2, RELU)}, hw // 4, 64
    for si, (planes, n) in enumerate(zip([64, 128, 256, 512], blocks)):
        for bi in range(n):
            s = 2 if (bi == 0 and si > 0) else 1
            if kind == "bottleneck":
                out |= {(planes, h, RELU), (planes, h // s, RELU), (planes * 4, h // s, ADD | RELU)}
            else:
                out |= {(planes, h // s, RELU), (planes, h // s, ADD | RELU)}
            if bi == 0 and (s != 1 or inpl != planes * exp):
                out.add((planes * exp, h // s, 0))
            inpl, h = planes * exp, h // s
    return out


BN_SHAPES = sorted(bn_shapes(18) | bn_shapes(50) | bn_shapes(152))


def test_the_model_has_16_bottleneck_and_12_basic_batchnorm_shapes():
    assert len(bn_shapes(50)) == len(bn_shapes(152)) == 16 and bn_shapes(50) == bn_shapes(152)
    assert len(bn_shapes(18)) == 12


def test_bn_symbols_are_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in BN_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    for name, value in (("SALVE_BN_RELU", RELU), ("SALVE_BN_ADD", ADD), ("SALVE_BN_EVAL", EVAL)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7
    assert "#define SALVE_HIP_ABI_VERSION 7" in header
    assert ctypes.sizeof(_lib.BnDesc) == 20


def _desc(rows, c, flags, eps=1e-5, momentum=0.1):
    return ctypes.byref(_lib.BnDesc(rows, c, flags, eps, momentum))


BAD = [(100, 12, 0), (100, 4, 0), (100, 0, 0), (100, -8, 0), (100, 4104, 0), (100, 8192, 0),   # C
       (1, 64, 0), (0, 64, 0), (-5, 64, 0),                                                    # rows
       (100, 64, 8), (100, 64, 1 << 30), (100, 64, -1)]                                        # unknown flag bits


def test_bn_workspace_accepts_the_model_shapes_and_refuses_the_rest():
    lib = _lib.load()
    for batch in (2, 256):
        for c, h, flags in BN_SHAPES:
            rows = batch * h * h
            assert lib.salve_bn_workspace_bytes(_desc(rows, c, flags), _lib.BN_FWD) > 0, (batch, c, h, flags)
            assert lib.salve_bn_workspace_bytes(_desc(rows, c, flags), _lib.BN_BWD) > 0, (batch, c, h, flags)
            assert lib.salve_bn_workspace_bytes(_desc(rows, c, flags | EVAL), _lib.BN_FWD) > 0, (batch, c, h, flags)
            assert lib.salve_bn_workspace_bytes(_desc(rows, c, flags | EVAL), _lib.BN_BWD) == 0, "the eval form has no backward pass"
    for c in (8, 24, 4096):
        assert lib.salve_bn_workspace_bytes(_desc(2, c, 0), _lib.BN_FWD) > 0, c
    for rows, c, flags in BAD:
        for p in (_lib.BN_FWD, _lib.BN_BWD):
            assert lib.salve_bn_workspace_bytes(_desc(rows, c, flags), p) == 0, (rows, c, flags, p)
    for p in (2, -1, 7):
        assert lib.salve_bn_workspace_bytes(_desc(100, 64, 0), p) == 0, p
    assert lib.salve_bn_workspace_bytes(None, _lib.BN_FWD) == 0
    assert lib.salve_last_error()


def test_bn_entries_refuse_bad_descriptors_and_null_pointers_without_a_device():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for fn, n in (("salve_bn_f32_forward", 9), ("salve_bn_bf16_forward", 9), ("salve_bn_f32_backward", 10), ("salve_bn_bf16_backward", 10)):
        call = getattr(lib, fn)
        assert call(None, *[null] * n, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, fn
        for rows, c, flags in BAD:
            assert call(_desc(rows, c, flags), *[null] * n, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, (fn, rows, c, flags)
        for flags in (0, RELU, ADD | RELU):
            assert call(_desc(6272, 64, flags), *[null] * n, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, (fn, flags)   # null pointers
    for fn in ("salve_bn_f32_forward", "salve_bn_bf16_forward"):
        assert getattr(lib, fn)(_desc(6272, 64, EVAL), *[null] * 9, null, 0, null) == _lib.SALVE_ERR_BAD_ARG, fn
    for fn in ("salve_bn_f32_backward", "salve_bn_bf16_backward"):   # backward in eval mode is not built
        assert getattr(lib, fn)(_desc(6272, 64, EVAL), *[null] * 10, null, 0, null) == _lib.SALVE_ERR_UNSUPPORTED, fn


def test_train_norm_switches_refuse_other_values():
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    assert model.train_norm == "torch"
    assert model.set_train_norm("hip") is model and model.train_norm == "hip"
    assert model.set_train_norm("torch").train_norm == "torch"
    with pytest.raises(ValueError, match="miopen"):
        model.set_train_norm("miopen")
    assert model.train_norm == "torch"
    with pytest.raises(ValueError, match="'x'"):
        training.train(config(), "/nonexistent/never-written", norm="x")
    with pytest.raises(ValueError):
        training.get_model(config(), norm="HIP")
    for prec in ("fp32", "bf16"):   # the two switches are independent
        assert model.set_train_precision(prec).set_train_norm("hip").train_precision == prec


def test_train_cli_help_lists_norm():
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--help"], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--norm" in r.stdout and "hip" in r.stdout and "torch" in r.stdout


def test_batchnorm_function_refuses_cpu_tensors_and_wrong_dtypes():
    bn = torch.nn.BatchNorm2d(64)
    args = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, True, 1e-5, 0.1, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BatchNormHipFunction.apply(torch.randn(2, 64, 8, 8), None, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BatchNormHipFunction.apply(torch.randn(2, 64, 8, 8).bfloat16(), None, *args)
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            BatchNormHipFunction.apply(torch.zeros(2, 64, 8, 8, dtype=dt), None, *args)
    assert int(bn.num_batches_tracked) == 0 and float(bn.running_mean.abs().max()) == 0.0


@pytest.mark.parametrize("layers", [18, 50])
def test_hip_norm_model_has_the_inference_models_state_dict(layers):
    args = SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"])
    a = EarlyFusionCEResnet(layers, False, 2, args).state_dict()
    for prec in ("fp32", "bf16"):
        b = TrainableEarlyFusionCEResnet(layers, False, 2, args).set_train_precision(prec).set_train_norm("hip").state_dict()
        assert list(a) == list(b)
        assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
