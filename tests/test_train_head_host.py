"""The HIP classifier head without a GPU: the float64 reference against torch's float64 head, the property of the cases' inputs that
keeps the arg-max away from rounding, the descriptor against the header, the exported symbols, the switches and the meter's formula."""

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from salve_amd import _lib, training
from salve_amd.evaluate import ClassAccuracyMeter, DeviceClassMeter
from salve_amd.models import trainable
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet
from tests import head_cases as hc

ROOT = Path(__file__).resolve().parents[1]
SMALL = [c for c in hc.CASES if c.B * c.HW * c.C <= 1 << 21] + [hc.Case(257, 50, 2048, 16, "bf16")]


def test_case_list_is_the_cross_product_and_the_two_special_cases():
    assert len(hc.GRID) == 4 * 3 * 4 * 3 * 2 == len(set(hc.GRID))
    assert {(c.B, c.HW, c.C, c.K, c.dtype) for c in hc.GRID} == {(b, hw, ch, k, dt) for b in (1, 3, 64, 257) for hw in (1, 49, 50)
                                                                 for ch in (8, 520, 512, 2048) for k in (2, 3, 16) for dt in ("fp32", "bf16")}
    assert len({c.id for c in hc.CASES}) == len(hc.CASES) == len(hc.GRID) + 4


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_float64_reference_is_torchs_head_in_float64(case):
    """The reference is numpy written from the formulas; torch's CPU operators in float64 evaluate them in another order: they agree
    to 1e-12 relative to each tensor's largest magnitude, with an upstream gradient other than 1."""
    d = hc.make(case)
    ref, t64 = hc.head_f64(g=0.75, **d), hc.head_torch(dtype=torch.float64, g=0.75, **d)
    for name in hc.NAMES:
        assert hc.err(t64[name], ref[name]) <= 1e-12 * max(float(np.abs(ref[name]).max()), 1e-300), (name, hc.err(t64[name], ref[name]))


def test_every_case_keeps_the_arg_max_away_from_rounding():
    """The two largest float64 logits of every row of every case differ by at least LOGIT_GAP (1e-2, a hundred thousand fp32 ulps of
    a logit of order 1 to 100): no implementation's rounding decides a prediction.  bf16 inputs are bf16 values."""
    for case in hc.CASES:
        d = hc.make(case)
        logits = hc.head_f64(**d)["logits"]
        assert float(hc.logit_gap(logits).min()) >= hc.LOGIT_GAP, case.id
        assert d["x"].dtype == d["w"].dtype == d["b"].dtype == np.float32 and d["t"].dtype == np.int64
        assert d["x"].shape == (case.B, case.HW, case.C) and d["w"].shape == (case.K, case.C)
        assert d["t"].min() >= 0 and d["t"].max() < case.K
        if case.dtype == "bf16":
            assert np.array_equal(hc.to_bf16_values(d["x"]), d["x"])
        if case.scale != 1.0:
            assert float(np.abs(logits).max()) > 80.0   # exp() of it overflows fp32 unless the maximum is subtracted
            assert np.isfinite(hc.head_f64(**d)["loss"])
        if case.one_class is not None:
            assert set(d["t"].tolist()) == {case.one_class}


def test_bound_is_ten_times_torchs_error_floored_at_an_ulp():
    ref = np.array([1.0, -3.0])
    assert hc.bound(ref, ref + 1e-3) == pytest.approx(1e-2)
    assert hc.bound(ref, ref) == float(np.spacing(np.float32(3.0))) == 2.0 ** -22
    assert hc.bound(ref, ref, "bf16") == 2.0 ** -6   # bf16 keeps 8 significant bits: the spacing in [2, 4) is 2^-6
    assert hc.err(np.array([np.nan]), np.array([0.0])) == float("inf")


def test_descriptor_and_meter_record_match_the_header():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} salve_head_desc_t;", header).group(1)
    assert re.match(r"\s*int32_t\b", body)
    assert tuple(re.findall(r"(\w+)\s*[;,]", body)) == tuple(n for n, _ in _lib.HeadDesc._fields_)
    assert all(t is _lib.ctypes.c_int32 for _, t in _lib.HeadDesc._fields_)
    meter = re.search(r"typedef struct \{([^}]*)\} salve_head_meter_t;", header).group(1)
    assert tuple(re.findall(r"(\w+)(?:\[\w+\])?\s*;", meter)) == _lib.HEAD_METER_DTYPE.names
    assert int(re.search(r"#define SALVE_HEAD_MAX_CLASSES (\d+)", header).group(1)) == _lib.HEAD_MAX_CLASSES == 16
    assert _lib.HEAD_METER_DTYPE.itemsize == (2 * 16 + 3) * 8
    for name, value in (("SALVE_HEAD_ACCUMULATE_LOSS", _lib.HEAD_ACCUMULATE_LOSS), ("SALVE_HEAD_FWD", _lib.HEAD_FWD), ("SALVE_HEAD_BWD", _lib.HEAD_BWD)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert int(re.search(r"#define SALVE_HIP_ABI_VERSION (\d+)", header).group(1)) == _lib.EXPECTED_ABI == 7   # additive


def test_symbols_are_declared_exported_and_built():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in ("salve_head_workspace_bytes", "salve_head_f32_forward", "salve_head_f32_backward", "salve_head_bf16_forward", "salve_head_bf16_backward"):
        assert name in _lib.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", header) and hasattr(lib, name), name


def test_workspace_query_refuses_what_the_contract_refuses():
    """(Host code only: the query launches nothing.)"""
    lib = _lib.load()
    ws = lambda *d, p=_lib.HEAD_FWD: int(lib.salve_head_workspace_bytes(_lib.ctypes.byref(_lib.HeadDesc(*d)), p))   # noqa: E731
    assert ws(256, 49, 2048, 2, 0) > 0 and ws(1, 1, 8, 16, 1, p=_lib.HEAD_BWD) > 0 and ws(65535, 1024, 4096, 16, 1) > 0
    for bad in ((0, 49, 512, 2, 0), (65536, 49, 512, 2, 0), (4, 0, 512, 2, 0), (4, 1025, 512, 2, 0), (4, 49, 0, 2, 0), (4, 49, 516, 2, 0),
                (4, 49, 4104, 2, 0), (4, 49, 512, 1, 0), (4, 49, 512, 17, 0), (4, 49, 512, 2, 2)):
        assert ws(*bad) == 0 and lib.salve_last_error().startswith(b"head:"), bad
    assert ws(4, 49, 512, 2, 0, p=2) == 0


def _model():
    return TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))


def test_head_switch_accepts_torch_and_hip_only():
    assert trainable.TRAIN_HEADS == ("torch", "hip")
    m = _model()
    assert m.train_head == "torch"   # the default
    assert m.set_train_head("hip") is m and m.train_head == "hip" and m.set_train_head("torch").train_head == "torch"
    with pytest.raises(ValueError, match="head"):
        m.set_train_head("fused")
    for ok in trainable.TRAIN_HEADS:
        training._check_head(ok)
    with pytest.raises(ValueError, match="head"):
        training._check_head("cuda")
    args = SimpleNamespace(num_layers=18, pretrained=False, num_ce_classes=2, modalities=["floor_rgb_texture"])
    with pytest.raises(ValueError, match="head"):   # refused before the device is asked for
        training.get_model(args, head="fused")
    with pytest.raises(ValueError, match="head"):
        training.train(args, "unused", head="fused")
    with pytest.raises(ValueError, match="head"):
        training.train_rendered(args, None, None, "unused", head="fused")
    from salve_amd import train as train_cli

    with pytest.raises(ValueError, match="head"):
        train_cli.main(["--config", "unused.yaml", "--head", "fused"])


def test_no_cpu_fallback_and_no_meter_for_the_torch_head():
    m = _model().set_train_head("hip")
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.forward_loss(x, x, None, None, None, None, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device only"):
        trainable.ClassifierHeadHipFunction.apply(torch.zeros(2, 8, 1, 1), torch.zeros(2, 8), torch.zeros(2), torch.zeros(2, dtype=torch.int64), None, False)
    with pytest.raises(ValueError, match="classes"):
        DeviceClassMeter(17, "cpu")
    with pytest.raises(ValueError, match="classes"):
        DeviceClassMeter(1, "cpu")


def _filled(k, total, correct, loss_sum=0.0, loss_rows=0, bad=0):
    m = DeviceClassMeter(k, "cpu")
    rec = np.zeros(1, dtype=_lib.HEAD_METER_DTYPE)
    rec["total"][0, :k], rec["correct"][0, :k] = total, correct
    rec["loss_sum"], rec["loss_rows"], rec["bad_targets"] = loss_sum, loss_rows, bad
    m.record.copy_(torch.from_numpy(rec.view(np.int64).copy()))
    return m


def test_device_meter_formula_is_the_host_meters():
    for k, total, correct in ((2, [7, 5], [6, 0]), (2, [0, 4], [0, 3]), (3, [1, 10 ** 10, 3], [1, 10 ** 10 - 1, 0]), (16, list(range(16)), [i // 2 for i in range(16)])):
        host = ClassAccuracyMeter(k)
        host.total[:], host.correct[:] = total, correct
        accs, macc, avg = _filled(k, total, correct, loss_sum=3.5, loss_rows=7).read()
        want_accs, want_macc = host.get_metrics()
        assert np.array_equal(accs, want_accs) and macc == want_macc and avg == 0.5
    accs, macc, avg = _filled(2, [0, 4], [0, 3]).read()
    assert accs[0] == 0.0 and accs[1] == 3 / (4 + 1e-10) and avg == 0.0   # an absent class: 0 / 1e-10; no accumulated batch: 0.0
    m = _filled(2, [1, 1], [1, 1], bad=3)
    with pytest.raises(RuntimeError, match="3 targets"):
        m.read()
    m.reset()
    assert not m.record.any() and m.read()[1] == 0.0
