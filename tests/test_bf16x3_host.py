"""The bf16x3 verifier's host side (CPU): the ABI symbol, the split rules, and the error statement -- the emulated scheme stays within the
derived per-convolution bound on every case the GPU test runs, emulated kernels that lose a cross term exceed it on every case, and
whole-network emulated logits keep a margin of 10 inside the absolute 1e-3 contract."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

import bf16x3_cases as bc
from oracle import resnet_oracle as ro
from salve_amd import _lib
from salve_amd.models import hip_resnet

ROOT = Path(__file__).resolve().parents[1]


def test_bf16x3_symbol_is_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    assert re.search(r"\bsalve_resnet_bf16x3_create\(", header)
    assert "salve_resnet_bf16x3_create" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "salve_resnet_bf16x3_create")
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7


def test_bf16x3_is_a_precision_with_the_fp32_blob():
    from types import SimpleNamespace

    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    assert hip_resnet.PRECISIONS == ("fp16", "fp32", "bf16x3")
    assert issubclass(hip_resnet.HipResNetBf16x3, hip_resnet.HipResNetF32)
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    assert model.set_precision("bf16x3") is model and model.precision == "bf16x3"
    a = hip_resnet.build_program(model.state_dict(), 18, precision="fp32")
    b = hip_resnet.build_program(model.state_dict(), 18, precision="bf16x3")
    assert b[1].dtype == np.float32
    assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(p, q) for p, q in zip(a[1:4], b[1:4])) and a[4] == b[4]


def test_split_rules():
    inf, nan, fmax = float("inf"), float("nan"), float(np.finfo(np.float32).max)
    x = torch.tensor([nan, inf, -inf, fmax, -fmax, 0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 3.14159274, -1e-30, 3.0e38])
    hi, lo = bc.split(x)
    assert torch.isnan(hi[0]) and lo[0] == 0
    assert hi[1] == inf and lo[1] == 0 and hi[2] == -inf and lo[2] == 0
    assert not torch.isnan(lo).any()
    assert hi[3] == bc.BF16_MAX and hi[4] == -bc.BF16_MAX and torch.isfinite(lo[3:5]).all()
    assert abs(float(hi[3].double() + lo[3].double()) - fmax) <= 2.0 ** -15 * fmax
    assert hi[5] == 0 and lo[5] == 0 and hi[6] == 0 and lo[6] == 0
    assert torch.signbit(hi[6]) and not torch.signbit(hi[5])
    assert hi[7] == 1.0 and lo[7] == 0
    assert hi[8] == 1.0 and lo[8] == 2.0 ** -8  # a tie rounds to the even neighbour (1, not 1 + 2^-7); the rest is lo
    # both pieces are bf16 values, hi is the nearest, and the two pieces leave at most 2^-16 |x| (8 significand bits each)
    fin = torch.isfinite(x)
    for t in (hi, lo):
        assert torch.equal(t[fin], t[fin].to(torch.bfloat16).float())
    g = torch.Generator().manual_seed(0)
    r = torch.randn(100000, generator=g) * torch.exp(torch.randn(100000, generator=g) * 8)
    rh, rl = bc.split(r)
    assert torch.equal(rh, r.to(torch.bfloat16).float())
    assert ((r.double() - rh.double() - rl.double()).abs() <= 2.0 ** -16 * r.double().abs()).all()


@pytest.fixture(scope="module")
def conv_case_data():
    out = {}
    for case in bc.CONV_CASES:
        x, w, b = bc.case_tensors(case)
        out[case["name"]] = (x, w, b) + bc.case_reference(case, x, w, b)
    return out


def _ratio(case, data, terms):
    x, w, b, ref, mag = data
    y = bc.emu_conv(x, w, b, case["s"], case["p"], terms)
    y = (y.clamp(min=0) if case["relu"] else y).permute(0, 2, 3, 1)
    return bc.worst_ratio(y, ref, mag)


@pytest.mark.parametrize("case", bc.CONV_CASES, ids=[c["name"] for c in bc.CONV_CASES])
def test_emulated_scheme_is_within_the_derived_bound(case, conv_case_data):
    r = _ratio(case, conv_case_data[case["name"]], bc.TERMS_ALL)
    print(f"{case['name']}: worst error / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", bc.CONV_CASES, ids=[c["name"] for c in bc.CONV_CASES])
def test_emulated_kernels_that_lose_a_term_exceed_the_bound(case, conv_case_data):
    for what, terms in bc.WRONG_KERNELS.items():
        r = _ratio(case, conv_case_data[case["name"]], terms)
        print(f"{case['name']}, {what}: worst error / bound {r:.1f}")
        assert r > 1.0, what


def test_emulated_scheme_with_activations_beyond_the_bf16_range():
    """Finite inputs that would round to inf take the clamped hi piece: finite outputs, within the single-product bound of the case; an
    emulation that loses a cross term exceeds it."""
    case, x, w, b = bc.beyond_bf16_case()
    assert torch.isinf(x.to(torch.bfloat16)).sum() == 3
    ref, mag = bc.case_reference(case, x, w, b)
    y = bc.emu_conv(x, w, b, 1, 0).permute(0, 2, 3, 1)
    r = bc.worst_ratio(y, ref, mag, bc.BEYOND_BF16_BOUND_FACTOR)
    print(f"beyond-bf16: worst error / bound {r:.3f}")
    assert torch.isfinite(y).all() and r <= 1.0
    for what, terms in bc.WRONG_KERNELS.items():
        assert bc.worst_ratio(bc.emu_conv(x, w, b, 1, 0, terms).permute(0, 2, 3, 1), ref, mag, bc.BEYOND_BF16_BOUND_FACTOR) > 1.0, what


@pytest.mark.parametrize("num_layers,modalities,batch,min_mag", bc.HEAD30_CASES, ids=["resnet50-6ch", "resnet152-12ch"])
def test_emulated_logits_keep_a_margin_of_ten(num_layers, modalities, batch, min_mag):
    """Head x 30: emulated logits within 1e-4 of the fp32 oracle, a tenth of the contract the GPU test holds the engine to."""
    model = bc.head30_model(num_layers, modalities)
    xs = bc.tile_like_inputs(len(modalities) * 2, batch)
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), num_layers, xs)
        got = bc.emu_forward(model.state_dict(), num_layers, xs)
    mag, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"resnet{num_layers} head x30 emulated bf16x3: |logit| max {mag:.2f}, max abs err {err:.2e}")
    assert mag >= min_mag
    assert err <= 1e-4
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_emulated_default_batchnorm_error_is_the_recorded_constant():
    """The constant the GPU test scales by 10 is what the emulation of the same case gives (to a factor of 2: CPU convolutions differ
    in their summation order)."""
    model, xs = bc.default_bn_case()
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), 152, xs)
        got = bc.emu_forward(model.state_dict(), 152, xs)
    scale = float(ref.abs().max())
    rel = float((got - ref).abs().max()) / scale
    print(f"resnet152 default BN emulated bf16x3: |logit| max {scale:.3e}, relative error {rel:.3e} (recorded {bc.EMULATED_DEFAULT_BN_REL_ERR:.3e})")
    assert torch.isfinite(got).all() and scale > 65504.0
    assert 0.5 * bc.EMULATED_DEFAULT_BN_REL_ERR <= rel <= 2.0 * bc.EMULATED_DEFAULT_BN_REL_ERR
