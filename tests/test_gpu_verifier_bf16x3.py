"""GPU parity of the bf16x3 verifier engine (salve_resnet_bf16x3_create, salve_amd/csrc/conv_bf16x3.h): per convolution against float64
torch with the derived bound of tests/bf16x3_cases.py, logits against the fp32 oracle with the ABSOLUTE 1e-3 contract, NaN propagation,
determinism, the pipeline's bf16x3 mode, refusals, check_checkpoint."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bf16x3_cases as bc  # noqa: E402
from oracle import resnet_oracle as ro  # noqa: E402
from salve_amd import _lib, status, synthetic  # noqa: E402
from salve_amd.models import hip_resnet  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from _helpers import randomise_bn  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def run_program(bld, x_nchw):
    """Run the ops of an fp32 _Builder (plus an AVGPOOL_FC over the last op's output, which every program ends in) through
    salve_resnet_bf16x3_create on the fp32 NCHW input x; returns the workspace's activation buffers as fp32 NHWC tensors (CPU) by buffer id."""
    lib = _lib.load()
    last = bld.ops[-1]
    C, Hl, Wl = last[9], last[7], last[8]
    bld.fc(torch.zeros(2, C), torch.zeros(2), last[2], Hl, Wl, C)
    ops = np.array(bld.ops, dtype=hip_resnet.OP_DTYPE)
    w = np.concatenate(bld.weights).astype(np.float32)
    p = np.concatenate(bld.params).astype(np.float32)
    k = np.concatenate(bld.ktab).astype(np.int32)
    B, Cx = int(x_nchw.shape[0]), int(x_nchw.shape[1])
    h = lib.salve_resnet_bf16x3_create(0, Cx, ops.ctypes.data_as(ctypes.c_void_p), len(ops), w.ctypes.data_as(ctypes.c_void_p), w.nbytes,
                                       p.ctypes.data_as(ctypes.c_void_p), p.nbytes, k.ctypes.data_as(ctypes.c_void_p), k.size, 0)
    assert h, lib.salve_last_error()
    h = ctypes.c_void_p(h)
    try:
        need = lib.salve_resnet_f32_workspace_bytes(h, B)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        logits = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
        xd = x_nchw.to(DEV).contiguous()
        st = lib.salve_resnet_f32_forward(h, ctypes.c_void_p(xd.data_ptr()), B, ctypes.c_void_p(logits.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                          ws.numel(), None, None)
        torch.cuda.synchronize()
        assert st == 0, lib.salve_last_error()
    finally:
        lib.salve_resnet_f32_destroy(h)
    conv = [o for o in bld.ops if o[0] != hip_resnet.OP_AVGPOOL_FC]
    max_act = max(o[7] * o[8] * o[9] for o in conv)
    base = ws[(-ws.data_ptr()) % 256:].view(torch.float32)
    out = {}
    for o in conv:
        b = o[2]
        out[b] = base[b * B * max_act: b * B * max_act + B * o[7] * o[8] * o[9]].cpu().reshape(B, o[7], o[8], o[9])
    return out


def assert_within_bound(got, ref, mag, what, factor=bc.BOUND_FACTOR):
    assert torch.isfinite(got).all(), what
    r = bc.worst_ratio(got, ref, mag, factor)
    print(f"{what}: worst error / bound {r:.3f}")
    assert r <= 1.0, f"{what}: worst error / bound {r:.2f}"


@pytest.mark.parametrize("case", bc.CONV_CASES, ids=[c["name"] for c in bc.CONV_CASES])
def test_bf16x3_convolution_is_within_the_derived_bound(case):
    """One convolution as a one-op program: the 7 x 7 / 2 stems (Cin padded to 8 / 16 / 24; the latter two walk the group-major k table) and
    the plain shapes, against float64 with |error| <= (3 x 2^-18 + 4e-6) x mag."""
    x, w, b = bc.case_tensors(case)
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, case["hw"], case["hw"], case["s"], case["p"], case["relu"],
             kw_pad=8 if case.get("stem") else 0)
    got = run_program(bld, x)[0]
    ref, mag = bc.case_reference(case, x, w, b)
    assert_within_bound(got, ref, mag, case["name"])


def test_bf16x3_finite_activations_beyond_the_bf16_range_stay_finite():
    """+-FLT_MAX and 3.399e38 would round to inf in bf16: their hi piece is the largest finite bf16, lo takes the rest, and the outputs are
    finite and within the case's single-product bound (the kernel's integer form of the split rules: the conversion instructions alone
    give inf and NaN)."""
    case, x, w, b = bc.beyond_bf16_case()
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, case["hw"], case["hw"], 1, 0, False)
    got = run_program(bld, x)[0]
    ref, mag = bc.case_reference(case, x, w, b)
    assert_within_bound(got, ref, mag, case["name"], bc.BEYOND_BF16_BOUND_FACTOR)


def test_bf16x3_residual_and_relu_are_within_the_bound():
    """out = relu(conv3x3(x) + b + res), the residual being an earlier op's output (buffer 1); outputs of both signs before the ReLU."""
    g = torch.Generator().manual_seed(7)
    B, hw = 2, 14
    x = torch.randn(B, 64, hw, hw, generator=g)
    wr, br = bc.rand_w(g, 256, 64, 1), torch.randn(256, generator=g) * 0.1
    w, b = bc.rand_w(g, 256, 64, 3), torch.randn(256, generator=g) * 0.1
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(wr, br, hip_resnet.NET_INPUT, 1, hip_resnet.NO_BUF, hw, hw, 1, 0, False)
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, 1, hw, hw, 1, 1, True)
    bufs = run_program(bld, x)
    res = bufs[1]
    ref, mag = bc.conv64(x, w, b, 1, 1)
    assert (ref + res.double() < 0).any() and (ref + res.double() > 0).any()
    assert_within_bound(bufs[0], (ref + res.double()).clamp(min=0), mag + res.double().abs(), "residual + relu")


@pytest.mark.parametrize("stride", [1, 2])
def test_bf16x3_projection_shortcut_as_second_source_is_within_the_bound(stride):
    """relu(w . t + w2 . y[::s, ::s] + b + b2): the `in2_buf` form of a down-sampling block's last convolution, on the engine's own t and y."""
    g = torch.Generator().manual_seed(11 + stride)
    B, hw, mid, cy, cout = 2, 14, 64, 128, 256
    x = torch.randn(B, 64, hw, hw, generator=g)
    wy, by = bc.rand_w(g, cy, 64, 1), torch.randn(cy, generator=g) * 0.1
    wt, bt = bc.rand_w(g, mid, 64, 3), torch.randn(mid, generator=g) * 0.1
    w, b = bc.rand_w(g, cout, mid, 1), torch.randn(cout, generator=g) * 0.1
    w2, b2 = bc.rand_w(g, cout, cy, 1), torch.randn(cout, generator=g) * 0.1
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(wy, by, hip_resnet.NET_INPUT, 1, hip_resnet.NO_BUF, hw, hw, 1, 0, True)        # y: buffer 1, hw x hw
    Ho, Wo = bld.conv(wt, bt, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, hw, hw, stride, 1, True)   # t: buffer 0, Ho x Wo
    bld.conv1x1_with_shortcut(w, b, 0, 2, Ho, Wo, w2, b2, 1, hw, hw, stride)
    bufs = run_program(bld, x)
    t = bufs[0].permute(0, 3, 1, 2).double()
    y = bufs[1].permute(0, 3, 1, 2)[:, :, ::stride, ::stride].double()
    ref = F.conv2d(t, w.double(), b.double()) + F.conv2d(y, w2.double(), b2.double())
    mag = F.conv2d(t.abs(), w.double().abs(), b.double().abs()) + F.conv2d(y.abs(), w2.double().abs(), b2.double().abs())
    assert_within_bound(bufs[2], ref.clamp(min=0).permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1), f"in2 stride {stride}")


def _run_bf16x3(model, xs):
    model.set_precision("bf16x3")
    with torch.no_grad():
        got = model.to(DEV)(*[x.to(DEV) for x in xs] + [None] * (6 - len(xs))).cpu()
    status.check(DEV, "bf16x3 forward")
    return got


MODALITY_SETS = {6: ["floor_rgb_texture"], 12: ["ceiling_rgb_texture", "floor_rgb_texture"],
                 18: ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]}


@pytest.mark.parametrize("num_layers", [18, 34, 50, 152])
@pytest.mark.parametrize("channels", [6, 12, 18])
def test_bf16x3_logits_match_oracle(num_layers, channels):
    """ABSOLUTE 1e-3 against the fp32 oracle on the same fp32 tiles (trained-looking BatchNorm), batch 2."""
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(num_layers, False, 2, SimpleNamespace(modalities=MODALITY_SETS[channels]))
    randomise_bn(model)
    model.eval()
    xs = bc.tile_like_inputs(channels // 3, 2, seed=num_layers)
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), num_layers, xs)
    got = _run_bf16x3(model, xs)
    err = float((got - ref).abs().max())
    print(f"resnet{num_layers} {channels}-ch bf16x3: |logit| max {float(ref.abs().max()):.3f}, max abs err {err:.2e}")
    assert err <= 1e-3


@pytest.mark.parametrize("num_layers,modalities,batch,min_mag", bc.HEAD30_CASES, ids=["resnet50-6ch", "resnet152-12ch"])
def test_bf16x3_logits_at_realistic_magnitude(num_layers, modalities, batch, min_mag):
    """Head x 30 (|logit| about 4.7 for ResNet-50, 11 for ResNet-152), where the fp16 engine misses the absolute bound: ABSOLUTE 1e-3 and the
    same arg-max.  (The host emulation of these cases stays within 1e-4: tests/test_bf16x3_host.py.)"""
    model = bc.head30_model(num_layers, modalities)
    xs = bc.tile_like_inputs(len(modalities) * 2, batch)
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), num_layers, xs)
    got = _run_bf16x3(model, xs)
    mag = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"resnet{num_layers} head x30 bf16x3: |logit| max {mag:.2f}, max abs err {err:.2e}")
    assert mag >= min_mag
    assert err <= 1e-3
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_bf16x3_default_batchnorm_resnet152_keeps_the_fp32_range():
    """Default BatchNorm statistics: activations of ~1e8, beyond fp16.  bf16 pieces have fp32's exponents: the logits are finite, no status
    bit is raised, and the relative error is within 10 x the host emulation's of the same case (bf16x3_cases.EMULATED_DEFAULT_BN_REL_ERR)."""
    model, xs = bc.default_bn_case()
    status.check(DEV, "before")
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), 152, xs)
    got = _run_bf16x3(model, xs)   # (status.check inside: raises on any bit)
    scale = float(ref.abs().max())
    rel = float((got - ref).abs().max()) / scale
    print(f"resnet152 default BN bf16x3: |logit| max {scale:.3e}, relative error {rel:.2e} (emulated {bc.EMULATED_DEFAULT_BN_REL_ERR:.2e})")
    assert torch.isfinite(got).all()
    assert scale > 65504.0
    assert rel <= 10 * bc.EMULATED_DEFAULT_BN_REL_ERR


def test_bf16x3_nan_input_propagates_to_that_sample_only():
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    randomise_bn(model)
    model.eval()
    xs = bc.tile_like_inputs(2, 3, seed=5)
    xs[1][1, 2, 100, 37] = float("nan")
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), 18, xs)
    got = _run_bf16x3(model, xs)
    assert torch.isnan(ref[1]).all() and torch.isnan(got[1]).all()
    keep = torch.tensor([True, False, True])
    assert torch.isfinite(got[keep]).all()
    assert float((got[keep] - ref[keep]).abs().max()) <= 1e-3


def test_bf16x3_is_deterministic():
    """Two engines built from the same weights, two runs each: equal bits (fixed MFMA order, no atomics, no split-K)."""
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(50, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    randomise_bn(model)
    x = torch.cat(bc.tile_like_inputs(2, 3, seed=9), 1).to(DEV)
    outs = []
    for _ in range(2):
        eng = hip_resnet.HipResNetBf16x3(model.state_dict(), 50, DEV)
        outs += [eng.forward_nchw(x).cpu(), eng.forward_nchw(x).cpu()]
        del eng
    assert torch.isfinite(outs[0]).all()
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_bf16x3_pipeline_mode():
    """RenderVerifyPipeline(precision="bf16x3"): the fp32 mode's tiles bit for bit, logits equal to the model's bf16x3 forward on those tiles
    and within 1e-3 of the oracle, the same valid_mask."""
    from salve_amd.pipeline import RenderVerifyPipeline

    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"])).eval()
    randomise_bn(model)
    dev = torch.device(DEV)
    model.to(dev)
    P, N = 8, 64
    panos = [synthetic.make_pano(i) for i in range(P)]
    rgb, depth = np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])
    hyp = synthetic.make_hypotheses(N, P, seed=3)
    res = {}
    for precision in ("fp32", "bf16x3"):
        pipe = RenderVerifyPipeline(model, dev, chunk=N, precision=precision)
        assert isinstance(pipe.engine, hip_resnet.HipResNetBf16x3) == (precision == "bf16x3")
        pipe.load_panos(rgb, depth)
        prepared = pipe.prepare(hyp)
        logits = pipe.score(prepared)
        torch.cuda.synchronize()
        pipe.check(f"pipeline {precision}")
        res[precision] = (logits.cpu(), pipe.tiles[:N].clone(), pipe.valid_mask(prepared))
        del pipe
    l32, t32, v32 = res["fp32"]
    lx3, tx3, vx3 = res["bf16x3"]
    assert tx3.dtype == torch.float32 and tuple(tx3.shape) == (N, 12, 224, 224)
    assert torch.equal(tx3, t32), "bf16x3 tiles differ from the fp32 mode's"
    assert np.array_equal(v32, vx3)
    xs = [tx3[:, 3 * k:3 * k + 3].contiguous() for k in range(4)]
    direct = _run_bf16x3(model, xs)
    assert torch.equal(direct, lx3), "pipeline logits differ from the model's bf16x3 forward on the same tiles"
    with torch.no_grad():
        ref = ro.forward({k: v.cpu() for k, v in model.state_dict().items()}, 18, [x.cpu() for x in xs])
    assert float((lx3 - ref).abs().max()) <= 1e-3
    model.set_precision("fp16")


def test_bf16x3_refusals():
    lib = _lib.load()
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"])).eval()
    sd = model.state_dict()
    with pytest.raises(_lib.SalveHipError, match="flags must be 0"):
        hip_resnet.HipResNetBf16x3(sd, 18, DEV, flags=1)
    ops, w, p, k, cin_p = hip_resnet.build_program(sd, 18, precision="bf16x3")
    args = lambda cin: (18, cin, ops.ctypes.data_as(ctypes.c_void_p), len(ops), w.ctypes.data_as(ctypes.c_void_p), w.nbytes,
                        p.ctypes.data_as(ctypes.c_void_p), p.nbytes, k.ctypes.data_as(ctypes.c_void_p), k.size, 0)
    assert not lib.salve_resnet_bf16x3_create(*args(6))                 # pads to 8, the stem reads 16 channels
    assert b"in_channels" in lib.salve_last_error()
    eng = hip_resnet.HipResNetBf16x3(sd, 18, DEV)
    assert eng.in_channels == 12 and eng.padded_channels == 16
    B = 2
    x = torch.zeros(B, 12, 224, 224, device=DEV)
    logits = torch.zeros(B, 2, device=DEV)
    need = eng.workspace_bytes(B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.salve_resnet_f32_forward(eng.handle, vp(x), B, vp(logits), vp(ws), need - 1, None, None) == -4
    assert b"workspace" in lib.salve_last_error()
    with pytest.raises(ValueError):
        eng.forward_nchw(torch.zeros(B, 16, 224, 224, device=DEV))
    model.set_precision("bf16x3")
    with pytest.raises(RuntimeError, match="forward_nhwc"):
        model.to(DEV).forward_nhwc(torch.zeros(B, 224, 224, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="layout"):
        from salve_amd.pipeline import RenderVerifyPipeline

        lm = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["layout"])).eval().to(DEV)
        RenderVerifyPipeline(lm, torch.device(DEV), chunk=2, precision="bf16x3")
    torch.cuda.synchronize()


def test_check_checkpoint_bf16x3_reports_the_contract_met(tmp_path, capsys):
    from salve_amd import check_checkpoint as cc

    model = bc.head30_model(152, ["ceiling_rgb_texture", "floor_rgb_texture"])
    torch.save({"epoch": 1, "state_dict": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, tmp_path / "train_ckpt.pth")
    rc = cc.main([str(tmp_path / "train_ckpt.pth"), "--layers", "152", "--precision", "bf16x3", "-n", "8"])
    out = capsys.readouterr().out
    print(out)
    assert "contract (bf16x3 engine: absolute 1e-3) MET" in out
    assert rc == 0
