"""GPU parity of the fp32 verifier engine (salve_resnet_f32_*, salve_amd/csrc/resnet_f32.hip): per convolution against float64 torch,
logits against the fp32 oracle with north_star's ABSOLUTE 1e-3 at any magnitude, NaN propagation, the pipeline's fp32 mode, refusals."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import resnet_oracle as ro  # noqa: E402
from salve_amd import _lib, status, synthetic  # noqa: E402
from salve_amd.models import hip_resnet  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from _helpers import randomise_bn  # noqa: E402

DEV = "cuda:0"
F = torch.nn.functional


def tile_like_inputs(n, batch, seed=0):
    """n fp32 [batch, 3, 224, 224] tensors with the value set of real tiles: (v - mean) / std of uint8 values."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 256, (n, batch, 3, 224, 224), generator=g).float()
    mean = torch.tensor([123.675, 116.28, 103.53]).view(1, 1, 3, 1, 1)
    std = torch.tensor([58.395, 57.12, 57.375]).view(1, 1, 3, 1, 1)
    return list(((v - mean) / std).unbind(0))


def run_program(bld, x_nchw):
    """Run the ops of an fp32 _Builder (plus an AVGPOOL_FC over the last op's output, which every program ends in) on the fp32 NCHW
    input x; returns the workspace's activation buffers as fp32 NHWC tensors (CPU) by buffer id."""
    lib = _lib.load()
    last = bld.ops[-1]
    C, Hl, Wl = last[9], last[7], last[8]
    bld.fc(torch.zeros(2, C), torch.zeros(2), last[2], Hl, Wl, C)
    ops = np.array(bld.ops, dtype=hip_resnet.OP_DTYPE)
    w = np.concatenate(bld.weights).astype(np.float32)
    p = np.concatenate(bld.params).astype(np.float32)
    k = np.concatenate(bld.ktab).astype(np.int32)
    B, Cx = int(x_nchw.shape[0]), int(x_nchw.shape[1])
    h = lib.salve_resnet_f32_create(0, Cx, ops.ctypes.data_as(ctypes.c_void_p), len(ops), w.ctypes.data_as(ctypes.c_void_p), w.nbytes,
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


def conv64(x, w, b, stride, pad):
    """float64 reference and Sum |a b| (+ |bias|) per output, NCHW in, NHWC out."""
    x, w = x.double(), w.double()
    ref = F.conv2d(x, w, b.double(), stride, pad)
    mag = F.conv2d(x.abs(), w.abs(), b.double().abs(), stride, pad)
    return ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def assert_close(got, ref, mag, what):
    assert torch.isfinite(got).all(), what
    err = (got.double() - ref).abs()
    bound = 4e-6 * mag
    assert (err <= bound).all(), f"{what}: max err {float(err.max()):.3e}, worst err / bound {float((err / bound.clamp(min=1e-30)).max()):.2f}"


def _w(g, cout, cin, k):
    return torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5


@pytest.mark.parametrize("cin", [6, 12, 18])
def test_f32_stem_convolution_matches_float64(cin):
    """7x7 / 2 stem with Cin padded to 8 / 16 / 24 (the 16- and 24-channel forms walk the group-major k table); the input is the
    caller's NCHW tensor with its real channel count, padded by the engine."""
    g = torch.Generator().manual_seed(cin)
    B, hw = 2, 34
    w, b = _w(g, 64, cin, 7), torch.randn(64, generator=g) * 0.1
    x = torch.randn(B, cin, hw, hw, generator=g)
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, hw, hw, 2, 3, True, kw_pad=8)
    got = run_program(bld, x)[0]
    ref, mag = conv64(x, w, b, 2, 3)
    assert_close(got, ref.clamp(min=0), mag, f"stem cin {cin}")


@pytest.mark.parametrize("case", [
    dict(cout=256, k=1, s=1, p=0, hw=14, relu=False),
    dict(cout=128, k=3, s=1, p=1, hw=14, relu=True),
    dict(cout=64, k=3, s=2, p=1, hw=15, relu=True),
    dict(cout=128, k=1, s=2, p=0, hw=15, relu=False),
])
def test_f32_convolution_matches_float64(case):
    g = torch.Generator().manual_seed(case["cout"] + case["k"] + case["s"])
    B = 3
    w, b = _w(g, case["cout"], 64, case["k"]), torch.randn(case["cout"], generator=g) * 0.1
    x = torch.randn(B, 64, case["hw"], case["hw"], generator=g)
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, case["hw"], case["hw"], case["s"], case["p"], case["relu"])
    got = run_program(bld, x)[0]
    ref, mag = conv64(x, w, b, case["s"], case["p"])
    assert_close(got, ref.clamp(min=0) if case["relu"] else ref, mag, str(case))


def test_f32_residual_and_relu_match_float64():
    """out = relu(conv3x3(x) + b + res), the residual being an earlier op's output (buffer 1)."""
    g = torch.Generator().manual_seed(7)
    B, hw = 2, 14
    x = torch.randn(B, 64, hw, hw, generator=g)
    wr, br = _w(g, 256, 64, 1), torch.randn(256, generator=g) * 0.1
    w, b = _w(g, 256, 64, 3), torch.randn(256, generator=g) * 0.1
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(wr, br, hip_resnet.NET_INPUT, 1, hip_resnet.NO_BUF, hw, hw, 1, 0, False)
    bld.conv(w, b, hip_resnet.NET_INPUT, 0, 1, hw, hw, 1, 1, True)
    bufs = run_program(bld, x)
    res = bufs[1]
    ref, mag = conv64(x, w, b, 1, 1)
    assert (ref + res.double() < 0).any() and (ref + res.double() > 0).any()
    assert_close(bufs[0], (ref + res.double()).clamp(min=0), mag + res.double().abs(), "residual + relu")


@pytest.mark.parametrize("stride", [1, 2])
def test_f32_projection_shortcut_as_second_source_matches_float64(stride):
    """relu(w . t + w2 . y[::s, ::s] + b + b2): the `in2_buf` form of a down-sampling block's last convolution."""
    g = torch.Generator().manual_seed(11 + stride)
    B, hw, mid, cy, cout = 2, 14, 64, 128, 256
    x = torch.randn(B, 64, hw, hw, generator=g)
    wy, by = _w(g, cy, 64, 1), torch.randn(cy, generator=g) * 0.1
    wt, bt = _w(g, mid, 64, 3), torch.randn(mid, generator=g) * 0.1
    w, b = _w(g, cout, mid, 1), torch.randn(cout, generator=g) * 0.1
    w2, b2 = _w(g, cout, cy, 1), torch.randn(cout, generator=g) * 0.1
    bld = hip_resnet._Builder(precision="fp32")
    bld.conv(wy, by, hip_resnet.NET_INPUT, 1, hip_resnet.NO_BUF, hw, hw, 1, 0, True)        # y: buffer 1, hw x hw
    Ho, Wo = bld.conv(wt, bt, hip_resnet.NET_INPUT, 0, hip_resnet.NO_BUF, hw, hw, stride, 1, True)   # t: buffer 0, Ho x Wo
    bld.conv1x1_with_shortcut(w, b, 0, 2, Ho, Wo, w2, b2, 1, hw, hw, stride)
    bufs = run_program(bld, x)
    t = bufs[0].permute(0, 3, 1, 2).double()
    y = bufs[1].permute(0, 3, 1, 2)[:, :, ::stride, ::stride].double()
    ref = F.conv2d(t, w.double(), b.double()) + F.conv2d(y, w2.double(), b2.double())
    mag = F.conv2d(t.abs(), w.double().abs(), b.double().abs()) + F.conv2d(y.abs(), w2.double().abs(), b2.double().abs())
    assert_close(bufs[2], ref.clamp(min=0).permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1), f"in2 stride {stride}")


def _run_f32(model, xs):
    model.set_precision("fp32")
    with torch.no_grad():
        got = model.to(DEV)(*[x.to(DEV) for x in xs] + [None] * (6 - len(xs))).cpu()
    status.check(DEV, "fp32 forward")
    return got


MODALITY_SETS = {6: ["floor_rgb_texture"], 12: ["ceiling_rgb_texture", "floor_rgb_texture"],
                 18: ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]}


@pytest.mark.parametrize("num_layers", [18, 34, 50, 152])
@pytest.mark.parametrize("channels", [6, 12, 18])
def test_f32_logits_match_oracle(num_layers, channels):
    """North_star's bound, ABSOLUTE 1e-3, against the fp32 oracle on the same fp32 tiles (trained-looking BatchNorm)."""
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(num_layers, False, 2, SimpleNamespace(modalities=MODALITY_SETS[channels]))
    randomise_bn(model)
    model.eval()
    xs = tile_like_inputs(channels // 3, 2, seed=num_layers)
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), num_layers, xs)
    got = _run_f32(model, xs)
    err = float((got - ref).abs().max())
    print(f"resnet{num_layers} {channels}-ch fp32: |logit| max {float(ref.abs().max()):.3f}, max abs err {err:.2e}")
    assert err <= 1e-3


@pytest.mark.parametrize("num_layers,modalities,batch,min_mag", [
    (50, ["floor_rgb_texture"], 8, 4.5),
    (152, ["ceiling_rgb_texture", "floor_rgb_texture"], 4, 9.0),
])
def test_f32_logits_at_realistic_magnitude(num_layers, modalities, batch, min_mag):
    """Where the fp16 engine misses the absolute bound (4.8e-3 at |logit| 11 in the CPU emulation of its rounding,
    profiles/r05_storage_precision.md): the fp32 engine holds ABSOLUTE 1e-3 with the same arg-max.  (Head x 30: |logit| 4.7 for
    ResNet-50, 11.2 for ResNet-152 on these inputs.)"""
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(num_layers, False, 2, SimpleNamespace(modalities=modalities))
    randomise_bn(model)
    synthetic.trained_looking_head(model, 30.0)
    model.eval()
    xs = tile_like_inputs(len(modalities) * 2, batch)
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), num_layers, xs)
    got = _run_f32(model, xs)
    mag = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"resnet{num_layers} head x30 fp32: |logit| max {mag:.2f}, max abs err {err:.2e}")
    assert mag >= min_mag
    assert err <= 1e-3
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_f32_default_batchnorm_resnet152_has_the_fp32_range():
    """Default BatchNorm statistics: activations of ~1e8 (the fp16 engine saturates and reports SALVE_STATUS_FP16_RANGE).  The fp32
    engine raises no status bit and matches the oracle to 1e-4 of the logit magnitude."""
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(152, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    xs = tile_like_inputs(2, 2, seed=2)
    status.check(DEV, "before")
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), 152, xs)
    got = _run_f32(model, xs)   # (status.check inside: raises on any bit)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"resnet152 default BN fp32: |logit| max {scale:.3e}, max abs err {err:.2e} ({err / scale:.1e} relative)")
    assert scale > 65504.0
    assert err <= 1e-4 * scale
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_f32_nan_input_propagates_to_that_sample_only():
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    randomise_bn(model)
    model.eval()
    xs = tile_like_inputs(2, 3, seed=5)
    xs[1][1, 2, 100, 37] = float("nan")
    with torch.no_grad():
        ref = ro.forward(model.state_dict(), 18, xs)
    got = _run_f32(model, xs)
    assert torch.isnan(ref[1]).all() and torch.isnan(got[1]).all()
    keep = torch.tensor([True, False, True])
    assert torch.isfinite(got[keep]).all()
    assert float((got[keep] - ref[keep]).abs().max()) <= 1e-3


def test_f32_pipeline_mode():
    """RenderVerifyPipeline(precision="fp32"): fp32 NCHW tiles that round to the fp16 pipeline's tiles bit for bit, logits equal to the
    model's fp32 forward on those tiles bit for bit and within 1e-3 of the oracle, the same valid_mask."""
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
    for precision in ("fp16", "fp32"):
        pipe = RenderVerifyPipeline(model, dev, chunk=N, precision=precision)
        pipe.load_panos(rgb, depth)
        prepared = pipe.prepare(hyp)
        logits = pipe.score(prepared)
        torch.cuda.synchronize()
        pipe.check(f"pipeline {precision}")
        res[precision] = (logits.cpu(), pipe.tiles[:N].clone(), pipe.valid_mask(prepared))
        del pipe
    l16, t16, v16 = res["fp16"]
    l32, t32, v32 = res["fp32"]
    assert t32.dtype == torch.float32 and tuple(t32.shape) == (N, 12, 224, 224)
    assert torch.equal(t32.half(), t16[..., :12].permute(0, 3, 1, 2)), "fp32 tiles do not round to the fp16 pipeline's tiles"
    assert np.array_equal(v16, v32)
    xs = [t32[:, 3 * k:3 * k + 3].contiguous() for k in range(4)]
    direct = _run_f32(model, xs)
    assert torch.equal(direct, l32), "pipeline logits differ from the model's fp32 forward on the same tiles"
    with torch.no_grad():
        ref = ro.forward({k: v.cpu() for k, v in model.state_dict().items()}, 18, [x.cpu() for x in xs])
    assert float((l32 - ref).abs().max()) <= 1e-3
    model.set_precision("fp16")


def test_f32_refusals():
    lib = _lib.load()
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"])).eval()
    sd = model.state_dict()
    with pytest.raises(_lib.SalveHipError, match="flags must be 0"):
        hip_resnet.HipResNetF32(sd, 18, DEV, flags=1)
    ops, w, p, k, cin_p = hip_resnet.build_program(sd, 18, precision="fp32")
    args = lambda cin: (18, cin, ops.ctypes.data_as(ctypes.c_void_p), len(ops), w.ctypes.data_as(ctypes.c_void_p), w.nbytes,
                        p.ctypes.data_as(ctypes.c_void_p), p.nbytes, k.ctypes.data_as(ctypes.c_void_p), k.size, 0)
    assert not lib.salve_resnet_f32_create(*args(6))                 # pads to 8, the stem reads 16 channels
    assert b"in_channels" in lib.salve_last_error()
    eng = hip_resnet.HipResNetF32(sd, 18, DEV)
    assert eng.in_channels == 12 and eng.padded_channels == 16
    B = 2
    x = torch.zeros(B, 12, 224, 224, device=DEV)
    logits = torch.zeros(B, 2, device=DEV)
    need = eng.workspace_bytes(B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.salve_resnet_f32_forward(eng.handle, vp(x), B, vp(logits), vp(ws), need - 1, None, None) == -4
    assert b"workspace" in lib.salve_last_error()
    assert lib.salve_resnet_f32_forward(eng.handle, None, B, vp(logits), vp(ws), need, None, None) == -1
    assert lib.salve_resnet_f32_forward(eng.handle, vp(x), 0, vp(logits), vp(ws), need, None, None) == -1
    with pytest.raises(ValueError):
        eng.forward_nchw(torch.zeros(B, 16, 224, 224, device=DEV))
    model.set_precision("fp32")
    with pytest.raises(RuntimeError, match="forward_nhwc"):
        model.to(DEV).forward_nhwc(torch.zeros(B, 224, 224, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="layout"):
        from salve_amd.pipeline import RenderVerifyPipeline

        lm = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["layout"])).eval().to(DEV)
        RenderVerifyPipeline(lm, torch.device(DEV), chunk=2, precision="fp32")
    torch.cuda.synchronize()


def test_check_checkpoint_fp32_reports_the_contract_met(tmp_path, capsys):
    from salve_amd import check_checkpoint as cc

    torch.manual_seed(0)
    model = EarlyFusionCEResnet(152, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    synthetic.trained_looking_head(model, 30.0)
    torch.save({"epoch": 1, "state_dict": {"module." + k: v for k, v in model.state_dict().items()}, "optimizer": {}}, tmp_path / "train_ckpt.pth")
    rc = cc.main([str(tmp_path / "train_ckpt.pth"), "--layers", "152", "--precision", "fp32", "-n", "8"])
    out = capsys.readouterr().out
    print(out)
    assert "contract (fp32 engine: absolute 1e-3) MET" in out
    assert rc == 0
