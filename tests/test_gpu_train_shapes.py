"""The training kernels across their whole accepted shape contract on the MI355X (tables: tests/train_cases.py): exact parity of
the fp32 and bf16 convolutions on integer probes at edge shapes, real batches and tensors beyond 2^32 bytes, random operands with
the existing bounds at odd and non-square shapes, the HIP BatchNorm at odd channel and row counts, the locality of non-finite
inputs, and one non-square training step."""

import time
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from salve_amd.models.trainable import Conv2dBF16Function, Conv2dF32Function, TrainableEarlyFusionCEResnet  # noqa: E402
from tests import test_gpu_train_norm as nm  # noqa: E402
from tests import train_cases as tc  # noqa: E402
from tests.test_gpu_train import MODS, ref_forward, rel  # noqa: E402
from tests.test_gpu_train_bf16 import check_rounded  # noqa: E402

DEV = torch.device("cuda:0")
PRECISIONS = ("fp32", "bf16")
ACT = {"fp32": torch.float32, "bf16": torch.bfloat16}
EXACT = {"fp32": tc.exact_f32, "bf16": tc.exact_bf16}   # forward and dgrad; dW is fp32 in both precisions


def run_conv(prec, x, w, dy, s, pad, want_dx):
    """One forward and backward pass of the precision's autograd function.  x, dy: [B, C, H, W] device tensors in the activation
    dtype, channels_last; w: the fp32 (master) weight on the device.  Returns y, dx (None unless wanted) and dW."""
    fn = Conv2dF32Function if prec == "fp32" else Conv2dBF16Function
    xg, wg = x.detach().requires_grad_(want_dx), w.detach().requires_grad_(True)
    y = fn.apply(xg, wg, s, pad)
    y.backward(dy)
    return y.detach(), xg.grad, wg.grad


def to_dev(t, prec):
    return t.to(ACT[prec]).to(DEV).contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------------- exact parity
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c", tc.CONV_CASES, ids=tc.conv_id)
def test_conv_exact_parity_on_integer_probes(c, prec):
    p = tc.build_probe(c)
    y, dx, dw = run_conv(prec, to_dev(p["x"], prec), p["w"].float().to(DEV), to_dev(p["dy"], prec), c.s, c.pad, c.k != 7)
    assert y.is_contiguous(memory_format=torch.channels_last)
    bad = [] if EXACT[prec](y, p["fwd"]) else ["fwd"]
    if c.k != 7 and not EXACT[prec](dx, p["dgrad"]):
        bad.append("dgrad")
    if not tc.exact_f32(dw, p["wgrad"]):
        bad.append("wgrad")
    for name in bad:
        got = {"fwd": y, "dgrad": dx, "wgrad": dw}[name].double().cpu()
        ref = p[name].to(ACT[prec]).double() if name != "wgrad" else p[name]
        print(f"{tc.conv_id(c)} {prec} {name}: {int((got != ref).sum())} of {ref.numel()} elements differ, first at "
              f"{(got != ref).nonzero()[:4].tolist()}, largest difference {float((got - ref).abs().max())}")
    assert not bad, (tc.conv_id(c), prec, bad)


REPLICATED = [(c, prec) for prec in PRECISIONS for c in tc.REAL_BATCH_CASES + tc.LARGE_CASES[prec]]


@pytest.mark.parametrize("c,prec", REPLICATED, ids=[f"{tc.conv_id(c)}-{prec}" for c, prec in REPLICATED])
def test_conv_exact_parity_on_replicated_batches(c, prec):
    """Batch 256 on every kernel path, and 64 -> 64 @ 112 x 112 at batches that put one tensor beyond 2^31 elements (fp32) or 2^32
    bytes (both).  Legal calls under check_desc; the comparison stays on the device."""
    if c in tc.LARGE_CASES[prec] and torch.cuda.mem_get_info(DEV)[0] < tc.LARGE_MIN_FREE_BYTES:
        pytest.skip(f"less than {tc.LARGE_MIN_FREE_BYTES} bytes of device memory free")
    p = tc.build_probe(c)
    idx = p["idx"].to(DEV)
    x = tc.replicate(p["x"].to(ACT[prec]).to(DEV), idx)
    dy = tc.replicate(p["dy"].to(ACT[prec]).to(DEV), idx)
    assert x.shape[0] == c.b and x.is_contiguous(memory_format=torch.channels_last)
    t0 = time.perf_counter()
    y, dx, dw = run_conv(prec, x, p["w"].float().to(DEV), dy, c.s, c.pad, c.k != 7)
    torch.cuda.synchronize()
    print(f"{tc.conv_id(c)} {prec}: x {x.numel()} elements, {x.numel() * x.element_size()} bytes; y {y.numel() * y.element_size()} bytes; "
          f"three passes {time.perf_counter() - t0:.2f} s")
    del x, dy
    ok = {"fwd": tc.exact_replicated(y, p["fwd"], idx, EXACT[prec]), "wgrad": tc.exact_f32(dw, p["wgrad"])}
    del y
    if c.k != 7:
        ok["dgrad"] = tc.exact_replicated(dx, p["dgrad"], idx, EXACT[prec])
    del dx
    torch.cuda.empty_cache()
    assert all(ok.values()), (tc.conv_id(c), prec, ok)


# ---------------------------------------------------------------------------------------------------- random operands
@pytest.mark.parametrize("c", tc.RANDOM_CASES, ids=tc.conv_id)
def test_conv_random_operands_fp32_against_float64(c):
    """test_conv_parity_against_float64's comparison and bounds (relative 1e-5, wgrad 3e-5) at odd and non-square shapes."""
    x, w, gy = tc.random_operands(c, bf16=False)
    ref = {"fwd": F.conv2d(x, w, stride=c.s, padding=c.pad), "wgrad": torch.nn.grad.conv2d_weight(x, w.shape, gy, stride=c.s, padding=c.pad)}
    if c.k != 7:
        ref["dgrad"] = torch.nn.grad.conv2d_input(x.shape, w, gy, stride=c.s, padding=c.pad)
    y, dx, dw = run_conv("fp32", to_dev(x, "fp32"), w.float().to(DEV), to_dev(gy, "fp32"), c.s, c.pad, c.k != 7)
    got = {"fwd": y, "dgrad": dx, "wgrad": dw}
    for name, r in ref.items():
        e = rel(got[name], r)
        bound = 3e-5 if name == "wgrad" else 1e-5
        print(f"{tc.conv_id(c)} {name}: HIP {e:.2e}")
        assert got[name].shape == r.shape and e <= bound, (name, e)


@pytest.mark.parametrize("c", tc.RANDOM_CASES, ids=tc.conv_id)
def test_conv_random_operands_bf16_against_float64(c):
    """test_bf16_conv_parity_against_float64's comparison and bounds (check_rounded; wgrad relative 3e-5) at the same shapes."""
    x, w, gy = tc.random_operands(c, bf16=True)
    y, dx, dw = run_conv("bf16", to_dev(x, "bf16"), w.float().to(DEV), to_dev(gy, "bf16"), c.s, c.pad, c.k != 7)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    print(tc.conv_id(c))
    check_rounded("fwd", y, F.conv2d(x, w, stride=c.s, padding=c.pad), F.conv2d(x.abs(), w.abs(), stride=c.s, padding=c.pad))
    if c.k != 7:
        assert dx.dtype == torch.bfloat16
        check_rounded("dgrad", dx, torch.nn.grad.conv2d_input(x.shape, w, gy, stride=c.s, padding=c.pad),
                      torch.nn.grad.conv2d_input(x.shape, w.abs(), gy.abs(), stride=c.s, padding=c.pad))
    assert dw.dtype == torch.float32
    e = rel(dw, torch.nn.grad.conv2d_weight(x, w.shape, gy, stride=c.s, padding=c.pad))
    print(f"  wgrad: rel {e:.2e}")
    assert dw.shape == w.shape and e <= 3e-5, e


# ---------------------------------------------------------------------------------------------------- BatchNorm
def _bn_parity(c, dtype):
    """The bodies of test_bn_parity_fp32_against_float64 / test_bn_parity_bf16_against_float64 on a case of the table."""
    relu = bool(c.flags & tc.BN_RELU)
    x, res, dy, p = tc.make_bn_case(c, dtype)
    got = nm.run_hip(x, res, dy, p, relu, dtype)
    got["save_mean"], got["save_invstd"] = nm.hip_saved_statistics(x, dtype)
    assert got["nbt"] == 1
    y64, _, stats = nm.ref_forward_bn(x, res, p, relu)
    mask = (got["y"].float().cpu() > 0).double() if relu else torch.ones_like(x)   # the device's own mask: no element is left out
    dx, dres, dgamma, dbeta = nm.ref_backward_bn(x, dy, mask, p)
    t32 = nm.torch_fp32(x, res, dy, mask, p, relu)
    print(f"{dtype} {tc.bn_id(c)}")
    if dtype == torch.float32:
        ref = {"y": y64, **stats, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
        if c.flags & tc.BN_ADD:
            ref["dres"] = dres
        for k, r in ref.items():
            nm.check32(k, got[k], r, t32[k])
        return
    assert got["y"].dtype == got["dx"].dtype == torch.bfloat16 and got["dgamma"].dtype == got["dbeta"].dtype == torch.float32
    dx_abs, dres_abs = nm.ref_backward_bn(x, dy, mask, p, absolute=True)
    check_rounded("y", got["y"], y64, nm.ref_forward_bn(x, res, p, relu, absolute=True))
    check_rounded("dx", got["dx"], dx, dx_abs)
    if c.flags & tc.BN_ADD:
        assert got["dres"].dtype == torch.bfloat16
        check_rounded("dres", got["dres"], dres, dres_abs)
    for k, r in {**stats, "dgamma": dgamma, "dbeta": dbeta}.items():   # fp32 quantities: the fp32 bound
        nm.check32(k, got[k], r, t32[k])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=PRECISIONS)
@pytest.mark.parametrize("c", tc.BN_CASES + tc.BN_REAL_BATCH_CASES, ids=tc.bn_id)
def test_bn_parity_across_the_contract(c, dtype):
    _bn_parity(c, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=PRECISIONS)
@pytest.mark.parametrize("c", tc.BN_DETERMINISM_CASES, ids=tc.bn_id)
def test_bn_is_deterministic_at_odd_shapes(c, dtype):
    """test_bn_is_deterministic's check at (C = 520, rows = 12,289) and (C = 8, rows = 3)."""
    shape = (c.b, c.c, c.h, c.w)
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(shape, generator=g) * 1.5 + 3).double()
    res, dy = torch.randn(shape, generator=g).double(), torch.randn(shape, generator=g).double()
    p = {k: torch.rand(shape[1], generator=g).double() + 0.5 for k in ("gamma", "beta", "rm", "rv")}
    outs = []
    for _ in range(2):
        o = nm.run_hip(x, res, dy, p, True, dtype)
        o["save_mean"], o["save_invstd"] = nm.hip_saved_statistics(x, dtype)
        outs.append(o)
    for k in ("y", "running_mean", "running_var", "save_mean", "save_invstd", "dx", "dres", "dgamma", "dbeta"):
        assert torch.equal(outs[0][k], outs[1][k]), k


# ---------------------------------------------------------------------------------------------------- non-finite locality
# (cin, cout, k, s, pad, h, w) and the non-finite input pixels (row, column).  The stem at the shipped 224 x 224 crop pads K with
# table entries; a padding entry that still named a tap (dy = -128, dx = 0) read x[2 oy - 131][2 ox - 3] for oy >= 66: pixel
# (51, 101) is that read of output (91, 52), whose own 7 x 7 window (rows 179..185) is nowhere near it.  (150, 100): a row beyond 128
# on an even column, which no stem window starts at.
LOCALITY = {"stem": ((12, 64, 7, 2, 3, 224, 224), [(51, 101), (150, 100)]), "k3s2": ((64, 64, 3, 2, 1, 161, 75), [(140, 33), (51, 50)])}


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("which", list(LOCALITY))
def test_non_finite_inputs_stay_local(which, prec, value):
    """A non-finite input pixel makes non-finite exactly the outputs whose window holds it (isfinite of the device output equals
    isfinite of F.conv2d in float64, element for element); the same for dW with a non-finite dy element."""
    (cin, cout, k, s, pad, h, w_), pixels = LOCALITY[which]
    g = torch.Generator().manual_seed(17)
    rnd = (lambda t: t.to(ACT[prec]).double())
    x0 = rnd(torch.randn(1, cin, h, w_, generator=g, dtype=torch.float64))
    w = rnd(torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5)
    ho, wo = (h + 2 * pad - k) // s + 1, (w_ + 2 * pad - k) // s + 1
    gy0 = rnd(torch.randn(1, cout, ho, wo, generator=g, dtype=torch.float64))
    for r, col in pixels:
        x = x0.clone()
        x[0, :, r, col] = value
        y, _, _ = run_conv(prec, to_dev(x, prec), w.float().to(DEV), to_dev(gy0, prec), s, pad, False)
        want = torch.isfinite(F.conv2d(x, w, stride=s, padding=pad))
        got = torch.isfinite(y).cpu()
        extra, missing = (~got & want).nonzero(), (got & ~want).nonzero()
        print(f"{which} {prec} {value} at ({r}, {col}): {int((~want).sum())} outputs see the pixel; the device has {len(extra)} more non-finite outputs "
              f"(first at [b, c, oy, ox] = {extra[:3].tolist()}) and lacks {len(missing)}")
        assert torch.equal(got, want), (which, prec, value, (r, col), len(extra), len(missing), extra[:3].tolist())
    # wgrad: one non-finite dy element, at an interior output pixel (every tap of its window lies inside the image)
    gy = gy0.clone()
    gy[0, 5, ho // 2 + 11, wo // 2 - 7] = value
    _, _, dw = run_conv(prec, to_dev(x0, prec), w.float().to(DEV), to_dev(gy, prec), s, pad, False)
    want = torch.isfinite(torch.nn.grad.conv2d_weight(x0, w.shape, gy, stride=s, padding=pad))
    got = torch.isfinite(dw).cpu()
    print(f"{which} {prec} {value} in dy: {int((~want).sum())} of {want.numel()} dW elements are non-finite in float64, {int((~got).sum())} on the device")
    assert int((~want).sum()) == cin * k * k and torch.equal(got, want), (which, prec, value)


# ---------------------------------------------------------------------------------------------------- one non-square training step
@pytest.mark.parametrize("norm", ["torch", "hip"])
def test_training_step_against_float64_non_square(norm):
    """test_training_step_against_float64's procedure and bound for ResNet-18 at a 4 x 3 x 96 x 160 input, with either norm in fp32."""
    layers, n_mod = 18, 1
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[n_mod])).set_train_norm(norm)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(4, 3, 96, 160, generator=g) for _ in range(2 * n_mod)]
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
    params = dict(model.named_parameters())
    for dt in (torch.float64, torch.float32):   # one Adam step from the GPU's own gradients, as the square test does
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
        if g64[k] is None:   # the trunk's own conv1 / fc: in the state dict, unused by the forward
            assert params[k].grad is None, k
        else:
            check(f"grad {k}", params[k].grad, g64[k], g32[k])
        check(f"adam {k}", params[k].detach(), p64[k], p32[k])
    sd = model.state_dict()
    for k in b64:
        if "running" in k:
            check(k, sd[k], b64[k], b32[k])
