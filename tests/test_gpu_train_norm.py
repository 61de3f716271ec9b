"""The opt-in HIP BatchNorm on the MI355X: every BatchNorm shape of the model against float64 in fp32 and bf16 (forward and
backward, with the fused ReLU and residual add), determinism, the eval form, whole training steps with set_train_norm("hip"), a
model that learns, and `python -m salve_amd.train --norm hip --precision bf16` end to end."""

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

from salve_amd import _lib, training  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import BatchNormHipFunction, TrainableEarlyFusionCEResnet, batch_norm_hip  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402
from tests.test_gpu_train import MODS, RENDERINGS, ref_forward, rel  # noqa: E402
from tests.test_gpu_train_bf16 import check_rounded  # noqa: E402
from tests.test_train_norm_host import BN_SHAPES  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")
RELU, ADD = _lib.BN_RELU, _lib.BN_ADD
EPS, MOMENTUM = 1e-5, 0.1
CASES = [(2, c, h, f) for c, h, f in BN_SHAPES] + [(64, 64, 56, RELU)]   # the last one: mu_c = 30 for every channel


def make_case(batch, c, h, flags, dtype):
    """Float64 CPU operands: x ~ N(mu_c, s_c) with mu_c up to 30 and s_c in [0.5, 2], random gamma, beta, residual, dy and running
    statistics.  dtype bfloat16: the activations (x, residual, dy) are rounded to bf16 first; the parameters stay fp32 values."""
    g = torch.Generator().manual_seed(c * 31 + h * 7 + flags + batch)
    mu = torch.full((c,), 30.0, dtype=torch.float64) if batch == 64 else 30.0 * torch.rand(c, generator=g, dtype=torch.float64)
    s = 0.5 + 1.5 * torch.rand(c, generator=g, dtype=torch.float64)
    x = torch.randn(batch, c, h, h, generator=g, dtype=torch.float64) * s[None, :, None, None] + mu[None, :, None, None]
    res = torch.randn(batch, c, h, h, generator=g, dtype=torch.float64) if flags & ADD else None
    dy = torch.randn(batch, c, h, h, generator=g, dtype=torch.float64)
    p = {"gamma": 0.5 + torch.rand(c, generator=g, dtype=torch.float64), "beta": torch.randn(c, generator=g, dtype=torch.float64),
         "rm": torch.randn(c, generator=g, dtype=torch.float64), "rv": 0.5 + torch.rand(c, generator=g, dtype=torch.float64)}
    p = {k: v.float().double() for k, v in p.items()}
    rnd = (lambda t: None if t is None else t.to(dtype).double())
    return rnd(x), rnd(res), rnd(dy), p


def ref_forward_bn(x, res, p, relu, absolute=False):
    """The train-mode arithmetic in x's dtype.  absolute: the same expression on absolute values (check_rounded's A)."""
    n = x.numel() // x.shape[1]
    mean = x.mean((0, 2, 3))
    var = x.var((0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + EPS)
    v = lambda t: t[None, :, None, None]   # noqa: E731
    if absolute:
        y = v(p["gamma"].abs() * invstd) * (x.abs() + v(mean.abs())) + v(p["beta"].abs())
        return y if res is None else y + res.abs()
    xhat = (x - v(mean)) * v(invstd)
    y = v(p["gamma"]) * xhat + v(p["beta"])
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    stats = {"save_mean": mean, "save_invstd": invstd, "running_mean": (1 - MOMENTUM) * p["rm"] + MOMENTUM * mean,
             "running_var": (1 - MOMENTUM) * p["rv"] + MOMENTUM * var * n / (n - 1)}
    return y, xhat, stats


def ref_backward_bn(x, dy, mask, p, absolute=False):
    """dx, dres, dgamma, dbeta with the ReLU mask given (the device's own y > 0)."""
    n = x.numel() // x.shape[1]
    v = lambda t: t[None, :, None, None]   # noqa: E731
    mean = x.mean((0, 2, 3))
    invstd = 1 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + EPS)
    g = dy * mask
    if absolute:
        g, xhat, gamma = g.abs(), (x.abs() + v(mean.abs())) * v(invstd), p["gamma"].abs()
        dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
        return v(gamma * invstd) * (g + v(dbeta) / n + xhat * v(dgamma) / n), g
    xhat = (x - v(mean)) * v(invstd)
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
    dx = v(p["gamma"] * invstd) * (g - v(dbeta) / n - xhat * v(dgamma) / n)
    return dx, g, dgamma, dbeta


def run_hip(x, res, dy, p, relu, dtype, training=True):
    """BatchNormHipFunction on the device: returns y, the updated buffers and the gradients."""
    cl = lambda t: t.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)   # noqa: E731
    xg = cl(x).requires_grad_(True)
    rg = None if res is None else cl(res).requires_grad_(True)
    gamma, beta = p["gamma"].float().to(DEV).requires_grad_(True), p["beta"].float().to(DEV).requires_grad_(True)
    rm, rv = p["rm"].float().to(DEV), p["rv"].float().to(DEV)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    y = BatchNormHipFunction.apply(xg, rg, gamma, beta, rm, rv, nbt, relu, EPS, MOMENTUM, training)
    out = {"y": y.detach(), "running_mean": rm, "running_var": rv, "nbt": int(nbt)}
    if training:
        y.backward(cl(dy))
        out.update(dx=xg.grad, dres=None if rg is None else rg.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return out


def hip_saved_statistics(x, dtype):
    """save_mean / save_invstd straight from the C entry (the autograd function keeps them to itself)."""
    import ctypes

    lib = _lib.load()
    b, c, h, w = x.shape
    xn = x.to(dtype).to(DEV).permute(0, 2, 3, 1).contiguous()
    desc = _lib.BnDesc(b * h * w, c, 0, EPS, MOMENTUM)
    nbytes = int(lib.salve_bn_workspace_bytes(ctypes.byref(desc), _lib.BN_FWD))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    mean, invstd, y = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty_like(xn)
    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())   # noqa: E731
    fn = lib.salve_bn_f32_forward if dtype == torch.float32 else lib.salve_bn_bf16_forward
    st = fn(ctypes.byref(desc), ptr(xn), ptr(None), ptr(gamma), ptr(beta), ptr(None), ptr(None), ptr(y), ptr(mean), ptr(invstd), ptr(ws), nbytes,
            ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _lib.check(st, "salve_bn_forward")
    return mean, invstd


def check32(what, got, r64, r32):
    """test_training_step_against_float64's bound: e <= max(10 * e32, 1e-5), e32 = torch's fp32 CPU error on the same case."""
    e, e32 = rel(got, r64), rel(r32, r64)
    print(f"  {what}: HIP {e:.2e}  torch-CPU-fp32 {e32:.2e}")
    assert got.shape == r64.shape, what
    assert e <= max(10 * e32, 1e-5), (what, e, e32)


def torch_fp32(x, res, dy, mask, p, relu):
    """torch's own fp32 CPU BatchNorm on the same case (native_batch_norm returns the saved statistics)."""
    x32, rm, rv = x.float(), p["rm"].float().clone(), p["rv"].float().clone()
    gamma, beta = p["gamma"].float(), p["beta"].float()
    y, sm, si = torch.native_batch_norm(x32, gamma, beta, rm, rv, True, MOMENTUM, EPS)
    if res is not None:
        y = y + res.float()
    if relu:
        y = F.relu(y)
    out = {"y": y, "save_mean": sm, "save_invstd": si, "running_mean": rm, "running_var": rv}
    if dy is not None:
        g = dy.float() * mask.float()
        dx, dgamma, dbeta = torch.ops.aten.native_batch_norm_backward(g, x32, gamma, rm, rv, sm, si, True, EPS, [True, True, True])
        out.update(dx=dx, dres=g, dgamma=dgamma, dbeta=dbeta)
    return out


IDS = [f"b{b}-c{c}-h{h}-f{f}" for b, c, h, f in CASES]


@pytest.mark.parametrize("batch,c,h,flags", CASES, ids=IDS)
def test_bn_parity_fp32_against_float64(batch, c, h, flags):
    relu = bool(flags & RELU)
    x, res, dy, p = make_case(batch, c, h, flags, torch.float32)
    got = run_hip(x, res, dy, p, relu, torch.float32)
    got["save_mean"], got["save_invstd"] = hip_saved_statistics(x, torch.float32)
    assert got["nbt"] == 1
    y64, _, stats = ref_forward_bn(x, res, p, relu)
    mask = (got["y"].cpu() > 0).double() if relu else torch.ones_like(x)   # the device's own mask: no element is left out
    dx, dres, dgamma, dbeta = ref_backward_bn(x, dy, mask, p)
    ref = {"y": y64, **stats, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}
    if flags & ADD:
        ref["dres"] = dres
    t32 = torch_fp32(x, res, dy, mask, p, relu)
    print(f"fp32 batch {batch} C {c} H {h} flags {flags}")
    for k, r in ref.items():
        check32(k, got[k], r, t32[k])


@pytest.mark.parametrize("batch,c,h,flags", CASES, ids=IDS)
def test_bn_parity_bf16_against_float64(batch, c, h, flags):
    relu = bool(flags & RELU)
    x, res, dy, p = make_case(batch, c, h, flags, torch.bfloat16)
    got = run_hip(x, res, dy, p, relu, torch.bfloat16)
    got["save_mean"], got["save_invstd"] = hip_saved_statistics(x, torch.bfloat16)
    assert got["y"].dtype == got["dx"].dtype == torch.bfloat16 and got["dgamma"].dtype == got["dbeta"].dtype == torch.float32
    y64, _, stats = ref_forward_bn(x, res, p, relu)
    mask = (got["y"].float().cpu() > 0).double() if relu else torch.ones_like(x)
    dx, dres, dgamma, dbeta = ref_backward_bn(x, dy, mask, p)
    dx_abs, dres_abs = ref_backward_bn(x, dy, mask, p, absolute=True)
    t32 = torch_fp32(x, res, dy, mask, p, relu)
    print(f"bf16 batch {batch} C {c} H {h} flags {flags}")
    check_rounded("y", got["y"], y64, ref_forward_bn(x, res, p, relu, absolute=True))
    check_rounded("dx", got["dx"], dx, dx_abs)
    if flags & ADD:
        assert got["dres"].dtype == torch.bfloat16
        check_rounded("dres", got["dres"], dres, dres_abs)
    for k, r in {**stats, "dgamma": dgamma, "dbeta": dbeta}.items():   # fp32 quantities: the fp32 bound
        check32(k, got[k], r, t32[k])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 256, 56, 56), (256, 2048, 7, 7)], ids=["8x256x56", "256x2048x7"])
def test_bn_is_deterministic(shape, dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(shape, generator=g) * 1.5 + 3).double()
    res, dy = torch.randn(shape, generator=g).double(), torch.randn(shape, generator=g).double()
    p = {k: torch.rand(shape[1], generator=g).double() + 0.5 for k in ("gamma", "beta", "rm", "rv")}
    outs = []
    for _ in range(2):
        o = run_hip(x, res, dy, p, True, dtype)
        o["save_mean"], o["save_invstd"] = hip_saved_statistics(x, dtype)
        outs.append(o)
    for k in ("y", "running_mean", "running_var", "save_mean", "save_invstd", "dx", "dres", "dgamma", "dbeta"):
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,h,flags", [(64, 56, RELU), (256, 56, ADD | RELU), (512, 28, 0)])
def test_bn_eval_form(c, h, flags, dtype):
    relu = bool(flags & RELU)
    x, res, _, p = make_case(2, c, h, flags, dtype)
    got = run_hip(x, res, None, p, relu, dtype, training=False)
    assert got["nbt"] == 0 and torch.equal(got["running_mean"].cpu(), p["rm"].float()) and torch.equal(got["running_var"].cpu(), p["rv"].float())
    v = lambda t: t[None, :, None, None]   # noqa: E731
    invstd = 1 / torch.sqrt(p["rv"] + EPS)
    y64 = v(p["gamma"] * invstd) * (x - v(p["rm"])) + v(p["beta"])
    a = v(p["gamma"].abs() * invstd) * (x.abs() + v(p["rm"].abs())) + v(p["beta"].abs())
    y32 = F.batch_norm(x.float(), p["rm"].float(), p["rv"].float(), p["gamma"].float(), p["beta"].float(), False, MOMENTUM, EPS)
    if res is not None:
        y64, a, y32 = y64 + res, a + res.abs(), y32 + res.float()
    if relu:
        y64, y32 = F.relu(y64), F.relu(y32)
    if dtype == torch.float32:
        check32("eval y", got["y"], y64, y32)
    else:
        check_rounded("eval y", got["y"], y64, a)
    # through the module: eval mode under no_grad leaves the buffers alone; with gradients enabled the eval form refuses to differentiate
    bn = torch.nn.BatchNorm2d(c).to(DEV).eval()
    with torch.no_grad():
        bn.running_mean.copy_(p["rm"]), bn.running_var.copy_(p["rv"]), bn.weight.copy_(p["gamma"]), bn.bias.copy_(p["beta"])
    xg = x.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = batch_norm_hip(bn, xg, None if res is None else res.to(dtype).to(DEV), relu)
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.cpu(), p["rm"].float())
    assert torch.equal(y, got["y"])


# ---------------------------------------------------------------------------------------------------- whole training step
@pytest.mark.parametrize("layers,n_mod", [(18, 1), (50, 2)])
def test_training_step_with_hip_norm_against_float64(layers, n_mod):
    """tests/test_gpu_train.py::test_training_step_against_float64's procedure and bound with set_train_norm("hip")."""
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[n_mod])).set_train_norm("hip")
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(4, 3, 112, 112, generator=g) for _ in range(2 * n_mod)]
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
    for dt in (torch.float64, torch.float32):   # one Adam step from the GPU's own gradients, as the fp32 test does
        p = {k: sd0[k].to(dt).clone().requires_grad_(True) for k in names}
        for k in names:
            p[k].grad = None if params[k].grad is None else params[k].grad.detach().cpu().to(dt)
        torch.optim.Adam([p[k] for k in names], lr=1e-3, weight_decay=1e-4).step()
        res[dt] = res[dt][:4] + ({k: p[k].detach() for k in names},)
    (lg64, ls64, g64, b64, p64), (lg32, ls32, g32, b32, p32) = res[torch.float64], res[torch.float32]
    worst = [0.0, ""]

    def check(what, got, r64, r32):
        e, e32 = rel(got, r64), rel(r32, r64)
        if e / max(10 * e32, 1e-5) > worst[0]:
            worst[:] = [e / max(10 * e32, 1e-5), f"{what}: HIP {e:.2e} torch-CPU-fp32 {e32:.2e}"]
        assert e <= max(10 * e32, 1e-5), (what, e, e32)

    check("logits", logits.detach(), lg64, lg32)
    check("loss", loss.detach().reshape(1), ls64.reshape(1), ls32.reshape(1))
    for k in names:
        if g64[k] is None:
            assert params[k].grad is None, k
        else:
            check(f"grad {k}", params[k].grad, g64[k], g32[k])
        check(f"adam {k}", params[k].detach(), p64[k], p32[k])
    sd = model.state_dict()
    for k in b64:
        if "running" in k:
            check(k, sd[k], b64[k], b32[k])
        if "num_batches_tracked" in k:
            assert int(sd[k]) == 1, k
    print(f"resnet{layers}: closest to its bound: {worst[1]} ({worst[0]:.2f} of the bound)")


@pytest.mark.parametrize("layers,loss_bound,cos_bound", [(18, 2e-2, 0.9), (50, 5e-2, None)])
def test_bf16_hip_norm_step_against_fp32_torch_norm_step(layers, loss_bound, cos_bound):
    """tests/test_gpu_train_bf16.py::test_bf16_step_against_fp32_step's bounds and reasoning for the bf16 step with the HIP norm; the
    shipped bf16 step with torch's norm is measured beside it in the same run (printed, not asserted here)."""
    torch.manual_seed(0)
    m32 = TrainableEarlyFusionCEResnet(layers, False, 2, SimpleNamespace(modalities=MODS[1])).to(DEV).train()
    m16t = copy.deepcopy(m32).set_train_precision("bf16")
    m16 = copy.deepcopy(m32).set_train_precision("bf16").set_train_norm("hip")
    stats0 = {k: v.clone() for k, v in m16.state_dict().items() if "running" in k}
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(8, 3, 224, 224, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=DEV)
    losses, grads = [], []
    for m in (m32, m16t, m16):
        logits = m(*xs)
        assert logits.dtype == torch.float32
        loss = F.cross_entropy(logits, y)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]))
    d_loss = [abs(v - losses[0]) / abs(losses[0]) for v in losses]
    cos = [float(F.cosine_similarity(grads[0].double(), gr.double(), dim=0)) for gr in grads]
    print(f"resnet{layers}: loss fp32 {losses[0]:.6f}; bf16 torch norm {losses[1]:.6f} (relative difference {d_loss[1]:.2e}, gradient cosine "
          f"{cos[1]:.6f}); bf16 hip norm {losses[2]:.6f} (relative difference {d_loss[2]:.2e}, gradient cosine {cos[2]:.6f})")
    assert d_loss[2] <= loss_bound, d_loss
    assert bool(torch.isfinite(grads[2]).all())
    if cos_bound is not None:
        assert cos[2] >= cos_bound, cos
    assert all(p.dtype == torch.float32 for p in m16.parameters())
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in m16.parameters())
    sd = m16.state_dict()
    assert all(v.dtype == torch.float32 for k, v in sd.items() if "num_batches" not in k)
    assert all(not torch.equal(sd[k], v) for k, v in stats0.items()), "running statistics not updated"
    assert all(int(v) == 1 for k, v in sd.items() if "num_batches" in k)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resnet18_learns_a_fixed_batch_with_hip_norm(precision):
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).set_train_precision(precision)
    model = model.set_train_norm("hip").to(DEV).train()
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
    print(f"{precision} hip norm: loss after 40 steps {loss.item():.4f}, accuracy {acc}")
    assert loss.item() < 0.1 and acc == 1.0


def test_train_cli_hip_norm_bf16_end_to_end(tmp_path):
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
                        "--data-root", str(root), "--seed", "0", "--out", str(out), "--precision", "bf16", "--norm", "hip"], cwd=str(ROOT),
                       capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"}
    assert all(v.dtype == torch.float32 for k, v in ck["state_dict"].items() if "num_batches" not in k)
    assert all(bool(torch.isfinite(v).all()) for k, v in ck["state_dict"].items() if "num_batches" not in k)
    res = json.loads((out / "results-e2e.json").read_text())
    assert set(res) == {"train_avg_loss", "train_mAcc", "val_avg_loss", "val_mAcc"} and all(len(v) == 2 for v in res.values())
    inf = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["ceiling_rgb_texture", "floor_rgb_texture"]))
    inf.load_state_dict(ck["state_dict"], strict=True)
