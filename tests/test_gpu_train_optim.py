"""HipAdam on the MI355X: one launch over every parameter against the float64 reference (tests/optim_cases.py), within 10 x the
error of torch's own fp32 Adam on the same inputs; fresh gradient tensors every step, a late parameter, param groups and a
changing lr, state dicts exchanged with torch.optim.Adam, the bf16 shadows bit for bit, determinism, and training end to end.

Every comparison prints its worst error / bound and error / torch's fp32 error (`_check`); DESIGN.md section 4.15 records them."""

import copy
import ctypes
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from salve_amd import _lib, optim, training  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet  # noqa: E402
from salve_amd.optim import CHUNK, HipAdam  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402
from tests import optim_cases as oc  # noqa: E402
from tests.test_gpu_train import MODS, RENDERINGS  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")
GUARD = 12345.0
CONTRACT = [1, 2, 3, 4, 5, 63, 64, 65, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
MISALIGNED = 9   # index into the sizes: this parameter (257 elements) starts one element into a 16-byte group


def _check(got, ref, t32, what):
    """p, exp_avg, exp_avg_sq of every tensor against float64 within oc.bound; prints the worst ratios first."""
    worst, worst32, bad = 0.0, 0.0, []
    for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
        for i, r in enumerate(ref[q]):
            if r is None:
                assert got[q][i] is None, (what, name, i)
                continue
            e, e32, b = oc.err(got[q][i], r), oc.err(t32[q][i], r), oc.bound(r, t32[q][i])
            worst = max(worst, e / b)
            if e32 > 0:
                worst32 = max(worst32, e / e32)
            if not e <= b:
                bad.append((name, i, r.size, e, b))
    print(f"{what}: worst error / bound {worst:.3f}; worst error / torch fp32 error {worst32:.3f}; {len(bad)} tensors over the bound")
    assert not bad, (what, bad[:5])


def _layout(sizes, misaligned=()):
    """Element offsets of the tensors in one flat storage: each starts on a 16-byte group (plus one element for `misaligned`)
    with at least 4 guard elements before and after it.  Returns (offsets, total)."""
    offs, end = [], 0
    for i, n in enumerate(sizes):
        o = (end + 4 + 3) // 4 * 4 + (1 if i in misaligned else 0)
        offs.append(o)
        end = o + n
    return offs, end + 8


def _flat(values, sizes, offs, total):
    buf = np.full(total, GUARD, dtype=np.float32)
    for v, n, o in zip(values, sizes, offs):
        buf[o:o + n] = 0.0 if v is None else v
    return torch.from_numpy(buf).to(DEV)


def _run_guarded(sizes, params, grads, misaligned=(MISALIGNED,)):
    """STEPS HipAdam steps with parameters, gradients and both moments as views into guarded flat storages.  Returns
    ((p, m, v) lists of numpy arrays, the four storages' guard elements untouched?)."""
    offs, total = _layout(sizes, misaligned)
    pf = _flat(params, sizes, offs, total)
    mf, vf = _flat([None] * len(sizes), sizes, offs, total), _flat([None] * len(sizes), sizes, offs, total)
    gfs = [_flat(g, sizes, offs, total) for g in grads]
    ps = [torch.nn.Parameter(pf[o:o + n]) for n, o in zip(sizes, offs)]
    opt = HipAdam(ps, lr=oc.LR, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    for p, n, o in zip(ps, sizes, offs):   # (a loaded state: the moments live where the test can see their neighbours)
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": mf[o:o + n], "exp_avg_sq": vf[o:o + n]}
    assert ps[MISALIGNED].data_ptr() % 16 == 4 and ps[0].data_ptr() % 16 == 0
    for gf in gfs:
        for p, n, o in zip(ps, sizes, offs):
            p.grad = gf[o:o + n]
        opt.step()
    torch.cuda.synchronize()
    mask = np.ones(total, dtype=bool)
    for n, o in zip(sizes, offs):
        mask[o:o + n] = False
    guards_ok = all(bool((f.cpu().numpy()[mask] == np.float32(GUARD)).all()) for f in [pf, mf, vf] + gfs)
    grads_ok = all(np.array_equal(gf.cpu().numpy()[o:o + n], g[i]) for gf, g in zip(gfs, grads) for i, (n, o) in enumerate(zip(sizes, offs)))
    out = tuple([f.cpu().numpy()[o:o + n].copy() for n, o in zip(sizes, offs)] for f in (pf, mf, vf))
    assert all(float(opt.state[p]["step"]) == len(grads) for p in ps)
    return out, guards_ok and grads_ok


@pytest.fixture(scope="module")
def contract():
    """The shape-contract problem, its float64 reference and torch's fp32 CPU result (computed once), and one HipAdam run."""
    rng = np.random.default_rng(1)
    sizes = CONTRACT + [int(n) for n in rng.integers(1, 8, 1200)]
    params, grads = oc.make_problem(sizes, seed=2)
    ref = oc.adam_f64(params, grads)
    t32 = oc.torch_adam(params, grads, torch.float32)
    got, untouched = _run_guarded(sizes, params, grads)
    return SimpleNamespace(sizes=sizes, params=params, grads=grads, ref=ref, t32=t32, got=got, untouched=untouched)


def test_shape_contract_in_one_step(contract):
    """1214 tensors in one launch per step: every path of the kernel (a lone element, tails, whole vectors, a full chunk, chunk
    boundaries, several chunks, the 4-byte-aligned path), three steps, against float64; nothing outside the tensors is written and
    the gradients are only read."""
    assert len(contract.sizes) == 1214
    _check(contract.got, contract.ref, contract.t32, "shape contract")
    assert contract.untouched, "an element outside the tensors (or a gradient) was written"


def test_same_inputs_give_the_same_bits(contract):
    again, _ = _run_guarded(contract.sizes, contract.params, contract.grads)
    for a, b in zip(contract.got, again):
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _steps(opt, ps, grads, keep=None):
    """Steps with freshly allocated gradient tensors (`keep` holds the old ones alive)."""
    for step_grads in grads:
        for p, g in zip(ps, step_grads):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
            if keep is not None and p.grad is not None:
                keep.append(p.grad)
        opt.step()


def _state(opt, ps):
    torch.cuda.synchronize()
    return ([p.detach().cpu().numpy() for p in ps],
            [opt.state[p]["exp_avg"].cpu().numpy() if p in opt.state and len(opt.state[p]) else None for p in ps],
            [opt.state[p]["exp_avg_sq"].cpu().numpy() if p in opt.state and len(opt.state[p]) else None for p in ps])


def _params(params):
    return [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in params]


SIZES = [3 * CHUNK + 5, 257, 64, 7]


def test_gradient_tensors_are_new_every_step():
    """zero_grad() frees the gradients, backward allocates new ones: the step must read THIS step's.  The old tensors stay alive, so
    no new gradient can land on an old address; a table built once would read step 1's values again."""
    params, grads = oc.make_problem(SIZES, seed=3)
    ps, keep = _params(params), []
    opt = HipAdam(ps, lr=oc.LR, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    _steps(opt, ps, grads, keep=keep)
    assert len({g.data_ptr() for g in keep}) == len(keep) == oc.STEPS * len(SIZES)
    _check(_state(opt, ps), oc.adam_f64(params, grads), oc.torch_adam(params, grads, torch.float32), "fresh gradients")


def test_late_parameter_keeps_its_own_step_count():
    params, grads = oc.make_problem(SIZES, seed=4)
    grads[0][1] = grads[1][1] = None
    ps = _params(params)
    opt = HipAdam(ps, lr=oc.LR, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    _steps(opt, ps, grads[:2])
    assert ps[1] not in opt.state or len(opt.state[ps[1]]) == 0
    assert np.array_equal(ps[1].detach().cpu().numpy(), params[1])
    _steps(opt, ps, grads[2:])
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0, 1.0, 3.0, 3.0]
    ref = oc.adam_f64(params, grads)
    assert ref[3] == [3, 1, 3, 3]
    _check(_state(opt, ps), ref, oc.torch_adam(params, grads, torch.float32), "late parameter")


def test_param_groups_and_a_changing_lr():
    lr = lambda k, i: (oc.LR if i < 2 else 3e-3) * (1.0 - k / 4.0) ** 0.9   # noqa: E731  (two groups, the poly schedule)
    wd = lambda k, i: oc.WEIGHT_DECAY if i < 2 else 0.0   # noqa: E731
    params, grads = oc.make_problem(SIZES, seed=5)
    ps = _params(params)
    opt = HipAdam([{"params": ps[:2]}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.0}], lr=oc.LR, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    for k, step_grads in enumerate(grads):
        for group, base in zip(opt.param_groups, (oc.LR, 3e-3)):   # as run_epoch writes it
            group["lr"] = base * (1.0 - k / 4.0) ** 0.9
        _steps(opt, ps, [step_grads])
    _check(_state(opt, ps), oc.adam_f64(params, grads, lr=lr, weight_decay=wd), oc.torch_adam(params, grads, torch.float32, lr=lr, weight_decay=wd),
           "two groups, lr per step")


@pytest.mark.parametrize("order", ["torch_then_hip", "hip_then_torch"])
def test_state_dicts_move_between_torch_adam_and_hip_adam(order):
    params, grads = oc.make_problem(SIZES, steps=4, seed=6)
    ps = _params(params)
    kw = dict(lr=oc.LR, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    first, second = (torch.optim.Adam, HipAdam) if order == "torch_then_hip" else (HipAdam, torch.optim.Adam)
    a = first(ps, **kw)
    _steps(a, ps, grads[:2])
    sd = copy.deepcopy(a.state_dict())
    b = second(ps, lr=1.0, eps=1.0, weight_decay=1.0)   # (everything comes from the state dict)
    b.load_state_dict(sd)
    assert type(b.param_groups[0]["lr"]) is float and b.param_groups[0]["lr"] == oc.LR
    _steps(b, ps, grads[2:])
    assert [float(b.state[p]["step"]) for p in ps] == [4.0] * len(ps)
    _check(_state(b, ps), oc.adam_f64(params, grads), oc.torch_adam(params, grads, torch.float32), order)
    # the two state dicts after the same steps: the same keys, types, dtypes and devices
    qs = _params(params)
    t = torch.optim.Adam(qs, **kw)
    h = HipAdam(_params(params), **kw)
    _steps(t, qs, grads[:1])
    _steps(h, h.param_groups[0]["params"], grads[:1])
    st, sh = t.state_dict(), h.state_dict()
    assert st["param_groups"] == sh["param_groups"] and set(st["state"]) == set(sh["state"])
    for i in st["state"]:
        assert set(st["state"][i]) == set(sh["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in st["state"][i]:
            x, y = st["state"][i][k], sh["state"][i][k]
            assert type(x) is type(y) and x.dtype == y.dtype and x.device == y.device and x.shape == y.shape, (i, k)


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu()


def test_shadow_is_the_bf16_cast_bit_for_bit():
    """Special values sit in the parameter before a zero-gradient step without weight decay (the update leaves them as they are):
    ties at bf16's half ulp both ways, the largest float (rounds to infinity), NaN, +-inf, denormals, -0."""
    special = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
                        np.finfo(np.float32).max, float("nan"), float("inf"), float("-inf"), 1e-40, -1e-40, 1.4e-45, 2.0 ** -126 - 2.0 ** -149,
                        2.0 ** -134 + 2.0 ** -142, -0.0, 0.0, 3.0e38, 0.1], dtype=np.float32)
    rng = np.random.default_rng(8)
    body = rng.standard_normal(CHUNK + 6 - special.size).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(np.concatenate([special, body])).to(DEV).reshape(-1, 1, 1, 2))
    before = p.detach().clone()
    opt = HipAdam([p], lr=oc.LR, eps=oc.EPS, weight_decay=0.0, bf16_shadow=True)
    assert optim.current_shadow(p) is None   # before the first step there is none
    p.grad = torch.zeros_like(p)
    opt.step()
    sh = optim.current_shadow(p)
    assert sh is not None and sh.dtype == torch.bfloat16 and sh.shape == p.shape
    assert torch.equal(p.detach().view(torch.int32), before.view(torch.int32))   # untouched, NaN and infinities included
    assert torch.equal(_bits16(sh), _bits16(p.detach().to(torch.bfloat16)))
    p.grad = torch.from_numpy(oc.mixed_scale(rng, tuple(p.shape))).to(DEV)   # a real step: the values that were just computed
    p.grad.view(-1)[:special.size] = 0
    opt.step()
    sh = optim.current_shadow(p)
    assert sh is not None and torch.equal(_bits16(sh), _bits16(p.detach().to(torch.bfloat16)))
    assert not torch.equal(p.detach()[special.size:], before[special.size:])
    v = HipAdam([torch.nn.Parameter(torch.zeros(8, device=DEV))], bf16_shadow=True)   # not 4-D: no shadow
    q = v.param_groups[0]["params"][0]
    q.grad = torch.ones_like(q)
    v.step()
    assert optim.current_shadow(q) is None and int(v.plan()[0]["shadow_bf16"][0]) == 0


def _resnet18_pair(hw, batch=2):
    torch.manual_seed(0)
    a = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).set_train_precision("bf16").set_train_norm("hip").to(DEV).train()
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(batch, 3, hw, hw, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1] * (batch // 2), device=DEV)
    return a, b, xs, y


def _train_step(model, opt, xs, y):
    loss = F.cross_entropy(model(*xs), y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


def test_bf16_step_with_shadows_is_bit_identical_to_the_step_without():
    a, b, xs, y = _resnet18_pair(224)
    oa = HipAdam(a.parameters(), lr=1e-3, weight_decay=1e-4, bf16_shadow=True)
    ob = HipAdam(b.parameters(), lr=1e-3, weight_decay=1e-4, bf16_shadow=False)
    for k in range(3):
        la, lb = _train_step(a, oa, xs, y), _train_step(b, ob, xs, y)
        assert torch.equal(la, lb), (k, float(la), float(lb))
        stepped = [p for p in a.parameters() if p.dim() == 4 and p in oa.state]
        assert len(stepped) == 20 and all(optim.current_shadow(p) is not None for p in stepped)   # the shadows ARE what the next forward reads
        assert all(optim.current_shadow(p) is None for p in b.parameters())
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    assert optim.current_shadow(a.resnet.conv1.weight) is None   # (never receives a gradient: no state, no shadow)


@pytest.mark.parametrize("write", ["mul_", "load_state_dict", "copy_"])
def test_a_stale_shadow_is_never_used(write):
    a, b, xs, y = _resnet18_pair(112)
    oa = HipAdam(a.parameters(), lr=1e-3, bf16_shadow=True)
    ob = HipAdam(b.parameters(), lr=1e-3)
    _train_step(a, oa, xs, y)
    _train_step(b, ob, xs, y)
    w = a.resnet.layer1[0].conv1.weight
    assert optim.current_shadow(w) is not None
    for m in (a, b):
        with torch.no_grad():
            if write == "mul_":
                m.resnet.layer1[0].conv1.weight.mul_(2)
            elif write == "copy_":
                m.resnet.layer1[0].conv1.weight.copy_(torch.full_like(w, 0.01))
            else:
                sd = {k: (v * 0.5 if v.dim() == 4 else v.clone()) for k, v in m.state_dict().items()}
                m.load_state_dict(sd, strict=True)
    assert optim.current_shadow(w) is None
    assert optim.current_shadow(a.resnet.layer2[0].conv1.weight) is (None if write == "load_state_dict" else oa._shadows[id(a.resnet.layer2[0].conv1.weight)])
    with torch.no_grad():
        la, lb = a(*xs), b(*xs)
    assert torch.equal(la, lb)
    assert torch.equal(_train_step(a, oa, xs, y), _train_step(b, ob, xs, y))   # and the next step writes them afresh
    assert optim.current_shadow(w) is not None


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resnet18_learns_a_fixed_batch_with_hip_adam(precision):
    """tests/test_gpu_train.py::test_resnet18_learns_a_fixed_batch (and its bf16 twin) with get_optimizer(..., optim="hip"): the
    same batch, steps and criterion."""
    torch.manual_seed(0)
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).set_train_precision(precision).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(8, 3, 112, 112, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1, 0, 1, 1, 0, 0, 1]).to(DEV)
    opt = training.get_optimizer(SimpleNamespace(optimizer_algo="adam", base_lr=1e-3, weight_decay=0.0), model, optim="hip")
    assert type(opt) is HipAdam and opt.bf16_shadow == (precision == "bf16")
    for _ in range(40):
        probs, loss = training.cross_entropy_forward(model, "train", xs[0], xs[1], None, None, None, None, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        probs, loss = training.cross_entropy_forward(model, "train", xs[0], xs[1], None, None, None, None, y)
    acc = float((probs.argmax(1) == y).float().mean())
    print(f"{precision}, HipAdam: loss after 40 steps {loss.item():.4f}, accuracy {acc}")
    assert loss.item() < 0.1 and acc == 1.0


def test_train_cli_with_hip_adam_end_to_end(tmp_path):
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
    r = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", str(cfg), "--epochs", "1", "--batch-size", "2",
                        "--data-root", str(root), "--seed", "0", "--out", str(out), "--precision", "bf16", "--norm", "hip", "--optim", "hip"],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    ck = torch.load(out / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "max_epochs", "curr_val_mAcc", "best_so_far_val_mAcc"}
    res = json.loads((out / "results-e2e.json").read_text())
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in res.values())
    from tests.test_gpu_train import config

    model = EarlyFusionCEResnet(18, False, 2, config(str(root)))
    model.load_state_dict(ck["state_dict"], strict=True)
    adam = torch.optim.Adam(model.parameters(), lr=1.0)
    adam.load_state_dict(ck["optimizer"])   # torch's format: groups and per-parameter state
    assert adam.param_groups[0]["lr"] < 1e-3 and adam.param_groups[0]["weight_decay"] == 1e-4
    stepped = [p for p in model.parameters() if p in adam.state]
    assert stepped and len(stepped) < len(list(model.parameters()))   # (conv1 / fc of the inner resnet never had a gradient)
    assert all(set(adam.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(adam.state[p]["step"]) >= 1 for p in stepped)
    for p in stepped:
        p.grad = torch.zeros_like(p)
    adam.step()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_abi_refuses_bad_tables():
    lib = _lib.load()
    table = torch.zeros(80 * 2, dtype=torch.uint8, device=DEV)
    vp = ctypes.c_void_p
    assert lib.salve_adam_step(vp(None), 1, vp(table.data_ptr()), 0, vp(None), vp(None), vp(None)) == _lib.SALVE_ERR_BAD_ARG
    assert lib.salve_adam_step(vp(table.data_ptr()), -1, vp(table.data_ptr()), 0, vp(None), vp(None), vp(None)) == _lib.SALVE_ERR_BAD_ARG
    assert lib.salve_adam_step(vp(table.data_ptr()), 1, vp(table.data_ptr()), -1, vp(None), vp(None), vp(None)) == _lib.SALVE_ERR_BAD_ARG
    assert lib.salve_adam_step(vp(table.data_ptr()), 1, vp(None), 1, vp(None), vp(None), vp(None)) == _lib.SALVE_ERR_BAD_ARG
    assert lib.salve_adam_step(vp(table.data_ptr()), 1, vp(None), 0, vp(None), vp(None), vp(None)) == _lib.SALVE_OK   # nothing to do
    # a chunk outside its segment, seen through the host copies
    p = torch.zeros(8, device=DEV)
    seg = optim.Segment(p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), 0, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    t, c = optim.build_tables([seg])
    for field, value in (("offset", CHUNK), ("offset", -CHUNK), ("offset", 4), ("segment", 1), ("segment", -1)):
        bad = c.copy()
        bad[field][0] = value
        st = lib.salve_adam_step(vp(table.data_ptr()), 1, vp(table.data_ptr() + 80), 1, vp(t.ctypes.data), vp(bad.ctypes.data), vp(None))
        assert st == _lib.SALVE_ERR_BAD_ARG, (field, value)
        assert b"chunk" in lib.salve_last_error()
    torch.cuda.synchronize()
    assert not p.any()


def test_a_malformed_loaded_state_is_refused_before_any_state_is_created():
    ps = _params([np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)])
    opt = HipAdam(ps, lr=oc.LR)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.state[ps[2]] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros(4, device=DEV), "exp_avg_sq": torch.zeros(8, device=DEV)}
    with pytest.raises(RuntimeError, match="exp_avg"):
        opt.step()
    opt.state[ps[2]] = {"step": torch.tensor(1.0, device=DEV), "exp_avg": torch.zeros(8, device=DEV), "exp_avg_sq": torch.zeros(8, device=DEV)}
    with pytest.raises(RuntimeError, match="CPU scalar"):   # (reading it would synchronise the device every step)
        opt.step()
    torch.cuda.synchronize()
    assert ps[0] not in opt.state and ps[1] not in opt.state and not any(bool(p.any()) for p in ps)


def test_backward_after_a_step_is_refused():
    """The packed weight a convolution saves for its backward pass can be a view of the optimiser's bf16 copy, which the next step
    rewrites in place: a step between a forward and its backward raises instead of computing gradients from the new weights."""
    a, _, xs, y = _resnet18_pair(112)
    opt = HipAdam(a.parameters(), lr=1e-3, bf16_shadow=True)
    _train_step(a, opt, xs, y)
    loss = F.cross_entropy(a(*xs), y)   # reads the copies of step 1
    opt.step()                          # (the gradients of step 1 are still there) rewrites them
    with pytest.raises(RuntimeError, match="before optimizer.step"):
        loss.backward()
    _train_step(a, opt, xs, y)          # the usual order goes on working


def test_bench_train_tool_runs_one_step_with_hip_adam():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "measure" / "bench_train.py"), "--configs", "18:1", "--batches", "2", "--hw", "112",
                        "--precision", "fp32,bf16", "--norm", "hip", "--optim", "torch,fused,hip", "--steps", "1", "--warmup", "0", "--no-torch"],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("resnet18")]
    assert len(lines) == 6 and sum("optim hip" in ln for ln in lines) == 2 and sum("optim fused" in ln for ln in lines) == 2, r.stdout
