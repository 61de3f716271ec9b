"""The HIP classifier head on the MI355X: the four entries against the float64 reference (tests/head_cases.py) within 10 x the error
of torch's own fp32 CPU head on the same inputs, the device meter record, determinism, the contract's refusals, bad targets, NaN,
three training steps against the torch head, `run_epoch`, and an iteration that never waits for the device.

Every comparison prints its error / bound and error / torch's fp32 error (`_compare`); DESIGN.md section 4.16 records the worst.

Measured on an MI355X: every case within its bound; worst error / bound per tensor: pooled 0.11, logits 0.26, probs 0.58, loss 0.56,
dlogits 0.35, dw 0.21, db 0.996 (B64-HW1-C512-K3-bf16), dx 0.50; three steps: 0.24-0.32 of the bound in fp32, 0.100 in bf16."""

import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from salve_amd import _lib, training  # noqa: E402
from salve_amd.evaluate import ClassAccuracyMeter, DeviceClassMeter  # noqa: E402
from salve_amd.models import trainable  # noqa: E402
from salve_amd.models.trainable import TrainableEarlyFusionCEResnet  # noqa: E402
from salve_amd.optim import HipAdam  # noqa: E402
from tests import head_cases as hc  # noqa: E402
from tests.test_gpu_train import MODS  # noqa: E402

DEV = torch.device("cuda:0")
ACT = {"fp32": torch.float32, "bf16": torch.bfloat16}
ENTRY = {"fp32": "salve_head_f32", "bf16": "salve_head_bf16"}
SENTINEL = 12345.0


def _entries(d, dtype, record=None, accumulate=False, g=1.0, backward=True):
    """The forward entry, then the backward entry, on device copies of a case's arrays.  Returns every output as a CPU tensor."""
    x = torch.tensor(d["x"]).to(DEV).to(ACT[dtype])
    w, b, t = (torch.tensor(d[k]).to(DEV) for k in ("w", "b", "t"))
    B, HW, C = x.shape
    K = w.shape[0]
    desc = _lib.HeadDesc(B, HW, C, K, _lib.HEAD_ACCUMULATE_LOSS if accumulate else 0)
    f32 = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=DEV)   # noqa: E731
    out = {"pooled": f32(B, C), "logits": f32(B, K), "probs": f32(B, K), "loss": f32()}
    trainable._run_head(ENTRY[dtype] + "_forward", desc, _lib.HEAD_FWD, (x, w, b, t, out["pooled"], out["logits"], out["probs"], out["loss"], record), DEV)
    if backward:
        out.update({"dlogits": f32(B, K), "dw": f32(K, C), "db": f32(K), "dx": torch.full((B, HW, C), SENTINEL, dtype=ACT[dtype], device=DEV)})
        gt = torch.tensor(g, dtype=torch.float32, device=DEV)
        trainable._run_head(ENTRY[dtype] + "_backward", desc, _lib.HEAD_BWD,
                            (out["pooled"], out["probs"], t, w, gt, out["dlogits"], out["dw"], out["db"], out["dx"]), DEV)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _compare(case, got, ref, t32):
    """Every tensor within hc.bound of the float64 reference; prints error / bound and error / torch's fp32 error for each."""
    bad = []
    for name in hc.NAMES:
        store = case.dtype if name == "dx" else "fp32"
        e, e32, bnd = hc.err(got[name].double().numpy(), ref[name]), hc.err(t32[name], ref[name]), hc.bound(ref[name], t32[name], store)
        print(f"{case.id} {name}: error {e:.3e}, torch fp32 error {e32:.3e}, error / torch {e / e32 if e32 > 0 else float('nan'):.3f}, "
              f"bound {bnd:.3e}, error / bound {e / bnd:.3f}")
        if not e <= bnd:
            bad.append((name, e, bnd))
    assert not bad, (case.id, bad)


@pytest.mark.parametrize("case", hc.CASES, ids=lambda c: c.id)
def test_entries_against_float64(case):
    d = hc.make(case)
    ref, t32 = hc.head_f64(g=0.75, **d), hc.head_torch(dtype=torch.float32, g=0.75, **d)
    got = _entries(d, case.dtype, g=0.75)
    _compare(case, got, ref, t32)
    assert torch.equal(got["probs"].argmax(1), torch.from_numpy(ref["probs"].argmax(1)))   # (the inputs keep the arg-max away from rounding)
    dx = got["dx"]
    assert torch.equal(dx, dx[:, :1].expand_as(dx))   # one row, broadcast over HW
    if case.scale != 1.0:
        assert float(got["logits"].abs().max()) > 80.0 and bool(torch.isfinite(got["probs"]).all()) and bool(torch.isfinite(got["loss"]))


def _record(meter):
    torch.cuda.synchronize()
    return meter.record.cpu().numpy().view(_lib.HEAD_METER_DTYPE)[0]


METER_CASES = [(hc.Case(64, 49, 512, 3, "bf16"), True), (hc.Case(3, 49, 512, 2, "fp32", one_class=1), False), (hc.Case(257, 50, 8, 3, "fp32"), True),
               (hc.Case(1, 1, 8, 3, "bf16"), False), (hc.Case(64, 1, 520, 3, "fp32"), True)]


def _meter_run():
    """Five batches of three classes (one of two), the loss accumulated on three of them.  Returns (record, per-batch outputs)."""
    meter = DeviceClassMeter(3, DEV)
    outs = [_entries(hc.make(case), case.dtype, record=meter.record, accumulate=acc) for case, acc in METER_CASES]
    return _record(meter).copy(), outs, meter


def test_meter_record_counts_what_the_host_meter_counts():
    rec, outs, meter = _meter_run()
    host = ClassAccuracyMeter(3)
    loss_sum, rows = 0.0, 0
    for (case, acc), out in zip(METER_CASES, outs):
        host.update(torch.argmax(out["probs"], dim=1).numpy(), hc.make(case)["t"])   # the kernel's own probabilities, as run_epoch feeds its meter
        if acc:
            loss_sum += float(out["loss"].item()) * case.B   # run_epoch's arithmetic
            rows += case.B
    assert rec["total"][:3].tolist() == host.total.tolist() and rec["correct"][:3].tolist() == host.correct.tolist()
    assert not rec["total"][3:].any() and not rec["correct"][3:].any()
    assert int(rec["loss_rows"]) == rows == 64 + 257 + 64 and int(rec["bad_targets"]) == 0
    assert np.float64(rec["loss_sum"]).tobytes() == np.float64(loss_sum).tobytes(), (float(rec["loss_sum"]), loss_sum)
    accs, macc, avg = meter.read()
    want = host.get_metrics()
    assert np.array_equal(accs, want[0]) and macc == want[1] and avg == loss_sum / rows
    meter.reset()
    assert not bool(meter.record.cpu().any())


def test_all_one_class_gives_the_absent_class_zero_accuracy():
    case = hc.ONE_CLASS[0]
    meter = DeviceClassMeter(2, DEV)
    out = _entries(hc.make(case), case.dtype, record=meter.record, backward=False)
    accs, macc, _ = meter.read()
    hits = int((out["probs"].argmax(1) == 1).sum())
    assert accs[0] == 0.0 and accs[1] == hits / (3 + 1e-10) and macc == (accs[0] + accs[1]) / 2


def test_same_inputs_give_the_same_bits():
    a_rec, a_outs, _ = _meter_run()
    b_rec, b_outs, _ = _meter_run()
    assert a_rec.tobytes() == b_rec.tobytes()
    for a, b in zip(a_outs, b_outs):
        for name in hc.NAMES:
            assert torch.equal(a[name].reshape(-1).view(torch.uint8), b[name].reshape(-1).view(torch.uint8)), name


def test_contract_refusals_launch_nothing():
    lib = _lib.load()
    vp = ctypes.c_void_p
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=DEV)   # every pointer argument: large enough for the valid call below
    tgt = torch.zeros(64, dtype=torch.int64, device=DEV)
    meter = DeviceClassMeter(2, DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)

    def call(fn, desc, x_ptr=None):
        p = vp(buf.data_ptr())
        x = vp(buf.data_ptr() if x_ptr is None else x_ptr)
        d = ctypes.byref(_lib.HeadDesc(*desc))
        if fn.endswith("forward"):
            return getattr(lib, fn)(d, x, p, p, vp(tgt.data_ptr()), p, p, p, p, vp(meter.record.data_ptr()), vp(ws.data_ptr()), 4096, vp(None))
        return getattr(lib, fn)(d, p, p, vp(tgt.data_ptr()), p, p, p, p, p, x, vp(ws.data_ptr()), 4096, vp(None))

    refused = [(0, 4, 8, 2, 0), (65536, 4, 8, 2, 0), (-1, 4, 8, 2, 0), (4, 0, 8, 2, 0), (4, 1025, 8, 2, 0), (4, 4, 0, 2, 0), (4, 4, 4, 2, 0),
               (4, 4, 12, 2, 0), (4, 4, 4104, 2, 0), (4, 4, 8, 1, 0), (4, 4, 8, 17, 0), (4, 4, 8, 2, 2)]
    for fn in ("salve_head_f32_forward", "salve_head_bf16_forward", "salve_head_f32_backward", "salve_head_bf16_backward"):
        for desc in refused:
            assert call(fn, desc) == _lib.SALVE_ERR_BAD_ARG and lib.salve_last_error().startswith(b"head:"), (fn, desc)
            assert int(lib.salve_head_workspace_bytes(ctypes.byref(_lib.HeadDesc(*desc)), _lib.HEAD_FWD)) == 0
        for off in (4, 8):   # x (forward) / dx (backward) not 16-byte aligned
            assert call(fn, (4, 4, 8, 2, 0), x_ptr=buf.data_ptr() + off) == _lib.SALVE_ERR_BAD_ARG and b"aligned" in lib.salve_last_error(), (fn, off)
        assert getattr(lib, fn)(None, *([vp(buf.data_ptr())] * 9), vp(ws.data_ptr()), 4096, vp(None)) == _lib.SALVE_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and not bool(meter.record.cpu().any())   # nothing ran
    assert call("salve_head_f32_forward", (4, 4, 8, 2, 0)) == _lib.SALVE_OK   # (the same call, inside the contract, does run)
    torch.cuda.synchronize()
    assert not bool((buf == SENTINEL).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_targets_outside_the_classes_contribute_nothing(dtype):
    case = hc.Case(3, 49, 520, 3, dtype)
    d = hc.make(case)
    extra = hc.make(hc.Case(3, 49, 520, 3, dtype, scale=0.5))["x"][:2]
    bad = {"x": np.concatenate([d["x"][:1], extra[:1], d["x"][1:], extra[1:]]), "w": d["w"], "b": d["b"],
           "t": np.array([d["t"][0], 3, d["t"][1], d["t"][2], -1], dtype=np.int64)}   # rows 1 and 4: targets K and -1
    meter = DeviceClassMeter(3, DEV)
    got = _entries(bad, dtype, record=meter.record, accumulate=True)
    rec = _record(meter)
    assert int(rec["bad_targets"]) == 2 and int(rec["total"].sum()) == 3 and int(rec["loss_rows"]) == 5
    assert not got["dx"][[1, 4]].any() and not got["dlogits"][[1, 4]].any() and bool(got["dx"][[0, 2, 3]].any())
    good = _entries(d, dtype)   # the three valid rows alone: the same sums over the same rows, scaled by 3 / 5
    assert float(got["loss"]) == pytest.approx(float(good["loss"]) * 3 / 5, rel=1e-6)
    assert torch.allclose(got["dw"], good["dw"] * 3 / 5, rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError, match="2 targets"):
        meter.read()


def test_nan_is_propagated_to_the_loss_and_the_loss_sum():
    case = hc.Case(3, 49, 8, 2, "fp32")
    d = hc.make(case)
    d["x"] = d["x"].copy()
    d["x"][1, 7, 3] = np.nan
    meter = DeviceClassMeter(2, DEV)
    got = _entries(d, "fp32", record=meter.record, accumulate=True, backward=False)
    rec = _record(meter)
    assert bool(torch.isnan(got["loss"])) and np.isnan(rec["loss_sum"]) and int(rec["loss_rows"]) == 3
    assert bool(torch.isfinite(got["probs"][[0, 2]]).all()) and bool(torch.isnan(got["probs"][1]).all())


# ---- model level -------------------------------------------------------------------------------------------------------------
def _models(precision, n, hw=224, batch=4, seed=0):
    """n copies of one ResNet-18 (norm hip) from one state dict, with HipAdam each, and a fixed batch."""
    torch.manual_seed(seed)
    first = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=MODS[1])).set_train_precision(precision).set_train_norm("hip").to(DEV).train()
    models = [first] + [copy.deepcopy(first) for _ in range(n - 1)]
    opts = [HipAdam(m.parameters(), lr=1e-4, weight_decay=1e-4, bf16_shadow=precision == "bf16") for m in models]
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(batch, 3, hw, hw, generator=g).to(DEV) for _ in range(2)]
    y = torch.tensor([0, 1] * (batch // 2), device=DEV)
    return models, opts, xs, y


def _f64_head_loss(model, feat, y):
    """torch's head on the CPU in float64 behind the model's trunk (autograd carries the gradients back to the device)."""
    f = feat.double().cpu()
    logits = F.linear(torch.flatten(F.adaptive_avg_pool2d(f, 1), 1), model.fc.weight.double().cpu(), model.fc.bias.double().cpu())
    return F.softmax(logits.detach().clone(), dim=1).float().to(feat.device), F.cross_entropy(logits, y.cpu())


def _max_diff(a, b):
    return max(float((p.detach().double() - q.detach().double()).abs().max()) for p, q in zip(a, b))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_three_steps_with_the_hip_head_follow_the_torch_head(precision):
    """Three Adam steps of ResNet-18 (norm hip, optim hip) on one batch: head torch (A), head hip (H), and head torch computed in
    float64 on the CPU (C), from one state dict.  The two heads sum in different orders, so H is not A bit for bit; the yardstick
    for how far rounding inside the head moves a training run is |A - C|, a difference made by nothing but the head's arithmetic.
    Bound: |H - A| <= 10 x |A - C| (the project's margin), for the logits after each step and for the
    parameters after the third, each floored at one fp32 ulp of the largest magnitude compared."""
    (a, h, c), (oa, oh, oc_), xs, y = _models(precision, 3)
    h.set_train_head("hip")
    for step in range(3):
        for m, o in ((a, oa), (h, oh)):
            _, loss = m.forward_loss(xs[0], xs[1], None, None, None, None, y)
            o.zero_grad()
            loss.backward()
            o.step()
        _, loss = _f64_head_loss(c, c._features(c._cat(xs), False), y)
        oc_.zero_grad()
        loss.backward()
        oc_.step()
        with torch.no_grad():
            la, lh, lc = (m(*xs).double() for m in (a, h, c))
        ref, got = float((la - lc).abs().max()), float((lh - la).abs().max())
        bnd = max(10.0 * ref, hc.ulp(float(la.abs().max()), "fp32"))
        print(f"{precision} step {step + 1}: logits |hip - torch| {got:.3e}, |torch - torch with a float64 head| {ref:.3e}, bound {bnd:.3e}, ratio {got / bnd:.3f}")
        assert got <= bnd, (precision, step, got, bnd)
    ref, got = _max_diff(a.parameters(), c.parameters()), _max_diff(h.parameters(), a.parameters())
    bnd = max(10.0 * ref, hc.ulp(max(float(p.detach().abs().max()) for p in a.parameters()), "fp32"))
    print(f"{precision} parameters after 3 steps: |hip - torch| {got:.3e}, |torch - torch with a float64 head| {ref:.3e}, bound {bnd:.3e}, ratio {got / bnd:.3f}")
    assert got <= bnd, (precision, got, bnd)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_packed_and_unpacked_input_give_the_same_bits(precision):
    (p, q), _, xs, y = _models(precision, 2, hw=112)
    p.set_train_head("hip")
    q.set_train_head("hip")
    mp, mq = DeviceClassMeter(2, DEV), DeviceClassMeter(2, DEV)
    packed = trainable._nhwc(torch.cat(xs, dim=1).to(ACT[precision]), 8)
    probs_p, loss_p = p.forward_packed_loss(packed, y, meters=mp, accumulate_loss=True)
    probs_q, loss_q = q.forward_loss(xs[0], xs[1], None, None, None, None, y, meters=mq, accumulate_loss=True)
    loss_p.backward()
    loss_q.backward()
    assert torch.equal(probs_p, probs_q) and torch.equal(loss_p, loss_q) and _record(mp).tobytes() == _record(mq).tobytes()
    assert int(_record(mp)["loss_rows"]) == 4 and int(_record(mp)["total"].sum()) == 4
    grads = [(n, u.grad, v.grad) for (n, u), v in zip(p.named_parameters(), q.parameters())]
    assert all((gu is None) == (gv is None) for _, gu, gv in grads) and sum(gu is not None for _, gu, _ in grads) > 60
    for n, gu, gv in grads:
        assert gu is None or torch.equal(gu, gv), n


# ---- run_epoch ---------------------------------------------------------------------------------------------------------------
class _Batches:
    """An in-memory batch source of 2-tuples (x_packed, is_match), the form train_render.RenderedTrainSource yields."""

    def __init__(self, n, batch, hw, seed):
        g = torch.Generator().manual_seed(seed)
        self.items = [(trainable._nhwc(torch.randn(batch, 6, hw, hw, generator=g), 8).to(DEV), torch.randint(0, 2, (batch, 1), generator=g).to(DEV))
                      for _ in range(n)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def _f64_forward_packed(model, split, x_packed, is_match, meters=None, accumulate_loss=False):
    """training.cross_entropy_forward_packed with the head in float64 on the CPU (the yardstick run of the run_epoch test)."""
    with torch.set_grad_enabled(split == "train" and torch.is_grad_enabled()):
        return _f64_head_loss(model, model._features(model._packed(x_packed), True), is_match.reshape(-1))


def test_run_epoch_with_the_hip_head(monkeypatch):
    """A train pass and a val pass over 5 batches of 4 (fp32, norm hip, optim hip) with head torch, head hip and -- for the bound --
    head torch in float64 on the CPU: the same keys, exactly the same mAcc, avg_loss within 10 x |torch - float64 head| (floored at
    an fp32 ulp of the loss), the model-level bound."""
    args = SimpleNamespace(num_ce_classes=2, num_epochs=1, base_lr=1e-4, lr_annealing_strategy="poly", poly_lr_power=0.9, print_every=2)
    (a, h, c), (oa, oh, oc_), _, _ = _models("fp32", 3)
    h.set_train_head("hip")
    train_src, val_src = _Batches(5, 4, 112, seed=5), _Batches(5, 4, 112, seed=6)

    def passes(model, opt):
        out = {"train": training.run_epoch(args, 0, model, train_src, opt, "train")}
        with torch.no_grad():
            out["val"] = training.run_epoch(args, 0, model, val_src, opt, "val")
        return out

    ra, rh = passes(a, oa), passes(h, oh)
    monkeypatch.setattr(training, "cross_entropy_forward_packed", _f64_forward_packed)
    rc = passes(c, oc_)
    for split in ("train", "val"):
        assert set(rh[split]) == set(ra[split]) == {"avg_loss", "mAcc"} and all(type(v) is float for v in rh[split].values())
        ref, got = abs(ra[split]["avg_loss"] - rc[split]["avg_loss"]), abs(rh[split]["avg_loss"] - ra[split]["avg_loss"])
        bnd = max(10.0 * ref, hc.ulp(ra[split]["avg_loss"], "fp32"))
        print(f"run_epoch {split}: torch {ra[split]}, hip {rh[split]}; avg_loss |hip - torch| {got:.3e}, |torch - float64 head| {ref:.3e}, bound {bnd:.3e}")
        assert rh[split]["mAcc"] == ra[split]["mAcc"], split
        assert got <= bnd, (split, got, bnd)
    assert rh["val"]["avg_loss"] == 0.0 and rh["train"]["avg_loss"] > 0.0   # as the reference: training batches only


def test_a_training_iteration_never_waits_for_the_device():
    """Under torch's synchronisation debug mode "error" a call that makes the host wait for the device raises.  First `loss.item()`
    must raise (else the mode reports nothing on this build and the test is skipped, not passed); then one whole iteration on
    tensors already on the device -- forward_packed_loss with a meter, backward, HipAdam.step -- must not."""
    (m,), (opt,), _, _ = _models("bf16", 1, hw=112)
    m.set_train_head("hip")
    meter = DeviceClassMeter(2, DEV)
    src = _Batches(2, 4, 112, seed=7)
    batches = [(x.to(torch.bfloat16), y) for x, y in src]

    def iteration(x, y):
        probs, loss = m.forward_packed_loss(x, y, meters=meter, accumulate_loss=True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    loss = iteration(*batches[0])   # (first use: code objects load, the allocator grows)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            loss.item()
            detected = False
        except RuntimeError:
            detected = True
        if detected:
            loss = iteration(*batches[1])
            meter.reset()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not detected:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag loss.item() on this torch build: nothing could be shown")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
