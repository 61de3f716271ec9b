"""HipAdam without a GPU: the float64 reference against torch.optim.Adam in float64, the deliberately wrong variants against the
bound the GPU tests use, the table / chunk-map builder, the refusals and the defaults."""

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from salve_amd import _lib, optim, training
from salve_amd.optim import CHUNK, HipAdam, Segment, adam_scalars, build_tables
from tests import optim_cases as oc

ROOT = Path(__file__).resolve().parents[1]
SIZES = [257, 64]   # parameter 1 receives its first gradient at step 3 (its own step count is 1 there)


def _late_problem(seed=7):
    params, grads = oc.make_problem(SIZES, seed=seed)
    grads[0][1] = grads[1][1] = None
    return params, grads


def test_float64_reference_is_torch_adam_in_float64():
    """The reference is numpy written from torch's documentation; torch.optim.Adam on the CPU in float64 runs the same algorithm in
    another operation order: they agree to float64 rounding (1e-13 relative to each tensor's largest magnitude, some 500 float64
    ulps: three steps of a dozen operations each)."""
    lr = lambda k, i: oc.LR * (1.0 - 0.2 * k) * (1 + i)   # noqa: E731  (changes per step and differs per parameter)
    wd = lambda k, i: oc.WEIGHT_DECAY * (i + 1)   # noqa: E731
    params, grads = _late_problem()
    ref = oc.adam_f64(params, grads, lr=lr, weight_decay=wd)
    t64 = oc.torch_adam(params, grads, torch.float64, lr=lr, weight_decay=wd)
    assert ref[3] == t64[3] == [3, 1]
    for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
        for a, b in zip(ref[q], t64[q]):
            assert oc.err(a, b) <= 1e-13 * np.abs(b).max(), (name, oc.err(a, b))
    none = oc.adam_f64(params, [[grads[0][0], None]])
    assert none[1][1] is None and none[2][1] is None and none[3] == [1, 0] and np.array_equal(none[0][1], params[1])


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_every_term_is_visible_at_the_test_hyperparameters(mutant):
    """Each wrong variant of the float64 reference moves a parameter by more than 100 x the bound the GPU tests grant (10 x torch's
    fp32 error, floored at an ulp): none of these mistakes can hide below the bound."""
    params, grads = _late_problem()
    ref = oc.adam_f64(params, grads)
    t32 = oc.torch_adam(params, grads, torch.float32)
    wrong = oc.adam_f64(params, grads, variant=mutant)
    ratios = [oc.err(wrong[0][i], ref[0][i]) / oc.bound(ref[0][i], t32[0][i]) for i in range(len(SIZES))]
    print(f"{mutant}: parameter difference / bound = {ratios}")
    assert max(ratios) > 100.0, ratios
    if mutant == "shared_step_count":   # visible on the late parameter, and only there
        assert ratios[0] == 0.0 and ratios[1] > 100.0


def test_scalars_are_the_double_precision_formulas():
    lr, b1, b2, eps, wd = 1e-2 * (1 - 17 / 400) ** 0.9, 0.9, 0.999, 1e-3, 0.1
    for t in (1, 2, 3, 1000, 100000):
        s = adam_scalars(lr, b1, b2, eps, wd, t)
        assert list(s) == list(_lib.ADAM_SEGMENT_DTYPE.names[6:])
        assert all(type(v) is np.float32 for v in s.values())
        assert s["step_size"] == np.float32(lr / (1.0 - b1 ** t))
        assert s["sqrt_bc2"] == np.float32((1.0 - b2 ** t) ** 0.5)
        assert s["one_minus_beta1"] == np.float32(1.0 - b1) and s["one_minus_beta2"] == np.float32(1.0 - b2)
        assert (s["beta1"], s["beta2"], s["eps"], s["weight_decay"]) == (np.float32(b1), np.float32(b2), np.float32(eps), np.float32(wd))
    # formed in float32 from the rounded beta2, 1 - beta2 would be off by 1e-5 relative: it has to come from the host in double
    assert abs(float(np.float32(1) - np.float32(b2)) / (1.0 - b2) - 1.0) > 1e-5 > abs(float(adam_scalars(lr, b1, b2, eps, wd, 1)["one_minus_beta2"]) / (1.0 - b2) - 1.0) * 100


def test_table_layout_matches_the_header():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    assert int(re.search(r"#define SALVE_ADAM_CHUNK (\d+)", header).group(1)) == CHUNK == _lib.ADAM_CHUNK
    body = re.search(r"typedef struct \{([^}]*)\} salve_adam_segment_t;", header).group(1)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert tuple(names) == _lib.ADAM_SEGMENT_DTYPE.names
    assert _lib.ADAM_SEGMENT_DTYPE.itemsize == 80 and _lib.ADAM_CHUNK_DTYPE.itemsize == 16
    assert "salve_adam_step" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), "salve_adam_step")


def test_build_tables_segments_chunks_and_scalars():
    ns = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 0, 5]
    segs = [Segment(1000 + i, 2000 + i, 3000 + i, 4000 + i, 5000 + i if i % 2 else 0, n, 1e-2 * (i + 1), 0.9, 0.999, 1e-3, 0.1 * i, 1 + i % 3)
            for i, n in enumerate(ns)]
    table, chunks = build_tables(segs)
    assert table.dtype == _lib.ADAM_SEGMENT_DTYPE and chunks.dtype == _lib.ADAM_CHUNK_DTYPE
    assert len(table) == len(ns)
    for i, (s, row) in enumerate(zip(segs, table)):   # segments in order, every field
        assert (row["param"], row["grad"], row["exp_avg"], row["exp_avg_sq"], row["shadow_bf16"], row["n"]) == s[:6]
        for k, v in adam_scalars(s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, s.t).items():
            assert row[k] == v, (i, k)
    want = [(i, c * CHUNK) for i, n in enumerate(ns) for c in range(-(-n // CHUNK))]
    assert [(int(c["segment"]), int(c["offset"])) for c in chunks] == want
    assert [int((chunks["segment"] == i).sum()) for i in range(len(ns))] == [1, 1, 1, 2, 3, 0, 1] == [optim.chunk_count(n) for n in ns]
    assert not chunks["reserved"].any()
    empty = build_tables([])
    assert len(empty[0]) == 0 and len(empty[1]) == 0
    with pytest.raises(ValueError):
        build_tables([segs[0]._replace(t=0)])
    big = build_tables([segs[0]._replace(n=2 ** 33 + 1)])[1]   # offsets past 2^31 elements stay exact
    assert len(big) == 2 ** 21 + 1 and int(big["offset"][-1]) == 2 ** 33 and big["offset"].dtype == np.int64


def test_plan_describes_this_steps_gradients_only():
    """`plan()` builds what `step()` uploads (host arithmetic only, so CPU tensors serve here): parameters without a gradient are
    absent and get no state, each parameter carries its own step count and its group's lr and weight decay."""
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (CHUNK + 1, 7, 3, 2 * CHUNK)]
    opt = HipAdam([{"params": ps[:2]}, {"params": ps[2:], "lr": 5e-3, "weight_decay": 0.0}], lr=1e-2, eps=1e-3, weight_decay=0.1)
    for i in (0, 2, 3):
        ps[i].grad = torch.ones_like(ps[i])
    opt.state[ps[0]] = {"step": torch.tensor(4.0), "exp_avg": torch.zeros_like(ps[0]), "exp_avg_sq": torch.zeros_like(ps[0])}
    table, chunks = opt.plan()
    assert [int(n) for n in table["n"]] == [CHUNK + 1, 3, 2 * CHUNK]
    assert [int(a) for a in table["param"]] == [ps[i].data_ptr() for i in (0, 2, 3)]
    assert [int(a) for a in table["grad"]] == [ps[i].grad.data_ptr() for i in (0, 2, 3)]
    assert [int(a) for a in table["exp_avg"]] == [opt.state[ps[i]]["exp_avg"].data_ptr() for i in (0, 2, 3)]
    assert not table["shadow_bf16"].any()
    assert ps[1] not in opt.state and set(opt.state[ps[2]]) == {"step", "exp_avg", "exp_avg_sq"}
    assert float(opt.state[ps[0]]["step"]) == 4.0 and float(opt.state[ps[2]]["step"]) == 0.0   # (plan advances nothing)
    assert table["step_size"][0] == adam_scalars(1e-2, 0.9, 0.999, 1e-3, 0.1, 5)["step_size"]
    assert table["step_size"][1] == adam_scalars(5e-3, 0.9, 0.999, 1e-3, 0.0, 1)["step_size"]
    assert (table["weight_decay"][0], table["weight_decay"][2]) == (np.float32(0.1), np.float32(0.0))
    assert [int(c) for c in chunks["segment"]] == [0, 0, 1, 2, 2]
    for group in opt.param_groups:   # run_epoch's poly schedule
        group["lr"] = 1e-4
    assert opt.plan()[0]["step_size"][1] == adam_scalars(1e-4, 0.9, 0.999, 1e-3, 0.0, 1)["step_size"]
    ps[0].grad = None   # zero_grad(): the next step describes what is there then
    assert [int(n) for n in opt.plan()[0]["n"]] == [3, 2 * CHUNK]


def test_state_dict_has_torchs_keys_and_loads_both_ways():
    def make(cls):
        ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]
        return ps, cls(ps, lr=1e-2, weight_decay=0.1)
    ps, hip = make(HipAdam)
    qs, ref = make(torch.optim.Adam)
    assert isinstance(hip, torch.optim.Optimizer)
    assert hip.state_dict()["param_groups"] == ref.state_dict()["param_groups"] and hip.defaults == ref.defaults
    for q in qs:
        q.grad = torch.ones_like(q)
    ref.step()
    hip.load_state_dict(ref.state_dict())
    for p, q in zip(ps, qs):
        assert set(hip.state[p]) == set(ref.state[q])
        for k in ref.state[q]:
            assert hip.state[p][k].dtype == ref.state[q][k].dtype and hip.state[p][k].device == ref.state[q][k].device
            assert torch.equal(hip.state[p][k], ref.state[q][k])
    ps[0].grad = torch.ones_like(ps[0])
    assert int(hip.plan()[0]["n"][0]) == 5 and hip.plan()[0]["step_size"][0] == adam_scalars(1e-2, 0.9, 0.999, 1e-8, 0.1, 2)["step_size"]
    ref.load_state_dict(hip.state_dict())
    ref.step()   # torch accepts what HipAdam saved


def test_refusals():
    p = torch.nn.Parameter(torch.zeros(8))
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}, {"fused": True}, {"foreach": True},
               {"decoupled_weight_decay": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            HipAdam([p], **kw)
    assert type(HipAdam([p], foreach=False, fused=None)) is HipAdam   # torch's constructor arguments, the two selectors accepted when off
    opt = HipAdam([p])
    p.grad = torch.zeros(8)
    with pytest.raises(RuntimeError, match="HIP device only"):   # a CPU parameter
        opt.step()
    assert p not in opt.state   # refused before anything was touched
    opt.param_groups[0]["amsgrad"] = True   # (set later, e.g. through a loaded state dict)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()

    nc = torch.nn.Parameter(torch.zeros(6, 4).t())   # a non-contiguous parameter
    nc.grad = torch.zeros(6, 4).t()
    with pytest.raises(RuntimeError, match="not contiguous"):
        HipAdam([nc]).step()
    b = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))   # a bf16 parameter
    b.grad = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32"):
        HipAdam([b]).step()
    s = torch.nn.Parameter(torch.zeros(4, 4))
    s.grad = torch.zeros(4, 4).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        HipAdam([s]).step()

    with pytest.raises(ValueError, match="optimiser"):
        training._check_optim("sgd")
    with pytest.raises(ValueError, match="optimiser"):
        training.get_optimizer(SimpleNamespace(optimizer_algo="adam", base_lr=1e-3, weight_decay=0.0), torch.nn.Linear(2, 2), optim="fused")
    from salve_amd import train as train_cli

    with pytest.raises(SystemExit):
        train_cli.main(["--config", "unused.yaml", "--optim", "sgd"])


def test_default_optimizer_is_unchanged():
    args = SimpleNamespace(optimizer_algo="adam", base_lr=2e-3, weight_decay=1e-4)
    model = torch.nn.Linear(3, 2)
    opt = training.get_optimizer(args, model)
    assert type(opt) is torch.optim.Adam and opt.defaults["lr"] == 2e-3 and opt.defaults["weight_decay"] == 1e-4
    assert type(training.get_optimizer(args, model, optim="torch")) is torch.optim.Adam
    hip = training.get_optimizer(args, model, optim="hip")
    assert type(hip) is HipAdam and hip.defaults == opt.defaults and hip.bf16_shadow is False
    model.train_precision = "bf16"
    assert training.get_optimizer(args, model, optim="hip").bf16_shadow is True
    assert training.OPTIMS == ("torch", "hip")


def test_current_shadow_follows_the_version_counter():
    p = torch.nn.Parameter(torch.ones(2, 2, 1, 1))
    assert optim.current_shadow(p) is None
    sh = p.detach().to(torch.bfloat16)
    setattr(p, optim._SHADOW_ATTR, (sh, p.data_ptr(), p._version))
    assert optim.current_shadow(p) is sh
    with torch.no_grad():
        p.mul_(2)   # any torch in-place write
    assert optim.current_shadow(p) is None
    setattr(p, optim._SHADOW_ATTR, (sh, p.data_ptr(), p._version))
    p.data = torch.zeros(2, 2, 1, 1)   # new storage (model.to(...), a loaded tensor)
    assert optim.current_shadow(p) is None
