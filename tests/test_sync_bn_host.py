"""The synchronised HIP BatchNorm on the host (CPU): the float64 restatement of its passes (tests/sync_bn_cases.py) against
full-batch BatchNorm over row splits of 1, 2, 3 and 5 ranks; emulated wrong kernels, which the cases must catch; the switch's
refusals (command line, train(), the model); the new symbols in the header, the binding and the built library; and the entries'
refusals, all decided before any launch."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from salve_amd import _lib, training
from salve_amd.models.trainable import SyncNorm, TrainableEarlyFusionCEResnet
from tests import sync_bn_cases as cases
from tests.test_train_host import config

ROOT = Path(__file__).resolve().parents[1]
SPLIT_SYMBOLS = ("salve_bn_f32_stats", "salve_bn_bf16_stats", "salve_bn_combine", "salve_bn_f32_apply", "salve_bn_bf16_apply",
                 "salve_bn_f32_backward_reduce", "salve_bn_bf16_backward_reduce", "salve_bn_f32_backward_apply", "salve_bn_bf16_backward_apply")
TOL = 1e-11   # float64 chains of a dozen rows against float64 full-batch formulas: rounding only
FLAGS = (0, cases.RELU, cases.ADD, cases.ADD | cases.RELU)


def _all_cases():
    for si, rows in enumerate(cases.SPLITS):
        for flags in FLAGS:
            yield rows, cases.make_case(int(sum(rows)), 8, seed=100 * si + flags, flags=flags)


def test_the_splits_cover_1_2_3_and_5_ranks_an_empty_rank_and_a_single_row():
    assert {len(r) for r in cases.SPLITS} == {1, 2, 3, 5}
    assert any(r[0] == 0 for r in cases.SPLITS) and any(0 in r[1:] for r in cases.SPLITS) and any(1 in r for r in cases.SPLITS)
    assert any(len(set(r)) > 1 for r in cases.SPLITS)


def test_the_split_chain_equals_full_batch_batchnorm():
    for rows, case in _all_cases():
        for name, err in cases.chain_errors(case, rows).items():
            assert err < TOL, (rows, case["flags"], name, err)


def test_full_batch_reference_is_torchs_batchnorm():
    torch = pytest.importorskip("torch")
    case = cases.make_case(12, 8, seed=7, flags=cases.RELU)
    bn = torch.nn.BatchNorm2d(8, eps=case["eps"], momentum=case["momentum"]).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(case["gamma"]))
        bn.bias.copy_(torch.from_numpy(case["beta"]))
        bn.running_mean.copy_(torch.from_numpy(case["running_mean"]))
        bn.running_var.copy_(torch.from_numpy(case["running_var"]))
    x = torch.from_numpy(case["x"]).reshape(12, 8, 1, 1).requires_grad_(True)
    y = torch.relu(bn(x))
    y.backward(torch.from_numpy(case["dy"]).reshape(12, 8, 1, 1))
    fwd = cases.full_forward(case)
    bwd = cases.full_backward(case, fwd)
    assert cases.max_rel(fwd["y"], y.detach().numpy().reshape(12, 8)) < TOL
    assert cases.max_rel(fwd["running_mean"], bn.running_mean.numpy()) < TOL and cases.max_rel(fwd["running_var"], bn.running_var.numpy()) < TOL
    assert cases.max_rel(bwd["dx"], x.grad.numpy().reshape(12, 8)) < TOL
    assert cases.max_rel(bwd["dgamma"], bn.weight.grad.numpy()) < TOL and cases.max_rel(bwd["dbeta"], bn.bias.grad.numpy()) < TOL


@pytest.mark.parametrize("wrong", cases.WRONG)
def test_an_emulated_wrong_kernel_fails_the_cases(wrong):
    worst = 0.0
    for rows, case in _all_cases():
        worst = max(worst, max(cases.chain_errors(case, rows, wrong).values()))
    assert worst > 1e-3, (wrong, worst)   # far outside TOL: the cases tell this kernel from the right one


def test_a_world_of_one_is_untouched_by_the_rank_bugs():
    """(What makes the multi-rank cases necessary: three of the wrong kernels are right with one rank.)"""
    case = cases.make_case(12, 8, seed=3, flags=cases.ADD | cases.RELU)
    for wrong in ("averaged_means", "local_rows", "empty_rank_not_skipped"):
        assert max(cases.chain_errors(case, (12,), wrong).values()) < TOL, wrong


# ---------------------------------------------------------------------------------------------------- the switch
def test_sync_norm_splits_the_batch_as_the_feeds_do():
    from salve_amd.train_feed import shard_bounds

    for world in (1, 2, 3, 5, 8):
        group = SimpleNamespace(world=world, rank=0)
        assert SyncNorm(group).batches(4) == [4] * world
        for n in (0, 1, 4, 7, 256):
            want = [hi - lo for lo, hi in (shard_bounds(n, r, world) for r in range(world))]
            assert SyncNorm(group, n).batches(want[0]) == want and sum(want) == n


def test_set_sync_norm_needs_the_hip_norm_and_an_active_group():
    model = TrainableEarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"]))
    active = SimpleNamespace(world=2, rank=1, active=True)
    with pytest.raises(ValueError, match="--norm hip") as e:
        model.set_sync_norm(active)
    assert str(e.value).count(".") <= 1 and "\n" not in str(e.value)   # one sentence
    assert model.sync_norm is None
    assert model.set_train_norm("hip").set_sync_norm(active, batch_size=4) is model
    assert model.sync_norm.group is active and model.sync_norm.batches(2) == [2, 2]
    assert model.set_sync_norm(SimpleNamespace(world=1, rank=0, active=False)).sync_norm is None   # a world of one, not forced: the fused entries
    assert model.set_sync_norm(active).set_sync_norm(None).sync_norm is None


def test_train_refuses_sync_bn_without_the_hip_norm():
    for fn, extra in ((training.train, ()), (training.train_rendered, (None, None))):
        with pytest.raises(ValueError, match="--norm hip"):
            fn(config(), *extra, "/nonexistent/never-written", sync_bn=True)
        with pytest.raises(ValueError, match="--norm hip"):
            fn(config(), *extra, "/nonexistent/never-written", norm="torch", sync_bn=True)
    assert training.TRAIN_NORMS == ("torch", "hip")


def test_the_command_line_refuses_sync_bn_without_the_hip_norm_and_lists_it():
    run = lambda *a: subprocess.run([sys.executable, "-m", "salve_amd.train", *a], cwd=str(ROOT), capture_output=True, text=True, timeout=120)  # noqa: E731
    r = run("--config", "x.yaml", "--sync-bn")
    lines = [l for l in (r.stdout + r.stderr).splitlines() if l.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--norm hip" in lines[0] and "--sync-bn" in lines[0], lines
    r = run("--config", "x.yaml", "--sync-bn", "--norm", "torch")
    assert r.returncode != 0 and "--norm hip" in r.stderr and "Traceback" not in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--sync-bn" in r.stdout


# ---------------------------------------------------------------------------------------------------- the library
def test_split_symbols_are_declared_listed_and_exported():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    declared = set(re.findall(r"\bint (salve_bn_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in SPLIT_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert {n for n in _lib.EXPORTED_SYMBOLS if n.startswith("salve_bn_")} == declared | {"salve_bn_workspace_bytes"}
    for name, value in (("SALVE_BN_STATS", _lib.BN_STATS), ("SALVE_BN_BWD_REDUCE", _lib.BN_BWD_REDUCE), ("SALVE_BN_MAX_WORLD", _lib.BN_MAX_WORLD)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert lib.salve_hip_version() == _lib.EXPECTED_ABI == 7 and "#define SALVE_HIP_ABI_VERSION 7" in header


def _desc(rows, c, flags=0, eps=1e-5, momentum=0.1):
    return ctypes.byref(_lib.BnDesc(rows, c, flags, eps, momentum))


BAD = [(100, 12, 0), (100, 4, 0), (100, 0, 0), (100, 4104, 0), (-1, 64, 0), (100, 64, 8), (100, 64, -1)]


def test_the_workspace_query_knows_the_split_passes():
    lib = _lib.load()
    ws = lambda rows, c, flags, p: int(lib.salve_bn_workspace_bytes(_desc(rows, c, flags), p))   # noqa: E731
    for rows in (0, 1, 2, 65, 4097, 256 * 56 * 56):
        for c in (8, 64, 2048):
            assert ws(rows, c, 0, _lib.BN_STATS) > 0 and ws(rows, c, cases.RELU, _lib.BN_BWD_REDUCE) > 0, (rows, c)
            if rows >= 2:   # the same kernels on the same partials: the fused passes' sizes
                assert ws(rows, c, 0, _lib.BN_STATS) == ws(rows, c, 0, _lib.BN_FWD) and ws(rows, c, 0, _lib.BN_BWD_REDUCE) == ws(rows, c, 0, _lib.BN_BWD)
    for p in (_lib.BN_STATS, _lib.BN_BWD_REDUCE):
        for rows, c, flags in BAD:
            assert ws(rows, c, flags, p) == 0, (rows, c, flags, p)
        assert ws(100, 64, _lib.BN_EVAL, p) == 0, "the eval form has no batch statistics to synchronise"
        assert int(lib.salve_bn_workspace_bytes(None, p)) == 0
    for rows in (0, 1):   # the fused passes still refuse what they refused
        assert ws(rows, 64, 0, _lib.BN_FWD) == 0 and ws(rows, 64, 0, _lib.BN_BWD) == 0


def test_split_entries_refuse_bad_descriptors_and_null_pointers_without_a_device():
    lib = _lib.load()
    null, i32, i64 = ctypes.c_void_p(0), ctypes.c_int32, ctypes.c_int64
    rows2 = (ctypes.c_int64 * 2)(50, 50)
    calls = {}
    for t in ("f32", "bf16"):
        calls[f"salve_bn_{t}_stats"] = lambda d, f: f(d, null, null, null, 0, null)
        calls[f"salve_bn_{t}_apply"] = lambda d, f: f(d, *[null] * 7, null)
        calls[f"salve_bn_{t}_backward_reduce"] = lambda d, f: f(d, *[null] * 6, null, 0, null)
        calls[f"salve_bn_{t}_backward_apply"] = lambda d, f: f(d, *[null] * 7, i32(2), i64(100), null, null, null)
    calls["salve_bn_combine"] = lambda d, f: f(d, null, ctypes.cast(rows2, ctypes.c_void_p), i32(2), null, null, null, null, null)
    for name, call in calls.items():
        f = getattr(lib, name)
        assert call(None, f) == _lib.SALVE_ERR_BAD_ARG, name
        for rows, c, flags in BAD:
            assert call(_desc(rows, c, flags), f) == _lib.SALVE_ERR_BAD_ARG, (name, rows, c, flags)
        assert call(_desc(100, 64, _lib.BN_EVAL), f) == _lib.SALVE_ERR_UNSUPPORTED, name
        for rows in (0, 1, 50):
            assert call(_desc(rows, 64, cases.ADD | cases.RELU), f) == _lib.SALVE_ERR_BAD_ARG, (name, rows)   # null pointers
    # combine: the world and the ranks' rows are checked before anything is launched (the pointers here are never read)
    one = ctypes.c_void_p(16)
    combine = lambda rows, world: lib.salve_bn_combine(_desc(0, 64), one, ctypes.cast((ctypes.c_int64 * len(rows))(*rows), ctypes.c_void_p),  # noqa: E731
                                                       i32(world), null, null, one, one, null)
    for rows, world in (((50, 50), 0), ((50, 50), -1), ((1,) * 65, 65), ((1, 0), 2), ((0, 0, 0), 3), ((1,), 1), ((5, -1), 2), ((1 << 31, 5), 2)):
        assert combine(rows, world) == _lib.SALVE_ERR_BAD_ARG, (rows, world)
        assert lib.salve_last_error()
    for t in ("f32", "bf16"):   # backward_apply: the total must cover this rank's rows and be at least 2
        f = getattr(lib, f"salve_bn_{t}_backward_apply")
        for rows, world, total in ((50, 0, 100), (50, 65, 100), (50, 2, 49), (1, 1, 1), (0, 2, 1)):
            assert f(_desc(rows, 64), *[one] * 7, i32(world), i64(total), one, one, null) == _lib.SALVE_ERR_BAD_ARG, (t, rows, world, total)
