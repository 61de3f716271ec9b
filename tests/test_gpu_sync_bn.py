"""The synchronised HIP BatchNorm on the MI355X (salve_bn_*_stats / salve_bn_combine / salve_bn_*_apply / salve_bn_*_backward_reduce /
salve_bn_*_backward_apply, SyncBatchNormHipFunction, `sync_bn=True`).

1. A world of one equals the fused entries bit for bit: y, save_mean, save_invstd, the running statistics, dx, dres, dgamma and
   dbeta, into sentinel-filled buffers with a guard behind each, fp32 and bf16, the four ADD / RELU combinations, rows 2, 63, 64, 65
   and 4097 (a partial wave, a full one, a second row per thread, a second workgroup), C 8 (the smallest accepted), 64 and 2048.
   One row alone is a statistics question only: salve_bn_*_forward refuses it as before and so does salve_bn_combine, while
   salve_bn_*_stats -- which a rank with one row of a larger batch calls -- gives the row itself and M2 = 0 exactly.
2. Emulated worlds in one process: one tensor cut into 2 and 3 unequal shards (a shard without rows and one with a single row
   among them), stats per shard -> combine -> apply per shard, and likewise backward.  Whichever "rank" combines gets the same
   bytes.  The error of y and dx against the float64 restatement (tests/sync_bn_cases.py) is held against the error of the fused
   entry on the uncut tensor against the same restatement: at most ERR_FACTOR times it.
3. Two gloo ranks on the one GPU, started as tests/test_gpu_dist_train.py starts its own: ResNet-18, 6 channels, batch 4 split
   2 + 2, 64 x 64 images, two Adam steps through `training._fit(..., sync_bn=True)` with the HIP norm, fp32 and bf16 (and, by the
   same two processes, once more with sync_bn=False).  (a) Both
   ranks' parameters and running statistics (taken before the broadcast in front of validation) are bit-identical; (b) they equal
   an in-process emulation exactly -- two threads, one per half, whose "all-gather" is a barrier and a torch.stack; (c) they agree
   with single-process training of the whole batch far better than the unsynchronised two-rank run does; (d) with sync_bn=False
   the two ranks' running statistics differ.

ERR_FACTOR and the figures of (c) were chosen after measuring; the measured figures are in profiles/r17_sync_bn.txt."""

import ctypes
import os
import socket
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, training  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402
from tests import sync_bn_cases as cases  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")
RELU, ADD = _lib.BN_RELU, _lib.BN_ADD
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64           # elements behind every output that must keep the sentinel
EPS, MOMENTUM = 1e-5, 0.1
# Test 2's bound: the split chain's error against float64 may be this many times the fused entry's on the same data.  The chain
# differs from the fused entry by one more Chan step per rank on (mean, M2) -- each a handful of fp32 roundings, against the dozens
# the fused statistics pass already makes -- and by one more fp32 addition per rank on the backward sums; y and dx are then formed
# by the same instructions.  Measured (profiles/r17_sync_bn.txt): between 0.83 and 1.44 times the fused entry's error.
ERR_FACTOR = 2.0


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _desc(rows, c, flags):
    return _lib.BnDesc(rows, c, flags, EPS, MOMENTUM)


def _ws(desc, p):
    n = int(_lib.load().salve_bn_workspace_bytes(ctypes.byref(desc), p))
    assert n > 0, _lib.load().salve_last_error()
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


class Out:
    """An output buffer of `shape` filled with a NaN sentinel, with GUARD sentinel elements behind it."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.n, self.shape = n, tuple(shape)
        self.raw = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.raw[:n].view(self.shape)

    def done(self, what):
        """The tensor, after checking that all of it was written and nothing behind it."""
        assert bool(torch.isnan(self.raw[self.n:]).all()), f"{what}: written past its end"
        assert not bool(torch.isnan(self.t).any()), f"{what}: not fully written"
        return self.t


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def make(rows, c, dtype, seed):
    """Finite inputs on the device; the channels' means and scales differ, gamma and beta are not trivial."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    scale = torch.rand(c, generator=g) * 2.5 + 0.5
    x = torch.randn((rows, c), generator=g) * scale + (torch.rand(c, generator=g) * 8 - 4)
    t = dict(x=x, residual=torch.randn((rows, c), generator=g), dy=torch.randn((rows, c), generator=g))
    t = {k: v.to(DEV).to(dtype).contiguous() for k, v in t.items()}
    t.update(gamma=(torch.rand(c, generator=g) + 0.5).to(DEV), beta=(torch.rand(c, generator=g) - 0.5).to(DEV),
             running_mean=torch.randn(c, generator=g).to(DEV), running_var=(torch.rand(c, generator=g) * 1.5 + 0.5).to(DEV))
    return t


def fused(name, t, flags):
    """salve_bn_*_forward and _backward on the whole tensor -> dict of outputs (None where the entry writes none)."""
    lib, dt = _lib.load(), DTYPES[name]
    rows, c = t["x"].shape
    d = _desc(rows, c, flags)
    res = t["residual"] if flags & ADD else None
    y, mean, invstd = Out((rows, c), dt), Out((c,), torch.float32), Out((c,), torch.float32)
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()
    ws, n = _ws(d, _lib.BN_FWD)
    st = getattr(lib, f"salve_bn_{name}_forward")(ctypes.byref(d), _ptr(t["x"]), _ptr(res), _ptr(t["gamma"]), _ptr(t["beta"]), _ptr(rm), _ptr(rv),
                                                  _ptr(y.raw), _ptr(mean.raw), _ptr(invstd.raw), _ptr(ws), n, _stream())
    _lib.check(st, "forward")
    dx, dres, dgamma, dbeta = Out((rows, c), dt), Out((rows, c), dt) if flags & ADD else None, Out((c,), torch.float32), Out((c,), torch.float32)
    ws, n = _ws(d, _lib.BN_BWD)
    st = getattr(lib, f"salve_bn_{name}_backward")(ctypes.byref(d), _ptr(t["dy"]), _ptr(t["x"]), _ptr(y.raw if flags & RELU else None), _ptr(t["gamma"]),
                                                   _ptr(mean.raw), _ptr(invstd.raw), _ptr(dx.raw), _ptr(None if dres is None else dres.raw),
                                                   _ptr(dgamma.raw), _ptr(dbeta.raw), _ptr(ws), n, _stream())
    _lib.check(st, "backward")
    return dict(y=y.done("y"), mean=mean.done("save_mean"), invstd=invstd.done("save_invstd"), running_mean=rm, running_var=rv, dx=dx.done("dx"),
                dres=None if dres is None else dres.done("dres"), dgamma=dgamma.done("dgamma"), dbeta=dbeta.done("dbeta"))


def split(name, t, flags, rows_of):
    """The split chain over emulated ranks holding `rows_of` rows each: the same dict; y, dx, dres concatenated in rank order,
    dgamma / dbeta [world, C] (every rank's own), and under "combined" what every rank's own salve_bn_combine call gave."""
    lib, dt = _lib.load(), DTYPES[name]
    c, world = t["x"].shape[1], len(rows_of)
    total = int(sum(rows_of))
    hi = np.cumsum(rows_of)
    cut = list(zip((hi - np.asarray(rows_of)).tolist(), hi.tolist()))
    host_rows = (ctypes.c_int64 * world)(*rows_of)
    partials = Out((world, 2, c), torch.float32)
    for r, (lo, up) in enumerate(cut):
        d = _desc(up - lo, c, flags)
        ws, n = _ws(d, _lib.BN_STATS)
        _lib.check(getattr(lib, f"salve_bn_{name}_stats")(ctypes.byref(d), _ptr(t["x"][lo:up]) if up > lo else _ptr(None), _ptr(partials.t[r]),
                                                          _ptr(ws), n, _stream()), "stats")
    partials.done("partials")
    combined = []
    for r in range(world):   # every rank combines for itself, with running statistics of its own
        mean, invstd = Out((c,), torch.float32), Out((c,), torch.float32)
        rm, rv = t["running_mean"].clone(), t["running_var"].clone()
        d = _desc(rows_of[r], c, flags)
        _lib.check(lib.salve_bn_combine(ctypes.byref(d), _ptr(partials.t), ctypes.cast(host_rows, ctypes.c_void_p), ctypes.c_int32(world), _ptr(rm),
                                        _ptr(rv), _ptr(mean.raw), _ptr(invstd.raw), _stream()), "combine")
        combined.append(dict(mean=mean.done("mean"), invstd=invstd.done("invstd"), running_mean=rm, running_var=rv))
    mean, invstd = combined[0]["mean"], combined[0]["invstd"]
    y = Out((total, c), dt)
    sums = Out((world, 2, c), torch.float32)
    for r, (lo, up) in enumerate(cut):
        d = _desc(up - lo, c, flags)
        live = up > lo
        _lib.check(getattr(lib, f"salve_bn_{name}_apply")(ctypes.byref(d), _ptr(t["x"][lo:up] if live else None),
                                                          _ptr(t["residual"][lo:up] if live and flags & ADD else None), _ptr(t["gamma"]), _ptr(t["beta"]),
                                                          _ptr(mean), _ptr(invstd), _ptr(y.t[lo:up] if live else None), _stream()), "apply")
    y.done("y")
    for r, (lo, up) in enumerate(cut):
        d = _desc(up - lo, c, flags)
        live = up > lo
        ws, n = _ws(d, _lib.BN_BWD_REDUCE)
        _lib.check(getattr(lib, f"salve_bn_{name}_backward_reduce")(ctypes.byref(d), _ptr(t["dy"][lo:up] if live else None),
                                                                    _ptr(t["x"][lo:up] if live else None),
                                                                    _ptr(y.t[lo:up] if live and flags & RELU else None), _ptr(mean), _ptr(invstd),
                                                                    _ptr(sums.t[r]), _ptr(ws), n, _stream()), "backward_reduce")
    sums.done("sums")
    dx, dres = Out((total, c), dt), Out((total, c), dt) if flags & ADD else None
    for r, (lo, up) in enumerate(cut):
        d = _desc(up - lo, c, flags)
        live = up > lo
        _lib.check(getattr(lib, f"salve_bn_{name}_backward_apply")(ctypes.byref(d), _ptr(t["dy"][lo:up] if live else None),
                                                                   _ptr(t["x"][lo:up] if live else None),
                                                                   _ptr(y.t[lo:up] if live and flags & RELU else None), _ptr(t["gamma"]), _ptr(mean),
                                                                   _ptr(invstd), _ptr(sums.t), ctypes.c_int32(world), ctypes.c_int64(total),
                                                                   _ptr(dx.t[lo:up] if live else None),
                                                                   _ptr(dres.t[lo:up] if live and dres is not None else None), _stream()), "backward_apply")
    out = dict(combined[0])
    out.update(y=y.t, dx=dx.done("dx"), dres=None if dres is None else dres.done("dres"), dgamma=sums.t[:, 1], dbeta=sums.t[:, 0], combined=combined)
    return out


# ---------------------------------------------------------------------------------------------------- 1. a world of one
@pytest.mark.parametrize("flags", [0, RELU, ADD, ADD | RELU])
@pytest.mark.parametrize("name", list(DTYPES))
def test_world_of_one_equals_the_fused_entries_bit_for_bit(name, flags):
    for rows in (2, 63, 64, 65, 4097):
        for c in (8, 64, 2048):
            t = make(rows, c, DTYPES[name], seed=rows * 7 + c)
            want, got = fused(name, t, flags), split(name, t, flags, [rows])
            for k in ("y", "mean", "invstd", "running_mean", "running_var", "dx", "dres"):
                assert (want[k] is None and got[k] is None) or _same(want[k], got[k]), (rows, c, k)
            assert _same(want["dgamma"], got["dgamma"][0]) and _same(want["dbeta"], got["dbeta"][0]), (rows, c)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(DTYPES))
def test_a_single_row_has_statistics_but_no_batchnorm_of_its_own(name):
    lib = _lib.load()
    for c in (8, 64, 2048):
        t = make(1, c, DTYPES[name], seed=c)
        d = _desc(1, c, 0)
        assert int(lib.salve_bn_workspace_bytes(ctypes.byref(d), _lib.BN_FWD)) == 0   # the fused forward refuses one row, as before
        part = Out((2, c), torch.float32)
        ws, n = _ws(d, _lib.BN_STATS)
        _lib.check(getattr(lib, f"salve_bn_{name}_stats")(ctypes.byref(d), _ptr(t["x"]), _ptr(part.raw), _ptr(ws), n, _stream()), "stats")
        p = part.done("partial")
        assert _same(p[0], t["x"][0].float()) and not bool(p[1].any()), c   # the row itself, M2 = 0 exactly
        one = (ctypes.c_int64 * 1)(1)
        st = lib.salve_bn_combine(ctypes.byref(d), _ptr(p), ctypes.cast(one, ctypes.c_void_p), ctypes.c_int32(1), _ptr(None), _ptr(None), _ptr(part.raw),
                                  _ptr(part.raw), _stream())
        assert st == _lib.SALVE_ERR_BAD_ARG   # ... and so does the combine of a world that holds one row in all
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 2. emulated worlds
WORLDS = ([500, 1037], [1037, 500], [0, 1537], [700, 1, 836], [512, 0, 1025], [3, 1533, 1])


def _f64(t, key):
    return t[key].double().cpu().numpy()


def _errors(t, flags, got):
    """(error of y, error of dx) of device results against the float64 restatement of full-batch BatchNorm on the same inputs.  The
    ReLU mask of the backward reference is taken from the results' own y, so that a y within rounding of 0 is not counted as an
    error of dx."""
    case = dict(x=_f64(t, "x"), residual=_f64(t, "residual"), dy=_f64(t, "dy"), gamma=_f64(t, "gamma"), beta=_f64(t, "beta"),
                running_mean=_f64(t, "running_mean"), running_var=_f64(t, "running_var"), flags=flags, eps=EPS, momentum=MOMENTUM)
    ref = cases.full_forward(case)
    masked = dict(ref, y=_f64(got, "y"))
    ref_b = cases.full_backward(case, masked)
    return cases.max_rel(_f64(got, "y"), ref["y"]), cases.max_rel(_f64(got, "dx"), ref_b["dx"]), ref


@pytest.mark.parametrize("flags", [0, ADD | RELU])
@pytest.mark.parametrize("name", list(DTYPES))
def test_emulated_worlds_agree_with_float64_as_the_fused_entry_does(name, flags):
    c = 64
    total = sum(WORLDS[0])
    t = make(total, c, DTYPES[name], seed=11 + flags)
    parent = fused(name, t, flags)
    ey0, edx0, ref = _errors(t, flags, parent)
    print(f"fused {name} flags {flags}: y error {ey0:.3e}, dx error {edx0:.3e}")
    assert ey0 > 0 and edx0 > 0
    for rows_of in WORLDS:
        assert sum(rows_of) == total
        got = split(name, t, flags, rows_of)
        first = got["combined"][0]
        for other in got["combined"][1:]:   # whichever rank combines: the same bytes
            assert all(_same(first[k], other[k]) for k in ("mean", "invstd", "running_mean", "running_var")), rows_of
        ey, edx, _ = _errors(t, flags, got)
        stat = max(cases.max_rel(_f64(got, k), ref[k]) for k in ("mean", "invstd", "running_mean", "running_var"))
        stat0 = max(cases.max_rel(_f64(parent, k), ref[k]) for k in ("mean", "invstd", "running_mean", "running_var"))
        print(f"split {name} flags {flags} rows {rows_of}: y error {ey:.3e} ({ey / ey0:.2f} x fused), dx error {edx:.3e} ({edx / edx0:.2f} x fused), "
              f"statistics {stat:.3e} (fused {stat0:.3e})")
        assert ey <= ERR_FACTOR * ey0, (rows_of, ey, ey0)
        assert edx <= ERR_FACTOR * edx0, (rows_of, edx, edx0)
        # the ranks' dgamma / dbeta add up to the whole batch's: every term goes through fewer than 64 fp32 additions on its way into a
        # sum (the rows of a thread, the LDS tree, the partials, the shuffle tree, the ranks), and xhat carries the statistics' error
        case_b = dict(x=_f64(t, "x"), dy=_f64(t, "dy"), gamma=_f64(t, "gamma"), flags=flags)
        ref_b = cases.full_backward(case_b, dict(ref, y=_f64(got, "y")))
        g = np.abs(np.where(_f64(got, "y") > 0, case_b["dy"], 0.0) if flags & RELU else case_b["dy"])
        xhat = np.abs((case_b["x"] - ref["mean"]) * ref["invstd"])
        for k, terms in (("dbeta", g), ("dgamma", g * (xhat + 1.0))):
            err = np.abs(got[k].double().sum(dim=0).cpu().numpy() - ref_b[k])
            assert bool((err <= 64 * 2.0 ** -24 * terms.sum(axis=0)).all()), (rows_of, k)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 3. two ranks on one GPU
VARIANTS = ("fp32", "bf16")
WORLD, STEPS = 2, 2
CONFIG = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=1, poly_lr_power=0.9,
              optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=68, resize_w=68, train_h=64, train_w=64,
              apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="sbn", num_epochs=1, workers=0, batch_size=4,
              data_root="", layout_data_root="", model_save_dirpath="")
# (c): the synchronised two-rank run must be at least this many times closer to single-process training of the whole batch than the
# unsynchronised two-rank run (the parent's behaviour) is, in the running statistics after two steps.  What separates the
# synchronised run from the single process is rounding alone (the order of the weight-gradient sums over 2 + 2 instead of 4 rows, one
# Chan step); what separates the unsynchronised run is statistics over 2 instead of 4 samples.  The parameters are held to a
# smaller factor: Adam's first steps move a parameter by the learning rate times the SIGN of its gradient, so a gradient within
# rounding of zero moves its parameter the other way, in fp32 here and there and in bf16 more often.  Distances are relative 2-norms
# over all elements.  Measured (profiles/r17_sync_bn.txt): statistics 5656 x (fp32) and 45 x (bf16) closer, parameters 192 x and 16 x.
CLOSER, CLOSER_PARAMS = 10.0, 4.0

_RANK_SCRIPT = '''
import logging
import sys
sys.path.insert(0, {root!r})
import torch
logging.basicConfig(level=logging.INFO)
from salve_amd import training
from salve_amd.dist_train import DataParallel, bn_statistics
from salve_amd.train_feed import shard_bounds
from salve_amd.training_config import TrainingConfig

precision, work = sys.argv[1:3]
dp = DataParallel.from_env("gloo", timeout_s=60)
assert dp.world == {world} and dp.active
dev = dp.device
args = TrainingConfig(**{config!r})
data = torch.load(work + "/batches.pt")
dtype = torch.bfloat16 if precision == "bf16" else torch.float32


class Batches(list):
    pass


def mine(batches):
    out = Batches()
    for x, y in batches:
        lo, hi = shard_bounds(x.shape[0], dp.rank, dp.world)
        out.append((x[lo:hi].to(dev).to(dtype).contiguous(), y[lo:hi].to(dev)))
    return out


made, before = [], []
get_model = training.get_model
training.get_model = lambda *a, **k: made.append(get_model(*a, **k)) or made[-1]
broadcast = dp.broadcast


def recording(tensors, src=0):   # the running statistics as training left them, before rank 0's are handed out for validation
    tensors = list(tensors)
    if made and len(tensors) == len(bn_statistics(made[-1])) and all(a is b for a, b in zip(tensors, bn_statistics(made[-1]))):
        before.append([t.detach().cpu().clone() for t in tensors])
    return broadcast(tensors, src)


dp.broadcast = recording
out = {{}}
for mode in ("sync", "plain"):   # the same two ranks train twice: with the switch and as the parent does
    torch.manual_seed(dp.rank)   # the ranks start from DIFFERENT parameters: rank 0's must win
    training._fit(args, mine(data["train"]), mine(data["val"]), work + "/run_" + mode, None, precision, "hip", "torch", "torch", dp,
                  sync_bn=mode == "sync")
    model = made[-1]
    assert (model.sync_norm is not None) == (mode == "sync") and len(before) == len(made) == len(out) + 1
    torch.cuda.synchronize()
    out[mode] = {{"params": [p.detach().cpu() for p in model.parameters()], "stats": before[-1]}}
torch.save(out, work + f"/rank{{dp.rank}}.pt")
dp.close()
print("RANK_DONE", dp.rank)
'''


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(nproc, tail, timeout=300):
    """torch.distributed.run as a CHILD process (nothing is exec'ed in place) -> CompletedProcess."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + [str(t) for t in tail]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=str(ROOT))


def _batches(seed=0):
    g = torch.Generator().manual_seed(seed)

    def one(rows):
        x = torch.randn((rows, 64, 64, 8), generator=g)
        x[..., 6:] = 0
        return x, torch.randint(0, 2, (rows, 1), generator=g)

    return {"train": [one(4) for _ in range(STEPS)], "val": [one(4)]}


def _on_device(batch, precision, lo=None, hi=None):
    x, y = batch
    return x[lo:hi].to(DEV).to(torch.bfloat16 if precision == "bf16" else torch.float32).contiguous(), y[lo:hi].to(DEV)


def _train(precision, data, group_of=None):
    """STEPS Adam steps from rank 0's parameters in this process -> (parameters, running statistics).  group_of None: one process,
    the whole batch, the fused HIP norm.  group_of(r): WORLD models, one per half of the batch, each on a thread of its own and
    synchronised through `group_of(r)`; the halves' gradients meet as g0 * 0.5 + g1 * 0.5, as the all-reduce adds them."""
    from salve_amd.dist_train import bn_statistics

    args = TrainingConfig(**CONFIG)
    n = 1 if group_of is None else WORLD
    _lib.load()   # (before any thread calls into it)
    torch.manual_seed(0)
    models = [training.get_model(args, precision, "hip", "torch")]
    for r in range(1, n):
        models.append(training.get_model(args, precision, "hip", "torch"))
        models[r].load_state_dict(models[0].state_dict())
    if group_of is not None:
        for r, m in enumerate(models):
            m.set_sync_norm(group_of(r), batch_size=args.batch_size)
    opts = [training.get_optimizer(args, m, "torch") for m in models]
    for m in models:
        m.train()
    for it, batch in enumerate(data["train"]):
        failed = []

        def work(r):
            try:
                rows = batch[0].shape[0]
                x, y = _on_device(batch, precision, r * rows // n, (r + 1) * rows // n)
                opts[r].zero_grad()
                with torch.autograd.set_multithreading_enabled(False):   # the whole backward pass on this thread: its gathers meet the other thread's
                    _, loss = training.cross_entropy_forward_packed(models[r], "train", x, y)
                    loss.backward()
            except BaseException as e:   # noqa: B902 (handed to the test's thread)
                failed.append(e)
                if group_of is not None:
                    group_of(r).barrier.abort()

        if n == 1:
            work(0)
        else:
            threads = [threading.Thread(target=work, args=(r,)) for r in range(n)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
        if failed:
            raise failed[0]
        if n > 1:
            for ps in zip(*(m.parameters() for m in models)):
                assert all((p.grad is None) == (ps[0].grad is None) for p in ps)
                if ps[0].grad is not None:
                    g = ps[0].grad * 0.5 + ps[1].grad * 0.5
                    for p in ps:
                        p.grad = g.clone()
        lr = training.poly_learning_rate(args.base_lr, it + 1, len(data["train"]), power=args.poly_lr_power)
        for opt in opts:
            opt.step()
            for group in opt.param_groups:
                group["lr"] = lr
    torch.cuda.synchronize()
    return [[p.detach().cpu() for p in m.parameters()] for m in models], [[b.cpu() for b in bn_statistics(m)] for m in models]


class ThreadGroup:
    """SyncBatchNormHipFunction's group for emulated ranks on threads of one process: `_gather` waits for every rank's tensor at a
    barrier and stacks them in rank order.  A rank that does not arrive breaks the barrier instead of hanging the test."""

    def __init__(self, world):
        self.world, self.barrier, self.slots = world, threading.Barrier(world, timeout=60), [None] * world

    def of(self, rank):
        outer = self

        class Rank:
            world, active, barrier = outer.world, True, outer.barrier

            def __init__(self):
                self.rank = rank

            def _gather(self, t):
                torch.cuda.current_stream(t.device).synchronize()
                outer.slots[rank] = t.detach().clone()
                outer.barrier.wait()
                out = torch.stack(list(outer.slots))
                outer.barrier.wait()   # nobody overwrites a slot before everyone has read it
                return out

        return Rank()


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _distance(a, b):
    """|a - b| / |b| in the 2-norm over all the tensors' elements."""
    num = sum(float((x.double() - y.double()).pow(2).sum()) for x, y in zip(a, b))
    return float(np.sqrt(num / sum(float(y.double().pow(2).sum()) for y in b)))


@pytest.mark.parametrize("precision", VARIANTS)
def test_two_ranks_keep_one_set_of_statistics(tmp_path, precision):
    data = _batches()
    torch.save(data, tmp_path / "batches.pt")
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=str(ROOT), world=WORLD, config=CONFIG))
    proc = _launch(WORLD, [script, precision, tmp_path])
    assert proc.returncode == 0 and proc.stdout.count("RANK_DONE") == WORLD, proc.stdout[-2000:] + proc.stderr[-6000:]
    ranks = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(WORLD)]
    runs = {mode: [ranks[r][mode] for r in range(WORLD)] for mode in ("sync", "plain")}
    sync, plain = runs["sync"], runs["plain"]
    # (a) one model and one set of running statistics on both ranks
    assert _equal(sync[0]["params"], sync[1]["params"]), "the ranks' parameters differ"
    assert _equal(sync[0]["stats"], sync[1]["stats"]), "the ranks' running statistics differ under sync_bn"
    assert all(bool(torch.isfinite(t).all()) for t in sync[0]["params"] + sync[0]["stats"])
    # (d) the parent's behaviour: every rank normalises its own rows, and the running statistics drift apart
    assert _equal(plain[0]["params"], plain[1]["params"])
    assert not _equal(plain[0]["stats"], plain[1]["stats"]), "without sync_bn the ranks' running statistics should differ"
    # (b) the emulation on two threads, exactly
    group = ThreadGroup(WORLD)
    ranks = [group.of(r) for r in range(WORLD)]
    params, stats = _train(precision, data, lambda r: ranks[r])
    assert _equal(params[0], params[1]) and _equal(stats[0], stats[1]), "the emulated ranks differ from each other"
    assert _equal(sync[0]["params"], params[0]), "the ranks' parameters differ from the emulation's"
    assert _equal(sync[0]["stats"], stats[0]), "the ranks' running statistics differ from the emulation's"
    # (c) single-process training of the whole batch
    (whole_params,), (whole_stats,) = _train(precision, data)
    d_sync, d_plain = _distance(sync[0]["stats"], whole_stats), _distance(plain[0]["stats"], whole_stats)
    p_sync, p_plain = _distance(sync[0]["params"], whole_params), _distance(plain[0]["params"], whole_params)
    print(f"{precision}: running statistics against one process: synchronised {d_sync:.3e}, unsynchronised rank 0 {d_plain:.3e} "
          f"({d_plain / max(d_sync, 1e-300):.1f} x); parameters: synchronised {p_sync:.3e}, unsynchronised {p_plain:.3e}")
    assert d_sync * CLOSER <= d_plain, (d_sync, d_plain)
    assert p_sync * CLOSER_PARAMS <= p_plain, (p_sync, p_plain)
