"""Data-parallel training on the MI355X (salve_amd.dist_train, training's `dist=`, `python -m salve_amd.train --gpus N`).

1. Two ranks on the one GPU (backend gloo: RCCL wants a GPU per rank), started with torch.distributed.run as a child process:
   ResNet-18, 96 x 96 inputs, a global batch of 4, three Adam steps under the poly schedule through `training._fit`.  The parent
   emulates the run on the same bytes -- the gradients of rows [0, 2) and of rows [2, 4) taken separately from the same
   parameters, each half with BatchNorm buffers of its own, g0 * 0.5 + g1 * 0.5, the same optimiser step -- and demands
   torch.equal: both ranks' parameters, rank 0's buffers against the emulation's half 0, the reduced metrics.  The emulation is run
   twice first and must equal itself.
2. RCCL in a world of one: three steps through the command line on a tiny --render-from directory, once plain and once under the
   launcher with --force-dist; the checkpoints' state dicts are torch.equal (pack at scale 1 is a bit copy, a sum over one rank is
   the identity).  Shows init_process_group("nccl"), the device all-reduce, the broadcasts, the meter reduce and
   destroy_process_group at work on this stack.
3. `--gpus 2` on a one-GPU box: one line, non-zero, nothing launched.

At most three processes have the GPU open at once (the parent and two ranks); every child has its own timeout and a 60 s
process-group timeout."""

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, synthetic, training  # noqa: E402
from salve_amd.evaluate import ClassAccuracyMeter, DeviceClassMeter  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda:0")
VARIANTS = {"fp32-torch": ("fp32", "torch", "torch", "torch"), "bf16-hip": ("bf16", "hip", "hip", "hip")}   # precision, norm, optim, head
CONFIG = dict(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=1, poly_lr_power=0.9,
              optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=100, resize_w=100, train_h=96, train_w=96,
              apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="dp", num_epochs=1, workers=0, batch_size=4,
              data_root="", layout_data_root="", model_save_dirpath="")
WORLD = 2


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
    """Three train batches and two val batches (4 and 2 rows) of packed input [B, 96, 96, 8] (channels 6 and 7 are the stem's zero
    padding) with labels, from a seeded generator; fp32 on the host -- every consumer casts the same bytes."""
    g = torch.Generator().manual_seed(seed)

    def one(rows):
        x = torch.randn((rows, 96, 96, 8), generator=g)
        x[..., 6:] = 0
        return x, torch.randint(0, 2, (rows, 1), generator=g)

    return {"train": [one(4) for _ in range(3)], "val": [one(4), one(2)]}


def _on_device(batch, precision, lo=None, hi=None):
    x, y = batch
    return x[lo:hi].to(DEV).to(torch.bfloat16 if precision == "bf16" else torch.float32).contiguous(), y[lo:hi].to(DEV)


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

precision, norm, optim, head, work = sys.argv[1:6]
dp = DataParallel.from_env("gloo", timeout_s=60)
assert dp.world == {world} and dp.active
dev = dp.device
args = TrainingConfig(**{config!r})
data = torch.load(work + "/batches.pt")
dtype = torch.bfloat16 if precision == "bf16" else torch.float32


def mine(batches):   # this rank's rows of every batch, as a sharded source yields them
    out = []
    for x, y in batches:
        lo, hi = shard_bounds(x.shape[0], dp.rank, dp.world)
        if hi > lo:
            out.append((x[lo:hi].to(dev).to(dtype).contiguous(), y[lo:hi].to(dev)))
    return out


class Batches(list):   # `len()` stays the number of whole batches, as the sharded sources keep it
    pass


train, val = Batches(mine(data["train"])), Batches(mine(data["val"]))
made = []
get_model = training.get_model
training.get_model = lambda *a, **k: made.append(get_model(*a, **k)) or made[-1]
torch.manual_seed(dp.rank)   # the ranks start from DIFFERENT parameters: rank 0's must win
results = training._fit(args, train, val, work + "/run", None, precision, norm, optim, head, dp)
model = made[0]
torch.cuda.synchronize()
torch.save({{"params": [p.detach().cpu() for p in model.parameters()], "stats": [b.cpu() for b in bn_statistics(model)], "results": results}},
           work + f"/rank{{dp.rank}}.pt")
dp.close()
print("RANK_DONE", dp.rank)
'''


def _emulate(variant, data):
    """The two-rank run in one process: (parameters, half 0's BatchNorm statistics, results)."""
    from salve_amd.dist_train import bn_statistics

    precision, norm, optim, head = VARIANTS[variant]
    args = TrainingConfig(**CONFIG)
    torch.manual_seed(0)   # rank 0's parameters
    model = training.get_model(args, precision, norm, head)
    opt = training.get_optimizer(args, model, optim)
    params = list(model.parameters())
    buffers = dict(model.named_buffers())
    halves = [{k: b.clone() for k, b in buffers.items()} for _ in range(WORLD)]   # every rank's own BatchNorm buffers
    hip_head = head == "hip"

    def new_meters():
        return [DeviceClassMeter(2, DEV) if hip_head else ClassAccuracyMeter(2) for _ in range(WORLD)]

    def forward(split, batch, r, meters):
        lo, hi = (r * batch[0].shape[0]) // WORLD, ((r + 1) * batch[0].shape[0]) // WORLD
        x, y = _on_device(batch, precision, lo, hi)
        probs, loss = training.cross_entropy_forward_packed(model, split, x, y, meters=meters[r] if hip_head else None, accumulate_loss=split == "train")
        if not hip_head:
            meters[r].update(torch.argmax(probs, dim=1).cpu().numpy(), y.squeeze().cpu().numpy())
        return loss, hi - lo

    def reduced(meters, loss_sums, loss_ns):
        if hip_head:
            recs = [m.record.cpu().numpy().view(_lib.HEAD_METER_DTYPE)[0] for m in meters]
            assert all(int(r["bad_targets"]) == 0 for r in recs)
            correct, total = (sum(r[k][:2].astype(np.float64) for r in recs) for k in ("correct", "total"))
            loss_sum, rows = sum(float(r["loss_sum"]) for r in recs), sum(int(r["loss_rows"]) for r in recs)
        else:
            correct, total = sum(m.correct for m in meters), sum(m.total for m in meters)
            loss_sum, rows = sum(loss_sums), sum(loss_ns)
        return {"avg_loss": loss_sum / rows if rows else 0.0, "mAcc": float(np.mean(correct / (total + 1e-10)))}

    results = {}
    model.train()
    meters, loss_sums, loss_ns = new_meters(), [0.0] * WORLD, [0] * WORLD
    for it, batch in enumerate(data["train"]):
        grads = []
        for r in range(WORLD):
            with torch.no_grad():
                for k, b in buffers.items():
                    b.copy_(halves[r][k])
            opt.zero_grad()
            loss, n = forward("train", batch, r, meters)
            loss.backward()
            grads.append([None if p.grad is None else p.grad.clone() for p in params])
            if not hip_head:
                loss_sums[r] += float(loss.item()) * n
                loss_ns[r] += n
            halves[r] = {k: b.clone() for k, b in buffers.items()}
        for p, g0, g1 in zip(params, *grads):
            assert (g0 is None) == (g1 is None)
            p.grad = None if g0 is None else g0 * 0.5 + g1 * 0.5
        opt.step()
        lr = training.poly_learning_rate(args.base_lr, it + 1, len(data["train"]), power=args.poly_lr_power)
        for group in opt.param_groups:
            group["lr"] = lr
    for k, v in reduced(meters, loss_sums, loss_ns).items():
        results[f"train_{k}"] = [v]
    with torch.no_grad():   # val sees rank 0's statistics on every rank
        for k, b in buffers.items():
            b.copy_(halves[0][k])
        model.eval()
        meters = new_meters()
        for batch in data["val"]:
            for r in range(WORLD):
                forward("val", batch, r, meters)
        for k, v in reduced(meters, [0.0] * WORLD, [0] * WORLD).items():
            results[f"val_{k}"] = [v]
    torch.cuda.synchronize()
    return [p.detach().cpu() for p in params], [b.cpu() for b in bn_statistics(model)], results


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_ranks_on_one_gpu_equal_the_emulation(tmp_path, variant):
    data = _batches()
    torch.save(data, tmp_path / "batches.pt")
    first, again = _emulate(variant, data), _emulate(variant, data)
    assert _equal(first[0], again[0]) and _equal(first[1], again[1]) and first[2] == again[2], "the emulation does not reproduce itself"
    params, stats, results = first
    assert all(bool(torch.isfinite(p).all()) for p in params)

    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=str(ROOT), world=WORLD, config=CONFIG))
    proc = _launch(WORLD, [script, *VARIANTS[variant], tmp_path])
    assert proc.returncode == 0 and proc.stdout.count("RANK_DONE") == WORLD, proc.stdout[-2000:] + proc.stderr[-6000:]
    ranks = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(WORLD)]
    print(f"{variant}: emulation {results}; rank 0 {ranks[0]['results']}")
    assert _equal(ranks[0]["params"], ranks[1]["params"]), "the ranks' parameters differ"
    assert _equal(ranks[0]["params"], params), "the ranks' parameters differ from the emulation's"
    assert _equal(ranks[0]["stats"], stats), "rank 0's BatchNorm statistics differ from the emulation's half 0"
    assert ranks[0]["results"] == ranks[1]["results"] == results
    # rank 0 alone wrote the checkpoint and the results JSON, and they are this run's
    ck = torch.load(tmp_path / "run" / "train_ckpt.pth", map_location="cpu", weights_only=False)
    assert json.loads((tmp_path / "run" / "results-dp.json").read_text()) == results
    assert _equal([v for k, v in ck["state_dict"].items() if k.endswith(("running_mean", "running_var"))], stats)
    assert "rows of 2 ranks" in proc.stderr and proc.stderr.count("train result at epoch") == 1   # one rank logs; the loss it logs is its own rows'


def _render_dir(tmp_path):
    data = tmp_path / "panos"
    data.mkdir()
    panos = synthetic.make_panos(4, scene="box")
    np.save(data / "panos_rgb.npy", np.stack([p[0] for p in panos]))
    np.save(data / "panos_depth.npy", np.stack([p[1] for p in panos]))
    for split, n, seed in (("train", 12, 0), ("val", 5, 1)):
        h = synthetic.make_hypotheses(n, 4, seed=seed)
        d = {"i1": h.i1.tolist(), "i2": h.i2.tolist(), "R": h.R.tolist(), "t": h.t.tolist(), "is_match": [k % 2 for k in range(n)]}
        (data / f"{split}.json").write_text(json.dumps(d))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("TrainingConfig:\n    _target_: salve.training_config.TrainingConfig\n    lr_annealing_strategy: poly\n    base_lr: 0.001\n"
                   "    weight_decay: 0.0001\n    num_ce_classes: 2\n    print_every: 10\n    poly_lr_power: 0.9\n    optimizer_algo: adam\n"
                   "    num_layers: 18\n    pretrained: False\n    dataparallel: True\n    resize_h: 234\n    resize_w: 234\n    train_h: 224\n"
                   "    train_w: 224\n    apply_photometric_augmentation: False\n    modalities: [\"floor_rgb_texture\"]\n"
                   "    cfg_stem: w1\n    num_epochs: 50\n    workers: 15\n    batch_size: 4\n    data_root: /nonexistent\n    layout_data_root:\n"
                   f"    model_save_dirpath: {tmp_path / 'models'}\n    gpu_ids:\n")
    return data, cfg


def test_rccl_world_of_one_equals_the_plain_run(tmp_path):
    data, cfg = _render_dir(tmp_path)
    common = ["--config", cfg, "--render-from", data, "--epochs", "1", "--precision", "bf16", "--norm", "hip", "--optim", "hip", "--head", "hip"]
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.pop("WORLD_SIZE", None)
    plain = subprocess.run([sys.executable, "-m", "salve_amd.train", *map(str, common), "--out", str(tmp_path / "plain")], cwd=str(ROOT),
                           capture_output=True, text=True, timeout=300, env=env)
    assert plain.returncode == 0, plain.stderr[-4000:]
    forced = _launch(1, ["-m", "salve_amd.train", *common, "--out", tmp_path / "forced", "--gpus", "1", "--force-dist", "--dist-timeout", "60"])
    assert forced.returncode == 0, forced.stdout[-2000:] + forced.stderr[-6000:]
    a, b = (torch.load(tmp_path / d / "train_ckpt.pth", map_location="cpu", weights_only=False) for d in ("plain", "forced"))
    assert list(a["state_dict"]) == list(b["state_dict"])
    for k in a["state_dict"]:
        assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k
    assert json.loads((tmp_path / "plain" / "results-w1.json").read_text()) == json.loads((tmp_path / "forced" / "results-w1.json").read_text())
    assert all(bool(torch.isfinite(v).all()) for v in a["state_dict"].values() if v.is_floating_point())


def test_more_gpus_than_the_box_has_is_refused_in_one_line(tmp_path):
    want = torch.cuda.device_count() + 1
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", "x.yaml", "--gpus", str(want), "--decode", "device"],
                          capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert proc.returncode != 0
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.strip()]
    assert len(lines) == 1 and f"--gpus {want}" in lines[0] and "nothing was launched" in lines[0], lines
    assert "torch.distributed" not in proc.stderr and "Traceback" not in proc.stderr
