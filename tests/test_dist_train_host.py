"""Data-parallel training without a device (salve_amd.dist_train, train_feed's shard helpers, the command line's refusals): the row
split, the bucket tables, the meter reduction and the element-count check on a gloo world of two over CPU tensors."""

import os
import re
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from salve_amd import _lib, dist_train, optim, train_feed

ROOT = Path(__file__).resolve().parents[1]
CHUNK = optim.CHUNK


def test_shard_bounds_cover_every_row_once():
    for n in range(10):
        for world in range(1, 5):
            bounds = [train_feed.shard_bounds(n, r, world) for r in range(world)]
            assert bounds[0][0] == 0 and bounds[-1][1] == n
            assert all(lo <= hi for lo, hi in bounds) and all(bounds[r][1] == bounds[r + 1][0] for r in range(world - 1))
            sizes = [hi - lo for lo, hi in bounds]
            assert max(sizes) - min(sizes) <= 1
    from salve_amd.synthetic import HypothesisTable

    assert train_feed.shard_bounds(7, 1, 3) == HypothesisTable.shard_bounds(7, 1, 3)
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            train_feed.shard_bounds(4, rank, world)


def test_slicing_draws_and_jitter_draws_picks_the_ranks_rows():
    """Rows [lo, hi) of the draws; of the per-image jitter draws, `images_per_example` consecutive ones per row."""
    E = 4
    draws = [(k, k + 1, bool(k & 1), False) for k in range(6)]
    jitter = [((0, 1, 2, 3), 15, float(k), 1.0, 1.0, 0.0) for k in range(6 * E)]
    for world in (2, 3):
        got_d, got_j = [], []
        for r in range(world):
            lo, hi = train_feed.shard_bounds(6, r, world)
            d, j = train_feed.shard_draws(draws, jitter, E, lo, hi)
            assert d == draws[lo:hi] and j == jitter[lo * E:hi * E] and len(j) == E * len(d)
            assert [x[2] for x in j] == [float(k) for k in range(lo * E, hi * E)]
            got_d += d
            got_j += j
        assert got_d == draws and got_j == jitter
    assert train_feed.shard_draws(draws, None, E, 2, 4) == (draws[2:4], None)


def test_shard_plan_cuts_every_batch_and_drops_an_empty_slice():
    plan = train_feed.plan_epoch(9, 4, "val")          # batches of 4, 4, 1
    for world in (2, 3):
        seen = []
        for r in range(world):
            mine, rows = train_feed.shard_plan(plan, r, world)
            assert len(mine) == len(rows) and all(len(m) == hi - lo > 0 for m, (n, lo, hi) in zip(mine, rows))
            seen += [int(i) for m in mine for i in m]
        assert sorted(seen) == list(range(9))
    mine, rows = train_feed.shard_plan(plan, 0, 2)     # rank 0 of 2 gets nothing of the one-row last batch: [0, 0)
    assert [m.tolist() for m in mine] == [[0, 1], [4, 5]] and rows == [(4, 0, 2), (4, 0, 2)]
    mine, rows = train_feed.shard_plan(plan, 1, 2)
    assert [m.tolist() for m in mine] == [[2, 3], [6, 7], [8]] and rows[-1] == (1, 0, 1)
    same, rows = train_feed.shard_plan(plan, 0, 1)
    assert all(a is b for a, b in zip(same, plan)) and rows == [(4, 0, 4), (4, 0, 4), (1, 0, 1)]


def test_batch_size_must_divide_over_the_ranks():
    train_feed.check_shard(6, "train", 1, 3)
    train_feed.check_shard(5, "val", 1, 3)             # val batches split as they come
    with pytest.raises(ValueError, match="multiple"):
        train_feed.check_shard(6, "train", 0, 4)
    from salve_amd.train_files import TileFileLoader, TileFileSource  # noqa: F401
    from salve_amd.train_render import RenderedTrainSource

    with pytest.raises(ValueError, match="multiple"):
        RenderedTrainSource("cuda:0", ["floor_rgb_texture"], batch_size=6, rank=0, world=4)
    with pytest.raises(ValueError, match="multiple"):
        TileFileSource("cuda:0", [], batch_size=5, rank=1, world=2)


def test_bucket_tables():
    lengths = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 64, 2359296]
    pointers = [4096 * (k + 1) for k in range(len(lengths))]
    table, chunk_map, total = dist_train.build_bucket_tables(pointers, lengths)
    off = table["offset"]
    assert (off % 4 == 0).all() and (np.diff(off) >= 0).all() and off[0] == 0
    ends = off + table["n"]
    pad = np.append(off[1:], total) - ends             # behind every segment, up to the next one (or the buffer's end)
    assert (pad >= 0).all() and (pad <= 3).all() and total % 4 == 0
    assert table["tensor"].tolist() == pointers and table["n"].tolist() == lengths
    segs = [optim.Segment(p, p, p, p, 0, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1) for p, n in zip(pointers, lengths)]
    adam_table, adam_chunks = optim.build_tables(segs)
    assert chunk_map.dtype == adam_chunks.dtype and np.array_equal(chunk_map, adam_chunks)
    assert np.array_equal(chunk_map, optim.build_chunk_map(lengths)) and len(chunk_map) == sum(optim.chunk_count(n) for n in lengths)
    offsets, elems = dist_train.bucket_offsets(lengths)
    assert np.array_equal(offsets, off) and elems == total
    assert dist_train.bucket_offsets([])[1] == 0
    with pytest.raises(ValueError):
        dist_train.bucket_offsets([4, -1])


def test_new_symbols_are_declared_and_bound():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    declared = set(re.findall(r"\b(salve_[a-z0-9_]+)\s*\(", header))
    for name in ("salve_flat_pack", "salve_flat_unpack"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    assert _lib.EXPECTED_ABI == 7 == int(re.search(r"#define SALVE_HIP_ABI_VERSION (\d+)", header).group(1))
    assert _lib.FLAT_SEGMENT_DTYPE.itemsize == 24 and "salve_flat_segment_t; /* 24 bytes */" in header


def test_a_world_of_one_runs_no_collective():
    dp = dist_train.DataParallel()                     # no process group exists: any collective would raise
    assert not dp.active and dp.is_main
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.full((3,), 2.0)
    g = p.grad
    dp.all_reduce_gradients([p])
    dp.broadcast([p])
    dp.check_elements(5)
    assert p.grad is g and dp.reduce_meter(None, loss=(1.5, 2)) == (1.5, 2)
    dp.close()
    with pytest.raises(ValueError):
        dist_train.DataParallel(backend="mpi")
    with pytest.raises(ValueError):
        dist_train.DataParallel(rank=2, world=2)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import datetime

    from salve_amd.evaluate import ClassAccuracyMeter

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    dp = dist_train.DataParallel(rank, world, None, "gloo")
    meter = ClassAccuracyMeter(2)
    meter.update(np.array([0, 1, 1]), np.array([0, 0, 1]) if rank == 0 else np.array([1, 1, 1]))
    loss = dp.reduce_meter(meter, loss=(0.1 + rank, 3 + rank))
    only_loss = dp.reduce_meter(None, loss=(float(rank), 1))
    # a DeviceClassMeter's record, on the host: int64 counts, the loss sum a double stored in one of the words
    rec = np.zeros(1, dtype=_lib.HEAD_METER_DTYPE)
    rec["total"][0, :2] = (2 + rank, 5)
    rec["correct"][0, :2] = (1, 4 * rank)
    rec["loss_sum"], rec["loss_rows"] = 0.25 + 0.5 * rank, 7 + rank
    from salve_amd.evaluate import DeviceClassMeter

    dm = DeviceClassMeter.__new__(DeviceClassMeter)
    dm.num_classes, dm.record = 2, torch.from_numpy(rec.view(np.int64).copy())
    dp.reduce_meter(dm)
    dp.check_elements(1000)                            # equal on both ranks: passes
    raised = None
    try:
        dp.check_elements(1000 + rank)                 # unequal: every rank raises, nobody waits for a collective that cannot match
    except RuntimeError as e:
        raised = str(e)
    torch.save({"correct": meter.correct, "total": meter.total, "loss": loss, "only_loss": only_loss, "record": dm.read(), "raised": raised},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_gloo_world_of_two_sums_meters_and_checks_the_element_count(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2)]
    for g in got:
        # rank 0: targets (0, 0, 1), predictions (0, 1, 1); rank 1: targets (1, 1, 1), predictions (0, 1, 1)
        assert g["total"].tolist() == [2.0, 4.0] and g["correct"].tolist() == [1.0, 3.0]
        assert g["loss"] == ((0.1 + 0) + (0.1 + 1), 7) and g["only_loss"] == (1.0, 2)
        accs, macc, avg = g["record"]
        assert accs.tolist() == [2 / (5 + 1e-10), 4 / (10 + 1e-10)] and avg == (0.25 + 0.75) / 15
        assert g["raised"] is not None and "[1000, 1001]" in g["raised"]


def _main(argv):
    from salve_amd import train

    with pytest.raises(SystemExit) as e:
        train.main(argv)
    return e.value.code


def test_command_line_refusals(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert "--gpus must be 1 .. 16, got 0" in str(_main(["--config", "x.yaml", "--gpus", "0"]))
    assert "--gpus must be 1 .. 16, got 17" in str(_main(["--config", "x.yaml", "--gpus", "17"]))
    import salve_amd.train as train

    started = []
    monkeypatch.setattr(train.subprocess, "run", lambda *a, **k: started.append(a) or subprocess.CompletedProcess(a, 0))
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    msg = str(_main(["--config", "x.yaml", "--gpus", "2", "--render-from", "d"]))
    assert "--gpus 2" in msg and "1 GPU(s)" in msg and not started
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    assert "--decode device" in str(_main(["--config", "x.yaml", "--gpus", "2"])) and not started   # the host feed is not sharded
    assert _main(["--config", "x.yaml", "--gpus", "4", "--decode", "device", "--epochs", "1"]) == 0
    (cmd,), = started
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-10:] == ["-m", "salve_amd.train", "--config", "x.yaml", "--gpus", "4", "--decode", "device", "--epochs", "1"]
    assert not torch.cuda.is_initialized()


def test_the_refusal_is_one_line_and_launches_nothing(tmp_path):
    """`python -m salve_amd.train --gpus 2` where fewer than two GPUs show: non-zero exit, one line, no launcher."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run([sys.executable, "-m", "salve_amd.train", "--config", "x.yaml", "--gpus", "16", "--decode", "device"], capture_output=True,
                          text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert proc.returncode != 0
    lines = [l for l in (proc.stdout + proc.stderr).splitlines() if l.strip()]
    assert len(lines) == 1 and "--gpus 16" in lines[0] and "GPU(s)" in lines[0] and "nothing was launched" in lines[0], lines


def test_host_decode_is_refused_in_a_world_of_two():
    from salve_amd import training
    from salve_amd.training_config import TrainingConfig

    args = TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=True, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=("floor_rgb_texture",), cfg_stem="dp", num_epochs=1,
                          workers=0, batch_size=4, data_root="", layout_data_root="", model_save_dirpath="")
    dp = dist_train.DataParallel(1, 2, None, "gloo")
    with pytest.raises(ValueError, match="--decode device"):
        training.train(args, "unused", decode="host", dist=dp)
