"""evaluate.run_fused_epoch(visual_overlap=True) on several ranks (gloo, CPU): the two pixel counts ride in the path's one all-gather as two
more fp32 columns beside the validity flag -- exact up to 2^24 -- and rank 0 writes the same "overlap" rows as a single process; images
of more than 2^24 pixels are refused when sharded.  A stub stands in for the pipeline (the real one needs the GPU)."""

import json
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from salve_amd import synthetic


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def counts_of(table):
    """int64 [N, 2, 2] (ceiling, floor): a deterministic function of the hypothesis, with values at both ends of what fp32 carries exactly."""
    k = np.round(np.abs(table.theta_deg) * 1000).astype(np.int64)
    union = (k * 46603) % (2 ** 24) + 1
    near = k % 3 == 0                                       # (by the hypothesis, not by its place in a shard)
    union[near] = 2 ** 24 - k[near] % 9                     # 2^24, 2^24 - 1, ..: odd values just below the limit must arrive unchanged
    inter = union - (k % 7) * (union > 7)
    floor = np.stack([inter, union], 1)
    return np.stack([floor // 2, floor], 1)


class StubPipeline:
    surfaces = ["ceiling", "floor"]

    def __init__(self, bev_hw=(4096, 4096)):
        self.ras = SimpleNamespace(bev_hw=bev_hw)
        self.asked = []

    def prepare(self, shard):
        return shard

    def score(self, shard, visual_overlap=False):
        self.asked.append(visual_overlap)
        return torch.from_numpy(np.stack([shard.t[:, 0], shard.t[:, 1]], 1).astype(np.float32))

    def visual_overlap(self, shard):
        assert self.asked[-1] is True
        return counts_of(shard)

    def valid_mask(self, shard):
        return shard.t[:, 0] <= 1.5

    def check(self, what):
        pass


def names(n):
    return [(f"/bev/gt_alignment_approx/0001/a_{j}.jpg", f"/bev/gt_alignment_approx/0001/b_{j}.jpg") for j in range(n)]


def _worker(rank, world, port, n, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from salve_amd import evaluate

    table = synthetic.make_hypotheses(n, 5, seed=1)
    evaluate.run_fused_epoch(StubPipeline(), table, names(n), np.arange(n) % 2, os.path.join(out_dir, "preds"), batch_size=16, world=world, rank=rank,
                             visual_overlap=True)
    with pytest.raises(RuntimeError, match="2\\^24"):
        evaluate.run_fused_epoch(StubPipeline((4097, 4096)), table, names(n), None, os.path.join(out_dir, "refused"), world=world, rank=rank, visual_overlap=True)
    dist.destroy_process_group()


def read(d):
    return [json.load(open(f)) for f in sorted(d.glob("batch_*.json"), key=lambda f: int(f.stem.split("_")[1]))]


@pytest.mark.parametrize("n,world", [(37, 2)])
def test_counts_ride_in_the_one_all_gather(tmp_path, n, world):
    from salve_amd import evaluate

    mp.spawn(_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
    table = synthetic.make_hypotheses(n, 5, seed=1)
    keep = np.nonzero(table.t[:, 0] <= 1.5)[0]
    assert 0 < len(keep) < n
    got = read(tmp_path / "preds")
    want = counts_of(table)[keep, 1].tolist()           # the floor's, of the kept rows, in table order
    assert sum((g["overlap"] for g in got), []) == want
    assert max(r[1] for r in want) >= 2 ** 24 - 7 and any(r[1] % 2 and r[1] > 2 ** 23 for r in want)
    assert not (tmp_path / "refused").exists()
    # a single process writes the same files; without the keyword the key is absent and the stub is never asked for the counts
    one, off = StubPipeline((5000, 5000)), StubPipeline()          # (large images are fine in a world of one: no fp32 in between)
    evaluate.run_fused_epoch(one, table, names(n), np.arange(n) % 2, str(tmp_path / "one"), batch_size=16, visual_overlap=True)
    evaluate.run_fused_epoch(off, table, names(n), np.arange(n) % 2, str(tmp_path / "off"), batch_size=16)
    assert read(tmp_path / "one") == got and one.asked == [True] and off.asked == [False]
    assert [{k: v for k, v in g.items() if k != "overlap"} for g in got] == read(tmp_path / "off")
