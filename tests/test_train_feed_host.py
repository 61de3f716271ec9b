"""What the two training feeds share (salve_amd.train_feed), the tile-file feed's job tables, and where the moved planning names live.
No test here needs a GPU."""

import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from salve_amd import _lib, pano_pool, train_feed, train_files, train_render  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DRAWS = [(3, 7, False, False), (0, 0, True, False), (10, 0, False, True), (1, 2, True, True)]


def test_the_moved_names_are_one_object_each():
    assert train_render.plan_epoch is train_feed.plan_epoch and train_render.batches_per_epoch is train_feed.batches_per_epoch
    assert train_render.PanoCache is pano_pool.PanoCache and train_render.epoch_next_use is pano_pool.epoch_next_use
    assert train_render.NEVER == pano_pool.NEVER and train_render.MAX_GATHER_THREADS == pano_pool.MAX_GATHER_THREADS


def test_aug_table_rows():
    aug = train_feed.aug_table(DRAWS)
    assert aug.dtype == _lib.TILE_AUG_DTYPE and aug.shape == (4,)
    flags = [0, _lib.TILE_HFLIP, _lib.TILE_VFLIP, _lib.TILE_HFLIP | _lib.TILE_VFLIP]
    assert len(set(flags)) == 4
    assert aug.tolist() == [(cy, cx, f, 0) for (cy, cx, _, _), f in zip(DRAWS, flags)]
    assert train_feed.aug_table([]).shape == (0,)


class _TablesOnly(train_files.TileFileSource):
    """The tile-file source's table building without a device or a file."""

    def __init__(self, pairs, bev_hw):
        self.per_sample, self.ras = pairs, SimpleNamespace(bev_hw=bev_hw)


def test_tile_tables():
    B, K, H, W = 3, 2, 5, 7
    position = np.array([7, 2, 11, 0, 5, 9, 1, 10, 3, 6, 4, 8], dtype=np.int64)   # image slot of each of the 12 paths, example-major
    assert sorted(position.tolist()) == list(range(12)) and position.tolist() != list(range(12))
    src = _TablesOnly(K, (H, W))
    jobs, aug = src.tile_tables(np.array([4, 0, 2]), DRAWS[:B], position)
    assert jobs.dtype == _lib.TILE_JOB_DTYPE and jobs.shape == (2, B, K)
    for b in range(B):
        for k in range(K):
            assert jobs["bev_offset"][0, b, k] == position[4 * b + 2 * k] * 35
            assert jobs["bev_offset"][1, b, k] == position[4 * b + 2 * k + 1] * 35
            assert jobs["slot"][0, b, k] == jobs["slot"][1, b, k] == b
            assert jobs["chan"][0, b, k] == 6 * k and jobs["chan"][1, b, k] == 6 * k + 3
    want = train_feed.aug_table(DRAWS[:B])
    assert aug.dtype == want.dtype and aug.tolist() == want.tolist()
    with pytest.raises(ValueError, match="3 examples, 2 draws"):
        src.tile_tables(np.array([4, 0, 2]), DRAWS[:2], position)


def test_the_rendered_feed_refuses_a_draw_count_that_is_not_the_batch_size():
    """`aug_table` sizes the table by the draws: a short one would leave the tile launch reading past it."""
    class _CountsOnly(train_render.RenderedTrainSource):
        def __init__(self):
            self.examples, self.surfaces, self.per_sample = {}, ["floor"], 1

    with pytest.raises(ValueError, match="3 examples, 2 draws"):
        _CountsOnly().batch_tables(np.arange(3), DRAWS[:2])


def test_upload_tables_is_one_buffer_sliced_by_cumulative_offsets():
    jobs = np.zeros((2, 3, 2), dtype=_lib.TILE_JOB_DTYPE)
    jobs["bev_offset"] = np.arange(12).reshape(2, 3, 2) * 35
    jobs["slot"], jobs["chan"] = 5, 9
    tables = [jobs, train_feed.aug_table(DRAWS), np.array([1, 0, 1], dtype=np.int64), np.zeros(0, dtype=_lib.LAYOUT_POSE_DTYPE)]
    buf, o = train_feed.upload_tables(tables, "cpu")
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    assert o.tolist() == np.cumsum([0] + [t.nbytes for t in tables]).tolist() and buf.numel() == o[-1]
    for k, t in enumerate(tables):
        back = buf[o[k]:o[k + 1]].numpy().view(t.dtype).reshape(t.shape)
        assert back.tolist() == t.tolist(), k
    assert buf[o[2]:o[3]].view(torch.int64).tolist() == [1, 0, 1]   # as the sources slice their labels


def test_draws_of_every_split_but_train_are_the_centre_crop():
    tf = SimpleNamespace(resize=234, crop=224, draw=lambda: (1, 2, True, False))
    assert train_feed.draws(tf, "train", 3) == [(1, 2, True, False)] * 3
    for split in ("val", "test"):
        assert train_feed.draws(tf, split, 2) == [(5, 5, False, False)] * 2


def test_shared_refusals_keep_their_messages():
    with pytest.raises(ValueError, match=r"split must be one of \('train', 'val', 'test'\), got 'dev'"):
        train_feed.check_arguments(4, "dev", train_files.SPLITS, "fp32")
    with pytest.raises(ValueError, match=r"split must be one of \('train', 'val'\), got 'test'"):
        train_feed.plan_epoch(8, 4, "test")
    with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16', got 'fp16'"):
        train_feed.check_arguments(4, "val", train_feed.SPLITS, "fp16")
    with pytest.raises(ValueError, match="batch size must be positive, got 0"):
        train_feed.check_arguments(0)
    train_feed.check_arguments(1, "test", train_files.SPLITS, "bf16")


def test_importing_the_tile_file_feed_leaves_the_render_feed_out():
    code = ("import sys, salve_amd.train_files; "
            "print([m for m in ('salve_amd.train_render', 'salve_amd.pipeline') if m in sys.modules])")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
