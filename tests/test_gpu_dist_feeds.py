"""The sharded feeds' contract on the MI355X, in one process and without a process group: for a world of 2 and of 3, the rows a
`(rank, world)` source yields are, batch by batch, rows [lo, hi) of the world-1 source's batch -- images and labels, torch.equal --
for two train epochs (the generators stay in step from one epoch to the next) and a val epoch whose last batch (2 rows) is shorter
than a world of 3, so one rank yields nothing for it.

RenderedTrainSource: 8 small synthetic panoramas, batches of 6, fp32 and bf16; again with a resident pool that prefetches, and with
the photometric augmentation.  TileFileSource: the golden renderings plus a few written tiles; again with read_ahead, and with the
photometric augmentation.  The world-1 batches of a mode are made once and shared by its two worlds."""

import functools
import random
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import synthetic, train_feed, train_render  # noqa: E402
from salve_amd.train_files import TileFileLoader, TileFileSource  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")
RENDERINGS = Path(__file__).resolve().parent / "golden" / "renderings"
FLOOR = ["floor_rgb_texture"]
P, B, N, SEED = 8, 6, 14, 5          # 14 examples in batches of 6: two train batches; val batches of 6, 6 and 2
EPOCHS = (("train", 21), ("train", 22), ("val", 23))

RENDERED_MODES = {
    "fp32": dict(precision="fp32"),
    "bf16": dict(precision="bf16"),
    "pool+prefetch": dict(precision="bf16", identity="batch", resident_panos=P, prefetch=True),
    "photometric": dict(precision="fp32", photometric="device"),
}
FILE_MODES = {
    "files": dict(),
    "files-read-ahead": dict(read_ahead=True),
    "files-photometric": dict(precision="bf16", photometric="device"),
}


@functools.lru_cache(maxsize=None)
def _panos():
    panos = synthetic.make_panos(P, scene="box")
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])


def _table(seed):
    hyp = synthetic.make_hypotheses(N, P, seed=seed)
    hyp.swap = (np.arange(N) % 3 == 1)
    return hyp, np.arange(N, dtype=np.int64)   # (the label IS the example's index: the rows show in the labels)


def _rendered(split, rank, world, **kw):
    src = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=B, split=split, seed=SEED, rank=rank, world=world, **kw)
    src.load_panos(*_panos())
    src.set_examples(*_table(6 if split == "train" else 7))
    return src


@pytest.fixture(scope="module")
def data_list(tmp_path_factory):
    """14 two-tile examples over the fixture's tiles and four written ones; the label is the example's index."""
    root = tmp_path_factory.mktemp("dist_tiles")
    files = []
    for f in sorted((RENDERINGS / "gt_alignment_approx" / "1208").glob("*.jpg")):
        shutil.copy(f, root / f.name)
        files.append(str(root / f.name))
        rgb = image_io.read_rgb(str(f))
        for tag, img in (("ud", rgb[::-1]), ("lr", rgb[:, ::-1])):
            image_io.write_jpeg(str(root / f"{tag}_{f.name}"), img.copy())
            files.append(str(root / f"{tag}_{f.name}"))
    assert len(files) >= 6
    return [(files[k % len(files)], files[(3 * k + 1) % len(files)], k) for k in range(N)]


def _files(data_list, split, rank, world, **kw):
    return TileFileSource(DEV, data_list, batch_size=B, split=split, seed=SEED, rank=rank, world=world, **kw)


def _epochs(make, rank, world):
    """[(split, [(x, y)])] of EPOCHS for one rank: one train source runs both train epochs, Python's and torch's generators are
    seeded alike in front of every epoch."""
    sources, out = {}, []
    for split, seed in EPOCHS:
        if split not in sources:
            sources[split] = make(split, rank, world)
        random.seed(seed)
        torch.manual_seed(seed)
        out.append((split, [(x.clone(), y.clone()) for x, y in sources[split]]))
    for src in sources.values():
        assert len(src) == (N // B if src.split == "train" else -(-N // B))   # whole batches, whatever the world
        if hasattr(src, "close"):
            src.close()
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _check(make, whole, world):
    seen_last_val = 0
    for rank in range(world):
        got = _epochs(make, rank, world)
        for (split, want), (_, mine) in zip(whole, got):
            expect = []
            for x, y in want:
                lo, hi = train_feed.shard_bounds(x.shape[0], rank, world)
                if hi > lo:
                    expect.append((x[lo:hi], y[lo:hi]))
            assert len(mine) == len(expect), (split, rank, world)
            for k, ((x, y), (xw, yw)) in enumerate(zip(mine, expect)):
                assert x.dtype == xw.dtype and x.shape == xw.shape, (split, rank, k)
                assert torch.equal(_bits(x), _bits(xw)), (split, rank, k)
                assert torch.equal(y, yw), (split, rank, k)
            if split == "val":
                seen_last_val += len(mine) == len(want)
            else:
                assert len(mine) == len(want) and all(x.shape[0] == B // world for x, _ in mine)
    assert seen_last_val == (2 if world == 3 else world)   # the 2-row last val batch: one of three ranks gets none of it


@pytest.fixture(scope="module")
def whole_rendered():
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = _epochs(functools.partial(_rendered, **RENDERED_MODES[mode]), 0, 1)
        return cache[mode]

    return get


@pytest.fixture(scope="module")
def whole_files(data_list):
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = _epochs(functools.partial(_files, data_list, **FILE_MODES[mode]), 0, 1)
        return cache[mode]

    return get


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", list(RENDERED_MODES))
def test_rendered_source_yields_its_rows_of_the_whole_batch(whole_rendered, mode, world):
    whole = whole_rendered(mode)
    assert [len(b) for _, b in whole] == [2, 2, 3] and [x.shape[0] for x, _ in whole[2][1]] == [6, 6, 2]
    if mode == "photometric":   # (the jitter draws are live: the two train epochs differ, and differ from the plain source's)
        assert not torch.equal(whole[0][1][0][0], whole_rendered("fp32")[0][1][0][0])
    _check(functools.partial(_rendered, **RENDERED_MODES[mode]), whole, world)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", list(FILE_MODES))
def test_tile_file_source_yields_its_rows_of_the_whole_batch(whole_files, data_list, mode, world):
    whole = whole_files(mode)
    assert [len(b) for _, b in whole] == [2, 2, 3] and [x.shape[0] for x, _ in whole[2][1]] == [6, 6, 2]
    _check(functools.partial(_files, data_list, **FILE_MODES[mode]), whole, world)


def test_tile_file_loader_splits_every_batch(data_list):
    """The evaluation loader's tuples, cut the same way: tiles, labels and the two lists of names."""
    whole = list(TileFileLoader(DEV, data_list, 6, (234, 234), (224, 224)))
    assert [b[0].shape[0] for b in whole] == [6, 6, 2]
    for world in (2, 3):
        for rank in range(world):
            mine = list(TileFileLoader(DEV, data_list, 6, (234, 234), (224, 224), rank=rank, world=world))
            expect = [(b, train_feed.shard_bounds(b[0].shape[0], rank, world)) for b in whole]
            expect = [(b, lo, hi) for b, (lo, hi) in expect if hi > lo]
            assert len(mine) == len(expect)
            for got, (b, lo, hi) in zip(mine, expect):
                assert torch.equal(got[0], b[0][lo:hi]) and torch.equal(got[1], b[1][lo:hi]) and torch.equal(got[2], b[2][lo:hi])
                assert got[3] == b[3][lo:hi] and got[4] == b[4][lo:hi]


def test_refusals():
    with pytest.raises(ValueError, match="multiple"):
        train_render.RenderedTrainSource(DEV, FLOOR, batch_size=B, split="train", rank=0, world=4)
    with pytest.raises(ValueError):
        train_render.RenderedTrainSource(DEV, FLOOR, batch_size=B, split="val", rank=3, world=3)
    train_render.RenderedTrainSource(DEV, FLOOR, batch_size=B, split="val", rank=3, world=4)   # val batches split as they come
