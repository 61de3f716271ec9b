"""Host side of training from panorama sets that do not fit in device memory (salve_amd.train_render): the slot planner `PanoCache`
and its next-use bookkeeping, the memory-mapped loader, the launch bound with identity rows, the new export and status bit, and the
command line's flag refusals.  No test here needs a GPU."""

import json
import re
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from salve_amd import _lib, train, train_render  # noqa: E402
from salve_amd.train_render import NEVER, PanoCache, epoch_next_use, plan_epoch  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "salve_hip.h").read_text()
FLOOR, BOTH = ["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"]


def _epoch(P, n, batch, seed=0):
    """Uniform random pairs (i1, then i2, from one generator) in plan_epoch's shuffled order: the distinct panoramas of every batch."""
    rng = np.random.default_rng(seed)
    i1 = rng.integers(0, P, n)
    i2 = rng.integers(0, P, n)
    plan = plan_epoch(n, batch, "train", torch.Generator().manual_seed(seed))
    return [np.unique(np.concatenate([i1[idx], i2[idx]])) for idx in plan]


def _run(cache, batches, P, check=False):
    """Plan a whole epoch as RenderedTrainSource.__iter__ does; with `check`, the planner's invariants after every batch."""
    next_use, after = epoch_next_use(batches, P)
    resident = set(np.flatnonzero(cache.slot_of >= 0).tolist())
    for b, need in enumerate(batches):
        before = cache.slot_of.copy()
        slots, uploads = cache.plan(need, next_use)
        if check:
            assert np.array_equal(slots, cache.slot_of[need]) and bool((slots >= 0).all()) and bool((slots < cache.capacity).all())   # resident
            held = cache.slot_of[cache.slot_of >= 0]
            assert len(set(held.tolist())) == len(held) <= cache.capacity                                                         # no shared slot
            assert all(cache.pano_in[cache.slot_of[p]] == p for p in np.flatnonzero(cache.slot_of >= 0))
            assert sorted(p for p, _ in uploads) == sorted(int(p) for p in need if before[p] < 0)                                 # uploads == misses
            assert all(cache.slot_of[p] == s for p, s in uploads)
            evicted = set(np.flatnonzero((before >= 0) & (cache.slot_of < 0)).tolist())
            assert not evicted & set(need.tolist())                                                                               # never a victim
            if evicted and cache.policy == "furthest":   # no resident panorama outside the batch is used later than a victim
                kept = [p for p in np.flatnonzero(cache.slot_of >= 0) if p not in set(need.tolist())]
                assert not kept or min(int(next_use[p]) for p in evicted) >= max(int(next_use[p]) for p in kept)
            resident = (resident - evicted) | set(need.tolist())
            assert resident == set(np.flatnonzero(cache.slot_of >= 0).tolist())
        next_use[need] = after[b]
    return cache


# ---------------------------------------------------------------------------------------------------- 1. planner
def test_epoch_next_use_names_the_next_batch():
    batches = [np.array([0, 1]), np.array([1, 2]), np.array([0, 3]), np.array([1])]
    first, after = epoch_next_use(batches, 5)
    assert first.tolist() == [0, 0, 1, 2, NEVER]
    assert [a.tolist() for a in after] == [[2, 1], [3, NEVER], [NEVER, NEVER], [NEVER]]


@pytest.mark.parametrize("policy", ["furthest", "lru"])
@pytest.mark.parametrize("P,n,batch,slots", [(96, 1024, 32, 64), (40, 300, 8, 16), (10, 64, 8, 16)])
def test_planner_invariants_over_a_seeded_epoch(P, n, batch, slots, policy):
    batches = _epoch(P, n, batch, seed=5)
    cache = _run(PanoCache(P, slots, batch, bytes_per_pano=7, policy=policy), batches, P, check=True)
    assert cache.hits + cache.misses == sum(len(b) for b in batches)
    assert cache.uploaded_bytes == 7 * cache.misses and cache.misses >= len(np.unique(np.concatenate(batches)))
    if slots >= P:   # everything fits: each panorama is uploaded once
        assert cache.misses == len(np.unique(np.concatenate(batches))) and cache.capacity == P
    again = _run(cache, batches, P, check=True)   # a second epoch on the warm cache keeps the invariants
    assert again.hits + again.misses == 2 * sum(len(b) for b in batches)


def test_victim_is_the_furthest_next_use_then_the_lower_id():
    c = PanoCache(8, 4, 2)
    c.plan([0, 1, 2, 3])
    nu = np.full(8, NEVER, dtype=np.int64)
    nu[[0, 1, 2, 3]] = [5, 9, 9, 2]
    slots, up = c.plan([4], nu)          # 1 and 2 tie at 9: the lower id goes
    assert [p for p, _ in up] == [4] and c.slot_of[1] == -1 and c.slot_of[2] >= 0
    nu[4] = 1
    c.plan([5, 6], nu)                   # 2 (9) and 0 (5) go; 3 (2) and 4 (1) stay
    assert c.slot_of[[0, 2]].tolist() == [-1, -1] and bool((c.slot_of[[3, 4, 5, 6]] >= 0).all())
    c.plan([7, 3, 4, 5])                 # no next_use: all "never", the lower id (6 is the only candidate)
    assert c.slot_of[6] == -1
    lru = PanoCache(8, 4, 2, policy="lru")
    lru.plan([0, 1]); lru.plan([2, 3]); lru.plan([0])
    lru.plan([4])
    assert lru.slot_of[1] == -1 and lru.slot_of[0] >= 0


def test_capacity_below_one_batch_is_refused():
    with pytest.raises(ValueError, match=r"cannot hold one batch.*at least 64"):
        PanoCache(96, 63, 32)
    with pytest.raises(ValueError, match="at least 10"):
        PanoCache(10, 9, 32)              # all of P is the smaller bound
    assert PanoCache(10, 10, 32).capacity == 10 and PanoCache(10, 500, 32).capacity == 10
    PanoCache(96, 64, 32)
    with pytest.raises(ValueError, match="policy"):
        PanoCache(96, 64, 32, policy="mru")
    with pytest.raises(ValueError, match="names panorama 96"):
        PanoCache(96, 64, 32).plan([3, 96])
    with pytest.raises(ValueError, match="65 panoramas"):
        PanoCache(96, 64, 32).plan(np.arange(65))


@pytest.mark.parametrize("P,n,batch,slots", [(96, 1024, 32, 64), (96, 1024, 32, 80), (200, 4096, 64, 128)])
def test_furthest_next_use_uploads_no_more_than_lru(P, n, batch, slots):
    batches = _epoch(P, n, batch, seed=0)
    lru = _run(PanoCache(P, slots, batch, policy="lru"), batches, P).misses
    far = _run(PanoCache(P, slots, batch, policy="furthest"), batches, P).misses
    print(f"P {P}, {n} examples, batch {batch}, {slots} slots: LRU {lru} uploads, furthest-next-use {far} uploads")
    assert far <= lru


# ---------------------------------------------------------------------------------------------------- 2. loader, launch bound, library
def _render_dir(root, rgb_dtype=np.uint8, depth_shape=(3, 8, 16)):
    np.save(root / "panos_rgb.npy", np.arange(3 * 8 * 16 * 3).reshape(3, 8, 16, 3).astype(rgb_dtype))
    np.save(root / "panos_depth.npy", np.arange(int(np.prod(depth_shape))).reshape(depth_shape).astype(np.uint16))
    for split in ("train", "val"):
        (root / f"{split}.json").write_text(json.dumps({"i1": [0, 1], "i2": [1, 2], "R": [[[1, 0], [0, 1]]] * 2, "t": [[0, 0]] * 2, "is_match": [0, 1]}))


def test_load_render_dir_mmap_returns_memmaps_and_keeps_its_refusals(tmp_path):
    _render_dir(tmp_path)
    rgb, depth, ex = train_render.load_render_dir(str(tmp_path), mmap=True)
    assert isinstance(rgb, np.memmap) and isinstance(depth, np.memmap) and not rgb.flags.writeable
    plain_rgb, plain_depth, _ = train_render.load_render_dir(str(tmp_path))
    assert not isinstance(plain_rgb, np.memmap) and np.array_equal(plain_rgb, rgb) and np.array_equal(plain_depth, depth)
    assert len(ex["train"][0]) == 2 and ex["val"][1].tolist() == [0, 1]
    (tmp_path / "val.json").unlink()
    with pytest.raises(SystemExit, match="val.json is missing"):
        train_render.load_render_dir(str(tmp_path), mmap=True)
    _render_dir(tmp_path, rgb_dtype=np.uint16)
    with pytest.raises(SystemExit, match="must be uint8"):
        train_render.load_render_dir(str(tmp_path), mmap=True)
    _render_dir(tmp_path, depth_shape=(3, 8, 15))
    with pytest.raises(SystemExit, match="must be uint8"):
        train_render.load_render_dir(str(tmp_path), mmap=True)


def test_check_launch_counts_the_identity_rows():
    train_render.check_launch(256, 2, 256)
    train_render.check_launch(32767, 1, 32768)
    train_render.check_launch(16383, 2, 16384)
    with pytest.raises(RuntimeError, match="65535"):
        train_render.check_launch(32768, 1, 32768)
    with pytest.raises(RuntimeError, match="65536 renders"):
        train_render.check_launch(16384, 2, 16384)
    with pytest.raises(ValueError):
        train_render.check_launch(8, 1, -1)
    train_render.check_launch(32767, 2)     # the default stays what it was
    # the source refuses at construction, before it touches a device: identity="batch" doubles the worst case
    with pytest.raises(RuntimeError, match="65535"):
        train_render.RenderedTrainSource("cuda:0", BOTH, batch_size=16384, identity="batch")
    with pytest.raises(ValueError, match="identity must be one of"):
        train_render.RenderedTrainSource("cuda:0", FLOOR, identity="fresh")
    with pytest.raises(ValueError, match='resident_panos needs identity="batch"'):
        train_render.RenderedTrainSource("cuda:0", FLOOR, resident_panos=64)
    with pytest.raises(ValueError, match="must be positive"):
        train_render.RenderedTrainSource("cuda:0", FLOOR, identity="batch", resident_panos=0)


def test_library_exports_the_index_update_and_its_status_bit():
    lib = _lib.load()
    assert hasattr(lib, "salve_bev_pano_index_update") and "salve_bev_pano_index_update" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bint salve_bev_pano_index_update\(", HEADER)
    assert int(re.search(r"#define SALVE_STATUS_BAD_PANO_SLOT (\d+)", HEADER).group(1)) == _lib.STATUS_BAD_PANO_SLOT == 2 * _lib.STATUS_BAD_TILE_JOB
    assert lib.salve_hip_version() == 7 == _lib.EXPECTED_ABI
    with pytest.raises(_lib.SalveHipError, match="slot outside the resident pool"):
        _lib.check_status_word(_lib.STATUS_BAD_PANO_SLOT, "an epoch")


# ---------------------------------------------------------------------------------------------------- 3. command line
@pytest.mark.parametrize("flags,message", [
    (["--render-from", "D", "--resident-panos", "64", "--identity", "kept"], "cannot be combined with --identity kept"),
    (["--render-from", "D", "--resident-panos", "0"], "must be positive"),
    (["--resident-panos", "64"], "belong to --render-from"),
    (["--identity", "batch"], "belong to --render-from"),
])
def test_cli_refuses_flag_combinations_before_anything_is_loaded(flags, message):
    with pytest.raises(SystemExit, match=message):   # (the config does not exist: the refusal comes first)
        train.main(["--config", "/nonexistent/config.yaml"] + flags)


def test_cli_refuses_an_unknown_identity(capsys):
    with pytest.raises(SystemExit):
        train.main(["--config", "/nonexistent/config.yaml", "--render-from", "D", "--identity", "fresh"])
    assert "invalid choice: 'fresh'" in capsys.readouterr().err
