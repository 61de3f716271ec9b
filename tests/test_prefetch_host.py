"""Host side of the resident pool's prefetch (salve_amd.train_render): `PanoCache.plan(keep=)` -- the planner that looks
one batch ahead while the batch before is still in flight --, the larger pool it needs, what a failed upload takes back, and the
refusals of the source and of the command line.  No test here needs a GPU."""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from salve_amd import train, train_render  # noqa: E402
from salve_amd.train_render import PanoCache, epoch_next_use, plan_epoch  # noqa: E402

FLOOR = ["floor_rgb_texture"]
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "pano_cache_plans.json").read_text())
SEEDED = [(96, 1024, 32, 64), (40, 300, 8, 16), (10, 64, 8, 16), (96, 1024, 32, 80), (200, 4096, 64, 128)]   # test_pano_cache_host.py's (P, n, batch, slots)


def _epoch(P, n, batch, seed=0):
    """test_pano_cache_host.py's sequences: uniform random pairs in plan_epoch's shuffled order, the distinct panoramas of every batch."""
    rng = np.random.default_rng(seed)
    i1 = rng.integers(0, P, n)
    i2 = rng.integers(0, P, n)
    plan = plan_epoch(n, batch, "train", torch.Generator().manual_seed(seed))
    return [np.unique(np.concatenate([i1[idx], i2[idx]])) for idx in plan]


def _serial(cache, batches, P, **kw):
    """The serial walk of RenderedTrainSource.__iter__: [(slots, uploads)] per batch."""
    next_use, after = epoch_next_use(batches, P)
    out = []
    for b, need in enumerate(batches):
        slots, uploads = cache.plan(need, next_use, **kw)
        out.append((slots.tolist(), uploads))
        next_use[need] = after[b]
    return out


def _ahead(cache, batches, P, check=False):
    """The walk of the prefetching iterator: batch 0 planned alone, batch b + 1 planned with keep = batch b's panoramas once batch b's
    next uses are entered.  With `check`, the invariants after every plan.  Returns the uploads per batch."""
    next_use, after = epoch_next_use(batches, P)
    per = []
    for b, need in enumerate(batches):
        keep = batches[b - 1] if b else None
        before = cache.slot_of.copy()
        slots, uploads = cache.plan(need, next_use, keep=keep)
        per.append(len(uploads))
        if check:
            evicted = set(np.flatnonzero((before >= 0) & (cache.slot_of < 0)).tolist())
            assert not evicted & set(need.tolist()), b                                   # no victim in the batch
            assert keep is None or not evicted & set(keep.tolist()), b                   # ... nor in keep
            assert keep is None or bool((cache.slot_of[keep] == before[keep]).all()), b  # the batch in flight keeps its slots
            held = cache.slot_of[cache.slot_of >= 0]
            assert len(set(held.tolist())) == len(held) <= cache.capacity, b             # no shared slot
            assert all(cache.pano_in[cache.slot_of[p]] == p for p in np.flatnonzero(cache.slot_of >= 0)), b
            assert sorted(p for p, _ in uploads) == sorted(int(p) for p in need if before[p] < 0), b   # uploads == misses
            assert np.array_equal(slots, cache.slot_of[need]) and bool((slots >= 0).all()), b           # every entry resident
            assert np.array_equal(cache.lookup(need), slots), b
            if evicted:   # ranking unchanged: no resident panorama outside the batch and keep is used later than a victim
                pinned = set(need.tolist()) | (set(keep.tolist()) if keep is not None else set())
                others = [p for p in np.flatnonzero(cache.slot_of >= 0) if p not in pinned]
                assert not others or min(int(next_use[p]) for p in evicted) >= max(int(next_use[p]) for p in others), b
        next_use[need] = after[b]
    return per


# ---------------------------------------------------------------------------------------------------- 1. planner
@pytest.mark.parametrize("keep", ["default", "none"])
@pytest.mark.parametrize("policy", ["furthest", "lru"])
@pytest.mark.parametrize("P,n,batch,slots", SEEDED)
def test_keep_none_is_the_plan_of_the_planner_before_keep(P, n, batch, slots, policy, keep):
    """Slots and uploads, batch for batch, over two epochs on one cache, against tests/golden/pano_cache_plans.json: the plans RECORDED from
    the planner as it was before `plan` took `keep` (the commit before this feature, run over these very sequences) -- a SHA-256 over every
    batch's slot vector and (panorama, slot) upload list as int64, the uploads per batch, the final counters and the final slot table.
    The reference is a record, not this code: with `keep` left out and with `keep=None` the planner must reproduce it exactly."""
    kw = {} if keep == "default" else {"keep": None}
    for seed in (0, 5):
        want = GOLDEN[f"P{P}-n{n}-b{batch}-s{slots}-{policy}-seed{seed}"]
        batches = _epoch(P, n, batch, seed=seed)
        cache = PanoCache(P, slots, batch, bytes_per_pano=7, policy=policy)
        digest, counts = hashlib.sha256(), []
        for _ in range(2):
            next_use, after = epoch_next_use(batches, P)
            for b, need in enumerate(batches):
                got_slots, uploads = cache.plan(need, next_use, **kw)
                digest.update(np.asarray(got_slots, dtype=np.int64).tobytes())
                digest.update(np.asarray(uploads, dtype=np.int64).reshape(-1, 2).tobytes())
                counts.append(len(uploads))
                next_use[need] = after[b]
        assert counts == want["uploads"], seed
        assert (cache.hits, cache.misses, cache.uploaded_bytes) == (want["hits"], want["misses"], want["uploaded_bytes"]), seed
        assert cache.slot_of.tolist() == want["slot_of"], seed
        assert digest.hexdigest() == want["sha256"], seed


@pytest.mark.parametrize("where", ["4B", "between", "P"])
@pytest.mark.parametrize("P,n,batch", [(96, 1024, 8, ), (40, 300, 4), (200, 2048, 16), (10, 64, 8)])
def test_look_ahead_invariants_over_seeded_epochs(P, n, batch, where):
    """Capacity exactly min(4B, P), exactly P, and half way: no victim in keep or in the batch, no shared slot, uploads == misses, every
    entry resident -- over two epochs on one cache (the second starts warm, with nothing kept for its first batch)."""
    least = min(4 * batch, P)
    capacity = {"4B": least, "P": P, "between": (least + P) // 2}[where]
    for seed in (1, 2, 3):
        batches = _epoch(P, n, batch, seed=seed)
        cache = PanoCache(P, capacity, batch, bytes_per_pano=3, prefetch=True)
        total = sum(_ahead(cache, batches, P, check=True)) + sum(_ahead(cache, batches, P, check=True))
        assert cache.misses == total and cache.uploaded_bytes == 3 * total
        assert cache.hits + cache.misses == 2 * sum(len(b) for b in batches)
        if capacity == P:
            assert total == len(np.unique(np.concatenate(batches)))   # everything fits: each panorama goes up once


def test_too_few_victims_outside_keep_is_an_error_not_an_eviction():
    c = PanoCache(12, 6, 3)                 # (no prefetch: 6 slots are accepted)
    c.plan([0, 1, 2, 3, 4, 5])
    before = (c.slot_of.copy(), c.pano_in.copy(), c.hits, c.misses, c.clock)
    with pytest.raises(ValueError, match=r"misses 3 panoramas, but only 2 of the pool's 6 slots.*no kept panorama is evicted"):
        c.plan([6, 7, 8], keep=[0, 1, 2, 3])
    assert np.array_equal(c.slot_of, before[0]) and np.array_equal(c.pano_in, before[1]) and (c.hits, c.misses, c.clock) == before[2:]   # nothing changed
    slots, up = c.plan([6, 7, 3], keep=[0, 1, 2, 3])       # two victims are there: 4 and 5
    assert sorted(p for p, _ in up) == [6, 7] and c.slot_of[[4, 5]].tolist() == [-1, -1] and bool((c.slot_of[[0, 1, 2, 3]] >= 0).all())
    with pytest.raises(ValueError, match="keep names panorama 12"):
        c.plan([0], keep=[12])
    with pytest.raises(ValueError, match="not resident"):
        c.lookup([4])


def test_pool_below_two_batches_is_refused_with_prefetch_only():
    with pytest.raises(ValueError, match=r"cannot hold two batches.*at least 128"):
        PanoCache(200, 127, 32, prefetch=True)
    assert PanoCache(200, 127, 32).capacity == 127                      # the same pool without prefetch
    assert PanoCache(200, 128, 32, prefetch=True).capacity == 128
    with pytest.raises(ValueError, match="at least 100"):
        PanoCache(100, 99, 32, prefetch=True)                           # all of P is the smaller bound
    assert PanoCache(100, 100, 32, prefetch=True).capacity == 100 and PanoCache(100, 99, 32).capacity == 99
    with pytest.raises(ValueError, match="cannot hold one batch"):      # below one batch: the old refusal without prefetch
        PanoCache(200, 63, 32)


def test_forget_takes_back_exactly_the_uploads_that_did_not_happen():
    c = PanoCache(20, 8, 2, bytes_per_pano=5, prefetch=True)
    c.plan([0, 1, 2, 3, 4, 5, 6, 7])
    nu = np.arange(20, dtype=np.int64)
    before = (c.hits, c.clock, c.last_used.copy())
    _, up = c.plan([8, 9, 0], nu, keep=[1, 2])
    assert len(up) == 2 and c.misses == 10 and c.hits == before[0] + 1
    victims = [p for p in range(8) if c.slot_of[p] < 0]
    c.forget(up)
    assert c.misses == 8 and c.uploaded_bytes == 40
    assert (c.hits, c.clock) == before[:2] and np.array_equal(c.last_used, before[2]) and c.hits + c.misses == 8   # hits + misses: the plans that stand
    with pytest.raises(ValueError, match="most recent plan only"):
        c.forget(up)
    assert c.slot_of[[8, 9]].tolist() == [-1, -1] and sorted(np.flatnonzero(c.pano_in < 0).tolist()) == sorted(sl for _, sl in up)
    assert all(c.slot_of[p] < 0 for p in victims)                       # the victims stay evicted: their slots are free
    _, again = c.plan([8, 9, 0], nu, keep=[1, 2])                        # ... and are the first to be filled again
    assert sorted(again) == sorted(up)


@pytest.mark.parametrize("P,n,batch,slots", [(96, 1024, 8, 32), (96, 1024, 8, 48), (200, 4096, 16, 64), (200, 4096, 16, 128), (40, 300, 4, 16)])
def test_look_ahead_uploads_no_more_than_lru(P, n, batch, slots):
    """Three epochs on one cache.  The look-ahead planner pins one more batch than the serial one, so it may upload more than the serial
    "furthest" planner; it must not give away the whole advantage over LRU.  The figures are recorded in DESIGN.md 4.14."""
    tot = {"ahead": 0, "furthest": 0, "lru": 0}
    caches = {"ahead": PanoCache(P, slots, batch, prefetch=True), "furthest": PanoCache(P, slots, batch), "lru": PanoCache(P, slots, batch, policy="lru")}
    for seed in (0, 1, 2):
        batches = _epoch(P, n, batch, seed=seed)
        tot["ahead"] += sum(_ahead(caches["ahead"], batches, P))
        tot["furthest"] += sum(len(u) for _, u in _serial(caches["furthest"], batches, P))
        tot["lru"] += sum(len(u) for _, u in _serial(caches["lru"], batches, P))
    print(f"P {P}, 3 x {n} examples, batch {batch}, {slots} slots: look-ahead {tot['ahead']} uploads, serial furthest-next-use {tot['furthest']}, LRU {tot['lru']}")
    assert tot["ahead"] <= tot["lru"]


# ---------------------------------------------------------------------------------------------------- 2. source and command line
def test_source_refuses_prefetch_without_a_pool_and_too_many_threads():
    with pytest.raises(ValueError, match="prefetch needs resident_panos"):
        train_render.RenderedTrainSource("cuda:0", FLOOR, prefetch=True)
    with pytest.raises(ValueError, match="prefetch needs resident_panos"):
        train_render.RenderedTrainSource("cuda:0", FLOOR, identity="batch", prefetch=True)
    for bad in (0, 9, 64):
        with pytest.raises(ValueError, match=r"gather_threads must be 1 \.\. 8"):
            train_render.RenderedTrainSource("cuda:0", FLOOR, identity="batch", resident_panos=64, prefetch=True, gather_threads=bad)
    assert train_render.MAX_GATHER_THREADS == 8


@pytest.mark.parametrize("flags,message", [
    (["--render-from", "D", "--prefetch"], "--prefetch belongs to --resident-panos"),
    (["--prefetch"], "--prefetch belongs to --resident-panos"),
    (["--render-from", "D", "--prefetch", "--identity", "kept"], "--prefetch .* cannot be combined with --identity kept"),
    (["--render-from", "D", "--resident-panos", "64", "--prefetch", "--identity", "kept"], "cannot be combined with --identity kept"),
])
def test_cli_refuses_prefetch_without_a_pool(flags, message):
    with pytest.raises(SystemExit, match=message):   # (the config does not exist: the refusal comes first)
        train.main(["--config", "/nonexistent/config.yaml"] + flags)
