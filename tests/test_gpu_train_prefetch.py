"""The resident pool's prefetch on the MI355X (salve_amd.train_render): the next batch's misses are gathered by worker
threads and uploaded on the pool's copy stream while the current batch is in flight.  40 panoramas, a pool of 16 slots, batches of 4
(4 x batch = 16: the smallest pool prefetch accepts), so every batch evicts.  Every comparison is exact: the batches are those of the
default, all-resident source."""

import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import status, synthetic, synthetic_layouts, train_render, training  # noqa: E402
from salve_amd.training_config import TrainingConfig  # noqa: E402

DEV = torch.device("cuda:0")
FLOOR, BOTH = ["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"]
ALL3 = BOTH + ["layout"]
P, POOL, B, N, NVAL, SEED = 40, 16, 4, 24, 10, 3


@functools.lru_cache(maxsize=None)
def _panos():
    panos = synthetic.make_panos(P, scene="box")
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])


def _table(n, seed):
    hyp = synthetic.make_hypotheses(n, P, seed=seed)
    hyp.swap = (np.arange(n) % 3 == 1)
    return hyp, np.arange(n, dtype=np.int64)   # (the label IS the example's index: the order shows in the labels)


def _source(mods, precision, split, **kw):
    if "layout" in mods:
        kw["layouts"] = synthetic_layouts.make_layouts(P, seed=9)
    return train_render.RenderedTrainSource(DEV, mods, batch_size=B, precision=precision, split=split, seed=SEED, **kw)


def _pair(mods, precision, rgb=None, depth=None, **kw):
    """(train source, val source sharing its panoramas) over the same two example tables."""
    tr = _source(mods, precision, "train", **kw)
    tr.load_panos(*(_panos() if rgb is None else (rgb, depth)))
    tr.set_examples(*_table(N, 6))
    va = _source(mods, precision, "val", **kw)
    va.share_panos(tr)
    va.set_examples(*_table(NVAL, 7))
    return tr, va


def _epoch(src, py_seed, stop=None):
    """The (cloned) batches of one epoch; `stop`: only the first `stop`, then the iterator is closed."""
    random.seed(py_seed)
    it = iter(src)
    out = []
    for x, y in it:
        out.append((x.clone(), y.clone()))
        if len(out) == stop:
            break
    it.close()
    return out


def _same(got, want):
    assert len(got) == len(want) > 0
    for k, ((x, y), (xw, yw)) in enumerate(zip(got, want)):
        assert x.dtype == xw.dtype and x.shape == xw.shape, k
        bits = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.view(bits), xw.view(bits)), k
        assert torch.equal(y, yw), k


def _predicted_uploads(schedule):
    """The look-ahead planner alone over the epochs the sources run -- [(split, batches rendered or None for all)] -- on one shared cache,
    the train shuffle from ONE generator: batch 0 of an epoch planned alone, batch b + 1 planned with keep = batch b behind every rendered batch."""
    cache = train_render.PanoCache(P, POOL, B, prefetch=True)
    gen = torch.Generator().manual_seed(SEED)
    per = []
    for split, stop in schedule:
        hyp = _table(N if split == "train" else NVAL, 6 if split == "train" else 7)[0]
        plan = train_render.plan_epoch(len(hyp), B, split, gen if split == "train" else None)
        panos = [np.unique(np.concatenate([hyp.i1[idx], hyp.i2[idx]])) for idx in plan]
        next_use, after = train_render.epoch_next_use(panos, P)
        n_planned = len(panos) if stop is None else min(stop + 1, len(panos))
        for b in range(n_planned):
            per.append(len(cache.plan(panos[b], next_use, keep=panos[b - 1] if b else None)[1]))
            next_use[panos[b]] = after[b]
    return per


def _check_counts(tr, va, schedule, builds, every_batch=True):
    per = _predicted_uploads(schedule)
    print(f"uploads per planned batch (look-ahead planner): {per}; source: {tr.uploads} uploads, {tr.cache.hits} hits, {tr.cache.misses} misses")
    assert sum(per) > P and (not every_batch or all(m > 0 for m in per))   # every batch misses, every batch behind the first two evicts
    assert tr.uploads == va.uploads == tr.cache.misses == sum(per)
    assert tr.cache.uploaded_bytes == tr.uploads * 512 * 1024 * 5
    assert (tr.ras.index_builds, va.ras.index_builds) == builds              # no full rebuild of the pool's index behind load_panos
    assert tr.pool.pending is None and tr.pool.stream.query()        # nothing left in flight
    status.check(DEV, "the prefetched epochs")


SCHEDULE = [("train", 11), ("val", 12), ("train", 13)]


@pytest.mark.parametrize("mods,precision", [(FLOOR, "fp32"), (FLOOR, "bf16"), (BOTH, "fp32"), (BOTH, "bf16"), (ALL3, "bf16")],
                         ids=["floor-fp32", "floor-bf16", "ceiling+floor-fp32", "ceiling+floor-bf16", "ceiling+floor+layout-bf16"])
def test_prefetched_pool_equals_the_default_source(mods, precision):
    """Two train epochs with a val epoch between them on the shared pool: every batch -- rendered while the copy stream writes the NEXT
    batch's slots -- and its labels equal the default all-resident source's; the uploads are the look-ahead planner's misses."""
    tr, va = _pair(mods, precision, identity="batch", resident_panos=POOL, prefetch=True)
    assert tr.uploads == 0 and tuple(tr.pano_rgb.shape) == (POOL, 512, 1024, 3) and va.pool is tr.pool and va.pool.stream is tr.pool.stream
    builds = (tr.ras.index_builds, va.ras.index_builds)
    assert builds == (1, 0)
    ref, vref = _pair(mods, precision)
    for split, py_seed in SCHEDULE:
        want = _epoch(ref if split == "train" else vref, py_seed)
        got = _epoch(tr if split == "train" else va, py_seed)
        assert len(got) == (N // B if split == "train" else (NVAL + B - 1) // B)
        _same(got, want)
    _check_counts(tr, va, [(s, None) for s, _ in SCHEDULE], builds)


def test_iterator_closed_or_dropped_mid_epoch_leaves_the_pool_usable():
    """Two batches, then close: the upload of batch 2 that was already started is completed and counted, nothing stays in flight, and a full
    val epoch and a full train epoch on the same pool equal the default source's.  The same with the iterator merely dropped."""
    tr, va = _pair(BOTH, "bf16", identity="batch", resident_panos=POOL, prefetch=True)
    builds = (tr.ras.index_builds, va.ras.index_builds)
    ref, vref = _pair(BOTH, "bf16")
    _same(_epoch(tr, 21, stop=2), _epoch(ref, 21, stop=2))
    assert tr.pool.pending is None and tr.pool.stream.query()
    held = tr.cache.slot_of[tr.cache.slot_of >= 0]
    assert len(set(held.tolist())) == len(held) and tr.uploads == tr.cache.misses
    _same(_epoch(va, 22), _epoch(vref, 22))
    _same(_epoch(tr, 23), _epoch(ref, 23))
    schedule = [("train", 2), ("val", None), ("train", None)]
    _check_counts(tr, va, schedule, builds, every_batch=False)
    # dropped, not closed: the generator's finaliser does the same
    random.seed(24)
    it = iter(tr)
    got = [tuple(t.clone() for t in next(it))]
    del it
    assert tr.pool.pending is None and tr.pool.stream.query()
    _same(got, _epoch(ref, 24, stop=1))
    _same(_epoch(va, 25), _epoch(vref, 25))
    _check_counts(tr, va, schedule + [("train", 1), ("val", None)], builds, every_batch=False)


def test_a_suspended_iterator_refuses_to_go_on_after_another_iteration_on_the_pool():
    """One batch of a train epoch, then a whole val epoch on the shared pool without closing the first iterator: the val iteration first
    completes the upload the suspended one had started (counted, nothing in flight), its batches are exact; the suspended iterator then
    refuses its next batch in one line instead of planning beside the pool's new owner, and the pool serves later epochs exactly."""
    tr, va = _pair(FLOOR, "bf16", identity="batch", resident_panos=POOL, prefetch=True)
    ref, vref = _pair(FLOOR, "bf16")
    random.seed(41)
    it = iter(tr)
    got = [tuple(t.clone() for t in next(it))]
    assert tr.pool.pending is not None
    _same(got, _epoch(ref, 41, stop=1))
    _same(_epoch(va, 42), _epoch(vref, 42))
    assert tr.pool.pending is None and tr.uploads == tr.cache.misses
    with pytest.raises(RuntimeError, match="one iteration at a time"):
        next(it)
    assert tr.pool.pending is None and tr.pool.stream.query() and tr.uploads == tr.cache.misses
    _same(_epoch(tr, 43), _epoch(ref, 43))
    _check_counts(tr, va, [("train", 1), ("val", None), ("train", None)], (1, 0), every_batch=False)


class _FailingReads:
    """A host array whose panorama `bad` cannot be read while `armed` (a memory-mapped file on a failing disk)."""

    def __init__(self, arr, bad):
        self.arr, self.bad, self.armed = arr, bad, True
        self.shape, self.dtype, self.nbytes = arr.shape, arr.dtype, arr.nbytes

    def __len__(self):
        return len(self.arr)

    def __getitem__(self, p):
        if self.armed and int(p) == self.bad:
            raise OSError(f"panorama {int(p)} cannot be read (injected)")
        return self.arr[p]


def test_a_worker_exception_reaches_the_loop_and_the_source_stays_usable():
    """The read of one panorama that batch 1 misses fails in a gather thread: the loop gets the exception with its message where it asks for
    batch 1; the planner's state is taken back to what was uploaded, nothing faults on the device, and the next epochs are the default source's."""
    hyp = _table(N, 6)[0]
    plan = train_render.plan_epoch(N, B, "train", torch.Generator().manual_seed(SEED))
    first, second = (set(np.concatenate([hyp.i1[idx], hyp.i2[idx]]).tolist()) for idx in plan[:2])
    bad = min(second - first)   # a miss of batch 1 on the cold pool: uploaded by the prefetch, not by batch 0
    rgb, depth = _panos()
    reads = _FailingReads(depth, bad)
    tr, va = _pair(FLOOR, "fp32", rgb=rgb, depth=reads, identity="batch", resident_panos=POOL, prefetch=True, gather_threads=3)
    ref, vref = _pair(FLOOR, "fp32")
    random.seed(31)
    it = iter(tr)
    got = [tuple(t.clone() for t in next(it))]
    with pytest.raises(OSError, match=rf"panorama {bad} cannot be read \(injected\)"):
        next(it)
    with pytest.raises(StopIteration):
        next(it)
    _same(got, _epoch(ref, 31, stop=1))
    cache = tr.cache
    assert tr.pool.pending is None and tr.pool.stream.query()
    assert cache.slot_of[bad] == -1 and tr.uploads == cache.misses == int((cache.slot_of >= 0).sum()) == len(first)   # batch 0's uploads alone
    assert all(cache.pano_in[cache.slot_of[p]] == p for p in np.flatnonzero(cache.slot_of >= 0))
    assert cache.hits == 0 and cache.hits + cache.misses == len(first)   # the failed plan's hits are taken back with its misses
    status.check(DEV, "after the failed upload")
    reads.armed = False
    _same(_epoch(va, 32), _epoch(vref, 32))
    _same(_epoch(tr, 33), _epoch(ref, 33))
    assert tr.uploads == cache.misses and tr.ras.index_builds == 1
    status.check(DEV, "the epochs after the failed upload")


def test_pool_and_sharing_refusals_with_prefetch():
    rgb, depth = _panos()
    small = _source(FLOOR, "fp32", "train", identity="batch", resident_panos=POOL - 1, prefetch=True)
    with pytest.raises(RuntimeError, match="cannot hold two batches.*at least 16"):
        small.load_panos(rgb, depth)
    plain = _source(FLOOR, "fp32", "train", identity="batch", resident_panos=POOL - 1)   # the same pool without prefetch
    plain.load_panos(rgb, depth)
    with pytest.raises(RuntimeError, match="same prefetch"):
        _source(FLOOR, "fp32", "val", identity="batch", resident_panos=POOL - 1, prefetch=True).share_panos(plain)


def _config():
    return TrainingConfig(lr_annealing_strategy="poly", base_lr=1e-3, weight_decay=1e-4, num_ce_classes=2, print_every=10 ** 9, poly_lr_power=0.9,
                          optimizer_algo="adam", num_layers=18, pretrained=False, dataparallel=False, resize_h=234, resize_w=234, train_h=224,
                          train_w=224, apply_photometric_augmentation=False, modalities=tuple(FLOOR), cfg_stem="prefetch", num_epochs=1, workers=0,
                          batch_size=B, data_root="", layout_data_root="", model_save_dirpath="")


def test_resnet18_epoch_fed_with_prefetch_equals_one_fed_by_the_plain_pool():
    """ResNet-18, bf16 + hip norm, fixed seed: one training.run_epoch fed by the prefetching pool -- the step's kernels running beside the copy
    stream's uploads -- gives the loss of the pool without prefetch exactly (the training path is deterministic for equal batches: DESIGN.md 4.11)."""
    rgb, depth = _panos()
    hyp, _ = _table(32, 8)
    hyp.swap = None
    labels = np.arange(32, dtype=np.int64) % 2
    args = _config()

    def run(**kw):
        src = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=B, precision="bf16", split="train", seed=0, identity="batch", resident_panos=POOL, **kw)
        src.load_panos(rgb, depth)
        src.set_examples(hyp, labels)
        random.seed(0)
        torch.manual_seed(0)
        model = training.get_model(args, "bf16", "hip")
        opt = training.get_optimizer(args, model)
        res = training.run_epoch(args, 0, model, src, opt, "train")
        return res["avg_loss"], res["mAcc"], src

    loss_a, acc_a, plain = run()
    loss_b, acc_b, ahead = run(prefetch=True)
    print(f"pool: loss {loss_a!r}, mAcc {acc_a}, {plain.uploads} uploads; pool + prefetch: loss {loss_b!r}, mAcc {acc_b}, {ahead.uploads} uploads")
    assert np.isfinite(loss_a) and loss_b == loss_a and acc_b == acc_a
    assert ahead.uploads == ahead.cache.misses > POOL and ahead.ras.index_builds == 1
    status.check(DEV, "the prefetch-fed epoch")
