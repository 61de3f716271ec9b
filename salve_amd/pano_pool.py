"""The resident panorama pool of the rendered training feed (salve_amd.train_render).

  PanoCache   which panorama lives in which slot: the planner, pure host code.
  PanoPool    the pool itself: the host arrays, the `PanoCache`, the slot tensors on the device with their panorama index, two pinned
              staging buffers, and -- with prefetch -- a copy stream and the upload job in flight.  `RenderedTrainSource.load_panos`
              builds it, `share_panos` hands the one object to a second source.

A batch's misses go up by ONE routine (`PanoPool._upload`): the rows gathered into a staging buffer, one host-to-device copy per array,
the slot list, `BevRasteriser.update_panos`.  `make_resident` runs it on the current stream; `plan_ahead` runs it one batch ahead, in
a worker thread, on the pool's copy stream.  `PanoCache` and `epoch_next_use` need no device.
"""

from __future__ import annotations

import time
from concurrent.futures import Future, ThreadPoolExecutor
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import tracing

MAX_GATHER_THREADS = 8   # prefetch: host threads that gather a batch's missed rows (a fixed small number, never the machine's CPU count)
NEVER = np.iinfo(np.int64).max   # next use of a panorama the rest of the epoch does not name


def epoch_next_use(batch_panos: Sequence[np.ndarray], n_panos: int) -> Tuple[np.ndarray, List[np.ndarray]]:
    """The next-use bookkeeping of one epoch whose batches name the DISTINCT panoramas `batch_panos[b]`: (`first`, `after`).
    first[p] is the first batch that names panorama p (NEVER if none does), after[b][k] the next batch behind b that names
    batch_panos[b][k] again.  A caller that walks the epoch keeps `next_use = first.copy()` and sets
    `next_use[batch_panos[b]] = after[b]` once batch b is planned: next_use[p] is then, for every panorama batch b + 1 does not
    name, the batch of its next use -- what `PanoCache.plan` ranks its victims by."""
    nxt = np.full(n_panos, NEVER, dtype=np.int64)
    after: List[np.ndarray] = [np.empty(0, dtype=np.int64)] * len(batch_panos)
    for b in range(len(batch_panos) - 1, -1, -1):
        after[b] = nxt[batch_panos[b]].copy()
        nxt[batch_panos[b]] = b
    return nxt, after


class PanoCache:
    """Which panorama lives in which slot of a resident pool of `capacity` slots (pure host code).  `plan` makes one batch's
    panoramas resident: no two panoramas share a slot, a panorama of the current batch is never the victim, the uploads are exactly
    the misses.  policy "furthest" (the product's): the victim is the resident panorama whose next use lies furthest ahead (one
    without further use counts as never), ties broken by the lower panorama id -- the epoch's order is known before its first batch.
    policy "lru" (kept for the test that compares the two): the least recently planned panorama.  Counters: hits, misses,
    uploaded_bytes (misses x bytes_per_pano)."""

    def __init__(self, n_panos: int, capacity: int, batch_size: int, bytes_per_pano: int = 0, policy: str = "furthest", prefetch: bool = False) -> None:
        if policy not in ("furthest", "lru"):
            raise ValueError(f"policy must be 'furthest' or 'lru', got {policy!r}")
        if n_panos <= 0 or batch_size <= 0:
            raise ValueError(f"n_panos and batch_size must be positive, got {n_panos} and {batch_size}")
        need = min(2 * batch_size, n_panos)
        if prefetch and capacity < min(4 * batch_size, n_panos):
            # the batch in flight and the batch being uploaded are pinned at once, up to 2 x batch_size panoramas each
            raise ValueError(f"a pool of {capacity} panorama slots cannot hold two batches: with prefetch the batch in flight and the next one are "
                             f"pinned at once, batch size {batch_size} names up to {min(4 * batch_size, n_panos)} of the {n_panos} panoramas in two "
                             f"batches (resident_panos must be at least {min(4 * batch_size, n_panos)})")
        if capacity < need:
            raise ValueError(f"a pool of {capacity} panorama slots cannot hold one batch: batch size {batch_size} names up to {need} of the "
                             f"{n_panos} panoramas at once (resident_panos must be at least {need})")
        self.n_panos, self.capacity, self.policy, self.bytes_per_pano = int(n_panos), int(min(capacity, n_panos)), policy, int(bytes_per_pano)
        self.slot_of = np.full(self.n_panos, -1, dtype=np.int64)
        self.pano_in = np.full(self.capacity, -1, dtype=np.int64)
        self.last_used = np.zeros(self.n_panos, dtype=np.int64)
        self.clock = 0
        self.hits = self.misses = self.uploaded_bytes = 0
        self._last = None

    def plan(self, batch_pano_ids, next_use: Optional[np.ndarray] = None, keep=None) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
        """(slot of every entry of `batch_pano_ids`, [(panorama, slot) to upload]) -- the uploads in panorama order.  `next_use`:
        int64 [n_panos], the batch of every panorama's next use (`epoch_next_use`; None: nothing is known, every panorama counts as
        never used again).  Entries of the current batch's own panoramas are not read.  `keep`: panorama ids that must not be chosen as
        victims either (the batch in flight, when this one is planned ahead of it); the ranking of the others is unchanged, and too few
        victims outside `keep` and the batch is a ValueError, raised before anything is changed."""
        ids = np.asarray(batch_pano_ids, dtype=np.int64)
        need = np.unique(ids)
        if need.size and (int(need[0]) < 0 or int(need[-1]) >= self.n_panos):
            raise ValueError(f"a batch names panorama {int(need[0]) if int(need[0]) < 0 else int(need[-1])}; the cache covers {self.n_panos}")
        if need.size > self.capacity:
            raise ValueError(f"a batch names {need.size} panoramas, the pool has {self.capacity} slots")
        miss = need[self.slot_of[need] < 0]
        if keep is not None:
            kept = np.unique(np.asarray(keep, dtype=np.int64))
            if kept.size and (int(kept[0]) < 0 or int(kept[-1]) >= self.n_panos):
                raise ValueError(f"keep names panorama {int(kept[0]) if int(kept[0]) < 0 else int(kept[-1])}; the cache covers {self.n_panos}")
            pinned = np.union1d(need, kept)
            room = self.capacity - int((self.slot_of[pinned] >= 0).sum())   # free slots + residents that may be evicted
            if miss.size > room:
                raise ValueError(f"a batch misses {miss.size} panoramas, but only {room} of the pool's {self.capacity} slots are free or hold a "
                                 f"panorama outside this batch and the {kept.size} kept ones: no kept panorama is evicted (a larger pool is needed)")
        self.clock += 1
        self.hits += int(need.size - miss.size)
        self.misses += int(miss.size)
        self.uploaded_bytes += int(miss.size) * self.bytes_per_pano
        slots = np.flatnonzero(self.pano_in < 0)[:miss.size]   # free slots first, the lowest first
        if slots.size < miss.size:
            mine = np.zeros(self.n_panos, dtype=bool)
            mine[need] = True
            if keep is not None:
                mine[kept] = True
            cand = self.pano_in[(self.pano_in >= 0) & ~mine[np.maximum(self.pano_in, 0)]]   # resident, not of this batch
            if self.policy == "lru":
                order = np.lexsort((cand, self.last_used[cand]))
            else:
                far = np.full(cand.size, NEVER, dtype=np.int64) if next_use is None else np.asarray(next_use, dtype=np.int64)[cand]
                order = np.lexsort((cand, -np.minimum(far, np.int64(2 ** 62))))   # furthest first (never = 2**62), then the lower id
            victims = cand[order[:miss.size - slots.size]]
            freed = np.sort(self.slot_of[victims])
            self.slot_of[victims] = -1
            slots = np.concatenate([slots, freed])
        self.slot_of[miss] = slots
        self.pano_in[slots] = miss
        self._last = (need, self.last_used[need].copy())   # what `forget` needs to take this plan back
        self.last_used[need] = self.clock
        return self.slot_of[ids], [(int(p), int(sl)) for p, sl in zip(miss, slots)]

    def lookup(self, pano_ids) -> np.ndarray:
        """Slot of every entry of `pano_ids`, all of them resident (planned earlier): no counter moves."""
        slots = self.slot_of[np.asarray(pano_ids, dtype=np.int64)]
        if slots.size and int(slots.min()) < 0:
            raise ValueError("lookup of a panorama that is not resident: plan the batch first")
        return slots

    def forget(self, uploads: Sequence[Tuple[int, int]]) -> None:
        """Take back the MOST RECENT `plan` call, whose `uploads` [(panorama, slot)] did not happen: their slots are free again (the
        victims stay evicted), and hits, misses, uploaded_bytes, the clock and the batch's last-use stamps are what they were before
        it, so that the state matches what was uploaded and hits + misses still counts the panoramas of the plans that stand."""
        if self._last is None or any(self.slot_of[p] != sl or self.pano_in[sl] != p for p, sl in uploads) \
                or not np.isin([p for p, _ in uploads], self._last[0]).all():
            raise ValueError("forget takes back the most recent plan only, with the uploads that plan returned")
        need, stamps = self._last
        for p, sl in uploads:
            self.slot_of[p], self.pano_in[sl] = -1, -1
        self.hits -= int(need.size) - len(uploads)
        self.misses -= len(uploads)
        self.uploaded_bytes -= len(uploads) * self.bytes_per_pano
        self.last_used[need] = stamps
        self.clock -= 1
        self._last = None


# ---------------------------------------------------------------------------------------------------- the pool
class _Stage:
    """One pinned staging buffer of `rows` panoramas (and their slot list) and the event behind the last copy that read it."""

    def __init__(self, rows: int, H: int, W: int) -> None:
        self.rgb = torch.empty((rows, H, W, 3), dtype=torch.uint8).pin_memory()
        self.depth = torch.empty((rows, H, W), dtype=torch.int16).pin_memory()
        self.slots = torch.empty(rows, dtype=torch.int32).pin_memory()
        self.copied: Optional[torch.cuda.Event] = None

    def wait(self) -> None:
        if self.copied is not None:
            self.copied.synchronize()   # the last copy has read the buffer


class _Job(NamedTuple):
    """A batch planned ahead: the uploads `PanoCache.plan` returned and, if there are any, the worker's future (-> the event behind the
    index update)."""
    uploads: List[Tuple[int, int]]
    future: Optional[Future]


class _Iteration:
    """The token of the one iteration that plans a prefetching pool, with the threads that iteration started."""

    def __init__(self, gather_threads: int) -> None:
        self.gather_threads = gather_threads
        self.worker, self.gatherers = ThreadPoolExecutor(1, "salve-upload"), ThreadPoolExecutor(gather_threads, "salve-gather")


def trace_only(tag: str, name: str):
    """The launch wrapper of a caller that keeps no timers: the trace range alone."""
    return tracing.range(name)


class PanoPool:
    """`cache.capacity` panorama slots on the device, filled on demand from the host arrays `rgb` / `depth` (np.memmap included).

    pano_rgb, pano_depth   the slot tensors (zero depth passes neither surface's z filter: an unfilled slot's index entries are empty boxes)
    stages                 two staging buffers of `n_stage` rows, taken in turn: the host writes one while an earlier copy may still read the other
    uploads                panoramas uploaded so far
    prefetch               whether batches are made resident one ahead (`plan_ahead`).  Then the pool owns
    index, stream            its index buffer (the slot writes come from another thread than the scatter: `BevRasteriser.update_panos`) and its copy stream,
    done, pending            the event behind the last batch's last launch, the `_Job` in flight if any,
    iteration, wait_s        the token of the iteration that plans the pool, and the host seconds its loop has waited for upload jobs so far.
    Without prefetch `index` is None: scatter and `update_panos` find the index with the depth tensor."""

    def __init__(self, ras, rgb, depth, cache: PanoCache, n_stage: int, prefetch: bool = False) -> None:
        H, W = ras.pano_hw
        self.ras, self.rgb, self.depth, self.cache, self.prefetch = ras, rgb, depth, cache, bool(prefetch)
        self.pano_rgb = torch.zeros((cache.capacity, H, W, 3), dtype=torch.uint8, device=ras.device)
        self.pano_depth = torch.zeros((cache.capacity, H, W), dtype=torch.int16, device=ras.device)
        index = ras.pano_index(self.pano_depth)
        self.stages, self.turn, self.uploads = [_Stage(n_stage, H, W) for _ in range(2)], 0, 0
        self.index = index if self.prefetch else None
        self.stream = torch.cuda.Stream(ras.device) if self.prefetch else None
        self.done, self.pending, self.iteration, self.wait_s = None, None, None, 0.0   # an event, a `_Job`, an `_Iteration`, seconds

    # ------------------------------------------------------------------ the one upload
    def _next_stage(self) -> _Stage:
        st = self.stages[self.turn]
        self.turn ^= 1
        return st

    def _gather(self, st: _Stage, uploads: Sequence[Tuple[int, int]], lo: int, hi: int) -> None:
        """Rows lo .. hi - 1 of the missed panoramas from the host arrays into the staging buffer (one gather thread's share; numpy
        copies rows of this size with the GIL released)."""
        rgb_np, depth_np = st.rgb.numpy(), st.depth.numpy().view(np.uint16)
        for k in range(lo, hi):
            p = uploads[k][0]
            rgb_np[k] = self.rgb[p]
            depth_np[k] = self.depth[p]

    def _upload(self, st: _Stage, uploads: Sequence[Tuple[int, int]], launch=trace_only, gather: Optional[_Iteration] = None) -> None:
        """`uploads` [(panorama, slot)] into their slots, on the current stream: the rows gathered into `st` (by the calling thread, or
        split over `gather`'s threads), one host-to-device copy per array and the slot list, the event behind them, then the slot writes
        and the index update.  `launch(tag, trace range)`: the caller's wrapper of a launch (`RenderedTrainSource._launch`)."""
        m = len(uploads)
        st.wait()
        if gather is None:
            self._gather(st, uploads, 0, m)
        else:
            T = gather.gather_threads
            cuts = [m * t // T for t in range(T + 1)]
            shares = [gather.gatherers.submit(self._gather, st, uploads, cuts[t], cuts[t + 1]) for t in range(T) if cuts[t + 1] > cuts[t]]
            errors = [f.exception() for f in shares]   # (every thread has left the buffer before the first failure is raised)
            for e in errors:
                if e is not None:
                    raise e
        st.slots.numpy()[:m] = [sl for _, sl in uploads]
        device = self.pano_rgb.device
        with launch("upload", "salve.pano_upload"):
            rgb_rows = st.rgb[:m].to(device, non_blocking=True)
            depth_rows = st.depth[:m].to(device, non_blocking=True)
            slots_dev = st.slots[:m].to(device, non_blocking=True)
            st.copied = torch.cuda.Event()
            st.copied.record()
        with launch("index update", "salve.pano_update"):
            self.ras.update_panos(self.pano_rgb, self.pano_depth, slots_dev, rgb_rows, depth_rows, index=self.index)

    # ------------------------------------------------------------------ on the current stream
    def make_resident(self, panos: np.ndarray, next_use: Optional[np.ndarray], launch=trace_only) -> np.ndarray:
        """Pool slot of every entry of `panos`; the misses are uploaded on the current stream, by the calling thread."""
        slots, uploads = self.cache.plan(panos, next_use)
        if uploads:
            self._upload(self._next_stage(), uploads, launch)
            self.uploads += len(uploads)
        return slots

    def lookup(self, panos: np.ndarray) -> np.ndarray:
        """Pool slot of every entry of `panos`, all made resident earlier (`plan_ahead`): nothing is planned or uploaded."""
        return self.cache.lookup(panos)

    # ------------------------------------------------------------------ one batch ahead
    def begin(self, gather_threads: int) -> _Iteration:
        """A new iteration takes the pool over: another one on this pool (the other source's, or one left suspended) may have a job
        out, which is completed first."""
        self.drain()
        self.stream.synchronize()
        self.iteration = _Iteration(gather_threads)
        return self.iteration

    def check(self, it: _Iteration) -> None:
        if self.iteration is not it:
            raise RuntimeError("another iteration over this resident pool was started while this one was suspended: with prefetch the "
                               "pool serves one iteration at a time (finish or close an epoch before the next begins)")

    def end(self, it: _Iteration) -> None:
        """Finished, closed or dropped mid-epoch, or an exception: nothing of `it` stays in flight, the cache matches the slots.  (An
        iteration that lost the pool to another one only ends its threads.)"""
        if self.iteration is it:
            self.drain()
        it.worker.shutdown(wait=True)
        it.gatherers.shutdown(wait=True)
        if self.iteration is it:
            self.stream.synchronize()

    def mark_done(self) -> Optional[torch.cuda.Event]:
        """Record `done` behind the batch just launched on the current stream; returns the event of the batch before it."""
        before, self.done = self.done, torch.cuda.Event()
        self.done.record()
        return before

    def _upload_ahead(self, st: _Stage, uploads: Sequence[Tuple[int, int]], after: Optional[torch.cuda.Event], it: _Iteration) -> torch.cuda.Event:
        """Worker thread: the upload on the copy stream, behind `after`.  Returns the event behind the index update: what the compute
        stream waits on before it reads the slots.  (No timers: the caller that reads them does not know when this thread records.)"""
        with torch.cuda.stream(self.stream):
            if after is not None:
                self.stream.wait_event(after)
            self._upload(st, uploads, gather=it)
            ready = torch.cuda.Event()
            ready.record()
        return ready

    def plan_ahead(self, panos: np.ndarray, next_use: np.ndarray, keep: np.ndarray, after: Optional[torch.cuda.Event], it: _Iteration) -> None:
        """Plan the batch ahead (its victims spare `keep`, the batch in flight) and start its upload behind `after`, the event of the
        last batch that may still read a victim's slot; the job is the pool's `pending`."""
        _, uploads = self.cache.plan(panos, next_use, keep=keep)
        future = it.worker.submit(self._upload_ahead, self._next_stage(), uploads, after, it) if uploads else None
        self.pending = _Job(uploads, future)

    def drain(self, raise_errors: bool = False) -> Optional[torch.cuda.Event]:
        """Complete the outstanding upload job, if any: join its worker and count its uploads; returns the event behind its index
        update.  A job that failed is taken back from the `PanoCache` (its slots are free again: the state matches what was uploaded) and
        the copy stream is synchronised; its exception is raised here only with `raise_errors` (the loop that needs the batch)."""
        job = self.pending
        if job is None or job.future is None:
            self.pending = None
            return None
        t0 = time.perf_counter()
        error = job.future.exception()   # joins the worker; an interrupt of THIS thread leaves the job pending, to be completed later
        self.wait_s += time.perf_counter() - t0
        self.pending = None
        if error is not None:   # the worker's own exception: nothing of the job's upload counts
            self.cache.forget(job.uploads)
            self.stream.synchronize()
            if raise_errors:
                raise error
            return None
        self.uploads += len(job.uploads)
        return job.future.result()
