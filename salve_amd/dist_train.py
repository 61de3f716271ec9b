"""Data-parallel training: one process per GPU, every rank trains rows [lo, hi) of the single-process batch, ONE all-reduce per step
sums the ranks' gradients (opt-in: `python -m salve_amd.train --gpus N`, `training.train(..., dist=DataParallel.from_env())`;
DESIGN.md 4.24).  The reference wraps its model in nn.DataParallel (salve/train_utils.py:214-215, scripts/train.py:1).

The contract is exact.  Rank r's batch is rows [lo_r, hi_r) of the batch the single process makes, bit for bit (the feeds' `rank` /
`world` keywords, salve_amd.train_feed.shard_bounds).  The update every rank applies is sum_r(g_r * (1 / world)): the gradients are
packed, scaled, into one flat fp32 buffer by ONE HIP launch (salve_amd/csrc/flat_bucket.hip: salve_flat_pack), the buffer is summed
by ONE collective, and every `p.grad` becomes its view of the buffer -- no unpack launch: torch.optim.Adam and HipAdam read
contiguous fp32 views as they read any gradient.  As under the reference's DataParallel, BatchNorm statistics are not synchronised:
every rank normalises its own rows, and rank 0's running statistics are the ones validation and the checkpoint see -- unless the
opt-in `sync_bn` is set (models/trainable.py: SyncBatchNormHipFunction), which gathers through `_gather` here.

  FlatBucket       the tables and the flat buffer of a list of fp32 device tensors; pack / unpack / views.
  DataParallel     the process group and the three things a step needs of it: all_reduce_gradients, broadcast, reduce_meter.

Backends: "nccl" (RCCL) reduces the device buffer.  "gloo" stages the buffer through one pinned host buffer and reduces there, so
that the feature does not depend on whether the installed gloo takes device tensors -- it is what several ranks on ONE GPU use,
since RCCL wants a GPU per rank.  A world of one without `force=True` is the identity everywhere and runs no collective.

Not here: overlap of the all-reduce with the backward pass, several buckets, a bf16 wire format, more than one node,
gradient accumulation, the host DataLoader feed in a world larger than one.
"""

from __future__ import annotations

import ctypes
import datetime
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from salve_amd import _lib
from salve_amd.optim import build_chunk_map

BACKENDS = ("nccl", "gloo")
MAX_GPUS = 16   # processes with the GPU open at once on one node
ALIGN = 4       # elements: every segment starts on a 16-byte boundary of the flat buffer


def bucket_offsets(lengths: Sequence[int]) -> Tuple[np.ndarray, int]:
    """(first element of each segment [len(lengths)], elements of the flat buffer) for segments of `lengths` elements laid one behind
    the other, each start rounded up to a multiple of 4 elements: at most 3 elements of padding behind a segment."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and int(n.min()) < 0:
        raise ValueError(f"a segment of {int(n.min())} elements")
    padded = (n + (ALIGN - 1)) // ALIGN * ALIGN
    offsets = np.cumsum(padded) - padded
    return offsets.astype(np.int64), int(padded.sum())


def build_bucket_tables(pointers: Sequence[int], lengths: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
    """(table, chunk_map, flat elements) of salve_flat_pack / salve_flat_unpack for tensors at `pointers` of `lengths` elements, in
    their order: one FLAT_SEGMENT_DTYPE record each, and the chunk map `optim.build_tables` makes for the same lengths."""
    if len(pointers) != len(lengths):
        raise ValueError(f"{len(pointers)} pointers, {len(lengths)} lengths")
    offsets, total = bucket_offsets(lengths)
    table = np.zeros(len(offsets), dtype=_lib.FLAT_SEGMENT_DTYPE)
    table["tensor"] = np.asarray(pointers, dtype=np.uint64)
    table["n"] = np.asarray(lengths, dtype=np.int64)
    table["offset"] = offsets
    return table, build_chunk_map(table["n"]), total


class FlatBucket:
    """One zero-initialised flat fp32 buffer on `device` behind a list of contiguous fp32 device tensors, each at an offset that is
    a multiple of 4 elements.  `pack(scale)`: flat <- tensors * scale, `unpack(scale)`: tensors <- flat * scale, ONE launch each on
    the current stream, no synchronisation; `views()`: the buffer's slice of every tensor, in its shape.  The tables are built once
    and rebuilt when a tensor's `data_ptr()` has changed since (`rebind` swaps the tensors for others of the same lengths: a step's
    gradients are new tensors).  `unpack` writes through raw pointers: like HipAdam's step it bumps no tensor's version counter."""

    def __init__(self, tensors: Sequence[Tensor], device) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SalveHipError("FlatBucket packs on the HIP device ('cuda:N'); there is no CPU path")
        self.tensors: List[Tensor] = []
        self.lengths: List[int] = [int(t.numel()) for t in tensors]
        self.offsets, self.elems = bucket_offsets(self.lengths)
        self.flat = torch.zeros(max(self.elems, ALIGN), dtype=torch.float32, device=self.device)[:self.elems]
        self._pointers: Optional[Tuple[int, ...]] = None
        self._host = self._dev = None    # [table | chunk map] in one pinned buffer and its device copy
        self._n_chunks = self._table_bytes = 0
        self.rebind(tensors)

    def rebind(self, tensors: Sequence[Tensor]) -> None:
        tensors = list(tensors)
        if [int(t.numel()) for t in tensors] != self.lengths:
            raise ValueError("FlatBucket.rebind: the tensors' lengths differ from those the bucket was built for")
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise RuntimeError(f"FlatBucket takes contiguous float32 tensors on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}"
                                   f"{'' if t.is_contiguous() else ', not contiguous'}")
        self.tensors = tensors

    def _tables(self) -> None:
        """(Re)build and upload the tables if a tensor lies elsewhere than when they were made: one pinned buffer, one asynchronous
        copy on the current stream, as HipAdam's step uploads its own."""
        pointers = tuple(int(t.data_ptr()) for t in self.tensors)
        if pointers == self._pointers:
            return
        table, chunk_map, total = build_bucket_tables(pointers, self.lengths)
        assert total == self.elems
        tb, cb = table.nbytes, chunk_map.nbytes
        host = torch.empty(max(tb + cb, 8), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        view[:tb] = table.view(np.uint8)
        view[tb:tb + cb] = chunk_map.view(np.uint8)
        with torch.cuda.device(self.device):
            self._dev = host.to(self.device, non_blocking=True)
        self._host, self._table_bytes, self._n_chunks, self._pointers = host, tb, len(chunk_map), pointers

    def _launch(self, name: str, scale: float) -> None:
        if not self.tensors:
            return
        lib = _lib.load()
        with torch.cuda.device(self.device):
            self._tables()
            stream = torch.cuda.current_stream(self.device).cuda_stream
            tb = self._table_bytes
            st = getattr(lib, name)(ctypes.c_void_p(self._dev.data_ptr()), len(self.tensors), ctypes.c_void_p(self._dev.data_ptr() + tb), self._n_chunks,
                                    ctypes.c_void_p(self._host.data_ptr()), ctypes.c_void_p(self._host.data_ptr() + tb),
                                    ctypes.c_void_p(self.flat.data_ptr()), self.elems, ctypes.c_float(float(np.float32(scale))), ctypes.c_void_p(stream))
        _lib.check(st, name)

    def pack(self, scale: float = 1.0) -> None:
        """flat[offset_s + i] = tensor_s[i] * scale (scale 1: a copy of the bits)."""
        self._launch("salve_flat_pack", scale)

    def unpack(self, scale: float = 1.0) -> None:
        """tensor_s[i] = flat[offset_s + i] * scale (scale 1: a copy of the bits)."""
        self._launch("salve_flat_unpack", scale)

    def views(self) -> List[Tensor]:
        return [self.flat[o:o + n].view_as(t) for o, n, t in zip(self.offsets.tolist(), self.lengths, self.tensors)]


def bn_statistics(model: torch.nn.Module) -> List[Tensor]:
    """The BatchNorm running_mean / running_var buffers of `model`, in its order (num_batches_tracked counts alike on every rank)."""
    return [b for name, b in model.named_buffers() if name.endswith(("running_mean", "running_var"))]


class DataParallel:
    """What a training step needs of the process group.  `rank`, `world`; `device`: this rank's HIP device (None: a host-only group,
    which can reduce meters and check counts but packs nothing).  The group itself is torch.distributed's default group:
    `from_env` initialises it and `close` destroys it; a DataParallel built directly uses the group its caller initialised.
    force: run the collectives in a world of one too."""

    def __init__(self, rank: int = 0, world: int = 1, device=None, backend: str = "nccl", force: bool = False, owns_group: bool = False) -> None:
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} of a world of {world}")
        self.rank, self.world, self.backend, self.force = int(rank), int(world), backend, bool(force)
        self.device = None if device is None else torch.device(device)
        self._owns_group = owns_group
        self._grads: Optional[FlatBucket] = None
        self._buckets = {}          # broadcast: lengths -> FlatBucket
        self._stage: Optional[Tensor] = None   # gloo: the pinned host buffer a flat buffer is reduced in
        self._counted = False

    @classmethod
    def from_env(cls, backend: str = "nccl", timeout_s: float = 600, force: bool = False) -> "DataParallel":
        """The DataParallel of a process started by a launcher (torch.distributed.run): RANK, WORLD_SIZE and LOCAL_RANK name it, the
        device is LOCAL_RANK % device_count(), and the default group is initialised here -- unless the world is one and `force` is
        not set, where nothing is initialised."""
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        rank, world, local = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
        device = None
        if torch.cuda.is_available():
            device = torch.device("cuda", local % torch.cuda.device_count())
            torch.cuda.set_device(device)
        elif backend == "nccl":
            raise RuntimeError("backend nccl needs the HIP device")
        owns = False
        if world > 1 or force:
            import torch.distributed as dist

            kw = {"device_id": device} if backend == "nccl" else {}
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=float(timeout_s)), **kw)
            owns = True
        return cls(rank, world, device, backend, force, owns_group=owns)

    @property
    def active(self) -> bool:
        """Whether collectives run: a world larger than one, or a forced world of one."""
        return self.world > 1 or self.force

    @property
    def is_main(self) -> bool:
        return self.rank == 0

    def close(self) -> None:
        if self._owns_group:
            import torch.distributed as dist

            dist.destroy_process_group()
            self._owns_group = False

    # ------------------------------------------------------------------ collectives on whatever memory the backend takes
    def _gather(self, t: Tensor) -> Tensor:
        """[world, *t.shape] on t's device: every rank's `t`, in rank order -- ONE all-gather (gloo: of a host copy)."""
        import torch.distributed as dist

        src = t.contiguous() if self.backend == "nccl" else t.detach().cpu().contiguous()
        if self.backend == "nccl" and src.device.type != "cuda":
            src = src.to(self.device)
        out = torch.empty(self.world * src.numel(), dtype=src.dtype, device=src.device)   # (flat on both sides: what every backend takes)
        dist.all_gather_into_tensor(out, src.reshape(-1))
        return out.view((self.world,) + tuple(src.shape)).to(t.device)

    def _on_wire(self, flat: Tensor, collective) -> None:
        """`collective(buffer)` on the flat device buffer (nccl) or on its pinned host copy, copied back (gloo)."""
        if self.backend == "nccl":
            collective(flat)
            return
        if self._stage is None or self._stage.numel() < flat.numel():
            self._stage = torch.empty(max(flat.numel(), 1), dtype=torch.float32, pin_memory=torch.cuda.is_available())
        host = self._stage[:flat.numel()]
        host.copy_(flat)        # (synchronises: the pack launch in front of it has run)
        collective(host)
        flat.copy_(host)

    def check_elements(self, n: int) -> None:
        """Every rank must bring the same number of gradient elements to the all-reduce: one all-gather of the count, and an error
        on a mismatch -- where the all-reduce itself would hang or sum unrelated elements."""
        if not self.active:
            return
        counts = self._gather(torch.tensor([int(n)], dtype=torch.int64)).reshape(-1).tolist()
        if any(c != counts[0] for c in counts):
            raise RuntimeError(f"data-parallel ranks hold different gradient sets: elements per rank {counts} (rank {self.rank} has {n}); "
                               "every rank must build the same model and take the same path through it")

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def all_reduce_gradients(self, params: Iterable[Tensor]) -> None:
        """Between `loss.backward()` and `optimizer.step()`: the gradients that are set are packed with scale 1 / world (one launch),
        summed over the ranks (one all-reduce of the flat buffer), and every `p.grad` becomes its view of the buffer."""
        if not self.active:
            return
        import torch.distributed as dist

        active = [p for p in params if p.grad is not None]
        if not active:
            return
        grads = [p.grad for p in active]
        for g in grads:
            if g.is_sparse:
                raise RuntimeError("data-parallel training does not support sparse gradients")
        if self._grads is None or self._grads.lengths != [int(g.numel()) for g in grads]:
            self._grads = FlatBucket(grads, self.device)
            self._counted = False
        else:
            self._grads.rebind(grads)
        if not self._counted:   # the first step (and the first after the gradient set changed)
            self.check_elements(self._grads.elems)
            self._counted = True
        self._grads.pack(1.0 / self.world)
        self._on_wire(self._grads.flat, lambda buf: dist.all_reduce(buf, op=dist.ReduceOp.SUM))
        for p, v in zip(active, self._grads.views()):
            p.grad = v

    @torch.no_grad()
    def broadcast(self, tensors: Iterable[Tensor], src: int = 0) -> None:
        """Every rank's `tensors` become rank `src`'s: pack, ONE broadcast of the flat buffer, unpack -- on every rank, at scale 1
        (bit copies)."""
        if not self.active:
            return
        import torch.distributed as dist

        tensors = [t.detach() for t in tensors]
        if not tensors:
            return
        key = tuple(int(t.numel()) for t in tensors)
        bucket = self._buckets.get(key)
        if bucket is None:
            bucket = self._buckets[key] = FlatBucket(tensors, self.device)
        else:
            bucket.rebind(tensors)
        bucket.pack(1.0)
        self._on_wire(bucket.flat, lambda buf: dist.broadcast(buf, src=src))
        bucket.unpack(1.0)

    def reduce_meter(self, meter=None, loss: Optional[Tuple[float, int]] = None) -> Optional[Tuple[float, int]]:
        """Once per pass: the ranks' counts and loss sums become their sums over the ranks, in place, by ONE all-gather whose rows
        every rank adds in rank order (so every rank ends with the same bits).  meter: an evaluate.DeviceClassMeter (its device
        record: int64 counts, summed as integers, and the loss sum, which salve_head_meter_t keeps as a double and which is summed
        as one), an evaluate.ClassAccuracyMeter (its two float64 arrays), or None.  loss: run_epoch's (loss_sum, loss_n), returned
        summed."""
        if not self.active:
            return loss
        from salve_amd.evaluate import DeviceClassMeter

        if isinstance(meter, DeviceClassMeter):
            rec = meter.record
            at = _lib.HEAD_METER_DTYPE.fields["loss_sum"][1] // 8
            rows = self._gather(rec)                                   # int64 [world, 35]
            total = rows.sum(dim=0)
            total[at:at + 1] = rows[:, at].contiguous().view(torch.float64).sum(dim=0, keepdim=True).view(torch.int64)   # the double, summed as one
            rec.copy_(total)
            meter = None
        parts = [] if meter is None else [np.asarray(meter.correct, dtype=np.float64), np.asarray(meter.total, dtype=np.float64)]
        if loss is not None:
            parts.append(np.array([float(loss[0]), float(loss[1])], dtype=np.float64))
        if not parts:
            return loss
        total = self._gather(torch.from_numpy(np.concatenate(parts))).sum(dim=0).numpy()
        if meter is not None:
            k = len(meter.correct)
            meter.correct, meter.total = total[:k].copy(), total[k:2 * k].copy()
        return None if loss is None else (float(total[-2]), int(total[-1]))
