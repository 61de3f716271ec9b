"""salve_flat_pack / salve_flat_unpack (salve_amd/csrc/flat_bucket.hip) against torch indexing, with torch.equal.

One table holds every segment length at which the kernel takes another path: 0 (a record and no chunk), 1 and 3 (tail only), 4 (one
16-byte group), 5 (a group and a tail), CHUNK - 1 (a partial chunk whose tail is 3), CHUNK (the full-chunk path), CHUNK + 1 (a full
chunk and a chunk of one element) and 2 * CHUNK + 7.  One tensor is a view that starts 4 bytes behind a 16-byte boundary: its
chunks take the element-by-element path.  Everything is pre-filled with a sentinel, so padding, the slack around the tensors and
the buffer behind the last segment must come back untouched.

Left out, for memory: a segment of more than 2^31 elements (8 GiB per side).  Element offsets are 64-bit in the kernel and in the
tables; the lengths here do not reach the width at which a 32-bit offset would wrap.
"""

import ctypes

import numpy as np
import pytest
import torch

from salve_amd import _lib
from salve_amd.dist_train import FlatBucket, build_bucket_tables
from salve_amd.optim import CHUNK

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 6]
MISALIGNED = 7          # LENGTHS[7] = CHUNK + 1 elements, starting 4 bytes behind a 16-byte boundary
SENTINEL = -12345.5     # exactly representable; times 0.5 and 1/3 it is still not a value the generator makes
SLACK = 8               # elements in front of and behind every tensor, which nothing may touch


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _tensors(dev, seed=0):
    """(backing stores pre-filled with the sentinel, the tensors: contiguous views SLACK elements in, one of them misaligned)."""
    g = torch.Generator().manual_seed(seed)
    stores, tensors = [], []
    for k, n in enumerate(LENGTHS):
        store = torch.full((n + 2 * SLACK + 1,), SENTINEL, dtype=torch.float32, device=dev)
        assert store.data_ptr() % 16 == 0
        lo = SLACK + (1 if k == MISALIGNED else 0)
        t = store[lo:lo + n]
        t.copy_(torch.randn(n, generator=g))
        assert (t.data_ptr() % 16 == 4) == (k == MISALIGNED)
        stores.append(store)
        tensors.append(t)
    return stores, tensors


def _outside(stores, tensors):
    """Every element of the backing stores that is no tensor element."""
    out = []
    for k, (s, t) in enumerate(zip(stores, tensors)):
        lo = SLACK + (1 if k == MISALIGNED else 0)
        out += [s[:lo], s[lo + t.numel():]]
    return torch.cat(out)


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_pack_and_unpack_equal_torch_indexing(dev, scale):
    stores, tensors = _tensors(dev)
    bucket = FlatBucket(tensors, dev)
    offsets = bucket.offsets.tolist()
    assert all(o % 4 == 0 for o in offsets) and bucket.elems == offsets[-1] + 8
    assert not bucket.flat.any()                       # zero-initialised
    flat = torch.full((bucket.elems + 64,), SENTINEL, dtype=torch.float32, device=dev)
    bucket.flat = flat[:bucket.elems]                  # (a sentinel-filled buffer with 64 elements behind the bucket)
    originals = [t.clone() for t in tensors]
    s32 = torch.tensor(np.float32(scale))

    bucket.pack(scale)
    torch.cuda.synchronize()
    expect = torch.full_like(flat, SENTINEL)
    for o, t in zip(offsets, originals):
        expect[o:o + t.numel()] = t * s32              # x * np.float32(scale) in fp32
    assert torch.equal(flat, expect)                   # padding and the 64 elements behind included
    for t, o in zip(tensors, originals):
        assert torch.equal(t, o)                       # pack reads the tensors only
    assert (_outside(stores, tensors) == SENTINEL).all()
    for v, t in zip(bucket.views(), tensors):
        assert v.shape == t.shape and v.data_ptr() % 16 == 0

    packed = flat.clone()
    for t in tensors:
        t.fill_(SENTINEL)
    bucket.unpack(scale)
    torch.cuda.synchronize()
    for o, t in zip(offsets, tensors):
        assert torch.equal(t, packed[o:o + t.numel()] * s32)
    assert torch.equal(flat, packed)                   # unpack reads the buffer only
    assert (_outside(stores, tensors) == SENTINEL).all()


def test_scale_one_copies_bits(dev):
    """NaN with a payload, +-inf, -0 and denormals cross pack and unpack at scale 1 as the same 32-bit words -- on the 16-byte path,
    in a tail and on the element-by-element path."""
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,
                        0x3F800000, 0x7F7FFFFF], dtype=np.uint32).view(np.int32)
    stores, tensors = _tensors(dev)
    words = []
    for t in tensors:
        n = t.numel()
        w = torch.from_numpy(np.resize(special, n).copy()).to(dev) if n else torch.zeros(0, dtype=torch.int32, device=dev)
        if n:
            t.view(torch.int32).copy_(torch.roll(w, n // 3))
        words.append(t.view(torch.int32).clone())
    bucket = FlatBucket(tensors, dev)
    bucket.pack(1.0)
    torch.cuda.synchronize()
    for o, w in zip(bucket.offsets.tolist(), words):
        assert torch.equal(bucket.flat[o:o + w.numel()].view(torch.int32), w)
    for t in tensors:
        t.zero_()
    bucket.unpack(1.0)
    torch.cuda.synchronize()
    for t, w in zip(tensors, words):
        assert torch.equal(t.view(torch.int32), w)


def test_the_tables_follow_the_tensors(dev):
    """A step's gradients are new tensors: `rebind` to tensors that lie elsewhere packs those."""
    _, a = _tensors(dev, seed=1)
    _, b = _tensors(dev, seed=2)
    bucket = FlatBucket(a, dev)
    bucket.pack(1.0)
    bucket.rebind(b)
    bucket.pack(1.0)
    torch.cuda.synchronize()
    for v, t in zip(bucket.views(), b):
        assert torch.equal(v, t)
    with pytest.raises(ValueError):
        bucket.rebind(b[:-1])


def _call(name, dev, table, chunk_map, flat, flat_elems=None, n_segments=None, n_chunks=None, null_host=False):
    """One raw library call with tables of the test's making -> status.  The host copies are the arrays themselves."""
    lib = _lib.load()
    raw = np.concatenate([table.view(np.uint8).reshape(-1), chunk_map.view(np.uint8).reshape(-1), np.zeros(8, np.uint8)])
    dev_tables = torch.from_numpy(raw).to(dev)
    tb = table.nbytes
    st = getattr(lib, name)(ctypes.c_void_p(dev_tables.data_ptr()), len(table) if n_segments is None else n_segments,
                            ctypes.c_void_p(dev_tables.data_ptr() + tb), len(chunk_map) if n_chunks is None else n_chunks,
                            None if null_host else ctypes.c_void_p(table.ctypes.data), None if null_host else ctypes.c_void_p(chunk_map.ctypes.data),
                            ctypes.c_void_p(flat.data_ptr()) if flat is not None else None, flat.numel() if flat_elems is None else flat_elems,
                            ctypes.c_float(0.5), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("name", ["salve_flat_pack", "salve_flat_unpack"])
def test_refusals_leave_the_buffers_alone(dev, name):
    """Every refusal of include/salve_hip.h returns SALVE_ERR_BAD_ARG before anything is launched: tensors and buffer unchanged."""
    lengths = [5, CHUNK + 1, 3]
    tensors = [torch.full((n,), 2.0, dtype=torch.float32, device=dev) for n in lengths]
    table, chunk_map, total = build_bucket_tables([t.data_ptr() for t in tensors], lengths)
    flat = torch.full((total,), SENTINEL, dtype=torch.float32, device=dev)
    assert table["offset"].tolist() == [0, 8, 8 + CHUNK + 4] and total == 8 + CHUNK + 4 + 4

    def edited(field, k, value):
        t = table.copy()
        t[field][k] = value
        return t

    bad = {
        "a negative n": dict(table=edited("n", 0, -1)),
        "an offset that is no multiple of 4": dict(table=edited("offset", 1, 6)),
        "overlapping segments": dict(table=edited("offset", 1, 4)),
        "descending offsets": dict(table=edited("offset", 2, 0)),
        "offset + n behind the buffer": dict(flat_elems=total - 2),
        "a chunk map that names another segment": dict(chunk_map=np.array([(0, 0, 0), (1, 0, 0), (2, 0, CHUNK), (2, 0, 0)], dtype=_lib.ADAM_CHUNK_DTYPE)),
        "a chunk map with another offset": dict(chunk_map=np.array([(0, 0, 0), (1, 0, 0), (1, 0, 2 * CHUNK), (2, 0, 0)], dtype=_lib.ADAM_CHUNK_DTYPE)),
        "a chunk too few": dict(chunk_map=chunk_map[:-1].copy()),
        "a chunk too many": dict(chunk_map=np.concatenate([chunk_map, chunk_map[-1:]])),
        "a null tensor with n > 0": dict(table=edited("tensor", 2, 0)),
        "a null buffer with n > 0": dict(flat=None, flat_elems=total),
        "a negative segment count": dict(n_segments=-1),
        "a negative chunk count": dict(n_chunks=-1),
        "no host copies": dict(null_host=True),
    }
    for what, kw in bad.items():
        args = dict(table=table, chunk_map=chunk_map, flat=flat)
        args.update(kw)
        assert _call(name, dev, **args) == _lib.SALVE_ERR_BAD_ARG, what
        assert (flat == SENTINEL).all() and all((t == 2.0).all() for t in tensors), what
    # no segment: OK, nothing launched -- with or without tables
    empty = np.zeros(0, dtype=_lib.FLAT_SEGMENT_DTYPE)
    assert _call(name, dev, empty, np.zeros(0, dtype=_lib.ADAM_CHUNK_DTYPE), flat) == _lib.SALVE_OK
    assert _call(name, dev, empty, np.zeros(0, dtype=_lib.ADAM_CHUNK_DTYPE), flat, null_host=True) == _lib.SALVE_OK
    assert (flat == SENTINEL).all()
    # and the unedited tables pass
    assert _call(name, dev, table, chunk_map, flat) == _lib.SALVE_OK
    if name == "salve_flat_pack":
        assert (flat[:5] == 1.0).all() and (flat[5:8] == SENTINEL).all() and (flat[8:8 + CHUNK + 1] == 1.0).all()
    else:
        assert (tensors[0] == SENTINEL * 0.5).all() and (flat == SENTINEL).all()
