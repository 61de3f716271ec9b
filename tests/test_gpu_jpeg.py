"""salve_bev_jpeg_roundtrip on the MI355X: equal to the integer emulator of tests/jpeg_cases.py and to Pillow's save -> open on the
host on every case (out of place and in place, one image and several of mixed contents per call), its refusals, run-to-run
identity, the zero top byte and the memory around the images."""

import ctypes

import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib  # noqa: E402
from salve_amd.jpeg import quality_tables  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402

DEV = torch.device("cuda:0")
GROUPS = sorted({(h, w, q) for _, h, w, q in jc.cases()})


@pytest.fixture(scope="module")
def ras():
    return BevRasteriser(DEV)


def _dev(packed: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(packed.astype(np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("h,w,q", GROUPS, ids=[f"{h}x{w}-q{q}" for h, w, q in GROUPS])
def test_entry_equals_emulator_and_pillow(ras, h, w, q):
    imgs = [jc.make_image(c, h, w) for c in jc.CONTENTS]
    pillow = np.stack([jc.pillow_reference((c, h, w, q)) for c in jc.CONTENTS])
    emulated = np.stack([jc.roundtrip(im, quality_tables(q)) for im in imgs])
    assert np.array_equal(emulated, pillow)
    want = _dev(jc.pack_bgr(pillow))
    src = _dev(jc.pack_bgr(np.stack(imgs)) | np.uint32(0xAB000000))   # (a top byte in the input is ignored and not passed on)
    before = src.clone()
    got = ras.jpeg_roundtrip(src, q)                                   # all contents in one call, out of place
    assert torch.equal(got, want) and torch.equal(src, before)
    for k in (0, len(imgs) - 1):                                       # one image per call
        assert torch.equal(ras.jpeg_roundtrip(src[k:k + 1].clone(), q), want[k:k + 1])
    assert torch.equal(ras.jpeg_roundtrip(src[2:5].contiguous(), q), want[2:5])   # three mixed contents
    work = src.clone()
    assert ras.jpeg_roundtrip(work, q, out=work) is work and torch.equal(work, want)   # in place
    one = src[3:4].clone()
    ras.jpeg_roundtrip(one, q, out=one)
    assert torch.equal(one, want[3:4])


def test_run_to_run_identical_and_top_byte_zero(ras):
    h, w = jc.PRODUCT_SIZE
    src = _dev(jc.pack_bgr(np.stack([jc.make_image(c, h, w, seed=1) for c in ("noise", "disc", "layout")])) | np.uint32(0xFF000000))
    a, b = ras.jpeg_roundtrip(src, 75), ras.jpeg_roundtrip(src, 75)
    assert torch.equal(a, b)
    assert int((a.view(torch.uint8).view(3, h, w, 4)[..., 3] != 0).sum()) == 0


def test_memory_around_the_images_is_untouched(ras):
    n, h, w, guard = 3, 33, 47, 4096
    src = _dev(jc.pack_bgr(np.stack([jc.make_image(c, h, w) for c in ("noise", "stripes", "hramp")])))
    flat = torch.full((2 * guard + n * h * w,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = flat[guard:guard + n * h * w].view(n, h, w)
    ras.jpeg_roundtrip(src, 75, out=out)
    assert torch.equal(out, ras.jpeg_roundtrip(src, 75))
    assert bool((flat[:guard] == 0x5A5A5A5A).all()) and bool((flat[guard + n * h * w:] == 0x5A5A5A5A).all())


def test_refusals(ras):
    lib = ras.lib
    n, h, w = 2, 17, 9
    img = torch.zeros((n, h, w), dtype=torch.int32, device=DEV)
    out = torch.empty_like(img)
    qt = np.ascontiguousarray(quality_tables(75))
    need = lib.salve_bev_jpeg_roundtrip_workspace_bytes(n, h, w)
    assert need == n * 32 * 16 * 3 // 2
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(bev_in=img.data_ptr(), bev_out=out.data_ptr(), n=n, h=h, w=w, q=qt, ws_ptr=ws.data_ptr(), ws_bytes=need):
        qp = None if q is None else q.ctypes.data_as(ctypes.c_void_p)
        return lib.salve_bev_jpeg_roundtrip(ctypes.c_void_p(bev_in), ctypes.c_void_p(bev_out), n, h, w, qp, ctypes.c_void_p(ws_ptr), ws_bytes, None)

    assert call() == _lib.SALVE_OK
    for kw in (dict(bev_in=0), dict(bev_out=0), dict(q=None), dict(ws_ptr=0),
               dict(n=0), dict(n=-1), dict(n=65536), dict(h=0), dict(h=4097), dict(w=0), dict(w=4097),
               dict(ws_bytes=need - 1), dict(ws_ptr=ws.data_ptr() + 1), dict(ws_ptr=ws.data_ptr() + 8)):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    for at, v in ((0, 0), (5, 256), (64, 0), (127, 1000)):
        bad = qt.copy()
        bad.reshape(-1)[at] = v
        assert call(q=bad) == _lib.SALVE_ERR_BAD_ARG, (at, v)
    for bad in ((0, h, w), (65536, h, w), (n, 0, w), (n, 4097, w), (n, h, 0), (n, h, 4097)):
        assert lib.salve_bev_jpeg_roundtrip_workspace_bytes(*bad) == 0, bad
    assert lib.salve_bev_jpeg_roundtrip_workspace_bytes(65535, 4096, 4096) == 65535 * 4096 * 4096 * 3 // 2
    torch.cuda.synchronize()
    # the wrapper's own refusals
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_roundtrip(img.to(torch.int64))
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_roundtrip(img, out=torch.empty((n, h, w + 1), dtype=torch.int32, device=DEV))
    assert ras.jpeg_roundtrip(img[:0]).shape == (0, h, w)
