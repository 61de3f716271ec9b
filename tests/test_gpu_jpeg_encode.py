"""salve_bev_jpeg_encode on the MI355X: the device's scans, wrapped by salve_amd.jpeg.file_bytes, equal Pillow's files and the
emulator of tests/jpeg_coder_cases.py byte for byte on every case; exact lengths; the slot bytes behind a scan and the memory around
the slots untouched; mixed batches; an image that overflows its slot; consistency with salve_bev_jpeg_roundtrip; run-to-run and
stream identity; the refusals; the bound."""

import ctypes
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_coder_cases as cc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, jpeg  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402

DEV = torch.device("cuda:0")
GROUPS = sorted({(h, w, q) for _, h, w, q in cc.cases()})
FILL, GUARD = 0x5A, 256


@pytest.fixture(scope="module")
def ras():
    return BevRasteriser(DEV)


def _dev(images) -> torch.Tensor:
    return torch.from_numpy(jc.pack_bgr(np.stack(images)).astype(np.uint32).view(np.int32)).to(DEV)


def _round4(v: int) -> int:
    return (v + 3) // 4 * 4


def _raw_encode(ras, src: torch.Tensor, q: int, stride: int):
    """The library call into slots pre-filled with a pattern, guard bytes in front of the first and behind the last slot.
    -> (slots uint8 [n, stride], scan_bytes [n]) on the host, after checking the guards and the words around scan_bytes."""
    n, h, w = (int(v) for v in src.shape)
    lib = ras.lib
    flat = torch.full((GUARD + n * stride + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    nbytes = torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)
    need = lib.salve_bev_jpeg_encode_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    qt = np.ascontiguousarray(jpeg.quality_tables(q))
    st = lib.salve_bev_jpeg_encode(ctypes.c_void_p(src.data_ptr()), n, h, w, qt.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(flat.data_ptr() + GUARD),
                                   stride, ctypes.c_void_p(nbytes.data_ptr() + 4), ctypes.c_void_p(ws.data_ptr()), need, None)
    assert st == _lib.SALVE_OK, lib.salve_last_error()
    torch.cuda.synchronize()
    flat, nbytes = flat.cpu().numpy(), nbytes.cpu().numpy()
    assert (flat[:GUARD] == FILL).all() and (flat[GUARD + n * stride:] == FILL).all() and nbytes[0] == -7 and nbytes[-1] == -7
    return flat[GUARD:GUARD + n * stride].reshape(n, stride), nbytes[1:-1]


def _assert_exact(slots, nbytes, want):
    for i, scan in enumerate(want):
        assert int(nbytes[i]) == len(scan), (i, int(nbytes[i]), len(scan))
        assert slots[i, :len(scan)].tobytes() == scan, i
        assert (slots[i, len(scan):] == FILL).all(), i   # nothing behind the scan


@pytest.mark.parametrize("h,w,q", GROUPS, ids=[f"{h}x{w}-q{q}" for h, w, q in GROUPS])
def test_files_equal_pillows_and_the_emulators(ras, h, w, q):
    group = [c for c in cc.cases() if c[1:] == (h, w, q)]
    refs = [cc.reference(c) for c in group]
    src = _dev([cc.make_image(c[0], h, w) for c in group])
    stride = _round4(max(len(r[1]) for r in refs) + 64)
    slots, nbytes = _raw_encode(ras, src, q, stride)     # all contents of the shape in one batch
    _assert_exact(slots, nbytes, [r[1] for r in refs])
    for i, (pillow, scan, _) in enumerate(refs):
        assert jpeg.file_bytes(slots[i, :nbytes[i]].tobytes(), h, w, q) == pillow == jpeg.file_bytes(scan, h, w, q)
    scan_t, n_t = ras.jpeg_encode(src, q)                # the wrapper at its default stride
    assert scan_t.shape == (len(group), _round4(ras.lib.salve_bev_jpeg_encode_max_bytes(h, w) // 8)) and scan_t.dtype == torch.uint8
    assert n_t.cpu().numpy().tolist() == nbytes.tolist()
    got = scan_t.cpu().numpy()
    for i in range(len(group)):   # (noise at a high quality outgrows the default slot at the small shapes: reported, not written whole)
        if nbytes[i] <= scan_t.shape[1]:
            assert got[i, :nbytes[i]].tobytes() == refs[i][1], i
    assert any(nbytes[i] <= scan_t.shape[1] for i in range(len(group)))


def test_mixed_batch_equals_one_image_per_call(ras):
    h, w, q = 33, 47, 75
    contents = ("noise", "constant", "hramp", "zrl", "ffheavy")
    want = [cc.reference((c, h, w, q))[1] for c in contents]
    assert len({len(s) for s in want}) == 5
    src = _dev([cc.make_image(c, h, w) for c in contents])
    stride = _round4(max(len(s) for s in want) + 8)
    slots, nbytes = _raw_encode(ras, src, q, stride)
    _assert_exact(slots, nbytes, want)
    for i in range(5):
        one, n_one = _raw_encode(ras, src[i:i + 1].contiguous(), q, stride)
        assert n_one[0] == nbytes[i] and np.array_equal(one[0], slots[i])


def test_an_image_that_overflows_its_slot_reports_its_length_and_disturbs_nothing(ras):
    h, w, q = 33, 47, 75
    contents = ("hramp", "noise", "constant")
    want = [cc.reference((c, h, w, q))[1] for c in contents]
    stride = _round4(max(len(want[0]), len(want[2])) + 8)
    assert len(want[0]) < stride and len(want[2]) < stride < len(want[1])
    slots, nbytes = _raw_encode(ras, _dev([cc.make_image(c, h, w) for c in contents]), q, stride)   # (checks the guards behind the last slot)
    assert nbytes.tolist() == [len(s) for s in want]          # the NEEDED length of image 1
    _assert_exact(slots[0::2], nbytes[0::2], want[0::2])      # its neighbours are whole, and the pattern behind their scans is intact
    ras.check("jpeg_encode overflow")                          # no status bit
    # the wrapper reports it the same way
    scan_t, n_t = ras.jpeg_encode(_dev([cc.make_image(c, h, w) for c in contents]), q, stride=stride)
    assert scan_t.shape == (3, stride) and n_t.cpu().numpy().tolist() == [len(s) for s in want]
    assert scan_t[2, :len(want[2])].cpu().numpy().tobytes() == want[2]


@pytest.mark.parametrize("h,w", [(33, 47), jc.PRODUCT_SIZE])
def test_pillow_decodes_the_device_file_to_the_device_round_trip(ras, h, w):
    from PIL import Image

    contents = ("disc", "noise", "layout")
    src = _dev([jc.make_image(c, h, w) for c in contents])
    scan, nbytes = ras.jpeg_encode(src, 75)
    scan, nbytes = scan.cpu().numpy(), nbytes.cpu().numpy()
    rt = jc.unpack_bgr(ras.jpeg_roundtrip(src, 75).cpu().numpy().view(np.uint32))
    for i in range(len(contents)):
        with Image.open(io.BytesIO(jpeg.file_bytes(scan[i, :nbytes[i]].tobytes(), h, w, 75))) as im:
            assert np.array_equal(np.asarray(im.convert("RGB")), rt[i]), contents[i]


def test_run_to_run_and_stream_identity(ras):
    h, w = jc.PRODUCT_SIZE
    src = _dev([jc.make_image(c, h, w, seed=1) for c in ("noise", "disc", "layout")])
    a, na = ras.jpeg_encode(src, 75)
    b, nb = ras.jpeg_encode(src, 75)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c, nc = ras.jpeg_encode(src, 75)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(na, nb) and torch.equal(na, nc)
    for i, n in enumerate(na.cpu().numpy().tolist()):
        assert torch.equal(a[i, :n], b[i, :n]) and torch.equal(a[i, :n], c[i, :n])


def test_refusals(ras):
    lib = ras.lib
    n, h, w = 2, 17, 9
    img = torch.zeros((n, h, w), dtype=torch.int32, device=DEV)
    qt = np.ascontiguousarray(jpeg.quality_tables(75))
    need = lib.salve_bev_jpeg_encode_workspace_bytes(n, h, w)
    stride = lib.salve_bev_jpeg_encode_max_bytes(h, w)
    assert need > 0 and stride == 2 * 2490
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    scan = torch.empty(n * stride, dtype=torch.uint8, device=DEV)
    nbytes = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(bev=img.data_ptr(), n=n, h=h, w=w, q=qt, scan_ptr=scan.data_ptr(), stride=stride, nb_ptr=nbytes.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need):
        qp = None if q is None else q.ctypes.data_as(ctypes.c_void_p)
        return lib.salve_bev_jpeg_encode(ctypes.c_void_p(bev), n, h, w, qp, ctypes.c_void_p(scan_ptr), stride, ctypes.c_void_p(nb_ptr),
                                         ctypes.c_void_p(ws_ptr), ws_bytes, None)

    assert call() == _lib.SALVE_OK
    for kw in (dict(bev=0), dict(q=None), dict(scan_ptr=0), dict(nb_ptr=0), dict(ws_ptr=0),
               dict(n=0), dict(n=-1), dict(n=65536), dict(h=0), dict(h=4097), dict(w=0), dict(w=4097),
               dict(bev=img.data_ptr() + 2), dict(nb_ptr=nbytes.data_ptr() + 2), dict(ws_ptr=ws.data_ptr() + 8), dict(ws_ptr=ws.data_ptr() + 1),
               dict(stride=0), dict(stride=stride + 2), dict(stride=5), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    for at, v in ((0, 0), (5, 256), (64, 0), (127, 1000)):
        bad = qt.copy()
        bad.reshape(-1)[at] = v
        assert call(q=bad) == _lib.SALVE_ERR_BAD_ARG, (at, v)
    torch.cuda.synchronize()
    # the wrapper's own refusals
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_encode(img.to(torch.int64))
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_encode(img, stride=6)
    empty_scan, empty_n = ras.jpeg_encode(img[:0])
    assert empty_scan.shape[0] == 0 and empty_n.shape == (0,)


def test_the_bound_holds_noise_at_quality_100_at_every_shape(ras):
    for h, w in jc.SMALL_SIZES + (jc.PRODUCT_SIZE,):
        img = jc.make_image("noise", h, w)
        bound = ras.lib.salve_bev_jpeg_encode_max_bytes(h, w)
        scan, nbytes = ras.jpeg_encode(_dev([img]), 100, stride=bound)
        n = int(nbytes[0])
        assert 0 < n <= bound, (h, w, n, bound)
        assert jpeg.file_bytes(scan[0, :n].cpu().numpy().tobytes(), h, w, 100) == cc.pillow_file(img, 100), (h, w)
