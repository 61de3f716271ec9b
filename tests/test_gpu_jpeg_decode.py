"""salve_bev_jpeg_decode on the MI355X: the device's pixels equal Pillow's on every case of tests/jpeg_coder_cases.py (one call per
(h, w, quality) group), on the reference's fixture files and on files with optimised Huffman tables; a mixed batch of 70 images at
odd byte offsets; malformed scans between good neighbours (only the kinds tests/test_jpeg_decode_host.py has put through the host
build of the same decoder under the sanitizers); run-to-run and stream identity; the refusals."""

import ctypes
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_coder_cases as cc
import jpeg_decode_cases as dc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, jpeg  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = Path(__file__).resolve().parents[1]
FIXTURES = sorted((ROOT / "tests" / "golden" / "renderings").rglob("*.jpg"))
GROUPS = sorted({(h, w, q) for _, h, w, q in cc.cases()})
OPTIMISED = [("noise", 33, 47, 75), ("disc", 33, 47, 75), ("zrl", 33, 47, 75), ("ffheavy", 33, 47, 75), ("checker", 16, 16, 100), ("noise", 1, 1, 75)]
PAD = jpeg.SCAN_PADDING


@pytest.fixture(scope="module")
def ras():
    return BevRasteriser(DEV)


def _pack(scans, gaps=None):
    """Scans laid out one behind the other (gaps[i] filler bytes in front of scan i), the padding behind the last:
    (uint8 device tensor, offsets, lengths)."""
    gaps = [0] * len(scans) if gaps is None else gaps
    buf, off = bytearray(), []
    for s, g in zip(scans, gaps):
        buf += b"\xee" * g
        off.append(len(buf))
        buf += s
    buf += b"\xee" * PAD
    return torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(DEV), np.array(off, dtype=np.int64), np.array([len(s) for s in scans], dtype=np.int64)


def _decode_files(ras, files, gaps=None):
    """Files that share their header -> (uint8 [n, h, w, 3], status [n]) on the host."""
    parsed = [jpeg.parse_file(f) for f in files]
    assert len({p.header_key for p in parsed}) == 1
    p = parsed[0]
    scans, off, nb = _pack([f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)], gaps)
    img, st = ras.jpeg_decode(scans, off, nb, p.h, p.w, p.qtab, p.huffman)
    assert img.shape == (len(files), p.h, p.w) and img.dtype == torch.int32 and st.shape == (len(files),) and st.dtype == torch.int32
    return jc.unpack_bgr(img.cpu().numpy().view(np.uint32)), st.cpu().numpy()


@pytest.mark.parametrize("h,w,q", GROUPS, ids=[f"{h}x{w}-q{q}" for h, w, q in GROUPS])
def test_pixels_equal_pillows(ras, h, w, q):
    group = [c for c in cc.cases() if c[1:] == (h, w, q)]
    files = [cc.reference(c)[0] for c in group]
    got, status = _decode_files(ras, files)          # all contents of the shape in one call
    assert status.tolist() == [0] * len(group)
    for i, c in enumerate(group):
        want = jc.pillow_reference(c) if c in jc.cases() else dc.pillow_pixels(files[i])
        assert np.array_equal(got[i], want), c
    ras.check("jpeg_decode")


def test_the_fixture_files_equal_read_rgb(ras):
    assert len(FIXTURES) == 4
    got, status = _decode_files(ras, [f.read_bytes() for f in FIXTURES])
    assert status.tolist() == [0, 0, 0, 0]
    for i, f in enumerate(FIXTURES):
        assert np.array_equal(got[i], image_io.read_rgb(str(f))), f.name


def test_files_with_huffman_tables_of_their_own(ras):
    for c, h, w, q in OPTIMISED:
        data = dc.pillow_file(cc.make_image(c, h, w), quality=q, optimize=True)
        assert not np.array_equal(jpeg.parse_file(data).huffman, dc.STANDARD_HUFFMAN)
        got, status = _decode_files(ras, [data])
        assert status.tolist() == [0] and np.array_equal(got[0], dc.pillow_pixels(data)), (c, h, w, q)


def test_mixed_batch_of_70_at_odd_offsets_equals_one_image_per_call(ras):
    h, w, q = 33, 47, 75
    contents = jc.CONTENTS + ("zrl", "ffheavy", "checker")
    images = [cc.make_image(contents[i % len(contents)], h, w, seed=i // len(contents)) for i in range(70)]
    files = [cc.pillow_file(img, q) for img in images]
    assert len({len(f) for f in files}) > 10
    gaps = [1 + 2 * (i % 5) for i in range(70)]      # every scan starts at an odd offset or right behind an odd-sized neighbour
    got, status = _decode_files(ras, files, gaps)
    assert not status.any()
    for i in range(70):
        one, st = _decode_files(ras, [files[i]])
        assert st[0] == 0 and np.array_equal(one[0], got[i]), i
        assert np.array_equal(got[i], dc.pillow_pixels(files[i])), i


def _hostile():
    """(huffman, qtab, good scan, [truncated, bit-flipped, empty]) of the 16 x 16 noise image at quality 75 -- the inputs of
    tests/test_jpeg_decode_host.py's hostile families; the flip is the first of its seeded positions that the emulator reports."""
    pillow = cc.reference(("noise", 16, 16, 75))[0]
    p = jpeg.parse_file(pillow)
    scan = pillow[p.scan_offset:p.scan_offset + p.scan_bytes]
    rng = np.random.RandomState(5)
    for at in rng.choice(8 * len(scan), size=200, replace=False):
        s = bytearray(scan)
        s[at >> 3] ^= 0x80 >> (at & 7)
        if dc.decode(bytes(s), p.huffman, 1, 1)[1] != 0:
            return p, pillow, scan, [scan[:len(scan) // 2], bytes(s), b""]
    raise AssertionError("no reported flip")


def test_malformed_scans_report_and_leave_their_neighbours_alone(ras):
    p, pillow, scan, bad = _hostile()
    want = dc.pillow_pixels(pillow)
    scans = [scan, bad[0], scan, bad[1], scan, bad[2], scan]
    buf, off, nb = _pack(scans, gaps=[3, 1, 0, 5, 0, 2, 0])
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    st = st.cpu().numpy()
    got = jc.unpack_bgr(img.cpu().numpy().view(np.uint32))
    assert st[0::2].tolist() == [0, 0, 0, 0] and all(int(s) != 0 for s in st[1::2]), st
    assert st[5] == dc.TRUNCATED   # the empty scan
    for i in (0, 2, 4, 6):
        assert np.array_equal(got[i], want), i
    assert "ok" != jpeg.describe_status(int(st[1]))
    ras.check("jpeg_decode of malformed scans")   # the device status word is clean: bad files are the images' own business
    # an empty scan decodes to the image of all-zero coefficients: mid grey
    assert (got[5] == 128).all()


def test_run_to_run_and_stream_identity(ras):
    files = [f.read_bytes() for f in FIXTURES]
    parsed = [jpeg.parse_file(f) for f in files]
    p = parsed[0]
    buf, off, nb = _pack([f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)])
    a, sa = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    b, sb = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c, sc = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(sa, sb) and torch.equal(sa, sc) and not sa.any()


def test_the_two_stages_called_apart_equal_the_whole_call(ras):
    """`stages`: the entropy stage alone writes the status and leaves the images alone; the inverse stage alone then makes the
    whole call's pixels from the coefficients in the workspace and leaves the status alone."""
    files = [f.read_bytes() for f in FIXTURES]
    parsed = [jpeg.parse_file(f) for f in files]
    p = parsed[0]
    scans = [f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)]
    scans[2] = scans[2][:len(scans[2]) // 3]           # one malformed image: its status comes from the entropy stage
    buf, off, nb = _pack(scans)
    whole, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    out = torch.full((4, p.h, p.w), 0x00ABCDEF, dtype=torch.int32, device=DEV)
    _, st_e = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, out=out, stages=_lib.JPEG_STAGE_ENTROPY)
    assert bool((out == 0x00ABCDEF).all()) and torch.equal(st_e, st) and st.cpu().numpy().tolist()[2] != 0
    ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, out=out, stages=_lib.JPEG_STAGE_INVERSE)
    assert torch.equal(out, whole)
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, stages=0)


def test_refusals(ras):
    lib = ras.lib
    n, h, w = 2, 17, 9
    files = [cc.reference((c, h, w, 75))[0] for c in ("noise", "disc")]
    parsed = [jpeg.parse_file(f) for f in files]
    buf, off, nb = _pack([f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)])
    off_d, nb_d = torch.from_numpy(off).to(DEV), torch.from_numpy(np.concatenate([nb.astype(np.int32), [0]]).astype(np.int32)).to(DEV)
    qt, hf = np.ascontiguousarray(parsed[0].qtab), np.ascontiguousarray(parsed[0].huffman)
    need = lib.salve_bev_jpeg_decode_workspace_bytes(n, h, w)
    assert need == n * (32 * 16 * 3 // 2 + 2 * 768)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    out = torch.empty((n, h, w), dtype=torch.int32, device=DEV)
    status = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 16 == 0

    def call(scans=buf.data_ptr(), size=buf.numel(), off_ptr=off_d.data_ptr(), nb_ptr=nb_d.data_ptr(), n=n, h=h, w=w, q=qt, huff=hf, out_ptr=out.data_ptr(),
             st_ptr=status.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need, stages=_lib.JPEG_STAGES_ALL):
        qp = None if q is None else q.ctypes.data_as(ctypes.c_void_p)
        hp = None if huff is None else huff.ctypes.data_as(ctypes.c_void_p)
        return lib.salve_bev_jpeg_decode(ctypes.c_void_p(scans), size, ctypes.c_void_p(off_ptr), ctypes.c_void_p(nb_ptr), n, h, w, qp, hp,
                                         ctypes.c_void_p(out_ptr), ctypes.c_void_p(st_ptr), ctypes.c_void_p(ws_ptr), ws_bytes, stages, None)

    assert call() == _lib.SALVE_OK
    for kw in (dict(scans=0), dict(off_ptr=0), dict(nb_ptr=0), dict(q=None), dict(huff=None), dict(out_ptr=0), dict(st_ptr=0), dict(ws_ptr=0),
               dict(n=0), dict(n=-1), dict(n=65536), dict(h=0), dict(h=4097), dict(w=0), dict(w=4097), dict(size=15),
               dict(off_ptr=off_d.data_ptr() + 4), dict(nb_ptr=nb_d.data_ptr() + 2), dict(out_ptr=out.data_ptr() + 2), dict(st_ptr=status.data_ptr() + 1),
               dict(ws_ptr=ws.data_ptr() + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(stages=0), dict(stages=4)):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    for at, v in ((0, 0), (5, 256), (64, 0), (127, 1000)):
        bad = qt.copy()
        bad.reshape(-1)[at] = v
        assert call(q=bad) == _lib.SALVE_ERR_BAD_ARG, (at, v)
    for t, at, v in ((0, 0, 3), (1, 1, 5), (3, 15, 255), (2, 2, 200)):   # BITS that over-subscribe the code space or sum past 256
        bad = hf.copy()
        bad[t, at] = v
        assert call(huff=bad) == _lib.SALVE_ERR_BAD_ARG, (t, at, v)
    for args in ((0, h, w), (65536, h, w), (n, 0, w), (n, h, 4097)):
        assert lib.salve_bev_jpeg_decode_workspace_bytes(*args) == 0
    # a slot that does not lie inside the buffer with its padding is not read: the image reports it, the call succeeds
    assert call(size=buf.numel() - 1) == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert status[:n].cpu().numpy().tolist() == [0, dc.BAD_SLOT]
    # the wrapper's own refusals
    p = parsed[0]
    with pytest.raises(_lib.SalveHipError, match="padding"):
        ras.jpeg_decode(buf[:-1], off, nb, h, w, p.qtab, p.huffman)
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_decode(buf.to(torch.int32), off, nb, h, w, p.qtab, p.huffman)
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_decode(buf, off[:1], nb, h, w, p.qtab, p.huffman)
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_decode(buf, -off - 1, nb, h, w, p.qtab, p.huffman)
    with pytest.raises(_lib.SalveHipError):
        ras.jpeg_decode(buf, off, nb, h, w, p.qtab[:1], p.huffman)
    img, st = ras.jpeg_decode(buf, off[:0], nb[:0], h, w, p.qtab, p.huffman)
    assert img.shape == (0, h, w) and st.shape == (0,)
