"""BevRasteriser.jpeg_decode(sampling=) on the MI355X: 4:2:2, 4:4:4 and greyscale files (and 4:2:0 through the same keyword) decode
to Pillow's pixels bit for bit on every case of tests/jpeg_sampling_cases.py, with either entropy stage; three files in one call;
salve_bev_jpeg_decode_sampled / _lanes_sampled at SALVE_JPEG_SAMPLING_420 against the entries without the argument; the refusals; the
malformed inputs tests/test_jpeg_sampling_host.py has put through the host build of the same decoders under the sanitizers (and no
others), between good neighbours."""

import ctypes

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_lanes_cases as lc
import jpeg_sampling_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, jpeg  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402

DEV = torch.device("cuda:0")
PAD = jpeg.SCAN_PADDING


@pytest.fixture(scope="module")
def ras():
    return BevRasteriser(DEV)


def _pack(files, gaps=None):
    """Whole files that share their header, laid out one behind the other (gaps[i] filler bytes in front of file i), the padding behind
    the last -> (uint8 device tensor, scan offsets, scan lengths, segment rows, the first file's ParsedFile)."""
    gaps = [0] * len(files) if gaps is None else gaps
    buf, off, nb, rows, first = bytearray(), [], [], [], None
    for i, (f, g) in enumerate(zip(files, gaps)):
        p = sc.parse(f)
        first = first or p
        assert p.header_key == first.header_key
        buf += b"\xee" * g
        base = len(buf) - p.scan_offset
        buf += f[p.scan_offset:p.scan_offset + p.scan_bytes]
        off.append(base + p.scan_offset)
        nb.append(p.scan_bytes)
        rows += [(base + o, n, i, m0, mc) for o, n, m0, mc in p.segments]
    buf += b"\xee" * PAD
    dev = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(DEV)
    return dev, np.array(off, dtype=np.int64), np.array(nb, dtype=np.int64), rows, first


def _rgb(img):
    return jc.unpack_bgr(img.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("sampling,name", sc.cases())
def test_both_entropy_stages_give_pillows_pixels_on_every_case(ras, sampling, name):
    data = sc.file_of(sampling, name)
    buf, off, nb, rows, p = _pack([data], gaps=[1])
    assert p.sampling == sampling
    want = sc.pillow_reference(sampling, name)
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=rows, sampling=sampling)
    assert st.cpu().numpy().tolist() == [0]
    assert np.array_equal(_rgb(img)[0], want)
    if name not in sc.RESTART_CASES:            # the serial stage takes no restart intervals
        img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="image", sampling=sampling)
        assert st.cpu().numpy().tolist() == [0]
        assert np.array_equal(_rgb(img)[0], want)
    ras.check("jpeg_decode(sampling=)")


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_three_files_in_one_call(ras, sampling):
    """The per-image plane and coefficient offsets: three files of one header_key at odd byte offsets, with a restart file's table in
    the lanes call (its own header, so a call of its own)."""
    files = [sc.pillow_file(jc.make_image("noise", 33, 47, seed=i), sampling, quality=75) for i in range(3)]
    want = [sc.pillow_rgb3(f) for f in files]
    buf, off, nb, rows, p = _pack(files, gaps=[1, 3, 5])
    for kw in (dict(entropy="lanes", segments=rows), dict(entropy="lanes"), dict(entropy="image")):
        img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, sampling=sampling, **kw)
        assert not st.cpu().numpy().any()
        got = _rgb(img)
        for i in range(3):
            assert np.array_equal(got[i], want[i]), (kw.get("entropy"), i)
    files = [sc.pillow_file(jc.make_image("noise", 33, 47, seed=i), sampling, quality=75, restart_marker_blocks=2) for i in range(3)]
    buf, off, nb, rows, p = _pack(files, gaps=[0, 7, 2])
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, sampling=sampling, entropy="lanes", segments=rows)
    assert not st.cpu().numpy().any()
    for i in range(3):
        assert np.array_equal(_rgb(img)[i], sc.pillow_rgb3(files[i])), i


def _direct(ras, entry, buf, off, nb, rows, p, n, sampling=None, ws_bytes=None, stages=_lib.JPEG_STAGES_ALL):
    """One library call outside the wrapper -> (return value, pixels, status, what the entry's size query says)."""
    lib = ras.lib
    more = () if sampling is None else (sampling,)
    qt, hf = np.ascontiguousarray(p.qtab, dtype=np.uint16), np.ascontiguousarray(p.huffman, dtype=np.uint8)
    need = getattr(lib, entry + "_workspace_bytes")(n, p.h, p.w, *((len(rows),) if "lanes" in entry else ()), *more)
    ws = torch.empty(max(need, ws_bytes or 0, 16), dtype=torch.uint8, device=DEV)
    out = torch.zeros((n, p.h, p.w), dtype=torch.int32, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    if "lanes" in entry:
        seg = np.zeros(len(rows), dtype=_lib.JPEG_SEGMENT_DTYPE)
        for k, field in enumerate(_lib.JPEG_SEGMENT_DTYPE.names):
            seg[field] = [r[k] for r in rows]
        table = torch.from_numpy(seg.view(np.uint8)).to(DEV)
        head = (ctypes.c_void_p(buf.data_ptr()), buf.numel(), ctypes.c_void_p(table.data_ptr()), len(rows))
    else:
        table = torch.from_numpy(np.concatenate([off.view(np.uint8), nb.astype(np.int32).view(np.uint8)])).to(DEV)
        head = (ctypes.c_void_p(buf.data_ptr()), buf.numel(), ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(table.data_ptr() + 8 * n))
    rv = getattr(lib, entry)(*head, n, p.h, p.w, *more, qt.ctypes.data_as(ctypes.c_void_p), hf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()),
                             ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(ws.data_ptr()), need if ws_bytes is None else ws_bytes, stages, None)
    torch.cuda.synchronize()
    return rv, out, status.cpu().numpy(), need


@pytest.mark.parametrize("name", ["size_17x33", "size_48x64"])
def test_sampling_420_through_the_new_entries_is_the_old_entries(ras, name):
    data = lc.file_of(name)
    buf, off, nb, rows, p = _pack([data, data], gaps=[1, 2])
    want = sc.pillow_rgb3(data)
    for old, new in (("salve_bev_jpeg_decode", "salve_bev_jpeg_decode_sampled"), ("salve_bev_jpeg_decode_lanes", "salve_bev_jpeg_decode_lanes_sampled")):
        rv_old, out_old, st_old, need_old = _direct(ras, old, buf, off, nb, rows, p, 2)
        rv_new, out_new, st_new, need_new = _direct(ras, new, buf, off, nb, rows, p, 2, sampling=_lib.JPEG_SAMPLINGS["4:2:0"])
        assert rv_old == rv_new == _lib.SALVE_OK and need_old == need_new > 0
        assert st_old.tolist() == st_new.tolist() == [0, 0] and torch.equal(out_old, out_new)
        assert np.array_equal(_rgb(out_new)[1], want)
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=rows, sampling="4:2:0")
    assert torch.equal(img, out_new) and not st.cpu().numpy().any()


def test_workspace_bytes_per_sampling(ras):
    """Planes of 1.5 / 2 / 3 / 1 bytes per MCU-rounded pixel, plus 128 bytes of coefficients per block."""
    lib = ras.lib
    n, h, w = 3, 33, 47
    for sampling, (mh, mw), plane_x2, blocks in (("4:2:0", (16, 16), 3, 6), ("4:2:2", (8, 16), 4, 4), ("4:4:4", (8, 8), 6, 3), ("grey", (8, 8), 2, 1)):
        gh, gw = -(-h // mh), -(-w // mw)
        want = n * (gh * mh * gw * mw * plane_x2 // 2 + gh * gw * blocks * 128)
        code = _lib.JPEG_SAMPLINGS[sampling]
        assert lib.salve_bev_jpeg_decode_sampled_workspace_bytes(n, h, w, code) == want, sampling
        assert lib.salve_bev_jpeg_decode_lanes_sampled_workspace_bytes(n, h, w, n, code) == want, sampling
    assert lib.salve_bev_jpeg_decode_sampled_workspace_bytes(n, h, w, 0) == lib.salve_bev_jpeg_decode_workspace_bytes(n, h, w)


def test_bad_samplings_and_small_workspaces_are_refused(ras):
    lib = ras.lib
    for sampling in ("4:2:2", "4:4:4", "grey"):
        data = sc.file_of(sampling, "24x40_noise")
        buf, off, nb, rows, p = _pack([data])
        code = _lib.JPEG_SAMPLINGS[sampling]
        for entry in ("salve_bev_jpeg_decode_sampled", "salve_bev_jpeg_decode_lanes_sampled"):
            rv, out, st, need = _direct(ras, entry, buf, off, nb, rows, p, 1, sampling=code)
            assert rv == _lib.SALVE_OK and st.tolist() == [0] and np.array_equal(_rgb(out)[0], sc.pillow_reference(sampling, "24x40_noise"))
            small = lib.salve_bev_jpeg_decode_sampled_workspace_bytes(1, p.h, p.w, _lib.JPEG_SAMPLINGS["grey"])
            for ws_bytes in (need - 1, 0) + ((small,) if sampling != "grey" else ()):      # (greyscale's bytes are too few for the others)
                rv, out, st, _ = _direct(ras, entry, buf, off, nb, rows, p, 1, sampling=code, ws_bytes=ws_bytes)
                assert rv == _lib.SALVE_ERR_BAD_ARG and lib.salve_last_error().decode() != "" and not out.any() and st.tolist() == [-1], (entry, ws_bytes)
    data = sc.file_of("4:2:2", "24x40_noise")
    buf, off, nb, rows, p = _pack([data])
    for bad in (4, -1, 1 << 20):
        assert lib.salve_bev_jpeg_decode_sampled_workspace_bytes(1, p.h, p.w, bad) == 0
        assert lib.salve_bev_jpeg_decode_lanes_sampled_workspace_bytes(1, p.h, p.w, 1, bad) == 0
        for entry in ("salve_bev_jpeg_decode_sampled", "salve_bev_jpeg_decode_lanes_sampled"):
            rv, out, st, _ = _direct(ras, entry, buf, off, nb, rows, p, 1, sampling=bad, ws_bytes=1 << 16)
            assert rv == _lib.SALVE_ERR_BAD_ARG and "sampling" in lib.salve_last_error().decode() and not out.any(), (entry, bad)
    with pytest.raises(_lib.SalveHipError, match="sampling"):
        ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, sampling="4:4:0")
    mcus = int(np.prod(jpeg.mcu_grid(p.h, p.w, "4:2:2")))
    with pytest.raises(_lib.SalveHipError, match="MCU range"):      # the wrapper counts in the sampling's MCUs: 4:2:0's count is too small a table ...
        ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=[(rows[0][0], rows[0][1], 0, 0, mcus + 1)], sampling="4:2:2")
    with pytest.raises(_lib.SalveHipError, match="tile"):
        ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=[(rows[0][0], rows[0][1], 0, 0, mcus // 2)], sampling="4:2:2")


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_a_malformed_scan_is_reported_and_its_neighbours_are_whole(ras, sampling):
    """The byte strings of jpeg_sampling_cases.malformed -- the ones the host build has passed under the sanitizers -- between two good
    images of the same header.  The table whose MCU range passes the image goes to the library directly: the wrapper refuses it."""
    good = sc.file_of(sampling, sc.MALFORMED_CASE)
    p = sc.parse(good)
    scan = good[p.scan_offset:p.scan_offset + p.scan_bytes]
    mcus = int(np.prod(jpeg.mcu_grid(p.h, p.w, sampling)))
    want = sc.pillow_reference(sampling, sc.MALFORMED_CASE)
    bad = {name: (b, rows) for name, b, rows in sc.malformed(sampling)}
    for name in ("cut_in_half", "noise_tail"):
        pieces = [scan, bad[name][0], scan]
        off = np.cumsum([0] + [len(x) + 3 for x in pieces[:-1]]).astype(np.int64)
        nb = np.array([len(x) for x in pieces], dtype=np.int64)
        blob = b"".join(x + b"\xee" * 3 for x in pieces) + b"\xee" * PAD
        buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)
        for entropy in ("lanes", "image"):
            img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy=entropy, sampling=sampling)
            st = st.cpu().numpy()
            assert st[0] == 0 and st[1] != 0 and st[2] == 0, (name, entropy, st)
            got = _rgb(img)
            assert np.array_equal(got[0], want) and np.array_equal(got[2], want), (name, entropy)
    _, b, rows = sc.malformed(sampling)[2]
    assert rows == [(0, len(scan), 0, 1, mcus)]
    blob = scan + scan + b"\xee" * PAD
    buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(DEV)
    table = [(0, len(scan), 0, 1, mcus), (len(scan), len(scan), 1, 0, mcus)]
    rv, out, st, _ = _direct(ras, "salve_bev_jpeg_decode_lanes_sampled", buf, None, None, table, p, 2, sampling=_lib.JPEG_SAMPLINGS[sampling])
    assert rv == _lib.SALVE_OK and st.tolist() == [dc.BAD_SLOT, 0]
    assert np.array_equal(_rgb(out)[1], want)
