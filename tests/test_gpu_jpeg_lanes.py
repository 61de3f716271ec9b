"""salve_bev_jpeg_decode_lanes on the MI355X: on every case of tests/jpeg_lanes_cases.py the lane-parallel entropy stage leaves the
serial stage's coefficients in the workspace (the emulator's, for files with restart intervals, which the serial stage refuses),
Pillow's pixels and a zero status; a mixed batch of 70 images at odd byte offsets; restart and plain files in one call; run-to-run
and stream identity; hostile scans between good neighbours (only scans tests/test_jpeg_lanes_host.py has put through the host build
of the same decoder under the sanitizers) reported exactly where the serial stage reports them; the refusals."""

import ctypes

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_coder_cases as cc
import jpeg_decode_cases as dc
import jpeg_lanes_cases as lc

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
    """Whole files laid out one behind the other (gaps[i] filler bytes in front of file i), the padding behind the last ->
    (uint8 device tensor, scan offsets, scan lengths, segment rows, the first file's ParsedFile).  The files share size and tables."""
    gaps = [0] * len(files) if gaps is None else gaps
    buf, off, nb, rows, first = bytearray(), [], [], [], None
    for i, (f, g) in enumerate(zip(files, gaps)):
        p = jpeg.parse_file(f, restart=True)
        first = first or p
        assert (p.h, p.w) == (first.h, first.w) and np.array_equal(p.qtab, first.qtab) and np.array_equal(p.huffman, first.huffman)
        buf += b"\xee" * g
        base = len(buf) - p.scan_offset
        buf += f[p.scan_offset:p.scan_offset + p.scan_bytes]
        off.append(base + p.scan_offset)
        nb.append(p.scan_bytes)
        rows += [(base + o, n, i, m0, mc) for o, n, m0, mc in p.segments]
    buf += b"\xee" * PAD
    dev = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(DEV)
    return dev, np.array(off, dtype=np.int64), np.array(nb, dtype=np.int64), rows, first


def _coefficients(ras, n, h, w):
    """The coefficients the last entropy stage left in the current stream's workspace: int16 [n, MCUs, 6, 64]."""
    Hm, Wm = -(-h // 16) * 16, -(-w // 16) * 16
    mcus = Hm * Wm // 256
    ws = ras._jpeg_ws[torch.cuda.current_stream(DEV).cuda_stream]
    at = n * Hm * Wm * 3 // 2
    return ws[at:at + n * mcus * 768].cpu().numpy().view(np.int16).reshape(n, mcus, 6, 64)


def _lanes(ras, files, gaps=None, **kw):
    buf, off, nb, rows, p = _pack(files, gaps)
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=rows, **kw)
    return jc.unpack_bgr(img.cpu().numpy().view(np.uint32)), st.cpu().numpy()


def test_the_subsequence_size_is_the_headers(ras):
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parents[1] / "salve_amd" / "csrc" / "jpeg_entropy_lanes.h").read_text()
    assert ras.lib.salve_bev_jpeg_subseq_bytes() == int(re.search(r"#define JE_SUBSEQ (\d+)", text).group(1))


@pytest.mark.parametrize("name", lc.cases())
def test_coefficients_pixels_and_status_on_every_case(ras, name):
    data = lc.file_of(name)
    buf, off, nb, rows, p = _pack([data], gaps=[1])
    out = torch.full((1, p.h, p.w), 0x00ABCDEF, dtype=torch.int32, device=DEV)
    _, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, out=out, entropy="lanes", segments=rows, stages=_lib.JPEG_STAGE_ENTROPY)
    got = _coefficients(ras, 1, p.h, p.w)
    assert bool((out == 0x00ABCDEF).all()) and st.cpu().numpy().tolist() == [0]
    if len(rows) == 1 and not name.startswith("restart"):        # the serial stage on the same bytes
        _, st_serial = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, out=out, stages=_lib.JPEG_STAGE_ENTROPY)
        assert st_serial.cpu().numpy().tolist() == [0]
        assert np.array_equal(got, _coefficients(ras, 1, p.h, p.w))
    else:                                                         # (it refuses restart intervals) the emulator, interval by interval
        assert np.array_equal(got.reshape(-1), lc.reference_levels(data)[0].reshape(-1))
    img, st = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=rows)
    assert st.cpu().numpy().tolist() == [0]
    assert np.array_equal(jc.unpack_bgr(img.cpu().numpy().view(np.uint32))[0], dc.pillow_pixels(data))
    ras.check("jpeg_decode(entropy='lanes')")


def test_default_segments_are_one_per_image(ras):
    files = [cc.reference((c, 33, 47, 75))[0] for c in ("noise", "disc", "zrl")]
    buf, off, nb, rows, p = _pack(files, gaps=[1, 3, 5])
    a, sa = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes")
    b, sb = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=rows)
    c, sc = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    assert torch.equal(a, b) and torch.equal(a, c) and not sa.any() and not sb.any() and not sc.any()
    seg = np.zeros(3, dtype=_lib.JPEG_SEGMENT_DTYPE)
    for k, name in enumerate(_lib.JPEG_SEGMENT_DTYPE.names):
        seg[name] = [r[k] for r in rows]
    d, sd = ras.jpeg_decode(buf, off, nb, p.h, p.w, p.qtab, p.huffman, entropy="lanes", segments=seg)
    assert torch.equal(a, d) and not sd.any()


def test_mixed_batch_of_70_at_odd_offsets_equals_one_image_per_call(ras):
    h, w, q = 33, 47, 75
    contents = jc.CONTENTS + ("zrl", "ffheavy", "checker")
    images = [cc.make_image(contents[i % len(contents)], h, w, seed=i // len(contents)) for i in range(70)]
    files = [cc.pillow_file(img, q) for img in images]
    assert len({len(f) for f in files}) > 10
    gaps = [1 + 2 * (i % 5) for i in range(70)]      # every scan starts at an odd offset or right behind an odd-sized neighbour
    got, status = _lanes(ras, files, gaps)
    assert not status.any()
    for i in range(70):
        one, st = _lanes(ras, [files[i]])
        assert st[0] == 0 and np.array_equal(one[0], got[i]), i
        assert np.array_equal(got[i], dc.pillow_pixels(files[i])), i


def test_restart_and_plain_files_in_one_call(ras):
    h, w = 48, 64
    files = []
    for i, kw in enumerate((dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=5), dict(), dict(restart_marker_rows=1), dict(restart_marker_blocks=100))):
        files.append(dc.pillow_file(jc.make_image(("noise", "disc")[i % 2], h, w, seed=i), quality=75, **kw))
    buf, off, nb, rows, p = _pack(files, gaps=[1, 0, 3, 5, 0, 7])
    assert [sum(1 for r in rows if r[2] == i) for i in range(6)] == [1, 12, 3, 1, 3, 1]
    got, status = _lanes(ras, files, gaps=[1, 0, 3, 5, 0, 7])
    assert not status.any()
    for i, f in enumerate(files):
        assert np.array_equal(got[i], dc.pillow_pixels(f)), i


def test_run_to_run_and_stream_identity(ras):
    files = [dc.pillow_file(jc.make_image("noise", 160, 160, seed=i), quality=90, **kw) for i, kw in enumerate((dict(), dict(restart_marker_rows=2), dict(), dict()))]
    buf, off, nb, rows, p = _pack(files)
    args = (buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    a, sa = ras.jpeg_decode(*args, entropy="lanes", segments=rows)
    b, sb = ras.jpeg_decode(*args, entropy="lanes", segments=rows)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c, sc = ras.jpeg_decode(*args, entropy="lanes", segments=rows)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(sa, sb) and torch.equal(sa, sc) and not sa.any()
    assert np.array_equal(jc.unpack_bgr(a.cpu().numpy().view(np.uint32))[1], dc.pillow_pixels(files[1]))


def test_the_two_stages_called_apart_equal_the_whole_call(ras):
    files = [lc.file_of("size_48x64"), lc.file_of("restart_blocks7"), lc.file_of("restart_longer_than_image")]
    buf, off, nb, rows, p = _pack(files)
    rows[2] = rows[2][:1] + (rows[2][1] // 3,) + rows[2][2:]            # one malformed interval: its image's status comes from the entropy stage
    args = (buf, off, nb, p.h, p.w, p.qtab, p.huffman)
    whole, st = ras.jpeg_decode(*args, entropy="lanes", segments=rows)
    out = torch.full((3, p.h, p.w), 0x00ABCDEF, dtype=torch.int32, device=DEV)
    _, st_e = ras.jpeg_decode(*args, out=out, entropy="lanes", segments=rows, stages=_lib.JPEG_STAGE_ENTROPY)
    assert bool((out == 0x00ABCDEF).all()) and torch.equal(st_e, st)
    assert [int(v) != 0 for v in st.cpu().numpy()] == [False, True, False]
    ras.jpeg_decode(*args, out=out, entropy="lanes", segments=rows, stages=_lib.JPEG_STAGE_INVERSE)
    assert torch.equal(out, whole)
    assert np.array_equal(jc.unpack_bgr(whole.cpu().numpy().view(np.uint32))[2], dc.pillow_pixels(files[2]))


def _between_good_neighbours(ras, good_file, hostile):
    """good, hostile[0], good, hostile[1], ..., good in ONE call through both entropy stages -> (lanes pixels, lanes status, serial status)."""
    p = jpeg.parse_file(good_file)
    good = good_file[p.scan_offset:p.scan_offset + p.scan_bytes]
    scans = [good]
    for s in hostile:
        scans += [s, good]
    blob, off = bytearray(), []
    for i, s in enumerate(scans):
        blob += b"\xee" * (i % 3)
        off.append(len(blob))
        blob += s
    blob += b"\xee" * PAD
    buf = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(DEV)
    nb = np.array([len(s) for s in scans], dtype=np.int64)
    args = (buf, np.array(off, dtype=np.int64), nb, p.h, p.w, p.qtab, p.huffman)
    img, st = ras.jpeg_decode(*args, entropy="lanes")
    again, st2 = ras.jpeg_decode(*args, entropy="lanes")
    assert torch.equal(img, again) and torch.equal(st, st2)              # a failing image's pixels are deterministic too
    _, serial = ras.jpeg_decode(*args)
    return jc.unpack_bgr(img.cpu().numpy().view(np.uint32)), st.cpu().numpy(), serial.cpu().numpy()


def test_hostile_scans_report_and_leave_their_neighbours_alone(ras):
    small = lc.hostile_small()
    n = jpeg.parse_file(lc.file_of("one_mcu")).scan_bytes
    hostile = small[:n:6] + small[n:n + 40] + small[n + 200:]            # prefixes (the empty scan first), 40 of the flips, the fixed ones
    good = lc.file_of("one_mcu")
    got, st, serial = _between_good_neighbours(ras, good, hostile)
    want = dc.pillow_pixels(good)
    assert not st[0::2].any() and not serial[0::2].any()
    for i in range(0, len(st), 2):
        assert np.array_equal(got[i], want), i
    assert [int(v) != 0 for v in st[1::2]] == [int(v) != 0 for v in serial[1::2]]
    reported = int((st[1::2] != 0).sum())
    assert len(hostile) - 40 <= reported <= len(hostile)                 # every prefix and fixed one; a flip of a value bit leaves a well-formed scan
    assert st[1] & dc.TRUNCATED and (got[1] == 128).all()                # the empty scan: all-zero coefficients, mid grey
    ras.check("jpeg_decode(entropy='lanes') of malformed scans")         # the device status word is clean: bad files are the images' own business


def test_hostile_scans_of_many_chunks(ras):
    good = lc.file_of("size_501x501")
    got, st, serial = _between_good_neighbours(ras, good, lc.hostile_large())
    want = dc.pillow_pixels(good)
    assert not st[0::2].any()
    for i in range(0, len(st), 2):
        assert np.array_equal(got[i], want), i
    assert [int(v) != 0 for v in st[1::2]] == [int(v) != 0 for v in serial[1::2]] and all(int(v) != 0 for v in st[1:12:2])


def test_refusals(ras):
    lib = ras.lib
    files = [lc.file_of("restart_blocks7"), lc.file_of("size_48x64")]
    buf, off, nb, rows, p = _pack(files)
    n, h, w = 2, p.h, p.w
    mcus = 12
    seg = np.zeros(4, dtype=_lib.JPEG_SEGMENT_DTYPE)
    for k, name in enumerate(_lib.JPEG_SEGMENT_DTYPE.names):
        seg[name][:3] = [r[k] for r in rows]
    seg_d = torch.from_numpy(seg.view(np.uint8)).to(DEV)
    qt, hf = np.ascontiguousarray(p.qtab), np.ascontiguousarray(p.huffman)
    need = lib.salve_bev_jpeg_decode_lanes_workspace_bytes(n, h, w, 3)
    assert need == lib.salve_bev_jpeg_decode_workspace_bytes(n, h, w) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((n, h, w), dtype=torch.int32, device=DEV)
    status = torch.empty(n, dtype=torch.int32, device=DEV)

    def call(scans=buf.data_ptr(), size=buf.numel(), seg_ptr=seg_d.data_ptr(), n_seg=3, n=n, h=h, w=w, q=qt, huff=hf, out_ptr=out.data_ptr(),
             st_ptr=status.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need, stages=_lib.JPEG_STAGES_ALL):
        qp = None if q is None else q.ctypes.data_as(ctypes.c_void_p)
        hp = None if huff is None else huff.ctypes.data_as(ctypes.c_void_p)
        return lib.salve_bev_jpeg_decode_lanes(ctypes.c_void_p(scans), size, ctypes.c_void_p(seg_ptr), n_seg, n, h, w, qp, hp, ctypes.c_void_p(out_ptr),
                                               ctypes.c_void_p(st_ptr), ctypes.c_void_p(ws_ptr), ws_bytes, stages, None)

    assert call() == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, 0]
    for kw in (dict(scans=0), dict(seg_ptr=0), dict(q=None), dict(huff=None), dict(out_ptr=0), dict(st_ptr=0), dict(ws_ptr=0),          # salve_bev_jpeg_decode's
               dict(n=0), dict(n=-1), dict(n=65536, n_seg=65536), dict(h=0), dict(h=4097), dict(w=0), dict(w=4097), dict(size=15),
               dict(out_ptr=out.data_ptr() + 2), dict(st_ptr=status.data_ptr() + 1), dict(ws_ptr=ws.data_ptr() + 8), dict(ws_bytes=need - 1),
               dict(ws_bytes=0), dict(stages=0), dict(stages=4),
               dict(n_seg=1), dict(n_seg=0), dict(n_seg=-1), dict(n_seg=(1 << 24) + 1), dict(seg_ptr=seg_d.data_ptr() + 4)):           # and its own
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != ""
    for args in ((0, h, w, 1), (n, h, w, 1), (n, h, w, (1 << 24) + 1), (n, 0, w, 2), (n, h, 4097, 2)):
        assert lib.salve_bev_jpeg_decode_lanes_workspace_bytes(*args) == 0
    # what the kernel makes of a table that lies (the wrapper refuses these; tests/test_jpeg_lanes_host.py has run them under the sanitizers):
    # a segment outside the image or the buffer decodes nothing and reports its image, one without an image is ignored
    lies = seg.copy()
    lies[1]["mcu_count"] += 1                     # image 0's second interval passes the image's end
    lies[3] = (0, 4, 7, 0, 1)                     # an image that is not there
    lies_d = torch.from_numpy(lies.view(np.uint8)).to(DEV)
    assert call(seg_ptr=lies_d.data_ptr(), n_seg=4) == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [dc.BAD_SLOT, 0]
    assert np.array_equal(jc.unpack_bgr(out.cpu().numpy().view(np.uint32))[1], dc.pillow_pixels(files[1]))
    lies = seg.copy()
    lies[2]["bytes"] = buf.numel()                # passes the buffer's end
    lies_d = torch.from_numpy(lies.view(np.uint8)).to(DEV)
    assert call(seg_ptr=lies_d.data_ptr()) == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0, dc.BAD_SLOT]
    # the wrapper's refusals
    args = (buf, off, nb, h, w, p.qtab, p.huffman)

    def rows_with(k, **change):
        names = _lib.JPEG_SEGMENT_DTYPE.names
        r = [list(x) for x in rows]
        for key, v in change.items():
            r[k][names.index(key)] = v
        return r

    for bad, word in ((rows_with(2, image=2), "outside"), (rows_with(0, image=-1), "outside"),
                      (rows_with(1, mcu_count=6), "MCU range"), (rows_with(1, first_mcu=-1), "MCU range"), (rows_with(2, mcu_count=0), "MCU range"),
                      (rows_with(1, first_mcu=6, mcu_count=5), "tile"), (rows_with(1, first_mcu=8, mcu_count=4), "tile"),      # an overlap, a gap
                      (rows_with(2, mcu_count=11), "tile"), ([rows[1], rows[0], rows[2]], "tile"), ([rows[2], rows[0], rows[1]], "tile"),
                      (rows[:2] + [rows[1]] + rows[2:], "tile"), (rows[:1], "segments for"), (rows[:2], "tile"), (rows[1:], "tile"),
                      (rows_with(2, bytes=buf.numel()), "padding"), (rows_with(0, offset=-1), "padding")):
        with pytest.raises(_lib.SalveHipError, match=word):
            ras.jpeg_decode(*args, entropy="lanes", segments=bad)
    with pytest.raises(_lib.SalveHipError, match="entropy"):
        ras.jpeg_decode(*args, entropy="subsequence")
    with pytest.raises(_lib.SalveHipError, match="lanes"):
        ras.jpeg_decode(*args, segments=rows)
    with pytest.raises(_lib.SalveHipError, match="padding"):
        ras.jpeg_decode(buf[:-1], off, nb, h, w, p.qtab, p.huffman, entropy="lanes")
    img, st = ras.jpeg_decode(buf, off[:0], nb[:0], h, w, p.qtab, p.huffman, entropy="lanes")
    assert img.shape == (0, h, w) and st.shape == (0,)
    # parse_file(data) still sends files with restart intervals to the host
    with pytest.raises(jpeg.Unsupported, match="restart"):
        jpeg.parse_file(files[0])


# ---------------------------------------------------------------------------------------------------- the tile-file route
@pytest.fixture(scope="module")
def restart_data_root(tmp_path_factory):
    """tests/test_gpu_train_files.py's small data set with two of its files rewritten with restart intervals."""
    from PIL import Image

    from salve_amd.utils import image_io
    from tests.test_gpu_train_files import _write_dataset

    root = _write_dataset(tmp_path_factory.mktemp("tiles_restart") / "bev")
    victims = sorted((root / "incorrect_alignment" / "1208").glob("*.jpg"))[:2]
    for k, victim in enumerate(victims):
        Image.fromarray(image_io.read_rgb(str(victim))).save(str(victim), format="JPEG", quality=75, **(dict(restart_marker_rows=2), dict(restart_marker_blocks=100))[k])
        with pytest.raises(jpeg.Unsupported, match="restart"):
            jpeg.parse_file(victim.read_bytes())
    return root


def test_tile_file_batches_equal_the_serial_routes_and_restart_files_stay_on_the_device(restart_data_root):
    from salve_amd.dataset.zind_data import ZindData
    from salve_amd.train_files import TileFileLoader, TileFileSource
    from tests.test_gpu_train_files import config

    args = config(restart_data_root)
    data = ZindData(split="train", transform=None, args=args)
    idx, draws = np.array([0, 1, 2]), [(1, 2, True, False), (3, 4, False, False), (9, 9, False, True)]
    with TileFileSource(DEV, data.data_list, batch_size=3, split="train") as serial, \
            TileFileSource(DEV, data.data_list, batch_size=3, split="train", entropy="lanes") as lanes:
        x0, y0 = serial.batch(idx, draws)
        x1, y1 = lanes.batch(idx, draws)
        assert torch.equal(x0, x1) and torch.equal(y0, y1)
        assert serial.fallbacks == 2 and lanes.fallbacks == 0           # Pillow took the restart files there, the device here
        serial._check_epoch("test")
        lanes._check_epoch("test")
    size = (args.resize_h, args.resize_w), (args.train_h, args.train_w)
    with TileFileLoader(DEV, data.data_list, 2, *size) as serial, TileFileLoader(DEV, data.data_list, 2, *size, entropy="lanes") as lanes:
        for a, b in zip(serial, lanes):
            assert all(torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v for u, v in zip(a, b))
        assert serial.fallbacks == 2 and lanes.fallbacks == 0
    with pytest.raises(ValueError, match="entropy"):
        TileFileSource(DEV, data.data_list, entropy="subsequence")


def test_the_entropy_argument_reaches_the_loaders(restart_data_root):
    from salve_amd import train_utils, training
    from salve_amd.train_files import TileFileLoader
    from tests.test_gpu_train_files import config

    args = config(restart_data_root)
    loader = train_utils.get_dataloader(args, "val", decode="device", entropy="lanes")
    assert isinstance(loader, TileFileLoader) and loader.entropy == "lanes"
    assert train_utils.get_dataloader(args, "val", decode="device").entropy == "image"
    with training.get_tile_file_source(args, "val", entropy="lanes") as src:
        assert src.entropy == "lanes"
    with pytest.raises(ValueError, match="decode"):
        train_utils.get_dataloader(args, "val", entropy="lanes")
    with pytest.raises(ValueError, match="decode"):
        training.train(args, "unused", entropy="lanes")
