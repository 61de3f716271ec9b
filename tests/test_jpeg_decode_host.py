"""The JPEG entropy decoder without a GPU: tests/jpeg_decode_cases.py's emulator against the coder's coefficients and Pillow's
pixels, its mutants, salve_amd.jpeg.parse_file, and the DEVICE's decoder (salve_amd/csrc/jpeg_entropy.h) compiled for the host as a
stand-alone program under AddressSanitizer and UBSan, on good and on hostile scans.

Single-bit flips: a flipped value bit leaves a well-formed scan that NO decoder can tell from an intended one.  So a flipped scan
must either be reported (a non-zero status word) or be well-formed by the emulator's judgement too, and then decode to the
emulator's coefficients: every flip that can be noticed is noticed, and the sanitizers see every one of them.
"""

import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_coder_cases as cc
import jpeg_decode_cases as dc
from salve_amd import jpeg
from salve_amd.utils import image_io

ROOT = Path(__file__).resolve().parents[1]
FIXTURES = sorted((ROOT / "tests" / "golden" / "renderings").rglob("*.jpg"))
GROUPS = sorted({(h, w, q) for _, h, w, q in cc.cases()})
OPTIMISED = [("noise", 33, 47, 75), ("disc", 33, 47, 75), ("zrl", 33, 47, 75), ("ffheavy", 33, 47, 75), ("checker", 16, 16, 100), ("noise", 1, 1, 75)]


def _optimised_file(case) -> bytes:
    c, h, w, q = case
    return dc.pillow_file(cc.make_image(c, h, w), quality=q, optimize=True)


def _mcus(p: jpeg.ParsedFile):
    return -(-p.h // 16), -(-p.w // 16)


# ---------------------------------------------------------------------------------------------------- the emulator
@pytest.mark.parametrize("h,w,q", GROUPS, ids=[f"{h}x{w}-q{q}" for h, w, q in GROUPS])
def test_emulator_gives_the_coders_coefficients_and_pillows_pixels(h, w, q):
    for case in (c for c in cc.cases() if c[1:] == (h, w, q)):
        pillow = cc.reference(case)[0]
        px, levels, status = dc.decode_file(pillow)
        assert status == 0, case
        assert np.array_equal(levels, cc.quantised_mcus(cc.make_image(case[0], h, w), jpeg.quality_tables(q))), case
        assert np.array_equal(px, dc.pillow_pixels(pillow)), case
        assert np.array_equal(px, jc.pillow_reference(case)) if case in jc.cases() else True


def test_emulator_on_the_fixture_files_and_on_optimised_tables():
    assert len(FIXTURES) == 4
    for f in FIXTURES:
        data = f.read_bytes()
        px, _, status = dc.decode_file(data)
        assert status == 0 and np.array_equal(px, dc.pillow_pixels(data)) and np.array_equal(px, image_io.read_rgb(str(f))), f.name
    for case in OPTIMISED:
        data = _optimised_file(case)
        p = jpeg.parse_file(data)
        assert not np.array_equal(p.huffman, dc.STANDARD_HUFFMAN), case   # tables of its own
        px, levels, status = dc.decode_file(data)
        assert status == 0 and np.array_equal(px, dc.pillow_pixels(data)), case
        assert np.array_equal(levels, cc.quantised_mcus(cc.make_image(*case[:3]), jpeg.quality_tables(case[3]))), case


def test_the_case_table_tells_every_mutant_from_the_decoder():
    alive = set(dc.MUTANTS)
    for case in cc.cases():
        if case[1:3] == jc.PRODUCT_SIZE or not alive:
            continue
        pillow = cc.reference(case)[0]
        want = dc.decode_file(pillow)[1]
        for m in sorted(alive):
            _, levels, status = dc.decode_file(pillow, mutant=m)
            if status != 0 or not np.array_equal(levels, want):
                alive.discard(m)
    assert not alive


def test_emulator_reports_malformed_scans():
    pillow = cc.reference(("noise", 16, 16, 75))[0]
    p = jpeg.parse_file(pillow)
    scan = pillow[p.scan_offset:p.scan_offset + p.scan_bytes]
    assert dc.decode(scan, p.huffman, 1, 1)[1] == 0
    assert dc.decode(scan[:-1], p.huffman, 1, 1)[1] != 0
    assert dc.decode(b"", p.huffman, 1, 1)[1] & dc.TRUNCATED
    assert dc.decode(scan + b"\xff\xff", p.huffman, 1, 1)[1] != 0
    assert dc.decode(scan + b"\x00", p.huffman, 1, 1)[1] & dc.LEFTOVER
    assert dc.decode(b"\xff" * 64, p.huffman, 1, 1)[1] & dc.MARKER


# ---------------------------------------------------------------------------------------------------- parse_file
def test_parse_file_returns_the_fields_of_pillows_files():
    for case in [("disc", 33, 47, 75), ("noise", 1, 1, 30), ("layout", 501, 501, 75), ("noise", 17, 9, 95)]:
        c, h, w, q = case
        data = cc.reference(case)[0]
        p = jpeg.parse_file(data)
        assert (p.h, p.w) == (h, w) and p.scan_offset == jpeg.HEADER_BYTES and p.scan_offset + p.scan_bytes + 2 == len(data)
        assert p.header_key == jpeg.file_header(h, w, q) == data[:p.scan_offset]
        assert p.qtab.dtype == np.uint16 and np.array_equal(p.qtab, jpeg.quality_tables(q))
        assert p.huffman.dtype == np.uint8 and np.array_equal(p.huffman, dc.STANDARD_HUFFMAN)
        assert data[p.scan_offset:p.scan_offset + p.scan_bytes] == cc.reference(case)[1]
    for f in FIXTURES:
        p = jpeg.parse_file(f.read_bytes())
        assert (p.h, p.w, p.scan_offset) == (501, 501, 623) and np.array_equal(p.qtab, jpeg.quality_tables(75))
        assert p.header_key == jpeg.file_header(501, 501, 75)
    a, b = (jpeg.parse_file(_optimised_file(c)) for c in OPTIMISED[:2])
    assert a.header_key != b.header_key and a.scan_offset != jpeg.HEADER_BYTES   # tables of their own: a group each


def test_parse_file_does_not_assume_the_layout():
    """A comment segment, fill bytes in front of a marker, and both quantisation tables in ONE DQT segment."""
    data = cc.reference(("disc", 33, 47, 75))[0]
    want = jpeg.parse_file(data)
    com = b"\xff\xfe\x00\x07hello"
    moved = data[:2] + com + b"\xff" + data[2:]
    p = jpeg.parse_file(moved)
    assert p.scan_offset == want.scan_offset + len(com) + 1 and p.scan_bytes == want.scan_bytes
    assert np.array_equal(p.qtab, want.qtab) and np.array_equal(p.huffman, want.huffman)
    at = data.index(b"\xff\xdb")
    merged = data[:at] + b"\xff\xdb\x00\x84" + data[at + 4:at + 69] + data[at + 73:at + 138] + data[at + 138:]
    p = jpeg.parse_file(merged)
    assert np.array_equal(p.qtab, want.qtab) and p.scan_bytes == want.scan_bytes


def test_parse_file_refuses_what_the_device_does_not_decode():
    from PIL import Image

    rgb = jc.make_image("disc", 33, 47)

    def saved(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", **kw)
        return buf.getvalue()

    for data, word in ((saved(rgb, progressive=True), "progressive"), (saved(rgb[..., 0]), "component"), (saved(rgb, subsampling=0), "sampling"),
                       (saved(rgb, restart_marker_blocks=4), "restart")):
        with pytest.raises(jpeg.Unsupported, match=word):
            jpeg.parse_file(data)
    good = saved(rgb)
    p = jpeg.parse_file(good)
    for cut in list(range(0, p.scan_offset, 7)) + [p.scan_offset - 1]:   # truncated headers
        with pytest.raises(jpeg.Unsupported):
            jpeg.parse_file(good[:cut])
    with pytest.raises(jpeg.Unsupported, match="EOI"):
        jpeg.parse_file(good[:-2])
    with pytest.raises(jpeg.Unsupported, match="EOI"):
        jpeg.parse_file(good[:-1])
    with pytest.raises(jpeg.Unsupported, match="inside the scan"):          # a further scan / a stray marker
        jpeg.parse_file(good[:-2] + b"\xff\xda\x00\x02" + good[-2:])
    at = good.index(b"\xff\xdb")
    with pytest.raises(jpeg.Unsupported, match="16-bit"):
        jpeg.parse_file(good[:at + 4] + b"\x10" + good[at + 5:])
    at = good.index(b"\xff\xc0")
    with pytest.raises(jpeg.Unsupported, match="12-bit"):
        jpeg.parse_file(good[:at + 4] + b"\x0c" + good[at + 5:])
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse_file(b"")
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse_file(b"\x89PNG\r\n\x1a\n" + bytes(64))
    assert issubclass(jpeg.Unsupported, ValueError)


# ---------------------------------------------------------------------------------------------------- the device's decoder on the host
@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpeg_decode_host") / "jpeg_decode_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "jpeg_decode_host.cpp")], check=True)

    def run(cases):
        """[(huffman uint8 [4, 272], mcus, scan bytes)] -> [(status, int16 [mcus, 6, 64])]; the program must end with status 0."""
        work = exe.parent
        with open(work / "in.bin", "wb") as f:
            f.write(np.int32(len(cases)).tobytes())
            for huffman, mcus, scan in cases:
                f.write(np.ascontiguousarray(huffman, dtype=np.uint8).tobytes())
                f.write(np.array([mcus, len(scan)], dtype=np.int32).tobytes())
                f.write(bytes(scan))
        done = subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-4000:]
        raw = (work / "out.bin").read_bytes()
        out, at = [], 0
        for _, mcus, _ in cases:
            status = int(np.frombuffer(raw, dtype=np.uint32, count=1, offset=at)[0])
            out.append((status, np.frombuffer(raw, dtype=np.int16, count=mcus * 384, offset=at + 4).reshape(mcus, 6, 64)))
            at += 4 + mcus * 768
        assert at == len(raw)
        return out

    return run


def _scan_case(data: bytes):
    p = jpeg.parse_file(data)
    mh, mw = _mcus(p)
    return p.huffman, mh * mw, data[p.scan_offset:p.scan_offset + p.scan_bytes]


def test_host_build_equals_the_emulator_on_good_scans(host_decoder):
    files = [cc.reference(c)[0] for c in cc.cases() if c[1:3] != jc.PRODUCT_SIZE or c[0] == "noise"]
    files += [f.read_bytes() for f in FIXTURES] + [_optimised_file(c) for c in OPTIMISED]
    got = host_decoder([_scan_case(d) for d in files])
    for data, (status, coef) in zip(files, got):
        _, levels, want_status = dc.decode_file(data)
        assert status == 0 == want_status
        assert np.array_equal(coef.reshape(levels.shape), levels)


def test_host_build_survives_hostile_scans_and_reports_them(host_decoder):
    pillow = cc.reference(("noise", 16, 16, 75))[0]
    huffman, mcus, scan = _scan_case(pillow)
    assert mcus == 1 and len(scan) > 100
    hostile = [scan[:k] for k in range(len(scan))]                      # every proper prefix, the empty scan (scan_bytes = 0) among them
    hostile += [b"\xff" * len(scan), b"\x00" * len(scan), b"\xff" * 5000, b"\x00" * 5000, scan + scan, scan + b"\xff\xd9"]
    for status, _ in host_decoder([(huffman, mcus, s) for s in hostile]):
        assert status != 0
    for status, _ in host_decoder([(huffman, 7, s) for s in hostile]):   # more MCUs asked for than any of them holds
        assert status != 0
    rng = np.random.RandomState(5)
    flipped = []
    for at in rng.choice(8 * len(scan), size=200, replace=False):
        s = bytearray(scan)
        s[at >> 3] ^= 0x80 >> (at & 7)
        flipped.append(bytes(s))
    got = host_decoder([(huffman, mcus, s) for s in flipped])
    reported = 0
    for s, (status, coef) in zip(flipped, got):
        levels, want_status = dc.decode(s, huffman, 1, 1)
        assert (status != 0) == (want_status != 0)
        if status == 0:   # a flip that left a well-formed scan (a value bit): decoded as what it now says
            assert np.array_equal(coef.reshape(levels.shape), levels)
        reported += status != 0
    assert 0 < reported < 200
    # a larger image: flips and cuts of a fixture file's scan (several staged chunks, many MCUs)
    huffman, mcus, scan = _scan_case(FIXTURES[0].read_bytes())
    big = [scan[:len(scan) // 2], scan[:4097], scan[:4096], scan[:4095]]
    for at in rng.choice(8 * len(scan), size=6, replace=False):
        s = bytearray(scan)
        s[at >> 3] ^= 0x80 >> (at & 7)
        big.append(bytes(s))
    got = host_decoder([(huffman, mcus, s) for s in big])
    assert all(status != 0 for status, _ in got[:4])


def test_host_build_refuses_tables_that_oversubscribe_the_code_space(host_decoder):
    bad = dc.STANDARD_HUFFMAN.copy()
    bad[1, 0] = 3   # three codes of length 1
    with pytest.raises(AssertionError, match="refused"):
        host_decoder([(bad, 1, b"\x00" * 8)])
