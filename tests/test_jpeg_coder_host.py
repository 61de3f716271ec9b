"""The JPEG entropy coder on the host: the emulator of tests/jpeg_coder_cases.py against Pillow's files, byte for byte on every case;
the header and the Annex K tables of salve_amd/jpeg.py against the segments of Pillow's files; the rules of the coder that the case
table exercises, counted in the emulator's symbol stream; five plausible wrong variants that the table must tell from the real coder;
and the C ABI's additive entries.  No device.

Cases: the round trip's table (tests/jpeg_cases.py: 1 x 1, 8 x 8, 16 x 16, 15 x 17, 17 x 9, 33 x 47 at qualities 75, 30, 95 and
501 x 501 at 75, seven contents each), quality 100 (all table entries 1: the largest coefficients) on the three smallest shapes, and
crafted images: single high-frequency coefficients (ZRL runs, coefficient 63), black / white blocks (DC category 11, both signs),
black | white edges inside blocks (AC category 10), mid-frequency coefficients with long codes (0xFF bytes), and an 8 x 8 noise image
found by a search over seeds whose padded last byte is 0xFF (so the padding itself is stuffed)."""

import re
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_coder_cases as cc
from salve_amd import _lib, jpeg

PIL_Image = pytest.importorskip("PIL.Image")

ROOT = Path(__file__).resolve().parents[1]
CASES = cc.cases()
NEW = ("salve_bev_jpeg_encode_workspace_bytes", "salve_bev_jpeg_encode_max_bytes", "salve_bev_jpeg_encode")


def _id(case):
    return f"{case[0]}-{case[1]}x{case[2]}-q{case[3]}"


def _segments(data: bytes):
    """(marker, payload) of every segment in front of the scan, and the offset of the scan."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + length]))
        at += 2 + length
        if marker == 0xDA:
            return out, at


def test_the_case_table_is_the_one_the_tests_document():
    assert len(CASES) == len(set(CASES)) == len(jc.cases()) + 3 * 7 + 7
    assert set(jc.cases()) <= set(CASES)
    assert {(h, w) for c, h, w, q in CASES if q == 100 and c in jc.CONTENTS} == set(jc.SMALL_SIZES[:3])
    assert {c for c, *_ in CASES} == set(jc.CONTENTS) | set(cc.CRAFTED)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulator_file_equals_pillows_file(case):
    _, h, w, q = case
    pillow, scan, _ = cc.reference(case)
    assert jpeg.file_bytes(scan, h, w, q) == pillow


@pytest.mark.parametrize("h,w,q", [(1, 1, 75), (501, 501, 75), (300, 4000, 95), (4096, 7, 30)])
def test_header_equals_pillows(h, w, q):
    pillow = cc.pillow_file(np.zeros((h, w, 3), dtype=np.uint8), q)
    segs, scan_at = _segments(pillow)
    assert scan_at == jpeg.HEADER_BYTES == 623 and jpeg.file_header(h, w, q) == pillow[:623]
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert [len(p) + 2 for _, p in segs] == [16, 67, 67, 17, 31, 181, 31, 181, 12]
    assert pillow[-2:] == b"\xff\xd9"


def test_annex_k_tables_equal_the_dht_segments_of_a_pillow_file():
    segs, _ = _segments(cc.pillow_file(jc.make_image("noise", 16, 16), 75))
    dht = {p[0]: (tuple(p[1:17]), tuple(p[17:])) for m, p in segs if m == 0xC4}
    assert dht == {0x00: (jpeg.BITS_DC_LUMA, jpeg.HUFFVAL_DC_LUMA), 0x10: (jpeg.BITS_AC_LUMA, jpeg.HUFFVAL_AC_LUMA),
                   0x01: (jpeg.BITS_DC_CHROMA, jpeg.HUFFVAL_DC_CHROMA), 0x11: (jpeg.BITS_AC_CHROMA, jpeg.HUFFVAL_AC_CHROMA)}
    # the derived tables: code << 5 | length; prefix-free, the lengths' census is BITS, known corners of tables K.3 - K.6
    for codes, bits, vals in ((jpeg.DC_CODES[0], jpeg.BITS_DC_LUMA, jpeg.HUFFVAL_DC_LUMA), (jpeg.AC_CODES[1], jpeg.BITS_AC_CHROMA, jpeg.HUFFVAL_AC_CHROMA),
                              (jpeg.AC_CODES[0], jpeg.BITS_AC_LUMA, jpeg.HUFFVAL_AC_LUMA), (jpeg.DC_CODES[1], jpeg.BITS_DC_CHROMA, jpeg.HUFFVAL_DC_CHROMA)):
        assert sorted(np.flatnonzero(codes).tolist()) == sorted(vals)
        assert np.bincount(codes[codes > 0] & 31, minlength=17)[1:].tolist() == list(bits)
        words = sorted(format(int(e) >> 5, f"0{int(e) & 31}b") for e in codes[codes > 0])
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))
    entry = lambda t, s: (int(t[s]) >> 5, int(t[s]) & 31)   # noqa: E731
    assert entry(jpeg.AC_CODES[0], 0x00) == (0b1010, 4) and entry(jpeg.AC_CODES[0], 0xF0) == (0b11111111001, 11)
    assert entry(jpeg.AC_CODES[1], 0x00) == (0b00, 2) and entry(jpeg.AC_CODES[1], 0xF0) == (0b1111111010, 10)
    assert entry(jpeg.DC_CODES[0], 0) == (0b00, 2) and entry(jpeg.DC_CODES[0], 11) == (0b111111110, 9) and entry(jpeg.DC_CODES[1], 11) == (0b11111111110, 11)
    assert jpeg.ZIGZAG[:8].tolist() == [0, 1, 8, 16, 9, 2, 3, 10] and sorted(jpeg.ZIGZAG.tolist()) == list(range(64)) and jpeg.ZIGZAG[63] == 63


def test_the_table_exercises_every_rule_of_the_coder():
    stats = [cc.reference(c)[2] for c in CASES]
    assert any(s["zrl"] > 0 for s in stats) and max(s["max_zrl_in_a_row"] for s in stats) >= 2
    assert any(s["blocks_without_eob"] > 0 for s in stats)           # coefficient 63 non-zero
    assert any(s["zero_ac_blocks"] > 0 for s in stats)
    dc = set().union(*(s["dc_categories"] for s in stats))
    assert {0, 11} <= dc and set().union(*(s["dc_signs"] for s in stats)) == {1, -1}
    assert 10 in set().union(*(s["ac_categories"] for s in stats))
    assert any(s["stuffed"] > 0 for s in stats)
    assert {0, 7} <= {s["pad_bits"] for s in stats}
    # the padded last byte is itself 0xFF and is stuffed: the search over 8 x 8 noise images found seed jpeg_coder_cases.PADFF_SEED
    pillow, scan, st = cc.reference(("padff", 8, 8, 100))
    assert st["pad_byte"] == 0xFF and st["pad_bits"] > 0 and scan[-2:] == b"\xff\x00" and pillow[-4:] == b"\xff\x00\xff\xd9"
    # what the crafted images are for
    assert cc.reference(("zrl", 33, 47, 75))[2]["max_zrl_in_a_row"] == 3 and cc.reference(("zrl", 33, 47, 75))[2]["blocks_without_eob"] > 0
    assert 11 in cc.reference(("checker", 16, 16, 100))[2]["dc_categories"] and cc.reference(("checker", 16, 16, 100))[2]["dc_signs"] == {1, -1}
    assert 10 in cc.reference(("halfstep", 16, 16, 100))[2]["ac_categories"]
    heavy, noise = cc.reference(("ffheavy", 33, 47, 75)), cc.reference(("noise", 33, 47, 75))
    assert heavy[2]["stuffed"] / len(heavy[1]) > 4 * noise[2]["stuffed"] / len(noise[1])


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_a_wrong_variant_changes_at_least_one_case(mutant):
    small = [c for c in CASES if c[1] <= 47]
    changed = [c for c in small if cc.scan(cc.make_image(*c[:3]), c[3], mutant=mutant)[0] != cc.reference(c)[1]]
    assert changed, f"no case tells the '{mutant}' variant from libjpeg's coder"


def test_file_header_refuses_sizes_a_file_cannot_hold():
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        with pytest.raises(ValueError):
            jpeg.file_header(h, w, 75)
    assert len(jpeg.file_header(65535, 65535, 75)) == 623 and len(jpeg.file_header(1, 1, 1)) == 623
    assert jpeg.file_bytes(b"\x12\x34", 8, 8, 75) == jpeg.file_header(8, 8, 75) + b"\x12\x34\xff\xd9"


def test_abi_stays_7_and_the_new_symbols_are_declared_listed_exported_and_built():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    assert int(re.search(r"#define SALVE_HIP_ABI_VERSION (\d+)", header).group(1)) == _lib.EXPECTED_ABI == 7   # additive
    abi_comment = header[header.index("#define SALVE_HIP_ABI_VERSION"):header.index("/* Device status word")]
    assert "additive within 7" in abi_comment and "salve_bev_jpeg_encode" in abi_comment
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", header) and hasattr(lib, name), name


def test_size_queries():
    """(Host code only: the queries launch nothing.)  The bound is 2490 bytes per 16 x 16 MCU -- six blocks of at most 22 + 63 x 26
    bits, every byte stuffed -- rounded up to a multiple of 4, and holds the largest scan of the table at every shape."""
    lib = _lib.load()
    assert lib.salve_bev_jpeg_encode_max_bytes(16, 16) == 2492 and lib.salve_bev_jpeg_encode_max_bytes(1, 1) == 2492
    assert lib.salve_bev_jpeg_encode_max_bytes(17, 9) == 2 * 2490 and lib.salve_bev_jpeg_encode_max_bytes(501, 501) == 32 * 32 * 2490
    assert lib.salve_bev_jpeg_encode_max_bytes(4096, 4096) == 256 * 256 * 2490
    for h, w in {(h, w) for _, h, w, _ in CASES}:
        assert lib.salve_bev_jpeg_encode_max_bytes(h, w) >= max(len(cc.reference(c)[1]) for c in CASES if c[1:3] == (h, w))
    for bad in ((0, 8), (8, 0), (4097, 8), (8, 4097), (-1, 8)):
        assert lib.salve_bev_jpeg_encode_max_bytes(*bad) == 0, bad
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 4097, 8), (1, 8, 0), (1, 8, 4097)):
        assert lib.salve_bev_jpeg_encode_workspace_bytes(*bad) == 0, bad
    one, two = lib.salve_bev_jpeg_encode_workspace_bytes(1, 501, 501), lib.salve_bev_jpeg_encode_workspace_bytes(2, 501, 501)
    assert one % 16 == 0 and 6144 * 132 + 1024 * 1245 <= one <= 2_200_000 and 2 * one - 64 <= two <= 2 * one
    assert lib.salve_bev_jpeg_encode_workspace_bytes(65535, 4096, 4096) > 65535 * 393216 * 132
