"""The lane-parallel JPEG entropy decoder without a GPU: salve_amd/csrc/jpeg_entropy_lanes.h compiled for the host as a stand-alone
program under AddressSanitizer and UBSan, at subsequences of 4 and 16 bytes and of the device's size, against
tests/jpeg_decode_cases.py's emulator on every case of tests/jpeg_lanes_cases.py and against the serial decoder of jpeg_entropy.h
on hostile scans; the case table's properties; tests/jpeg_lanes_cases.py's emulator of the three passes and its wrong variants;
salve_amd.jpeg.parse_file(restart=True).
"""

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_lanes_cases as lc
from salve_amd import jpeg

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "salve_amd" / "csrc" / "jpeg_entropy_lanes.h"
DEVICE_SUBSEQ = int(re.search(r"#define JE_SUBSEQ (\d+)", HEADER.read_text()).group(1))
LANES = int(re.search(r"#define JL_LANES (\d+)", HEADER.read_text()).group(1))
SUBSEQS = sorted({4, 16, DEVICE_SUBSEQ})
SEGMENT = np.dtype([("offset", "<i8"), ("bytes", "<i4"), ("image", "<i4"), ("first_mcu", "<i4"), ("mcu_count", "<i4")])
SMALL = [c for c in lc.cases() if c not in ("size_501x501", "size_1024x2048")]


def test_the_device_subsequence_is_the_one_the_seeds_were_found_for():
    assert DEVICE_SUBSEQ == lc.SUBSEQ and SEGMENT.itemsize == 24


# ---------------------------------------------------------------------------------------------------- the case table
def _scan(name):
    data = lc.file_of(name)
    p = jpeg.parse_file(data, restart=True)
    return p, data[p.scan_offset:p.scan_offset + p.scan_bytes]


def test_every_case_parses_and_the_emulators_agree_with_pillow():
    assert len(set(lc.cases())) == len(lc.cases())
    for name in SMALL:
        data = lc.file_of(name)
        p = jpeg.parse_file(data, restart=True)
        levels, status = lc.reference_levels(data)
        assert status == 0, name
        assert np.array_equal(dc.pixels(levels, p.qtab, p.h, p.w), dc.pillow_pixels(data)), name
    sizes = {(jpeg.parse_file(lc.file_of(f"size_{h}x{w}")).h, jpeg.parse_file(lc.file_of(f"size_{h}x{w}")).w) for h, w in lc.SIZES}
    assert sizes == set(lc.SIZES) == {(16, 16), (17, 33), (48, 64), (501, 501), (1024, 2048)}


def test_the_length_cases_have_their_lengths():
    S = DEVICE_SUBSEQ
    assert 0 < _scan("short")[0].scan_bytes < S
    for k in (1, 2, 3):
        assert _scan(f"exact{k}")[0].scan_bytes == k * S
    assert _scan("size_501x501")[0].scan_bytes > 2 * LANES * S      # three chunks
    assert _scan("size_1024x2048")[0].scan_bytes > 8 * LANES * S
    assert _scan("size_1024x2048")[0].scan_bytes > 200_000


def test_flat_q5_packs_hundreds_of_blocks_into_a_subsequence():
    """Every block is a DC code and an EOB, 32 bits per MCU: 192 blocks per 128 bytes, 2400 blocks in all."""
    p, scan = _scan("flat_q5")
    tr = lc.trace(scan, p.huffman, 400)
    assert len(tr) == 2 * 2400
    first = {}
    for a, _, _, blk in tr:
        first.setdefault(blk, a // (8 * DEVICE_SUBSEQ))
    per = np.bincount(list(first.values()))
    assert per.max() >= 192 and per[:-1].min() >= 190


def _block_spans(name, mcus):
    p, scan = _scan(name)
    lo, hi = {}, {}
    for a, _, c, blk in lc.trace(scan, p.huffman, mcus):
        lo.setdefault(blk, a)
        hi[blk] = c
    return [(lo[b], hi[b]) for b in sorted(lo)]


def test_a_block_spans_three_subsequences():
    """Quality 100 on noise gives the longest blocks an 8-bit image has -- under 128 bytes, so they straddle one boundary at most; the
    hand-made "long_block" (63 coefficients of 17 bits) begins in the first subsequence and ends in the third: the second lane
    completes no block."""
    S8 = 8 * DEVICE_SUBSEQ
    spans = _block_spans("noise_q100", 9)
    assert 8 * 80 < max(b - a for a, b in spans) < S8 and any(a // S8 != (b - 1) // S8 for a, b in spans)
    assert any(a // S8 == 0 and (b - 1) // S8 == 2 for a, b in _block_spans("long_block", 1))


def test_the_stuffing_and_straddle_cases_have_their_properties():
    S = DEVICE_SUBSEQ
    _, scan = _scan("split_stuffing")
    assert any(scan[b - 1] == 0xFF and scan[b] == 0 for b in range(S, len(scan), S))
    p, scan = _scan("straddling_symbol")
    tr = lc.trace(scan, p.huffman, 4)
    assert any(a < b and b % (8 * S) == 0 and b < c for a, b, c, _ in tr)                      # the code | the value bits
    assert any(a < B < b for a, b, c, _ in tr for B in range(8 * S, 8 * len(scan), 8 * S))     # a boundary inside a code
    assert any(b < B < c for a, b, c, _ in tr for B in range(8 * S, 8 * len(scan), 8 * S))     # a boundary inside the value bits
    p, scan = _scan("ffrun")
    run = re.search(rb"(?:\xff\x00){3,}", scan)
    assert run is not None and run.start() < S < run.end() and scan[S - 1] == 0xFF and scan[S] == 0   # one run, split by the boundary
    tr = lc.trace(scan, p.huffman, 1)
    assert any(a < 8 * S < c and 8 * run.start() <= b <= 8 * run.end() for a, b, c, _ in tr)         # and a symbol across it, its code ending in the run
    assert not np.array_equal(p.huffman, dc.STANDARD_HUFFMAN)
    p, scan = _scan("ffend")
    assert scan[S - 1] == 0xFF and scan[S] == 0 and any(c == 8 * (S + 1) for _, _, c, _ in lc.trace(scan, p.huffman, 1))   # a symbol ends with that 0xFF
    for name in ("optimised_noise", "optimised_disc", "restart_optimised"):
        assert not np.array_equal(_scan(name)[0].huffman, dc.STANDARD_HUFFMAN), name


def test_the_restart_cases_have_their_intervals():
    want = {"restart_blocks1": [(k, 1) for k in range(12)], "restart_blocks7": [(0, 7), (7, 5)], "restart_rows1": [(4 * k, 4) for k in range(10)],
            "restart_longer_than_image": [(0, 12)], "restart_optimised": [(0, 5), (5, 5), (10, 2)]}
    for name, intervals in want.items():
        data = lc.file_of(name)
        with pytest.raises(jpeg.Unsupported, match="restart"):
            jpeg.parse_file(data)
        p = jpeg.parse_file(data, restart=True)
        assert [(s[2], s[3]) for s in p.segments] == intervals, name
    assert len(jpeg.parse_file(lc.file_of("restart_blocks1"), restart=True).segments) > 8     # the marker index wraps


# ---------------------------------------------------------------------------------------------------- the emulator of the passes and its mutants
def test_lanes_emulator_gives_the_serial_coefficients():
    for name in SMALL:
        want = lc.reference_levels(lc.file_of(name))[0]
        for subseq, lanes in ((4, 8), (16, 4), (DEVICE_SUBSEQ, 8)):
            got, _ = lc.lanes_decode_file(lc.file_of(name), subseq, lanes)
            assert np.array_equal(got, want), (name, subseq)


@pytest.mark.parametrize("mutant,name,subseq,lanes", [
    ("one_round", "noise_q100", 4, 8),                    # a symbol longer than a subsequence: the truth needs several rounds to pass
    ("stuffing_not_skipped", "ffend", lc.SUBSEQ, 8),             # (a wrong GUESS heals in pass B; a wrong TRUE start does not)
    ("counts_not_carried", "size_48x64", lc.SUBSEQ, 8),   # 15 subsequences: two chunks of eight lanes
    ("dc_not_restarted", "restart_blocks7", lc.SUBSEQ, 8),
    ("dc_not_restarted", "restart_blocks1", lc.SUBSEQ, 8),
    ("straddler_zeroes", "straddling_symbol", lc.SUBSEQ, 8),
    ("straddler_zeroes", "long_block", lc.SUBSEQ, 8),
])
def test_each_wrong_decoder_fails_the_case_built_for_it(mutant, name, subseq, lanes):
    data = lc.file_of(name)
    want = lc.reference_levels(data)[0]
    assert np.array_equal(lc.lanes_decode_file(data, subseq, lanes)[0], want)
    assert not np.array_equal(lc.lanes_decode_file(data, subseq, lanes, mutant=mutant)[0], want)


# ---------------------------------------------------------------------------------------------------- parse_file(restart=True)
def test_parse_file_restart_fields():
    for name in lc.cases():
        data = lc.file_of(name)
        p = jpeg.parse_file(data, restart=True)
        mh, mw = lc.mcus_of(p)
        assert p.scan_offset + p.scan_bytes + 2 == len(data) and p.header_key == data[:p.scan_offset]
        assert p.segments[0][0] == p.scan_offset and p.segments[-1][0] + p.segments[-1][1] == p.scan_offset + p.scan_bytes
        at = 0
        for k, (off, nb, first, count) in enumerate(p.segments):
            assert first == at and count >= 1 and nb >= 1
            assert jpeg._MARKER_IN_SCAN.search(data, off, off + nb) is None       # the marker bytes are excluded
            if k:
                assert data[off - 2:off] == bytes([0xFF, 0xD0 + (k - 1) % 8])
            at += count
        assert at == mh * mw
        if not name.startswith("restart"):       # without a DRI segment: the very fields of parse_file(data)
            q = jpeg.parse_file(data)
            assert all(np.array_equal(a, b) for a, b in zip(p, q)) and q.segments == ((q.scan_offset, q.scan_bytes, 0, mh * mw),)


def test_parse_file_restart_refusals():
    data = lc.file_of("restart_blocks1")
    p = jpeg.parse_file(data, restart=True)
    second = p.segments[1][0] - 2                 # FF D0 in front of the second interval
    assert data[second:second + 2] == b"\xff\xd0"
    with pytest.raises(jpeg.Unsupported, match="is due"):
        jpeg.parse_file(data[:second + 1] + b"\xd1" + data[second + 2:], restart=True)          # markers out of order
    third = p.segments[2][0] - 2
    with pytest.raises(jpeg.Unsupported, match="is due"):
        jpeg.parse_file(data[:third] + data[p.segments[3][0] - 2:], restart=True)                # an interval (and its marker) missing
    with pytest.raises(jpeg.Unsupported, match="MCU count"):
        jpeg.parse_file(data[:p.segments[-1][0] - 2] + data[-2:], restart=True)                  # the last interval missing: too few
    at = data.index(b"\xff\xdd")
    with pytest.raises(jpeg.Unsupported, match="MCU count"):
        jpeg.parse_file(data[:at + 4] + b"\x00\x02" + data[at + 6:], restart=True)               # intervals of 2 MCUs declared, 1 each present
    with pytest.raises(jpeg.Unsupported, match="MCU count"):
        jpeg.parse_file(data[:-2] + b"\xff\xd3" + data[p.segments[-1][0]:], restart=True)        # an interval too many
    with pytest.raises(jpeg.Unsupported, match="DRI"):
        jpeg.parse_file(data[:at + 2] + b"\x00\x05\x00\x00\x01" + data[at + 6:], restart=True)
    with pytest.raises(jpeg.Unsupported, match="is due"):
        jpeg.parse_file(data[:-2] + b"\xff\xda\x00\x02" + data[-2:], restart=True)               # a further scan
    from PIL import Image
    import io

    rgb = jc.make_image("disc", 33, 47)
    for kw, word in ((dict(progressive=True), "progressive"), (dict(subsampling=0), "sampling"), (dict(subsampling=1), "sampling")):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="JPEG", restart_marker_blocks=2, **kw)
        with pytest.raises(jpeg.Unsupported, match=word):
            jpeg.parse_file(buf.getvalue(), restart=True)
    buf = io.BytesIO()
    Image.fromarray(rgb[..., 0]).save(buf, format="JPEG", restart_marker_blocks=2)
    with pytest.raises(jpeg.Unsupported, match="component"):
        jpeg.parse_file(buf.getvalue(), restart=True)
    with pytest.raises(jpeg.Unsupported, match="EOI"):
        jpeg.parse_file(data[:-2], restart=True)


# ---------------------------------------------------------------------------------------------------- the device's decoder on the host
@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    work = tmp_path_factory.mktemp("jpeg_lanes_host")
    exes = {}
    for subseq in SUBSEQS:
        exes[subseq] = work / f"jpeg_lanes_host_{subseq}"
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", f"-DJE_SUBSEQ={subseq}", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                        str(exes[subseq]), str(ROOT / "tests" / "host" / "jpeg_lanes_host.cpp")], check=True)

    def run(subseq, cases):
        """[(huffman, mcus, buffer bytes, segments or None: the whole buffer as one)] -> [(status, serial status, rounds, same as serial,
        int16 [mcus, 6, 64])]; the program must end with status 0."""
        with open(work / "in.bin", "wb") as f:
            f.write(np.int32(len(cases)).tobytes())
            for huffman, mcus, buf, segments in cases:
                if segments is None:
                    segments = [(0, len(buf), 0, 0, mcus)]
                f.write(np.ascontiguousarray(huffman, dtype=np.uint8).tobytes())
                f.write(np.array([mcus, len(buf), len(segments)], dtype=np.int32).tobytes())
                f.write(np.array([tuple(s) for s in segments], dtype=SEGMENT).tobytes())
                f.write(bytes(buf))
        done = subprocess.run([str(exes[subseq]), str(work / "in.bin"), str(work / "out.bin")], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-4000:]
        raw = (work / "out.bin").read_bytes()
        out, at = [], 0
        for _, mcus, _, _ in cases:
            status, serial, rounds, size, same = (int(v) for v in np.frombuffer(raw, dtype=np.uint32, count=5, offset=at))
            assert size == subseq
            out.append((status, serial, rounds, same, np.frombuffer(raw, dtype=np.int16, count=mcus * 384, offset=at + 20).reshape(mcus, 6, 64)))
            at += 20 + mcus * 768
        assert at == len(raw)
        return out

    return run


def _file_case(name):
    data = lc.file_of(name)
    p = jpeg.parse_file(data, restart=True)
    mh, mw = lc.mcus_of(p)
    return p.huffman, mh * mw, data, [(off, nb, 0, first, count) for off, nb, first, count in p.segments]


@pytest.mark.parametrize("subseq", SUBSEQS)
def test_host_build_equals_the_emulator_on_every_case(host_decoder, subseq):
    names = lc.cases()
    got = host_decoder(subseq, [_file_case(n) for n in names])
    rounds = {}
    for name, (status, serial, r, same, coef) in zip(names, got):
        data = lc.file_of(name)
        p = jpeg.parse_file(data, restart=True)
        assert status == 0, name
        chunks = sum(-(-nb // (LANES * subseq)) for _, nb, _, _ in p.segments)
        assert chunks <= r <= sum(-(-nb // subseq) for _, nb, _, _ in p.segments), name   # every chunk ends its rounds: at least one, at most a round per lane with bytes
        rounds[name] = (r, chunks)
        if name in SMALL:
            assert np.array_equal(coef.reshape(-1), lc.reference_levels(data)[0].reshape(-1)), name
        else:                                                     # the large ones: the serial host decoder (which IS the emulator, by
            q = jpeg.parse_file(data)                             # tests/test_jpeg_decode_host.py) on the scan, and Pillow's pixels
            (_, _, _, same, coef2), = host_decoder(subseq, [(q.huffman, coef.shape[0], data[q.scan_offset:q.scan_offset + q.scan_bytes], None)])
            assert same == 1 and np.array_equal(coef, coef2), name
            mh, mw = lc.mcus_of(p)
            assert np.array_equal(dc.pixels(coef.astype(np.int64).reshape(mh, mw, 6, 64), p.qtab, p.h, p.w), dc.pillow_pixels(data)), name
    print(f"rounds of pass B at {subseq} bytes (rounds, chunks):", rounds)
    r, chunks = rounds["noise_q100"]
    if subseq == 4:       # symbols longer than a subsequence: the truth travels a lane per round, the early exit comes late
        assert r >= 16 * chunks
    else:                 # a guess falls into step within a few subsequences: the early exit is taken
        assert rounds["size_501x501"][0] < rounds["size_501x501"][1] * LANES // 4


def test_host_build_survives_hostile_scans_and_reports_what_the_serial_decoder_reports(host_decoder):
    huffman, mcus, scan = lc.scan_case(lc.file_of("one_mcu"))
    assert mcus == 1 and len(scan) == 299
    hostile = lc.hostile_small()
    for subseq in SUBSEQS:
        got = host_decoder(subseq, [(huffman, mcus, s, None) for s in hostile])
        reported = 0
        for s, (status, serial, _, same, coef) in zip(hostile, got):
            assert (status != 0) == (serial != 0)
            if status == 0:   # a flip that left a well-formed scan (a value bit): decoded as what it now says
                assert same == 1
            reported += status != 0
        assert 200 < reported < len(hostile)
        for status, serial, _, _, _ in host_decoder(subseq, [(huffman, 7, s, None) for s in hostile]):   # more MCUs asked for than any of them holds
            assert status != 0 and serial != 0
    huffman, mcus, scan = lc.scan_case(lc.file_of("size_501x501"))
    big = lc.hostile_large()
    for subseq in (4, DEVICE_SUBSEQ):
        got = host_decoder(subseq, [(huffman, mcus, s, None) for s in big])
        for status, serial, _, same, _ in got:
            assert (status != 0) == (serial != 0) and (status != 0 or same == 1)
        assert all(status != 0 for status, *_ in got[:6])


def test_host_build_bounds_segment_tables_that_lie(host_decoder):
    data = lc.file_of("restart_blocks7")
    huffman, mcus, _, good = _file_case("restart_blocks7")
    (o0, n0, _, f0, c0), (o1, n1, _, f1, c1) = good
    lying = [
        [(o0, n0, 0, f0, c0), (o1, n1, 0, f1, c1 + 1)],          # an MCU range that passes the image's end
        [(o0, n0, 0, f0, c0), (o1, n1, 0, -1, c1)],
        [(o0, n0, 0, f0, c0), (o1, n1, 0, f1, 0)],
        [(o0, n0, 0, f0, c0), (o1, n1, 0, 2 ** 31 - 1, 2 ** 31 - 1)],
        [(o0, n0, 0, f0, c0), (o1, len(data), 0, f1, c1)],       # bytes that pass the buffer's end
        [(o0, n0, 0, f0, c0), (-1, n1, 0, f1, c1)],
        [(o0, n0, 0, f0, c0), (o1, -5, 0, f1, c1)],
        [(o0, n0, 0, f0, c0), (2 ** 62, n1, 0, f1, c1)],
        [(o0, n0, 0, f0, c0), (o1, n1, 3, f1, c1)],              # an image that is not there
        [(o0, n0, 0, f0, c0), (o1, n1, -1, f1, c1)],
        [(o0, n0, 0, f0, c0)],                                    # an interval missing: not seen by the kernel (the wrapper checks the tiling)
        [(o0, n0, 0, f0, c0), (o0, n0, 0, f1, c1)],              # the wrong bytes for the second interval: too many blocks for it
        [(o1, n1, 0, f0, c0), (o1, n1, 0, f1, c1)],              # too few blocks for the first
        [(o0, n0 + 2 + n1, 0, f0, c0), (o1, n1, 0, f1, c1)],     # the marker inside a segment
        [(o0, n0, 0, 0, mcus), (o1, n1, 0, f1, c1)],
    ]
    for subseq in SUBSEQS:
        got = host_decoder(subseq, [(huffman, mcus, data, segs) for segs in lying] + [(huffman, mcus, data, [s for s in good])])
        for k, (status, *_rest) in enumerate(got[:-1]):
            assert (status != 0) == (k != 10), k
        assert all(got[k][0] & dc.BAD_SLOT for k in range(10))
        assert got[-1][0] == 0 and np.array_equal(got[-1][4].reshape(-1), lc.reference_levels(data)[0].reshape(-1))


def test_host_build_refuses_tables_that_oversubscribe_the_code_space(host_decoder):
    bad = dc.STANDARD_HUFFMAN.copy()
    bad[1, 0] = 3   # three codes of length 1
    with pytest.raises(AssertionError, match="refused"):
        host_decoder(4, [(bad, 1, b"\x00" * 8, None)])
