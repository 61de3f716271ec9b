"""The JPEG decoder's samplings beyond 4:2:0 without a GPU: salve_amd.jpeg.parse_file(samplings=) and its colour-space rule;
tests/jpeg_sampling_cases.py's emulator against Pillow on every case (which pins the upsampling formulas on the CPU) and its wrong
variants; the two entropy decoders of salve_amd/csrc compiled for the host in every sampling, as a stand-alone program under
AddressSanitizer and UBSan, against the emulator and against each other, on the case files and on the malformed inputs the GPU tests
reuse.

The cases, per sampling ("grey": one channel of the image saved as mode L):
  8 x 8, 8 x 16 noise            one MCU for 4:4:4 / grey and for 4:2:2
  5 x 3, 7 x 4 noise             chroma of at most 2 samples a row: replication
  8 x 5 noise                    cw = 3, the first fancy row
  9 x 17, 33 x 47 noise          partial MCUs on both edges
  24 x 40 disc, noise at 75      several MCU rows;  at 30 coarse quantisation;  noise at 95 the colour conversion's clamps;  at 100
                                 quantisation entries of 1;  at 75 with optimize=True tables from the file
  33 x 47 noise, restart markers per MCU, per 3 MCUs (the last interval of 4:2:2 and of greyscale's sibling sizes is short), per MCU row
  48 x 64 noise at 95            scans of at least 4 subsequences of 128 bytes: the lanes case
  128 x 256 layout image         a small panorama
"""

import io
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_sampling_cases as sc
from salve_amd import _lib, jpeg

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "salve_amd" / "csrc" / "jpeg_entropy_lanes.h"
SUBSEQ = int(re.search(r"#define JE_SUBSEQ (\d+)", HEADER.read_text()).group(1))
SEGMENT = np.dtype([("offset", "<i8"), ("bytes", "<i4"), ("image", "<i4"), ("first_mcu", "<i4"), ("mcu_count", "<i4")])
NEW = tuple(s for s in sc.SAMPLINGS if s != "4:2:0")


def _save(rgb, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **kw)
    return buf.getvalue()


# ---------------------------------------------------------------------------------------------------- parse_file(samplings=)
def test_the_names_and_numbers_agree_between_the_layers():
    assert jpeg.SAMPLINGS == ("4:2:0", "4:2:2", "4:4:4", "grey") == tuple(_lib.JPEG_SAMPLINGS)
    # the samplings measured faster on the device than in the reader threads (profiles/r12_jpeg_samplings.txt): 4:4:4 only when named
    assert jpeg.DEVICE_SAMPLINGS == ("4:2:0", "4:2:2", "grey") and set(jpeg.DEVICE_SAMPLINGS) < set(jpeg.SAMPLINGS)
    header = (ROOT / "include" / "salve_hip.h").read_text()
    for name, word in zip(jpeg.SAMPLINGS, ("420", "422", "444", "GREY")):
        assert int(re.search(rf"#define SALVE_JPEG_SAMPLING_{word} (\d)", header).group(1)) == _lib.JPEG_SAMPLINGS[name]
    assert jpeg.ParsedFile._fields[-1] == "sampling" and jpeg.ParsedFile._fields[-2] == "segments"
    assert jpeg.MCU_BLOCKS == {"4:2:0": 6, "4:2:2": 4, "4:4:4": 3, "grey": 1}


def test_parse_file_names_the_sampling_and_counts_its_mcus():
    for sampling, name in sc.cases():
        data = sc.file_of(sampling, name)
        h, w, _, save = sc.CASES[name]
        p = sc.parse(data)
        assert (p.h, p.w, p.sampling) == (h, w, sampling), (sampling, name)
        mh, mw = {"4:2:0": (16, 16), "4:2:2": (8, 16), "4:4:4": (8, 8), "grey": (8, 8)}[sampling]
        mcus = -(-h // mh) * -(-w // mw)
        assert p.scan_offset + p.scan_bytes + 2 == len(data) and p.header_key == data[:p.scan_offset]
        at = 0
        for k, (off, nb, first, count) in enumerate(p.segments):
            assert first == at and count >= 1 and nb >= 1
            if k:
                assert data[off - 2:off] == bytes([0xFF, 0xD0 + (k - 1) % 8])
            at += count
        assert at == mcus, (sampling, name)
        if name == "restart_blocks1":
            assert len(p.segments) == mcus
        elif name == "restart_blocks3":
            assert [s[3] for s in p.segments] == [3] * (mcus // 3) + ([mcus % 3] if mcus % 3 else [])
        elif name == "restart_rows1":
            assert [s[3] for s in p.segments] == [-(-w // mw)] * -(-h // mh)
        else:
            assert p.segments == ((p.scan_offset, p.scan_bytes, 0, mcus),)
        if sampling == "grey":      # the luma tables stand in the chroma slots
            assert np.array_equal(p.qtab[0], p.qtab[1]) and np.array_equal(p.huffman[:2], p.huffman[2:])
        assert (not np.array_equal(p.huffman[:2], dc.STANDARD_HUFFMAN[:2])) == (name == "24x40_optimised")
    keys = {sc.parse(sc.file_of(s, "24x40_noise")).header_key for s in sc.SAMPLINGS}
    assert len(keys) == 4           # the SOF bytes are in the key: files of different samplings never share a call


def test_the_lanes_and_restart_cases_have_their_lengths():
    """The 48 x 64 case: scans of at least 4 subsequences.  The new samplings' files with a restart marker per MCU: EVERY segment is
    shorter than one subsequence.  (Not so the other restart files the table prescribes: 33 x 47 noise at quality 75 has intervals of 3
    MCUs of 41 .. 312 bytes and MCU rows of 84 .. 488 bytes, and 4:2:0's single MCUs reach 160 -- segments of one lane AND of several.)"""
    for sampling in sc.SAMPLINGS:
        assert sc.parse(sc.file_of(sampling, "lanes_48x64")).scan_bytes >= 4 * SUBSEQ, sampling
    for sampling in NEW:
        assert max(s[1] for s in sc.parse(sc.file_of(sampling, "restart_blocks1")).segments) < SUBSEQ, sampling
        assert min(s[1] for s in sc.parse(sc.file_of(sampling, "restart_blocks3")).segments) < SUBSEQ, sampling
        assert max(s[1] for s in sc.parse(sc.file_of(sampling, "restart_rows1")).segments) > SUBSEQ, sampling


def test_the_default_refuses_exactly_what_it_refused():
    rgb = jc.make_image("disc", 33, 47)
    for kw, word in ((dict(subsampling=0), "sampling"), (dict(subsampling=1), "sampling"), (dict(progressive=True), "progressive"),
                     (dict(restart_marker_blocks=2), "restart")):
        with pytest.raises(jpeg.Unsupported, match=word):
            jpeg.parse_file(_save(rgb, **kw))
    with pytest.raises(jpeg.Unsupported, match="sampling factors other than 4:2:0$"):
        jpeg.parse_file(_save(rgb, subsampling=0), restart=True)
    with pytest.raises(jpeg.Unsupported, match=r"^1 component\(s\): greyscale or CMYK$"):
        jpeg.parse_file(_save(rgb[..., 0]))
    keep = _save(rgb, subsampling=0, keep_rgb=True)     # the default neither reads APP14 nor the ids: its sampling refuses the file
    with pytest.raises(jpeg.Unsupported, match="sampling"):
        jpeg.parse_file(keep)
    p, q = jpeg.parse_file(_save(rgb)), jpeg.parse_file(_save(rgb), samplings=("4:2:0",))
    assert p.sampling == "4:2:0" and all(np.array_equal(a, b) for a, b in zip(p, q))
    with pytest.raises(ValueError, match="samplings"):
        jpeg.parse_file(_save(rgb), samplings=("4:1:1",))


def test_the_wider_set_still_refuses_what_the_device_does_not_decode():
    rgb = jc.make_image("disc", 33, 47)
    wide = dict(restart=True, samplings=jpeg.SAMPLINGS)
    data = _save(rgb, subsampling=1)
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x21
    with pytest.raises(jpeg.Unsupported, match="sampling"):      # 4:4:0 (Y 1x2): Pillow has no name for it, so the SOF byte is patched
        jpeg.parse_file(data[:sof + 11] + b"\x12" + data[sof + 12:], **wide)
    with pytest.raises(jpeg.Unsupported, match="sampling"):      # 4:1:1 (Y 4x1)
        jpeg.parse_file(data[:sof + 11] + b"\x41" + data[sof + 12:], **wide)
    with pytest.raises(jpeg.Unsupported, match="progressive"):
        jpeg.parse_file(_save(rgb, subsampling=0, progressive=True), **wide)
    with pytest.raises(jpeg.Unsupported, match="colour space"):
        jpeg.parse_file(_save(rgb, subsampling=0, keep_rgb=True), **wide)
    with pytest.raises(jpeg.Unsupported, match="sampling"):      # a subset that leaves 4:4:4 out
        jpeg.parse_file(_save(rgb, subsampling=0), samplings=("4:2:0", "4:2:2"))
    with pytest.raises(jpeg.Unsupported, match="component"):     # ... or greyscale
        jpeg.parse_file(_save(rgb[..., 0]), samplings=("4:2:0", "4:4:4"))
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[..., :1]]), mode="CMYK").save(buf, format="JPEG")
    with pytest.raises(jpeg.Unsupported, match="component"):
        jpeg.parse_file(buf.getvalue(), **wide)


def test_the_colour_space_rule_is_libjpegs():
    """jdapimin.c: default_decompress_parms for three components -- JFIF: YCbCr; else Adobe: transform 0 RGB, else YCbCr; else the ids
    'R' 'G' 'B': RGB; else YCbCr.  Every variant is checked against what Pillow (libjpeg) makes of the very same bytes."""
    rgb = jc.make_image("disc", 24, 40)
    wide = dict(samplings=jpeg.SAMPLINGS)
    plain = _save(rgb, subsampling=0)                                        # APP0 JFIF, ids 1 2 3
    keep = _save(rgb, subsampling=0, keep_rgb=True)                          # APP14 Adobe transform 0, ids 'R' 'G' 'B', no JFIF
    assert plain[2:4] == b"\xff\xe0" and plain[6:11] == b"JFIF\x00" and b"Adobe" in keep and b"JFIF" not in keep
    app0 = plain[2:2 + 2 + int.from_bytes(plain[4:6], "big")]
    at = keep.index(b"\xff\xee")
    app14 = keep[at:at + 2 + int.from_bytes(keep[at + 2:at + 4], "big")]
    assert app14[4:9] == b"Adobe" and app14[15] == 0

    def rgb_ids(d):          # the frame's and the scan's component ids 1 2 3 -> 'R' 'G' 'B'
        sof, sos = d.index(b"\xff\xc0"), d.index(b"\xff\xda")
        d = bytearray(d)
        for k, letter in enumerate(b"RGB"):
            assert d[sof + 10 + 3 * k] == d[sos + 5 + 2 * k] == k + 1
            d[sof + 10 + 3 * k] = d[sos + 5 + 2 * k] = letter
        return bytes(d)

    no_jfif = plain[:2] + plain[2 + len(app0):]
    variants = {
        "jfif": (plain, False),
        "jfif_and_rgb_ids": (rgb_ids(plain), False),
        "jfif_and_adobe_0": (plain[:2 + len(app0)] + app14 + plain[2 + len(app0):], False),
        "adobe_0": (plain[:2] + app14 + plain[2 + len(app0):], True),
        "adobe_1": (plain[:2] + app14[:15] + b"\x01" + plain[2 + len(app0):], False),
        "adobe_1_and_rgb_ids": (rgb_ids(plain[:2] + app14[:15] + b"\x01" + plain[2 + len(app0):]), False),
        "no_marker_ids_123": (no_jfif, False),
        "no_marker_rgb_ids": (rgb_ids(no_jfif), True),
        "keep_rgb": (keep, True),
    }
    ycc = dc.pillow_pixels(plain)
    for name, (data, is_rgb) in variants.items():
        got = dc.pillow_pixels(data)
        assert (not np.array_equal(got, ycc)) == is_rgb or name == "keep_rgb", name      # libjpeg's own verdict on these bytes
        if is_rgb:
            with pytest.raises(jpeg.Unsupported, match="colour space"):
                jpeg.parse_file(data, **wide)
        else:
            assert jpeg.parse_file(data, **wide).sampling == "4:4:4", name
            assert np.array_equal(sc.decode_file(data)[0], got), name


# ---------------------------------------------------------------------------------------------------- the emulator and its mutants
def test_emulator_pixels_equal_pillows_for_every_case():
    assert len(sc.cases()) == 4 * len(sc.CASES)
    for sampling, name in sc.cases():
        got, status = sc.decode_file(sc.file_of(sampling, name))
        assert status == 0, (sampling, name)
        assert np.array_equal(got, sc.pillow_reference(sampling, name)), (sampling, name)


def test_the_conversion_applied_to_pillows_ycbcr_equals_pillows_rgb():
    """jpeg_pixels_kernel's jdcolor.c arithmetic holds for 4:4:4 and 4:2:2 files: Pillow's own YCbCr draft output through it gives
    Pillow's RGB."""
    from PIL import Image

    for sampling in ("4:4:4", "4:2:2"):
        for name in ("5x3", "8x5", "9x17", "33x47", "24x40_noise_q95", "24x40_noise_q100"):
            data = sc.file_of(sampling, name)
            with Image.open(io.BytesIO(data)) as im:
                im.draft("YCbCr", im.size)
                ycc = np.asarray(im).astype(np.int64)
            assert ycc.shape[2] == 3
            assert np.array_equal(jc.ycc_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2]), sc.pillow_reference(sampling, name)), (sampling, name)


@pytest.mark.parametrize("mutant,sampling,name", [
    ("h2v2_for_422", "4:2:2", "24x40_disc"),
    ("rounding_swapped", "4:2:2", "8x5"),
    ("no_replication", "4:2:2", "5x3"),
    ("no_replication", "4:2:2", "7x4"),
    ("order_y_cb_y_cr", "4:2:2", "8x16"),
    ("dc_shared_by_chroma", "4:4:4", "8x16"),
    ("dc_shared_by_chroma", "4:2:2", "33x47"),
    ("grey_mcus_of_16", "grey", "9x17"),
])
def test_each_wrong_decoder_fails_a_case(mutant, sampling, name):
    assert mutant in sc.MUTANTS
    data = sc.file_of(sampling, name)
    assert np.array_equal(sc.decode_file(data)[0], sc.pillow_reference(sampling, name))
    assert not np.array_equal(sc.decode_file(data, mutant=mutant)[0], sc.pillow_reference(sampling, name))


def test_every_wrong_decoder_is_in_the_table_above():
    assert len(sc.MUTANTS) >= 5
    assert set(sc.MUTANTS) == {"h2v2_for_422", "rounding_swapped", "no_replication", "order_y_cb_y_cr", "dc_shared_by_chroma", "grey_mcus_of_16"}


# ---------------------------------------------------------------------------------------------------- the device's decoders on the host
@pytest.fixture(scope="module")
def host_decoders(tmp_path_factory):
    work = tmp_path_factory.mktemp("jpeg_sampling_host")
    exe = work / "jpeg_sampling_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "jpeg_sampling_host.cpp")], check=True)

    def run(cases):
        """[(sampling, huffman, mcus, buffer bytes, segment rows)] -> [(lanes status, serial status, rounds, same as serial, int16 [mcus,
        blocks, 64])]; the program must end with status 0: nothing for the sanitizers to report."""
        with open(work / "in.bin", "wb") as f:
            f.write(np.int32(len(cases)).tobytes())
            for sampling, huffman, mcus, buf, segments in cases:
                f.write(np.int32(_lib.JPEG_SAMPLINGS[sampling]).tobytes())
                f.write(np.ascontiguousarray(huffman, dtype=np.uint8).tobytes())
                f.write(np.array([mcus, len(buf), len(segments)], dtype=np.int32).tobytes())
                f.write(np.array([tuple(s) for s in segments], dtype=SEGMENT).tobytes())
                f.write(bytes(buf))
        done = subprocess.run([str(exe), str(work / "in.bin"), str(work / "out.bin")], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-4000:]
        raw = (work / "out.bin").read_bytes()
        out, at = [], 0
        for sampling, _, mcus, _, _ in cases:
            blocks = jpeg.MCU_BLOCKS[sampling]
            status, serial, rounds, same = (int(v) for v in np.frombuffer(raw, dtype=np.uint32, count=4, offset=at))
            out.append((status, serial, rounds, same, np.frombuffer(raw, dtype=np.int16, count=mcus * blocks * 64, offset=at + 16).reshape(mcus, blocks, 64)))
            at += 16 + mcus * blocks * 128
        assert at == len(raw)
        return out

    return run


def _file_case(sampling, name):
    data = sc.file_of(sampling, name)
    p = sc.parse(data)
    return sampling, p.huffman, int(np.prod(jpeg.mcu_grid(p.h, p.w, sampling))), data, [(off, nb, 0, first, count) for off, nb, first, count in p.segments]


def test_host_builds_equal_the_emulator_on_every_case(host_decoders):
    got = host_decoders([_file_case(s, n) for s, n in sc.cases()])
    for (sampling, name), (status, serial, rounds, same, coef) in zip(sc.cases(), got):
        assert status == 0 and serial == 0 and same == 1, (sampling, name)
        want, st = sc.reference_levels(sc.file_of(sampling, name))
        assert st == 0 and np.array_equal(coef, want), (sampling, name)
        assert rounds >= len(sc.parse(sc.file_of(sampling, name)).segments)


def test_host_builds_survive_the_malformed_inputs_and_agree_on_them(host_decoders):
    """The scan cut in half, its last 40 bytes replaced by seeded noise, a segment table whose MCU range passes the image: a clean run
    under the sanitizers, and the two decoders agree on zero / non-zero.  Only these byte strings go to the device afterwards."""
    for sampling in sc.SAMPLINGS:
        p = sc.parse(sc.file_of(sampling, sc.MALFORMED_CASE))
        mcus = int(np.prod(jpeg.mcu_grid(p.h, p.w, sampling)))
        bad = sc.malformed(sampling)
        assert [b[0] for b in bad] == ["cut_in_half", "noise_tail", "mcu_range_passes_image"]
        got = host_decoders([(sampling, p.huffman, mcus, buf, rows) for _, buf, rows in bad])
        for (name, _, _), (status, serial, _, _, _) in zip(bad, got):
            assert status != 0 and serial != 0, (sampling, name)
        assert got[2][0] & dc.BAD_SLOT and not got[2][4].any()       # nothing decoded


def test_host_builds_keep_to_a_short_output(host_decoders):
    """More data than MCUs asked for (the whole scan, one MCU fewer; one MCU alone): no coefficient written behind the image's
    mcus * blocks * 64 -- the output block is exactly that long -- and both decoders report the scan."""
    cases = []
    for sampling in sc.SAMPLINGS:
        s, huffman, mcus, data, rows = _file_case(sampling, "24x40_noise")
        (off, nb, _, _, _), = rows
        cases += [(s, huffman, mcus - 1, data[off:off + nb], [(0, nb, 0, 0, mcus - 1)]), (s, huffman, 1, data[off:off + nb], [(0, nb, 0, 0, 1)])]
    for status, serial, _, _, _ in host_decoders(cases):
        assert status != 0 and serial != 0
