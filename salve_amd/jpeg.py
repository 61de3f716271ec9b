"""The quantisation tables of the reference's JPEG hop, and the file around a device-coded scan.

The reference writes every BEV render with `imageio.imwrite(path.jpg, img)` (bev_rendering_utils.py:629-630) -- Pillow's encoder
over libjpeg at quality 75, baseline, 4:2:0 -- and reads the file back (zind_data.py:306-315).  `BevRasteriser.jpeg_roundtrip`
reproduces decode(encode(img)) on the device (salve_amd/csrc/jpeg_roundtrip.hip); the tables it divides by come from here.
`BevRasteriser.jpeg_encode` leaves the entropy-coded scan of that very file (salve_amd/csrc/jpeg_encode.hip); `file_bytes` puts
Pillow's header in front of it and the end marker behind it.  `parse_file` goes the other way for `BevRasteriser.jpeg_decode`
(salve_amd/csrc/jpeg_decode.hip): size, tables and the scan's place in a file from disk.
Pure host arithmetic, no device.
"""

from __future__ import annotations

import re
import threading
from typing import Dict, NamedTuple, Tuple

import numpy as np

# ITU-T T.81 Annex K tables 1 and 2 in natural (row-major) order: what libjpeg's jpeg_set_defaults installs
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
STD_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)


def quality_scaling(quality: int) -> int:
    """libjpeg's jpeg_quality_scaling: quality clamped to 1..100, below 50 -> 5000 / q, from 50 -> 200 - 2 q (per cent)."""
    q = min(max(int(quality), 1), 100)
    return 5000 // q if q < 50 else 200 - 2 * q


def quality_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64] (luma, chroma; natural order): libjpeg's jpeg_set_quality(quality, force_baseline=TRUE) of the standard
    tables -- (entry * scale + 50) / 100, clamped to 1..255 -- i.e. the tables of Pillow's `save(path, quality=quality)`."""
    scale = quality_scaling(quality)
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------- the file around the scan
# ITU-T T.81 Annex K.3, tables K.3 - K.6: the Huffman tables libjpeg's jpeg_set_defaults installs and Pillow's default
# (optimize=False) writes.  BITS: the number of codes of each length 1 .. 16; HUFFVAL: the symbols in code order.
BITS_DC_LUMA = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
HUFFVAL_DC_LUMA = (
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b)

BITS_AC_LUMA = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
HUFFVAL_AC_LUMA = (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa)

BITS_DC_CHROMA = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
HUFFVAL_DC_CHROMA = (
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b)

BITS_AC_CHROMA = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
HUFFVAL_AC_CHROMA = (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa)


def huffman_codes(bits, huffval) -> np.ndarray:
    """uint32 [256]: code << 5 | length of every symbol of a table (0: not a symbol), by T.81 Annex C -- the codes of one length are
    consecutive, the first code of the next length is the successor shifted left.  The layout the device coder's tables have."""
    out = np.zeros(256, dtype=np.uint32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[huffval[k]] = (code << 5) | length
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = np.stack([huffman_codes(BITS_DC_LUMA, HUFFVAL_DC_LUMA), huffman_codes(BITS_DC_CHROMA, HUFFVAL_DC_CHROMA)])   # [luma, chroma][category]
AC_CODES = np.stack([huffman_codes(BITS_AC_LUMA, HUFFVAL_AC_LUMA), huffman_codes(BITS_AC_CHROMA, HUFFVAL_AC_CHROMA)])   # [luma, chroma][run << 4 | size]

# natural (row-major) index of zigzag position k (T.81 figure A.6)
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8))), dtype=np.int64)

HEADER_BYTES = 623


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def file_header(h: int, w: int, quality: int) -> bytes:
    """The 623 bytes Pillow's `Image.fromarray(rgb).save(path, quality=quality)` writes in front of the entropy-coded scan of an
    h x w RGB image: SOI, APP0 (JFIF 1.01, no units, density 1 x 1), the two quantisation tables in zigzag order, SOF0 (4:2:0),
    the four standard Huffman tables, SOS."""
    h, w = int(h), int(w)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"a JPEG file holds 1..65535 rows and columns, got {h} x {w}")
    qt = quality_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k in range(2):
        out += _segment(0xDB, bytes([k]) + bytes(int(v) for v in qt[k][ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, bits, vals in ((0x00, BITS_DC_LUMA, HUFFVAL_DC_LUMA), (0x10, BITS_AC_LUMA, HUFFVAL_AC_LUMA),
                              (0x01, BITS_DC_CHROMA, HUFFVAL_DC_CHROMA), (0x11, BITS_AC_CHROMA, HUFFVAL_AC_CHROMA)):
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))
    assert len(out) == HEADER_BYTES
    return out


def file_bytes(scan: bytes, h: int, w: int, quality: int) -> bytes:
    """The whole file around an entropy-coded scan (BevRasteriser.jpeg_encode's bytes of one image): header + scan + EOI."""
    return file_header(h, w, quality) + bytes(scan) + b"\xff\xd9"


# ---------------------------------------------------------------------------------------------------- reading a file's header
class Unsupported(ValueError):
    """A file outside what `BevRasteriser.jpeg_decode` takes (baseline, 8-bit, three components, 4:2:0, one interleaved scan, no
    restart interval -- or, where the caller asks for them, another of SAMPLINGS): the caller decodes it on the host."""


# The samplings salve_bev_jpeg_decode_sampled / _lanes_sampled decode (include/salve_hip.h: SALVE_JPEG_SAMPLING_*), by the frame's sampling
# factors (Y, Cb, Cr as H << 4 | V; greyscale has one component); the MCU in pixels (rows, columns) and its blocks.
# DEVICE_SAMPLINGS: those whose device route loads a floor of panoramas faster than Pillow in the reader threads by more than the spread
# between repeats (profiles/r12_jpeg_samplings.txt) -- what callers pass as `samplings=` to take all that pays.  4:4:4 is
# decoded bit for bit as well but measured level with the host (1.05 x, inside the spread): name it, or pass SAMPLINGS, to have it.
SAMPLINGS = ("4:2:0", "4:2:2", "4:4:4", "grey")
DEVICE_SAMPLINGS = ("4:2:0", "4:2:2", "grey")
_SAMPLING_OF_FACTORS = {(0x22, 0x11, 0x11): "4:2:0", (0x21, 0x11, 0x11): "4:2:2", (0x11, 0x11, 0x11): "4:4:4"}
MCU_SIZE = {"4:2:0": (16, 16), "4:2:2": (8, 16), "4:4:4": (8, 8), "grey": (8, 8)}
MCU_BLOCKS = {"4:2:0": 6, "4:2:2": 4, "4:4:4": 3, "grey": 1}


def mcu_grid(h: int, w: int, sampling: str = "4:2:0") -> Tuple[int, int]:
    """(MCU rows, MCUs across) of an h x w image.  A greyscale scan is not interleaved: its "MCUs" are its 8 x 8 blocks."""
    mh, mw = MCU_SIZE[sampling]
    return -(-int(h) // mh), -(-int(w) // mw)


class ParsedFile(NamedTuple):
    h: int
    w: int
    qtab: np.ndarray          # uint16 [2, 64], natural order: the luma component's table, the chroma components' table
    huffman: np.ndarray       # uint8 [4, 272]: DC luma, AC luma, DC chroma, AC chroma; each 16 BITS + 256 HUFFVAL (zero-filled)
    scan_offset: int          # the entropy-coded scan is data[scan_offset : scan_offset + scan_bytes] (stuffed, padded; no EOI)
    scan_bytes: int
    header_key: bytes         # the bytes before the scan: files with equal keys share size and tables and may go into one call
    segments: Tuple[Tuple[int, int, int, int], ...] = ()   # (file offset, bytes, first MCU, MCUs) of the scan's restart intervals, the RSTn
    #                           markers excluded; a scan without restart markers is one segment.  For BevRasteriser.jpeg_decode(entropy="lanes")
    sampling: str = "4:2:0"   # one of SAMPLINGS: BevRasteriser.jpeg_decode(sampling=); MCUs count in MCU_SIZE[sampling]


HUFFMAN_TABLE_BYTES = 272
SCAN_PADDING = 16             # include/salve_hip.h: SALVE_JPEG_SCAN_PADDING
DEVICE_MAX_SIDE = 4096        # salve_bev_jpeg_decode / _lanes refuse a taller or wider image (parse_file itself has no limit) ...
DEVICE_MAX_SEGMENT_BYTES = 1 << 27   # ... and the lanes report a longer segment as SALVE_JPEG_BAD_SLOT: callers send such files to the host
_MARKER_IN_SCAN = re.compile(rb"\xff[^\x00]")   # inside entropy-coded data every 0xFF is followed by a stuffed 0x00
# include/salve_hip.h: SALVE_JPEG_*, the bits of salve_bev_jpeg_decode's per-image status
STATUS_BITS = {1: "a bit pattern that is no Huffman code of its table", 2: "a run past coefficient 63", 4: "the scan ends before the last MCU",
               8: "a DC coefficient out of range", 16: "bits left over behind the last MCU", 32: "a marker inside the scan",
               64: "the scan lies outside the buffer"}


def describe_status(word: int) -> str:
    """The names of the bits set in one image's status word."""
    return "; ".join(text for bit, text in STATUS_BITS.items() if int(word) & bit) or "ok"


def parse_file(data: bytes, restart: bool = False, samplings: Tuple[str, ...] = ("4:2:0",)) -> ParsedFile:
    """Walks the marker segments of a JPEG file (ITU-T T.81 Annex B) up to its scan and returns what salve_bev_jpeg_decode needs.
    Raises `Unsupported(reason)` for everything outside part 1 of what the device decodes: progressive and other non-baseline
    frames, greyscale, other sampling factors, 12-bit samples, 16-bit quantisation entries, a restart interval, more than one scan,
    a missing EOI, a truncated segment.  Pure host arithmetic.
    restart=True (for salve_bev_jpeg_decode_lanes) also takes a DRI segment and the RSTn markers inside the scan: the markers must
    count D0 .. D7 in order, and there must be exactly as many intervals as the image's MCUs need (interval i starts at MCU i * Ri:
    every interval but the last holds Ri MCUs by position); `segments` then names the intervals, the marker bytes excluded.
    samplings: the members of SAMPLINGS the caller takes (for salve_bev_jpeg_decode_sampled / _lanes_sampled); `sampling`
    names the file's, and the MCUs of `segments` count in its MCU (16 x 8 for 4:2:2, 8 x 8 for 4:4:4; a greyscale scan's blocks).  A
    greyscale file has the luma tables in the chroma slots of `qtab` and `huffman` as well.  With anything beyond the default, a
    three-component file must also be YCbCr by libjpeg's rule (jdapimin.c: default_decompress_parms) -- a JFIF segment: yes; else an
    Adobe segment: its transform byte, 0 is RGB; else the component ids 'R', 'G', 'B': RGB -- or it is refused ("colour space"):
    Pillow's `save(keep_rgb=True)` writes a 1x1 1x1 1x1 frame that is RGB.  The default neither reads APP14 nor looks at the ids."""
    samplings = _check_samplings(samplings)
    data = bytes(data)
    return _parse_scan(data, *_walk_header(data, restart, samplings))


class HeaderCache:
    """`parse_file` for the files of a data set written by one program, whose headers are the same bytes: `parse(data)` is
    `parse_file(data, restart=restart, samplings=samplings)` for every input -- the same ParsedFile field for field, or the same
    Unsupported with the same message -- but the marker walk runs once per distinct `header_key`.  A file that starts with a key the
    cache has met takes size, tables, sampling and the scan's offset from that key's entry (the walk reads nothing behind the key, so it
    would find the same) and runs only the per-file half: the EOI check, the marker-in-scan search, the restart intervals.  A file
    whose header the walk refuses leaves no entry and is walked in full every time.
    The options belong to the cache, not to the call: an entry made under one `restart` / `samplings` cannot answer for another.
    The ParsedFiles of one header share their `qtab` and `huffman` arrays: read them, do not write them.
    `parse` may be called from several threads at once (entries are only ever added, under a lock; two threads that meet a new
    header together both walk it and keep one entry)."""

    def __init__(self, restart: bool = False, samplings: Tuple[str, ...] = ("4:2:0",)) -> None:
        self.restart, self.samplings = bool(restart), _check_samplings(samplings)
        self._lock = threading.Lock()
        self._by_length: Dict[int, Dict[bytes, tuple]] = {}   # len(header_key) -> header_key -> `_walk_header`'s tuple

    def __len__(self) -> int:
        return sum(len(d) for d in self._by_length.values())

    def parse(self, data: bytes) -> ParsedFile:
        data = bytes(data)
        for length, entries in list(self._by_length.items()):   # (a data set has one length, or a few)
            header = entries.get(data[:length])
            if header is not None:
                return _parse_scan(data, *header)
        header = _walk_header(data, self.restart, self.samplings)
        with self._lock:
            self._by_length.setdefault(header[4], {}).setdefault(data[:header[4]], header)
        return _parse_scan(data, *header)


def _check_samplings(samplings) -> Tuple[str, ...]:
    samplings = tuple(samplings)
    if not samplings or any(s not in SAMPLINGS for s in samplings):
        raise ValueError(f"samplings must name members of {SAMPLINGS}, got {samplings!r}")
    return samplings


def _walk_header(data: bytes, restart: bool, samplings: Tuple[str, ...]):
    """The first half of `parse_file`: the marker segments up to and including SOS -> (h, w, qtab, huffman, the scan's offset, the
    restart interval in MCUs or 0, sampling).  Depends on nothing behind the scan's offset: a file that starts with the same bytes
    gives the same answer (what `HeaderCache` rests on)."""
    colour_rule = samplings != ("4:2:0",)
    jfif, adobe = False, None
    sampling = "4:2:0"
    interval = 0
    if data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI marker")
    qt: Dict[int, np.ndarray] = {}
    huff: Dict[int, np.ndarray] = {}
    frame = None
    at = 2
    while True:
        if at + 4 > len(data):
            raise Unsupported("truncated: the file ends in front of its scan")
        if data[at] != 0xFF:
            raise Unsupported(f"no marker at byte {at}")
        marker = data[at + 1]
        if marker == 0xFF:      # fill bytes in front of a marker
            at += 1
            continue
        if marker in (0xD8, 0xD9, 0x01) or 0xD0 <= marker <= 0xD7:
            raise Unsupported(f"marker FF{marker:02X} in front of the scan")
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if length < 2 or at + 2 + length > len(data):
            raise Unsupported(f"truncated: segment FF{marker:02X} at byte {at} runs past the end of the file")
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantisation entries")
                if tq > 3 or k + 65 > len(body):
                    raise Unsupported("a malformed DQT segment")
                table = np.zeros(64, dtype=np.uint16)
                table[ZIGZAG] = np.frombuffer(body, dtype=np.uint8, count=64, offset=k + 1)
                if table.min() < 1:
                    raise Unsupported("a quantisation entry of 0")
                qt[tq] = table
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise Unsupported("a malformed DHT segment")
                tc, th = body[k] >> 4, body[k] & 15
                bits = np.frombuffer(body, dtype=np.uint8, count=16, offset=k + 1)
                count = int(bits.sum())
                if tc > 1 or th > 3 or count > 256 or k + 17 + count > len(body):
                    raise Unsupported("a malformed DHT segment")
                code = 0
                for length_bits in range(1, 17):
                    code += int(bits[length_bits - 1])
                    if code > (1 << length_bits):
                        raise Unsupported("a Huffman table that over-subscribes its code space")
                    code <<= 1
                table = np.zeros(HUFFMAN_TABLE_BYTES, dtype=np.uint8)
                table[:16] = bits
                table[16:16 + count] = np.frombuffer(body, dtype=np.uint8, count=count, offset=k + 17)
                huff[(tc << 4) | th] = table
                k += 17 + count
        elif marker == 0xC0:
            if frame is not None:
                raise Unsupported("more than one frame")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise Unsupported("a malformed SOF0 segment")
            if body[0] != 8:
                raise Unsupported(f"{body[0]}-bit samples")
            h, w, nc = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            if nc == 1 and "grey" in samplings:
                comps = [(body[6], body[7], body[8])]
                if comps[0][1] != 0x11:
                    raise Unsupported("sampling factors other than 1x1 in a greyscale frame")
                sampling = "grey"
            elif nc != 3:
                raise Unsupported(f"{nc} component(s): greyscale or CMYK")
            else:
                comps = [(body[6 + 3 * c], body[7 + 3 * c], body[8 + 3 * c]) for c in range(3)]   # id, sampling, table
                sampling = _SAMPLING_OF_FACTORS.get(tuple(c[1] for c in comps))
                if sampling not in samplings:
                    raise Unsupported(f"sampling factors other than {', '.join(s for s in samplings if s != 'grey') or 'greyscale'}")
                if comps[1][2] != comps[2][2]:
                    raise Unsupported("Cb and Cr use different quantisation tables")
            if h < 1 or w < 1:
                raise Unsupported("an empty frame (or DNL)")
            frame = (h, w, comps)
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise Unsupported({0xC2: "progressive (SOF2)", 0xC1: "extended sequential (SOF1)"}.get(marker, f"frame type FF{marker:02X}"))
        elif marker == 0xCC:
            raise Unsupported("arithmetic coding conditioning (DAC)")
        elif marker == 0xDD:
            if len(body) != 2:
                raise Unsupported("a malformed DRI segment")
            interval = int.from_bytes(body, "big")
            if interval != 0 and not restart:
                raise Unsupported("a restart interval")
        elif marker == 0xDA:
            if frame is None:
                raise Unsupported("a scan in front of its frame")
            h, w, comps = frame
            nc = len(comps)
            if nc == 3 and (len(body) != 10 or body[0] != 3):
                raise Unsupported("a scan that does not interleave all three components")
            if nc == 1 and (len(body) != 6 or body[0] != 1):
                raise Unsupported("a scan that does not hold the frame's one component")
            sel = [(body[1 + 2 * c], body[2 + 2 * c]) for c in range(nc)]
            if [s[0] for s in sel] != [c[0] for c in comps]:
                raise Unsupported("a scan whose components are not in the frame's order")
            if nc == 3 and sel[1][1] != sel[2][1]:
                raise Unsupported("Cb and Cr use different Huffman tables")
            if tuple(body[-3:]) != (0, 63, 0):
                raise Unsupported("a spectral selection or successive approximation")
            if colour_rule and nc == 3:
                if jfif:
                    rgb = False
                elif adobe is not None:
                    rgb = adobe == 0
                else:
                    rgb = [c[0] for c in comps] == [0x52, 0x47, 0x42]
                if rgb:
                    raise Unsupported("colour space: libjpeg reads this three-component file as RGB, not YCbCr")
            comps, sel = (comps * 2)[:2], (sel * 2)[:2]      # (greyscale: the luma tables in the chroma slots)
            try:
                qtab = np.stack([qt[comps[0][2]], qt[comps[1][2]]])
                huffman = np.stack([huff[0x00 | (sel[0][1] >> 4)], huff[0x10 | (sel[0][1] & 15)],
                                    huff[0x00 | (sel[1][1] >> 4)], huff[0x10 | (sel[1][1] & 15)]])
            except KeyError:
                raise Unsupported("a table the scan names is missing") from None
            break
        elif colour_rule and marker == 0xE0 and len(body) >= 14 and body[:5] == b"JFIF\x00":      # (jdmarker.c: examine_app0)
            jfif = True
        elif colour_rule and marker == 0xEE and len(body) >= 12 and body[:5] == b"Adobe":         # (examine_app14: the transform byte)
            adobe = body[11]
        # every other segment (APPn, COM, ...) is skipped
    return h, w, qtab, huffman, at, interval, sampling


def _parse_scan(data: bytes, h: int, w: int, qtab: np.ndarray, huffman: np.ndarray, at: int, interval: int, sampling: str) -> ParsedFile:
    """The second half of `parse_file`, on the file itself: the EOI check, the marker-in-scan search and, with a restart interval, the
    RSTn walk and the MCU count check."""
    if data[-2:] != b"\xff\xd9":
        raise Unsupported("no EOI marker at the end of the file")
    end = len(data) - 2
    mcus = int(np.prod(mcu_grid(h, w, sampling)))
    if interval == 0:
        found = _MARKER_IN_SCAN.search(data, at, end)
        if found is not None:
            raise Unsupported(f"marker FF{data[found.start() + 1]:02X} inside the scan: restart markers or a further scan")
        return ParsedFile(h, w, qtab, huffman, at, end - at, data[:at], ((at, end - at, 0, mcus),), sampling)
    segments, lo = [], at
    for k, found in enumerate(_MARKER_IN_SCAN.finditer(data, at, end)):
        marker = data[found.start() + 1]
        if marker != 0xD0 + (k & 7):
            raise Unsupported(f"marker FF{marker:02X} inside the scan where restart marker FF{0xD0 + (k & 7):02X} is due")
        segments.append((lo, found.start() - lo, k * interval, interval))
        lo = found.start() + 2
    first = len(segments) * interval
    if first >= mcus or first + interval < mcus:
        raise Unsupported(f"{len(segments) + 1} restart intervals of {interval} MCUs in a scan of {mcus} MCUs: wrong MCU count per interval")
    segments.append((lo, end - lo, first, mcus - first))
    return ParsedFile(h, w, qtab, huffman, at, end - at, data[:at], tuple(segments), sampling)
