"""The lane-parallel JPEG entropy decoder's case table and emulator, shared by tests/test_jpeg_lanes_host.py (the host build of
salve_amd/csrc/jpeg_entropy_lanes.h == tests/jpeg_decode_cases.py's emulator; every case has the property it is named for; the wrong
decoders fail) and tests/test_gpu_jpeg_lanes.py (salve_bev_jpeg_decode_lanes == the serial stage == Pillow).

`cases()` names files; `file_of(name)` makes one (once per process).  The stuffing and straddle cases are noise images whose SEEDS a
CPU search found (for subsequences of 128 bytes, so also of 4 and 16); `trace` is what the property checks look at.
`lanes_decode` is the three passes of jpeg_entropy_lanes.h over the UNSTUFFED bits (a subsequence boundary at stuffed byte b is the
bit 8 * (data bytes in front of b); a stuffed 0x00 AT the boundary belongs to neither side), with a few lanes per chunk so that
small scans have several chunks; a guessing lane that meets a non-symbol goes on by jl_run's rules, as the device's does.
`mutant=` switches one rule to a plausible wrong variant.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

import jpeg_cases as jc
import jpeg_decode_cases as dc
from salve_amd import jpeg

MUTANTS = ("one_round", "stuffing_not_skipped", "counts_not_carried", "dc_not_restarted", "straddler_zeroes")

SIZES = ((16, 16), (17, 33), (48, 64), (501, 501), (1024, 2048))
# noise images (jpeg_cases.make_image("noise", h, w, seed)) found by a seeded search; the host test asserts what each is named for
SUBSEQ = 128                          # the subsequence the seeds and the hand-made files were found for: jpeg_entropy_lanes.h's JE_SUBSEQ
SPLIT_STUFFING = (32, 32, 95, 4)      # (h, w, quality, seed): a 0xFF is the last byte of a 128-byte subsequence, its stuffed 0x00 the first of the next
STRADDLING_SYMBOL = (32, 32, 95, 1)   # a symbol's code ends exactly at a 128-byte boundary, its value bits lie behind it; other boundaries fall inside codes
EXACT = {1: (16, 16, 60, 5), 2: (16, 16, 92, 35), 3: (16, 32, 85, 2)}   # scans of exactly 1, 2, 3 subsequences of 128 bytes
# Hand-made 16 x 16 files at quality 100 (`_crafted_file`).  Their luma AC table gives (run 0, size 1) the 16-bit code 0 11111111111111 0 and
# (run 0, size 10) the code 0 111111111111111, so a coefficient of +-1 costs 17 bits -- a block of 63 of them is 134 bytes, longer than a
# subsequence -- and (run 0, size 10) with the value 1023 is 25 one-bits: FF 00 FF 00 FF 00 in the scan.  Each luma block is
# (DC difference, coefficients of +-1, whether the 1023 follows them[, coefficients of +-2 in front, 5 bits each]); the numbers were found by search, the host test asserts the properties.
CRAFTED_AC_BITS = (0, 1) + (1,) * 13 + (2,)
CRAFTED_AC_SYMBOLS = (0x00, 0x02, 0x03, 0x04, 0x11, 0x12, 0x21, 0x31, 0x41, 0x05, 0x06, 0x07, 0x08, 0x09, 0x01, 0x0A)
CRAFTED = {
    "ffrun": ((-255, 41, True), (0, 0, False), (0, 0, False), (0, 0, False)),          # one 0xFF run that holds the 128-byte boundary: a stuffed pair split by it and a symbol that straddles it
    "ffend": ((-200, 37, True, 15), (5, 0, False), (0, 0, False), (0, 0, False)),      # the symbol ENDS with the 0xFF that closes the first subsequence: the next lane's true start lies behind the stuffed 0x00
    "long_block": ((0, 25, False), (3, 63, False), (-3, 2, False), (0, 0, False)),     # a block that begins in the first subsequence and ends in the third: the second lane completes no block
}


def _pillow(rgb: np.ndarray, **save) -> bytes:
    return dc.pillow_file(rgb, **save)


def _crafted_file(luma_blocks) -> bytes:
    ac_luma = jpeg.huffman_codes(CRAFTED_AC_BITS, CRAFTED_AC_SYMBOLS)
    bits: List[int] = []

    def put(table, symbol, value=None):
        code, n = int(table[symbol]) >> 5, int(table[symbol]) & 31
        bits.extend((code >> (n - 1 - i)) & 1 for i in range(n))
        if value is not None:
            size = symbol & 15
            v = value if value >= 0 else value + (1 << size) - 1
            bits.extend((v >> (size - 1 - i)) & 1 for i in range(size))

    assert len(luma_blocks) == 4
    for dc_diff, ones, big, *twos in luma_blocks:
        size = int(abs(dc_diff)).bit_length()
        put(jpeg.DC_CODES[0], size, dc_diff if size else None)
        for i in range(twos[0] if twos else 0):
            put(ac_luma, 0x02, 2 if i % 2 else -2)           # 5 bits each: the fine adjustment
        for i in range(ones):
            put(ac_luma, 0x01, 1 if i % 2 else -1)
        if big:
            put(ac_luma, 0x0A, 1023)
        if ones + big + (twos[0] if twos else 0) < 63:
            put(ac_luma, 0x00)
    for _ in range(2):
        put(jpeg.DC_CODES[1], 0)
        put(jpeg.AC_CODES[1], 0x00)
    bits.extend([1] * (-len(bits) % 8))
    scan = np.packbits(np.array(bits, dtype=np.uint8)).tobytes().replace(b"\xff", b"\xff\x00")
    header = jpeg.file_header(16, 16, 100)
    at = header.index(b"\xff\xc4", header.index(b"\xff\xc4") + 2)     # the second DHT segment: AC luma
    end = at + 2 + int.from_bytes(header[at + 2:at + 4], "big")
    assert header[at + 4] == 0x10
    header = header[:at] + jpeg._segment(0xC4, bytes([0x10]) + bytes(CRAFTED_AC_BITS) + bytes(CRAFTED_AC_SYMBOLS)) + header[end:]
    return header + scan + b"\xff\xd9"


_FILES: Dict[str, bytes] = {}


def cases() -> List[str]:
    out = ["short", "exact1", "exact2", "exact3", "flat_q5", "noise_q100", "split_stuffing", "straddling_symbol", "ffrun", "ffend", "long_block", "optimised_noise", "optimised_disc"]
    out += [f"size_{h}x{w}" for h, w in SIZES]
    out += ["restart_blocks1", "restart_blocks7", "restart_rows1", "restart_longer_than_image", "restart_optimised"]
    return out


def file_of(name: str) -> bytes:
    if name not in _FILES:
        _FILES[name] = _make(name)
    return _FILES[name]


def _make(name: str) -> bytes:
    if name == "short":                 # a scan shorter than one subsequence
        return _pillow(jc.make_image("constant", 16, 16), quality=75)
    if name.startswith("exact"):
        h, w, q, seed = EXACT[int(name[5:])]
        return _pillow(jc.make_image("noise", h, w, seed), quality=q)
    if name == "flat_q5":               # 2400 EOB-only blocks, 192 to a subsequence of 128 bytes
        return _pillow(jc.make_image("constant", 320, 320), quality=5)
    if name == "noise_q100":            # the longest blocks an 8-bit image gives: 97 bytes, so no block spans three subsequences of 128 bytes ("long_block" does)
        return _pillow(jc.make_image("noise", 33, 47), quality=100)
    if name == "split_stuffing":
        h, w, q, seed = SPLIT_STUFFING
        return _pillow(jc.make_image("noise", h, w, seed), quality=q)
    if name == "straddling_symbol":
        h, w, q, seed = STRADDLING_SYMBOL
        return _pillow(jc.make_image("noise", h, w, seed), quality=q)
    if name in CRAFTED:
        return _crafted_file(CRAFTED[name])
    if name == "one_mcu":      # (not in the table) one MCU, 299 bytes: the scan the hostile families are cut from
        return _pillow(jc.make_image("noise", 16, 16, 0), quality=95)
    if name == "optimised_noise":
        return _pillow(jc.make_image("noise", 33, 47), quality=75, optimize=True)
    if name == "optimised_disc":
        return _pillow(jc.make_image("disc", 48, 64), quality=75, optimize=True)
    if name.startswith("size_"):
        h, w = (int(v) for v in name[5:].split("x"))
        content = "noise" if h * w <= 48 * 64 else "disc"   # (the large ones stay a few hundred KB)
        return _pillow(jc.make_image(content, h, w), quality=75)
    rgb = jc.make_image("noise", 48, 64)                     # 12 MCUs, 4 across
    if name == "restart_blocks1":       # 12 intervals: the marker index wraps behind D7
        return _pillow(rgb, quality=75, restart_marker_blocks=1)
    if name == "restart_blocks7":       # the last interval is short
        return _pillow(rgb, quality=75, restart_marker_blocks=7)
    if name == "restart_rows1":
        return _pillow(jc.make_image("disc", 160, 64), quality=75, restart_marker_rows=1)   # 10 intervals of 4 MCUs
    if name == "restart_longer_than_image":
        return _pillow(rgb, quality=75, restart_marker_blocks=100)
    if name == "restart_optimised":
        return _pillow(rgb, quality=90, optimize=True, restart_marker_blocks=5)
    raise KeyError(name)


def mcus_of(p: jpeg.ParsedFile) -> Tuple[int, int]:
    return -(-p.h // 16), -(-p.w // 16)


def reference_levels(data: bytes) -> Tuple[np.ndarray, int]:
    """jpeg_decode_cases.decode, one restart interval at a time (the predictors start at 0 in each) -> ([mh, mw, 6, 64], status)."""
    p = jpeg.parse_file(data, restart=True)
    mh, mw = mcus_of(p)
    out = np.zeros((mh * mw, 6, 64), dtype=np.int64)
    status = 0
    for off, nb, first, count in p.segments:
        levels, st = dc.decode(data[off:off + nb], p.huffman, 1, count)
        out[first:first + count] = levels[0]
        status |= st
    return out.reshape(mh, mw, 6, 64), status


# ---------------------------------------------------------------------------------------------------- the symbols of a scan
class _Stream:
    """The unstuffed bits of a scan, and where the stuffed bytes lie in them."""

    def __init__(self, scan: bytes, huffman: np.ndarray):
        self.tables = [dc._decoder_table(np.asarray(huffman[t])) for t in range(4)]
        data, ubit_of_byte, stuffing = bytearray(), [], []
        i = 0
        while i < len(scan):
            ubit_of_byte.append(8 * len(data))
            stuffing.append(False)
            data.append(scan[i])
            if scan[i] == 0xFF and i + 1 < len(scan) and scan[i + 1] == 0:
                ubit_of_byte.append(8 * len(data))   # the stuffed byte holds no bit: it maps to the bit behind the 0xFF
                stuffing.append(True)
                i += 1
            i += 1
        ubit_of_byte.append(8 * len(data))
        self.ubit_of_byte, self.stuffing, self.nbytes = ubit_of_byte, stuffing, len(scan)
        self.byte_of_data = [b for b in range(len(scan)) if not stuffing[b]]   # the stuffed index of data byte i
        self.total = 8 * len(data)
        self.bits = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8)).tolist() + [0] * 64
        self.zigzag = jpeg.ZIGZAG.tolist()

    def take(self, bits: List[int], at: int, n: int) -> int:
        v = 0
        for bit in bits[at:at + n]:
            v = (v << 1) | bit
        return v

    def symbol(self, bits: List[int], at: int, slot: int, k: int, go_on: bool = False):
        """One symbol at bit `at` in state (slot, k) -> (bits of the code, bits of the value, k after it or 64 for a finished block,
        coefficient index or -1, value) or None: no symbol.  go_on: jpeg_entropy_lanes.h's rules for what is no symbol instead of
        None (jl_run) -- a non-code costs one bit, a DC category above 11 has no value bits, a run past coefficient 63 ends the block."""
        table = self.tables[(0 if slot < 4 else 2) + (1 if k else 0)]
        code, sym, length = 0, -1, 0
        for length in range(1, 17):
            code = (code << 1) | (bits[at + length - 1] if at + length - 1 < len(bits) else 0)
            if (length, code) in table:
                sym = table[(length, code)]
                break
        if sym < 0:
            return (1, 0, k, -1, 0) if go_on else None
        if k == 0:
            if sym > 11:
                return (length, 0, 1, -1, 0) if go_on else None
            size, idx, nk = sym, 0, 1
        else:
            run, size = sym >> 4, sym & 15
            if size == 0:
                if run != 15:
                    return length, 0, 64, -1, 0
                if k + 16 > 64:
                    return (length, 0, 64, -1, 0) if go_on else None
                return length, 0, k + 16, -1, 0
            if k + run > 63:
                return (length, 0, 64, -1, 0) if go_on else None
            idx, nk = k + run, k + run + 1
        v = self.take(bits, at + length, size)
        if size and v < (1 << (size - 1)):
            v += (-1 << size) + 1
        return length, size, nk, idx, v


def trace(scan: bytes, huffman: np.ndarray, mcus: int):
    """The symbols of a well-formed scan in the STUFFED stream: [(first bit, first bit behind the code, first bit behind the symbol,
    block index)]; bit positions count the stuffed bytes' bits too."""
    s = _Stream(scan, huffman)
    byte_of_data = s.byte_of_data

    def stuffed(u: int) -> int:   # (a boundary behind a 0xFF points behind its stuffed byte, as the decoder's states do)
        if u >= s.total:
            return 8 * s.nbytes
        return 8 * byte_of_data[u >> 3] + (u & 7)

    out, at, slot, k, blk = [], 0, 0, 0, 0
    while blk < 6 * mcus:
        got = s.symbol(s.bits, at, slot, k)
        assert got is not None and at < s.total
        length, size, nk, _, _ = got
        out.append((stuffed(at), stuffed(at + length), stuffed(at + length + size), blk))
        at += length + size
        k = nk
        if k == 64:
            k, slot, blk = 0, (slot + 1) % 6, blk + 1
    return out


# ---------------------------------------------------------------------------------------------------- the three passes
def lanes_decode(scan: bytes, huffman: np.ndarray, mcus: int, subseq: int, lanes: int = 8, mutant: Optional[str] = None):
    """One segment -> (levels [mcus, 6, 64] with DC DIFFERENCES at index 0, rounds of pass B).  For well-formed scans."""
    assert mutant is None or mutant in MUTANTS
    s = _Stream(scan, huffman)
    out = np.zeros((mcus + 1, 6, 64), dtype=np.int64)   # (one MCU of slack for the wrong decoders)
    total_blocks = 6 * mcus

    def run(at, slot, k, end, first_block=None):
        """Symbols from `at` until one would start at or behind `end` -> (at, slot, k, blocks).  A guessing lane goes on over what is
        no symbol, by the device's rules."""
        blocks, bits, shift = 0, s.bits, 0
        if mutant == "stuffing_not_skipped" and at % 8 == 0 and 0 < at < s.total and scan[s.byte_of_data[at // 8] - 1] == 0 \
                and s.stuffing[s.byte_of_data[at // 8] - 1] and (s.byte_of_data[at // 8] - 1) % subseq == 0:
            bits, shift, end = s.bits[:at] + [0] * 8 + s.bits[at:], 8, end + 8   # the 0x00 at the boundary read as eight data bits
        if first_block is not None and mutant == "straddler_zeroes" and k and first_block < total_blocks:
            out.reshape(-1, 64)[first_block, 1:] = 0
        while at < end:
            if first_block is not None and first_block + blocks >= total_blocks:
                break
            length, size, nk, idx, v = s.symbol(bits, at, slot, k, go_on=True)
            if first_block is not None and idx >= 0 and v:
                out.reshape(-1, 64)[first_block + blocks, s.zigzag[idx]] = v
            at += length + size
            k = nk
            if k == 64:
                k, slot, blocks = 0, (slot + 1) % 6, blocks + 1
        return at - shift, slot, k, blocks

    nsub = -(-s.nbytes // subseq)
    carry, base, rounds = (0, 0, 0), 0, 0
    for c0 in range(0, nsub, lanes):
        n = min(lanes, nsub - c0)
        ends = [s.ubit_of_byte[min((c0 + j + 1) * subseq, s.nbytes)] for j in range(n)]
        starts, exits, counts = [], [], []
        for j in range(n):   # pass A
            start = carry if j == 0 else (s.ubit_of_byte[(c0 + j) * subseq], 0, 0)
            got = run(start[0], start[1], start[2], ends[j])
            starts.append(start)
            exits.append(got[:3])
            counts.append(got[3])
        for _ in range(n):   # pass B
            rounds += 1
            new_exits, changed = list(exits), False
            for j in range(1, n):
                if exits[j - 1] != starts[j]:
                    starts[j] = exits[j - 1]
                    got = run(starts[j][0], starts[j][1], starts[j][2], ends[j])
                    new = got[:3]
                    counts[j] = got[3]
                    changed |= new != exits[j]
                    new_exits[j] = new
            exits = new_exits
            if not changed or mutant == "one_round":
                break
        first = base
        for j in range(n):   # pass C
            run(starts[j][0], starts[j][1], starts[j][2], ends[j], first_block=min(first, total_blocks))
            first += counts[j]
        base = 0 if mutant == "counts_not_carried" else first
        carry = exits[n - 1]
    return out[:mcus], rounds


def lanes_decode_file(data: bytes, subseq: int, lanes: int = 8, mutant: Optional[str] = None):
    """A whole file through lanes_decode, segment by segment, and the DC scan -> (levels [mh, mw, 6, 64], rounds)."""
    p = jpeg.parse_file(data, restart=True)
    mh, mw = mcus_of(p)
    out = np.zeros((mh * mw, 6, 64), dtype=np.int64)
    rounds = 0
    for off, nb, first, count in p.segments:
        levels, r = lanes_decode(data[off:off + nb], p.huffman, count, subseq, lanes, mutant)
        out[first:first + count] = levels
        rounds += r
    for off, nb, first, count in (p.segments if mutant != "dc_not_restarted" else ((0, 0, 0, mh * mw),)):
        seg = out[first:first + count]
        seg[:, :4, 0] = np.cumsum(seg[:, :4, 0].reshape(-1)).reshape(-1, 4)
        seg[:, 4, 0] = np.cumsum(seg[:, 4, 0])
        seg[:, 5, 0] = np.cumsum(seg[:, 5, 0])
    return out.reshape(mh, mw, 6, 64), rounds


# ---------------------------------------------------------------------------------------------------- hostile scans
def scan_case(data: bytes):
    """A file without restart markers -> (huffman, MCUs, its scan)."""
    p = jpeg.parse_file(data)
    mh, mw = mcus_of(p)
    return p.huffman, mh * mw, data[p.scan_offset:p.scan_offset + p.scan_bytes]


def flips(scan: bytes, count: int, seed: int) -> List[bytes]:
    out = []
    for at in np.random.RandomState(seed).choice(8 * len(scan), size=count, replace=False):
        s = bytearray(scan)
        s[at >> 3] ^= 0x80 >> (at & 7)
        out.append(bytes(s))
    return out


def hostile_small() -> List[bytes]:
    """Hostile variants of a one-MCU scan of 299 bytes (16 x 16 noise, quality 95): what tests/test_jpeg_lanes_host.py puts through the
    sanitizers, and tests/test_gpu_jpeg_lanes.py then feeds to the device."""
    _, _, scan = scan_case(file_of("one_mcu"))
    out = [scan[:k] for k in range(len(scan))]                      # every proper prefix, the empty scan among them
    out += flips(scan, 200, 5)
    out += [b"\xff" * len(scan), b"\x00" * len(scan), b"\xff" * 40000, b"\x00" * 40000, scan + scan, scan + b"\xff\xd9", scan + b"\x00"]
    return out


def hostile_large(chunk: int = 256 * SUBSEQ) -> List[bytes]:
    """Hostile variants of the 501 x 501 case's scan: 65 765 bytes, three chunks of 256 subsequences of 128 bytes; cuts around the
    first chunk's end."""
    _, _, scan = scan_case(file_of("size_501x501"))
    out = [scan[:len(scan) // 2], scan[:chunk + 1], scan[:chunk], scan[:chunk - 1], scan[:-1], scan + scan]
    out += flips(scan, 6, 7)
    return out
