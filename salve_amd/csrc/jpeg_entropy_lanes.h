// jpeg_entropy_lanes.h -- the entropy decoder of a baseline JPEG scan with ONE LANE PER SUBSEQUENCE of the stuffed stream: self-synchronising
// Huffman decoding in the manner of Weissenberger and Schmidt ("Massively Parallel Huffman Decoding on GPUs", ICPP 2018; applied to JPEG
// in "Accelerating JPEG Decompression on GPUs", HiPC 2021).  jpeg_entropy.h walks an image's bits with one wavefront whose symbol loop is
// scalar; here the JL_LANES lanes of a workgroup each decode JE_SUBSEQ bytes, and a Huffman decoder that starts at a wrong bit falls into
// step with the right one after a few symbols.  The SAME function bodies compile for the device (jpeg_decode.hip: one workgroup per scan
// segment) and, with g++, for the host (tests/host/jpeg_lanes_host.cpp under AddressSanitizer and UBSan): on the host the lanes of a phase
// run one after the other (JL_FOR_LANES), and everything a lane keeps from one phase to the next lives in JlShared.
//
// Units: a SEGMENT is a whole scan or one restart interval of it (the marker excluded); it starts with the DC predictors at 0 and holds
//   `mcus` MCUs = 6 * mcus blocks.  It is walked in CHUNKS of JL_LANES subsequences of JE_SUBSEQ bytes.
//   (6 blocks, slots 0..5, coef [mcus][6][64] and mcus * 384 are 4:2:0's, the default of the template argument S; with another of
//   jpeg_entropy.h's JeSampling they read 4 / 3 / 1 blocks, and the slot runs 0 .. blocks - 1.)
// State at a symbol boundary: (bit position in the STUFFED stream, block slot 0..5 of the MCU, zigzag index 0..63, 0: a DC code is next).
//   A boundary behind a 0xFF byte points behind its stuffed 0x00.
// Per chunk:
//   pass A  every lane decodes from the first bit of its subsequence in state (slot 0, index 0) -- a leading stuffed 0x00 skipped -- until
//           a symbol would start at or behind the subsequence's end, and records its exit state and the blocks it completed.  Lane 0
//           starts from the truth: the segment's start, or the converged exit state of the chunk before.
//   pass B  rounds: lane j > 0 looks at lane j - 1's exit state; where that is not what it started from, it decodes again from there.
//           A round that changes nothing ends the pass; by induction from lane 0 every recorded state is then the serial decoder's.
//           At most a round per lane that has bytes.  A lane whose guess was wrong meets things no scan holds: a non-code, a run past
//           coefficient 63, a DC category above 11.  None of them is an error there, and none of them stops the lane: it goes on by fixed
//           rules (jl_run), because a lane that gives up cannot fall into step, and falling into step takes long enough as it is -- the
//           bit position agrees within a few bytes, the zigzag index at the next end of block, but the block SLOT only where the luma
//           and chroma tables have thrown the two decoders apart and together again: some 110 bytes in the median, up to 1 KB
//           (DESIGN.md 4.20).  Lanes that gave up instead left 227 of a chunk's 256 lanes (of 32 bytes) to be reached a round at a time.
//   pass C  a prefix sum of the block counts gives each lane its first block; the lane decodes once more and stores every non-zero
//           coefficient at its natural-order place of the PRE-ZEROED coefficients (a DC code leaves its DIFFERENCE).  A block that
//           straddles two lanes is written by both, at different indices.  Blocks at or behind 6 * mcus are never written.  Errors are
//           taken from this pass alone: every lane now starts from the truth, so what it meets IS in the scan.  (Behind the first
//           such thing the serial decoder stops; this one goes on by jl_run's rules, in every pass alike: one deterministic walk.)
// After the last chunk a scan over each component's blocks turns the DC differences into values (restarted per segment, as T.81 E.1.4).
// Bounds: no byte at or behind scan + nbytes is read (bits asked for beyond it are zeros that are counted, and a symbol that consumes
//   one is reported as JE_TRUNCATED by pass C and leaves the position behind every end); no coefficient outside coef[0 .. mcus * 384)
//   is written; every loop has a trip count known on entry (chunks, rounds, scan steps) or consumes at least one bit per turn of at
//   most 8 * nbytes.  Integer arithmetic and plain stores only; every
//   coefficient has one writer.
// Status (the bits of jpeg_entropy.h): 0 for a well-formed segment, non-zero exactly when jpeg_entropy.h's decoder reports the same
//   bytes (the bits themselves may differ: this decoder checks the DC range after the scan and names the first thing IT meets).
#ifndef SALVE_JPEG_ENTROPY_LANES_H
#define SALVE_JPEG_ENTROPY_LANES_H

#include "jpeg_entropy.h"

#ifndef JE_SUBSEQ
#define JE_SUBSEQ 128        // bytes of the stuffed stream per lane (a multiple of 4; profiles/r11_lane_entropy.txt has the alternatives tried)
#endif
#ifndef JL_LANES
#define JL_LANES 256         // subsequences per chunk = threads of the workgroup
#endif
#define JL_CHUNK (JL_LANES * JE_SUBSEQ)
#define JL_SLACK 64          // staged bytes behind the chunk: the last lane's final symbol and the reader's look-ahead (at most 12 bytes)
// The lanes read bytes JE_SUBSEQ apart: 4 bytes of padding per subsequence put them an odd number of words apart -- 64 lanes on 64 banks.
#define JL_STAGED(o) ((o) + (((o) / JE_SUBSEQ) << 2))
#define JL_STAGE_BYTES (JL_STAGED(JL_CHUNK + JL_SLACK) + 4)
#define JL_MAX_BYTES (1 << 27)   // a segment's bytes: bit positions stay below 2^30

#if defined(__HIP_DEVICE_COMPILE__)
#define JL_FOR_LANES(lane) for (int lane = (int)threadIdx.x, jl_once = 0; jl_once < 1; jl_once++)
#else
#define JL_FOR_LANES(lane) for (int lane = 0; lane < JL_LANES; lane++)
#endif

struct JlShared {            // LDS on the device: 53 KB per segment in flight (33 KB of it the staged chunk)
    uint16_t look[4][1 << JE_LOOK];
    int32_t maxcode[4][17];
    int32_t valoff[4][17];
    uint8_t huffval[4][256];
    uint8_t nat[64];
    uint8_t stage[JL_STAGE_BYTES];
    int32_t start_pos[JL_LANES];       // the state the lane last decoded from
    uint32_t start_sk[JL_LANES];       // slot << 8 | index
    int32_t exit_pos[2][JL_LANES];     // ping-pong by round
    uint32_t exit_sk[2][JL_LANES];     // slot << 8 | index
    int32_t count[JL_LANES];           // blocks completed by the lane
    int32_t scan[2][3][JL_LANES];      // prefix sums: the block counts, then the DC sums per component
    int32_t changed[3];                // pass B: did round r change an exit state (rotating, so that a flag is cleared a barrier away from its readers)
    int32_t carry_pos;                 // the true state at the next chunk's first bit
    uint32_t carry_sk;
    int32_t base;                      // blocks completed in front of the chunk
    int32_t done;                      // a lane completed the segment's last block (and looked at what follows it)
    int32_t dc_bad;                    // a DC value outside +-2047
    int32_t any_err;                   // pass C: a lane met something that no well-formed scan holds
    uint32_t lane_err[JL_LANES];
    uint32_t status;
};

struct JlSegment {           // include/salve_hip.h: salve_jpeg_segment_t
    int64_t offset;          // the segment's first byte in the scan buffer
    int32_t bytes;
    int32_t image;
    int32_t first_mcu, mcu_count;
};

// Does the segment lie inside a buffer of scans_size bytes (with its JE-padding of 16 behind it) and inside an image of `mcus` MCUs?
JE_FN bool jl_segment_inside(const JlSegment& s, uint64_t scans_size, int32_t mcus) {
    if (s.offset < 0 || s.bytes < 0 || s.bytes > JL_MAX_BYTES || (uint64_t)s.offset + (uint64_t)s.bytes + 16u > scans_size) return false;
    return s.first_mcu >= 0 && s.mcu_count >= 1 && (int64_t)s.first_mcu + s.mcu_count <= mcus;
}

struct JlReader {
    const JlShared* sh;
    int32_t nbytes;          // bytes of the segment
    int32_t base, staged;    // stage[] holds the segment's bytes base .. base + staged
    int32_t pos;             // next byte to take
    int32_t cnt, fake;       // valid bits at the low end of acc; how many of them (the lowest) are zeros from beyond the segment
    uint64_t acc;
    uint64_t stf;            // bit b set: acc's bit b is the lowest bit of a 0xFF whose stuffed 0x00 was skipped
    uint32_t marker;         // a 0xFF that no 0x00 follows was taken
};

JE_FN uint32_t jl_byte(const JlReader& r, int32_t p) {
    const uint32_t o = (uint32_t)(p - r.base);
    return o < (uint32_t)r.staged ? r.sh->stage[JL_STAGED(o)] : 0u;
}

// The reader at bit position p (0 <= p <= 8 * nbytes).  spec: p is a lane's guess (the first bit of its subsequence, which is not the
// segment's or the chunk's first byte): a 0x00 there that follows a 0xFF is stuffing.
JE_FN void jl_start(JlReader& r, int32_t p, bool spec) {
    r.pos = p >> 3;
    r.cnt = r.fake = 0;
    r.acc = r.stf = 0;
    r.marker = 0;
    const int bit = p & 7;
    if (bit && r.pos < r.nbytes) {
        const uint32_t b = jl_byte(r, r.pos);
        r.pos++;
        r.acc = b & (0xFFu >> bit);
        r.cnt = 8 - bit;
        if (b == 0xFFu) {
            if (r.pos < r.nbytes && jl_byte(r, r.pos) == 0) {
                r.pos++;
                r.stf = 1;
            } else {
                r.marker = 1;
            }
        }
    } else if (spec && r.pos < r.nbytes && jl_byte(r, r.pos) == 0 && jl_byte(r, r.pos - 1) == 0xFFu) {
        r.pos++;
    }
}

// More than 32 valid bits into acc (at most 40), a byte at a time, dropping the 0x00 stuffed behind a 0xFF; zeros, counted in `fake`,
// beyond the end.  (jpeg_entropy.h's four-bytes-at-once path was tried here and LOST 15 %: four more LDS reads per turn in every lane
// whose neighbours take the byte path -- profiles/r11_lane_entropy.txt.)
JE_FN void jl_fill(JlReader& r) {
    while (r.cnt <= 32) {
        r.acc <<= 8;
        r.stf <<= 8;
        r.cnt += 8;
        if (r.pos >= r.nbytes) {
            r.fake += 8;
            continue;
        }
        const uint32_t b = jl_byte(r, r.pos);
        r.pos++;
        r.acc |= b;
        if (b == 0xFFu) {
            if (r.pos < r.nbytes && jl_byte(r, r.pos) == 0) {
                r.pos++;
                r.stf |= 1;
            } else {
                r.marker = 1;
            }
        }
    }
}

// The stuffed-stream bit position of the next bit: the bytes taken, less the bits still held and the stuffed bytes behind them.
JE_FN int32_t jl_bitpos(const JlReader& r) {
    const uint64_t held = r.stf & ((1ull << r.cnt) - 1ull);   // (cnt <= 40)
    return 8 * r.pos + r.fake - r.cnt - 8 * (int32_t)__builtin_popcountll(held);
}

JE_FN int32_t jl_symbol(const JlShared& sh, JlReader& r, int t) {   // je_symbol, per lane
    const uint32_t p = (uint32_t)(r.acc >> (r.cnt - 16)) & 0xFFFFu;
    const uint32_t e = sh.look[t][p >> (16 - JE_LOOK)];
    if (e) {
        r.cnt -= (int32_t)(e >> 8);
        return (int32_t)(e & 255u);
    }
    for (int l = JE_LOOK + 1; l <= 16; l++) {
        const int32_t code = (int32_t)(p >> (16 - l));
        if (code <= sh.maxcode[t][l]) {
            r.cnt -= l;
            return (int32_t)sh.huffval[t][(sh.valoff[t][l] + code) & 255];
        }
    }
    return -1;
}

JE_FN int32_t jl_value(JlReader& r, int32_t s) {   // je_value
    const int32_t v = (int32_t)((uint32_t)(r.acc >> (r.cnt - s)) & ((1u << s) - 1u));
    r.cnt -= s;
    return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One lane, one pass: symbols from the reader's position in state sk until one would start at or behind bit `endbit`.  Returns 0, or
// the JE_* bits of what it met that no well-formed scan holds -- and goes on all the same, by rules that only have to be the same in
// every pass: a non-code costs one bit; a DC category above 11 has no value bits; a run past coefficient 63 ends the block.
// blocks: + the blocks completed.  WRITE (pass C): coef is the segment's [mcus][6][64], gb the index of the block the lane starts in,
// total = 6 * mcus; the lane stops in front of block `total`, and the one that completes block total - 1 judges what is left
// (JE_LEFTOVER) and sets *done.
template <bool WRITE, int S = JE_SAMPLING_420>
JE_FN uint32_t jl_run(const JlShared& sh, JlReader& r, int32_t endbit, uint32_t& sk, int32_t& blocks, int16_t* coef, int32_t gb, int32_t total, int32_t* done) {
    int32_t slot = (int32_t)(sk >> 8) & 7, k = (int32_t)(sk & 63u);
    uint32_t err = 0;
    for (;;) {   // every turn consumes at least one bit, or ends
        jl_fill(r);
        if (jl_bitpos(r) >= endbit) break;
        if (WRITE && gb >= total) break;
        const int t = je_comp<S>(slot) ? 2 : 0;
        bool complete = false;
        if (k == 0) {   // DC: the difference stays
            const int32_t s = jl_symbol(sh, r, t);
            if (s < 0) {
                err |= JE_BAD_CODE;
                r.cnt -= 1;
            } else {
                int32_t v = 0;
                if (s > 11) err |= JE_DC_RANGE;
                else v = jl_value(r, s);
                if (WRITE && v) coef[(int64_t)gb * 64] = (int16_t)v;
                k = 1;
            }
        } else {
            const int32_t rs = jl_symbol(sh, r, t + 1);
            const int32_t run = rs >> 4, s = rs & 15;
            if (rs < 0) {
                err |= JE_BAD_CODE;
                r.cnt -= 1;
            } else if (s == 0) {
                if (run != 15) {
                    complete = true;   // EOB (the runs 1 .. 14 with size 0 as well, as jpeg_entropy.h)
                } else {
                    k += 16;
                    if (k > 64) err |= JE_COEF_OVERRUN;
                    complete = k >= 64;
                }
            } else if (k + run > 63) {
                err |= JE_COEF_OVERRUN;
                complete = true;
            } else {
                k += run;
                const int32_t v = jl_value(r, s);
                if (WRITE) coef[(int64_t)gb * 64 + sh.nat[k]] = (int16_t)v;
                k++;
                complete = k == 64;
            }
        }
        if (r.cnt < r.fake) err |= JE_TRUNCATED;   // the symbol took bits from beyond the segment: the position is now behind every end
        if (complete) {
            k = 0;
            slot = slot >= JeSampling<S>::blocks - 1 ? 0 : slot + 1;
            blocks++;
            gb++;
            if (WRITE && gb == total) {   // what is left must be the padding: at most 7 bits, all 1
                jl_fill(r);
                const int32_t left = r.cnt - r.fake;
                if (r.pos < r.nbytes || left < 0 || left > 7 || ((uint32_t)(r.acc >> r.fake) & ((1u << left) - 1u)) != (1u << left) - 1u) err |= JE_LEFTOVER;
                *done = 1;
                break;
            }
        }
    }
    sk = ((uint32_t)slot << 8) | (uint32_t)k;
    if (WRITE && r.marker) err |= JE_MARKER;
    return err;
}

// All lanes: an inclusive prefix sum over the lanes of scan[0][c][..], c < ncomp (Hillis and Steele); returns the array (0 / 1) that holds it.
JE_FN int jl_prefix(JlShared& sh, int ncomp) {
    int cur = 0;
    for (int d = 1; d < JL_LANES; d <<= 1) {
        JE_SYNC();
        JL_FOR_LANES(lane) {
            for (int c = 0; c < ncomp; c++) sh.scan[cur ^ 1][c][lane] = sh.scan[cur][c][lane] + (lane >= d ? sh.scan[cur][c][lane - d] : 0);
        }
        cur ^= 1;
    }
    JE_SYNC();
    return cur;
}

// All lanes of the workgroup: one segment -> coef [mcus][6][64] int16 in natural order, which the caller has ZEROED; returns the status
// word (the same in every lane).  sh holds je_prepare_tables' tables.  rounds (host): + the rounds of pass B.
template <int S = JE_SAMPLING_420>
JE_FN uint32_t jl_decode_segment(JlShared& sh, const uint8_t* scan, int32_t nbytes, int32_t mcus, int16_t* coef, int32_t* rounds) {
    if (nbytes < 0) nbytes = 0;
    if (mcus < 0) mcus = 0;
    constexpr int BLK = JeSampling<S>::blocks;
    const int32_t total = BLK * mcus;
    JE_SYNC();
    JL_FOR_LANES(lane) {
        if (lane == 0) {
            sh.carry_pos = 0;
            sh.carry_sk = 0;
            sh.base = 0;
            sh.done = 0;
            sh.dc_bad = 0;
            sh.any_err = 0;
            sh.status = nbytes > JL_MAX_BYTES ? JE_BAD_SLOT : 0u;
        }
    }
    JE_SYNC();
    const int32_t chunks = sh.status ? 0 : (int32_t)(((int64_t)nbytes + JL_CHUNK - 1) / JL_CHUNK);
    for (int32_t c = 0; c < chunks; c++) {
        const int32_t base = c * JL_CHUNK;
        const int32_t staged = nbytes - base < JL_CHUNK + JL_SLACK ? nbytes - base : JL_CHUNK + JL_SLACK;
        const int32_t active = nbytes - base < JL_CHUNK ? (nbytes - base + JE_SUBSEQ - 1) / JE_SUBSEQ : JL_LANES;   // the lanes that have bytes: 1 .. JL_LANES
        JL_FOR_LANES(lane) {   // the chunk and its slack into LDS, 4 consecutive bytes per lane and step
            for (int32_t j = 4 * lane; j < staged; j += 4 * JL_LANES) {
                const int32_t m = staged - j < 4 ? staged - j : 4;
                if (m == 4) {   // one dword load at whatever alignment the scan has, one aligned dword into LDS
                    uint32_t word;
                    __builtin_memcpy(&word, scan + (int64_t)base + j, 4);
                    __builtin_memcpy(&sh.stage[JL_STAGED(j)], &word, 4);
                } else {
                    for (int32_t i = 0; i < m; i++) sh.stage[JL_STAGED(j) + i] = scan[(int64_t)base + j + i];
                }
            }
            if (lane < 3) sh.changed[lane] = 0;
        }
        JE_SYNC();
        JL_FOR_LANES(lane) {   // pass A
            JlReader r;
            r.sh = &sh;
            r.nbytes = nbytes;
            r.base = base;
            r.staged = staged;
            const int64_t first = (int64_t)base + (int64_t)lane * JE_SUBSEQ, last = first + JE_SUBSEQ;
            const int32_t endbit = 8 * (int32_t)(last < nbytes ? last : nbytes);
            const int32_t p = lane == 0 ? sh.carry_pos : 8 * (int32_t)(first < nbytes ? first : nbytes);
            uint32_t sk = lane == 0 ? sh.carry_sk : 0u;
            sh.start_pos[lane] = p;
            sh.start_sk[lane] = sk;
            int32_t blocks = 0;
            if (lane < active) {
                jl_start(r, p, lane != 0);
                jl_run<false, S>(sh, r, endbit, sk, blocks, nullptr, 0, 0, nullptr);
                sh.exit_pos[0][lane] = jl_bitpos(r);
            } else {
                sh.exit_pos[0][lane] = p;
            }
            sh.exit_sk[0][lane] = sk;
            sh.count[lane] = blocks;
            sh.lane_err[lane] = 0;
        }
        int cur = 0;
        for (int round = 0; round < active; round++) {   // pass B
            JE_SYNC();
            JL_FOR_LANES(lane) {
                int32_t xp = sh.exit_pos[cur][lane];
                uint32_t xs = sh.exit_sk[cur][lane];
                if (lane == 0) sh.changed[(round + 1) % 3] = 0;
                if (lane > 0 && lane < active) {
                    const int32_t pp = sh.exit_pos[cur][lane - 1];
                    const uint32_t ps = sh.exit_sk[cur][lane - 1];
                    uint32_t ns = xs;
                    if (pp != sh.start_pos[lane] || ps != sh.start_sk[lane]) {
                        JlReader r;
                        r.sh = &sh;
                        r.nbytes = nbytes;
                        r.base = base;
                        r.staged = staged;
                        const int64_t last = (int64_t)base + (int64_t)(lane + 1) * JE_SUBSEQ;
                        const int32_t endbit = 8 * (int32_t)(last < nbytes ? last : nbytes);
                        sh.start_pos[lane] = pp;
                        sh.start_sk[lane] = ps;
                        jl_start(r, pp, false);
                        uint32_t sk = ps;
                        int32_t blocks = 0;
                        jl_run<false, S>(sh, r, endbit, sk, blocks, nullptr, 0, 0, nullptr);
                        xp = jl_bitpos(r);
                        ns = sk;
                        sh.count[lane] = blocks;
                    }
                    if (xp != sh.exit_pos[cur][lane] || ns != xs) sh.changed[round % 3] = 1;
                    xs = ns;
                }
                sh.exit_pos[cur ^ 1][lane] = xp;
                sh.exit_sk[cur ^ 1][lane] = xs;
            }
            cur ^= 1;
            JE_SYNC();
            if (rounds) *rounds += 1;
            if (!sh.changed[round % 3]) break;
        }
        JL_FOR_LANES(lane) { sh.scan[0][0][lane] = sh.count[lane]; }
        const int at = jl_prefix(sh, 1);
        const int32_t before = sh.base;
        JL_FOR_LANES(lane) {   // pass C
            const int64_t gb = (int64_t)before + sh.scan[at][0][lane] - sh.count[lane];
            if (lane < active && gb < total) {
                JlReader r;
                r.sh = &sh;
                r.nbytes = nbytes;
                r.base = base;
                r.staged = staged;
                const int64_t last = (int64_t)base + (int64_t)(lane + 1) * JE_SUBSEQ;
                const int32_t endbit = 8 * (int32_t)(last < nbytes ? last : nbytes);
                jl_start(r, sh.start_pos[lane], false);
                uint32_t sk = sh.start_sk[lane];
                int32_t blocks = 0;
                const uint32_t err = jl_run<true, S>(sh, r, endbit, sk, blocks, coef, (int32_t)gb, total, &sh.done);
                if (err) {
                    sh.lane_err[lane] = err;
                    sh.any_err = 1;   // (several lanes may: the same value)
                }
            }
        }
        JE_SYNC();
        JL_FOR_LANES(lane) {
            if (lane == 0) {
                const int64_t sum = (int64_t)before + sh.scan[at][0][JL_LANES - 1];
                sh.base = sum < total ? (int32_t)sum : total;
                sh.carry_pos = sh.exit_pos[cur][active - 1];
                sh.carry_sk = sh.exit_sk[cur][active - 1];
                if (sh.any_err)
                    for (int j = 0; j < JL_LANES; j++) sh.status |= sh.lane_err[j];
            }
        }
        JE_SYNC();
        if (sh.status || sh.done) break;
    }
    JE_SYNC();
    // the DC differences -> values: each lane takes a run of MCUs; sums, a prefix sum over the lanes, the running values
    const int32_t per = (mcus + JL_LANES - 1) / JL_LANES;
    JL_FOR_LANES(lane) {
        const int32_t lo = lane * per < mcus ? lane * per : mcus, hi = lo + per < mcus ? lo + per : mcus;
        int32_t s[3] = {0, 0, 0};
        for (int32_t m = lo; m < hi; m++)
            for (int b = 0; b < BLK; b++) s[je_comp<S>(b)] += coef[((int64_t)m * BLK + b) * 64];
        for (int cmp = 0; cmp < 3; cmp++) sh.scan[0][cmp][lane] = s[cmp];
    }
    const int at = jl_prefix(sh, 3);
    JL_FOR_LANES(lane) {
        const int32_t lo = lane * per < mcus ? lane * per : mcus, hi = lo + per < mcus ? lo + per : mcus;
        int32_t s[3];
        for (int cmp = 0; cmp < 3; cmp++) s[cmp] = lane ? sh.scan[at][cmp][lane - 1] : 0;
        bool bad = false;
        for (int32_t m = lo; m < hi; m++)
            for (int b = 0; b < BLK; b++) {
                int16_t* dc = coef + ((int64_t)m * BLK + b) * 64;
                int32_t& v = s[je_comp<S>(b)];
                v += *dc;
                bad |= v < -2047 || v > 2047;
                *dc = (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
            }
        if (bad) sh.dc_bad = 1;   // (several lanes may: the same value)
    }
    JE_SYNC();
    const uint32_t status = sh.status ? sh.status : (sh.done ? 0u : JE_TRUNCATED);
    return status | (sh.dc_bad ? JE_DC_RANGE : 0u);
}

#endif  // SALVE_JPEG_ENTROPY_LANES_H
