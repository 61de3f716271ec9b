// jpeg_entropy.h -- the entropy decoder of a baseline JPEG scan (ITU-T T.81 Annex F.2.2), one image per caller, written so that the
// SAME function bodies compile for the device (jpeg_decode.hip: one wavefront of 64 lanes per image) and, with g++, for the host
// (tests/host/jpeg_decode_host.cpp: one "lane", under AddressSanitizer and UBSan).  The input comes from files on disk: nothing in
// it may make the decoder read outside scan[0 .. nbytes), write outside its outputs, or loop without end.
//
// What it decodes: 8-bit, three components, 4:2:0, one interleaved scan without restart intervals, MCU = Y0 Y1 Y2 Y3 Cb Cr; the scan
// as it stands in the file (stuffed, padded, no header, no EOI), at any byte alignment.  The MCU's block pattern is a template
// argument (JeSampling: 4:2:0 by default, 4:2:2 = Y0 Y1 Cb Cr, 4:4:4 = Y Cb Cr, greyscale = Y); nothing else depends on it.
//   DC      the category's Huffman code, then that many value bits with the EXTEND rule; a predictor per component that runs across
//           the whole scan
//   AC      (run << 4 | size) symbols in zigzag order; 0xF0 (ZRL) skips 16 positions, 0x00 (EOB) ends the block
//   codes   a look-ahead table of JE_LOOK bits (length << 8 | symbol; 0: longer than that), then Annex F.2.2.3's maxcode walk for the
//           lengths JE_LOOK + 1 .. 16.  The look-ahead is expanded from maxcode / valoff / huffval (je_make_tables, on the host, from
//           the file's BITS and HUFFVAL) into the caller's shared memory by the lanes themselves: 2048 entries, 32 per lane.
//   bytes   the lanes copy the scan into shared memory in runs of 64 consecutive bytes (je_restage), JE_STAGE bytes at a time; the
//           bit reader takes four bytes at once when none of them is 0xFF, else one byte, dropping the 0x00 stuffed behind a 0xFF.
//           Every lane runs the symbol loop on the same values (on the device they are made wave-uniform with readfirstlane, so the
//           loop is scalar code); lane 0 alone writes the block, and all lanes store it: 128 contiguous bytes of int16 in NATURAL
//           order.
// Bounds: the byte position never passes nbytes (bits asked for beyond it are zeros that are COUNTED: once one of them has been
// consumed the image fails with JE_TRUNCATED); the coefficient index never passes 63; a code that is not in the table fails; a DC
// category above 11 or a predictor outside +-2047 fails; every iteration of the AC loop consumes a code of at least one bit or ends.
// A failing image keeps what it had decoded, every later coefficient is zero, and the loop over blocks runs to its fixed end.
// Integer arithmetic and plain stores only.
#ifndef SALVE_JPEG_ENTROPY_H
#define SALVE_JPEG_ENTROPY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define JE_FN __host__ __device__ __forceinline__
#else
#define JE_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define JE_SYNC() __syncthreads()
#define JE_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))   // the value is the same in every lane: keep it in a scalar register
#else
#define JE_SYNC() ((void)0)
#define JE_UNI(x) ((uint32_t)(x))
#endif

// bits of an image's status word (include/salve_hip.h: SALVE_JPEG_*)
#define JE_BAD_CODE 1u       // a bit pattern that is no code of the table
#define JE_COEF_OVERRUN 2u   // a run that passes coefficient 63
#define JE_TRUNCATED 4u      // the scan ended before the last MCU
#define JE_DC_RANGE 8u       // a DC category above 11, or a DC predictor outside +-2047
#define JE_LEFTOVER 16u      // more than 7 bits left behind the last MCU, or pad bits that are not all 1
#define JE_MARKER 32u        // 0xFF followed by something other than 0x00 inside the scan, or as its last byte
#define JE_BAD_SLOT 64u      // (set by the kernel) the image's offset / length do not lie inside the scan buffer with its padding

#define JE_LOOK 9            // look-ahead bits: 4 tables x 512 entries x 2 bytes = 4 KB (a full 16-bit table per Huffman table does not fit)
#define JE_STAGE 4096        // staged scan bytes (a multiple of 4)
#define JE_TABLE_BYTES 272   // 16 BITS + 256 HUFFVAL per table; the four tables: DC luma, AC luma, DC chroma, AC chroma

// The samplings (include/salve_hip.h: SALVE_JPEG_SAMPLING_*) and what the entropy stage needs of one: the blocks of an MCU and the
// component of block slot k (0 Y, 1 Cb, 2 Cr).  A compile-time argument everywhere: no lane branches on it.
#define JE_SAMPLING_420 0    // Y0 Y1 Y2 Y3 Cb Cr
#define JE_SAMPLING_422 1    // Y0 Y1 Cb Cr
#define JE_SAMPLING_444 2    // Y Cb Cr
#define JE_SAMPLING_GREY 3   // Y (one component: the "MCU" of its non-interleaved scan is one block)
#define JE_MAX_BLOCKS 6      // blocks of the largest MCU

template <int S>
struct JeSampling {
    static_assert(S >= JE_SAMPLING_420 && S <= JE_SAMPLING_GREY, "a sampling of JE_SAMPLING_*");
    static constexpr int blocks = S == JE_SAMPLING_420 ? 6 : S == JE_SAMPLING_422 ? 4 : S == JE_SAMPLING_444 ? 3 : 1;
    static constexpr int luma = S == JE_SAMPLING_GREY ? 1 : blocks - 2;   // the luma blocks lead the MCU
    static constexpr int coefs = blocks * 64;                              // coefficients of an MCU
};

template <int S>
JE_FN int je_comp(int slot) { return slot < JeSampling<S>::luma ? 0 : slot - JeSampling<S>::luma + 1; }

struct JeTables {            // Annex F.2.2.3's decoder tables, by table and code length 1 .. 16
    int32_t maxcode[4][17];  // the largest code of that length, -1: none
    int32_t valoff[4][17];   // index of the length's first symbol in huffval, minus its first code
    uint8_t huffval[4][256];
};

struct JeShared {            // LDS on the device: 9.8 KB per image in flight
    uint16_t look[4][1 << JE_LOOK];
    int32_t maxcode[4][17];
    int32_t valoff[4][17];
    uint8_t huffval[4][256];
    uint32_t stage[JE_STAGE / 4 + 1];   // one word of slack: the four-byte path reads two whole words
    int16_t blk[64];
    uint8_t nat[64];                    // natural (row-major) index of zigzag position k
};

struct JeReader {
    const uint8_t* src;
    int32_t nbytes;          // bytes of the scan (cut short at a marker)
    int32_t base, staged;    // stage[] holds src[base .. base + staged)
    int32_t pos;             // next byte to take
    int32_t cnt, fake;       // valid bits at the low end of acc; how many of them (the lowest) are zeros from beyond the scan
    uint64_t acc;
    uint32_t status;
    int lane, nlanes;
};

// HOST: BITS / HUFFVAL of the four tables -> the decoder tables.  false: a BITS array that over-subscribes the code space or sums
// past 256.
static inline bool je_make_tables(const uint8_t* huffman, JeTables* out) {
    for (int t = 0; t < 4; t++) {
        const uint8_t* bits = huffman + t * JE_TABLE_BYTES;
        int32_t code = 0, k = 0;
        for (int l = 1; l <= 16; l++) {
            const int32_t c = bits[l - 1];
            if (code + c > (1 << l) || k + c > 256) return false;
            out->maxcode[t][l] = c ? code + c - 1 : -1;
            out->valoff[t][l] = k - code;
            code = (code + c) << 1;
            k += c;
        }
        out->maxcode[t][0] = -1;
        out->valoff[t][0] = 0;
        for (int i = 0; i < 256; i++) out->huffval[t][i] = bits[16 + i];
    }
    return true;
}

// All lanes: the tables into shared memory, the look-ahead expanded from them.  Sh: JeShared, or jpeg_entropy_lanes.h's JlShared
// (the members look, maxcode, valoff, huffval and nat).
template <class Sh>
JE_FN void je_prepare_tables(Sh& sh, const JeTables& tab, int lane, int nlanes) {
    constexpr uint8_t zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    for (int j = lane; j < 64; j += nlanes) sh.nat[j] = zigzag[j];
    for (int j = lane; j < 4 * 17; j += nlanes) {
        sh.maxcode[j / 17][j % 17] = tab.maxcode[j / 17][j % 17];
        sh.valoff[j / 17][j % 17] = tab.valoff[j / 17][j % 17];
    }
    for (int j = lane; j < 4 * 256; j += nlanes) sh.huffval[j >> 8][j & 255] = tab.huffval[j >> 8][j & 255];
    JE_SYNC();
    for (int e = lane; e < 4 << JE_LOOK; e += nlanes) {
        const int t = e >> JE_LOOK, p = e & ((1 << JE_LOOK) - 1);
        uint32_t entry = 0;
        for (int l = 1; l <= JE_LOOK; l++) {
            const int32_t code = p >> (JE_LOOK - l);
            if (code <= sh.maxcode[t][l]) {
                entry = ((uint32_t)l << 8) | sh.huffval[t][(sh.valoff[t][l] + code) & 255];
                break;
            }
        }
        sh.look[t][e & ((1 << JE_LOOK) - 1)] = (uint16_t)entry;
    }
    JE_SYNC();
}

JE_FN void je_prepare(JeShared& sh, const JeTables& tab, int lane, int nlanes) {
    for (int j = lane; j < 64; j += nlanes) sh.blk[j] = 0;
    for (int j = lane; j < JE_STAGE / 4 + 1; j += nlanes) sh.stage[j] = 0;
    je_prepare_tables(sh, tab, lane, nlanes);
}

// All lanes: stage[] <- src[pos ..), 64 consecutive bytes per step.  Called with pos < nbytes.
JE_FN void je_restage(JeShared& sh, JeReader& r) {
    JE_SYNC();
    r.base = r.pos;
    const int32_t left = r.nbytes - r.base;
    r.staged = left < JE_STAGE ? left : JE_STAGE;
    uint8_t* st = reinterpret_cast<uint8_t*>(sh.stage);
#pragma unroll 4
    for (int32_t j = r.lane; j < r.staged; j += r.nlanes) st[j] = r.src[(int64_t)r.base + j];
    JE_SYNC();
}

JE_FN uint32_t je_byte(const JeShared& sh, int32_t o) { return (JE_UNI(sh.stage[o >> 2]) >> (8 * (o & 3))) & 255u; }

// More than 32 valid bits into acc: four bytes at once where none is 0xFF, else a byte at a time (unstuffing); zeros, counted in
// `fake`, beyond the scan's end.
JE_FN void je_fill(JeShared& sh, JeReader& r) {
    while (r.cnt <= 32) {
        const int32_t o = r.pos - r.base;
        if (o + 4 <= r.staged) {
            const uint32_t lo = JE_UNI(sh.stage[o >> 2]), hi = JE_UNI(sh.stage[(o >> 2) + 1]);
            const uint32_t s8 = 8u * (uint32_t)(o & 3);
            const uint32_t w = __builtin_bswap32(s8 ? (lo >> s8) | (hi << (32u - s8)) : lo);
            if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {   // no byte of w is 0xFF
                r.acc = (r.acc << 32) | w;
                r.cnt += 32;
                r.pos += 4;
                continue;
            }
        }
        if (r.pos >= r.nbytes) {
            r.acc <<= 8;
            r.cnt += 8;
            r.fake += 8;
            continue;
        }
        if (r.pos - r.base >= r.staged) je_restage(sh, r);
        const uint32_t b = je_byte(sh, r.pos - r.base);
        r.pos++;
        if (b == 0xFFu) {
            uint32_t next = 1;   // a scan whose last byte is 0xFF: as a marker
            if (r.pos < r.nbytes) {
                if (r.pos - r.base >= r.staged) je_restage(sh, r);
                next = je_byte(sh, r.pos - r.base);
            }
            if (next != 0) {     // a marker: the scan ends in front of it
                r.status |= JE_MARKER;
                r.pos -= 1;
                r.nbytes = r.pos;
                r.staged = r.pos - r.base;
                continue;
            }
            r.pos++;
        }
        r.acc = (r.acc << 8) | b;
        r.cnt += 8;
    }
}

// The next symbol of table t (0 .. 255), or -1.  Needs cnt >= 16; consumes the code's 1 .. 16 bits.
JE_FN int32_t je_symbol(const JeShared& sh, JeReader& r, int t) {
    const uint32_t p = (uint32_t)(r.acc >> (r.cnt - 16)) & 0xFFFFu;
    const uint32_t e = JE_UNI(sh.look[t][p >> (16 - JE_LOOK)]);
    if (e) {
        r.cnt -= (int32_t)(e >> 8);
        return (int32_t)(e & 255u);
    }
    for (int l = JE_LOOK + 1; l <= 16; l++) {
        const int32_t code = (int32_t)(p >> (16 - l));
        if (code <= (int32_t)JE_UNI(sh.maxcode[t][l])) {
            r.cnt -= l;
            return (int32_t)JE_UNI(sh.huffval[t][((int32_t)JE_UNI(sh.valoff[t][l]) + code) & 255]);
        }
    }
    return -1;
}

// s value bits (0 .. 15) and T.81's EXTEND.  Needs cnt >= s.
JE_FN int32_t je_value(JeReader& r, int32_t s) {
    const int32_t v = (int32_t)((uint32_t)(r.acc >> (r.cnt - s)) & ((1u << s) - 1u));
    r.cnt -= s;
    return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// All lanes: the scan of one image -> coef [mcus][blocks of an MCU][64] int16 in natural order ([mcus][6][64] for the default, 4:2:0);
// returns the status word (the same in every lane).
template <int S = JE_SAMPLING_420>
JE_FN uint32_t je_decode_image(JeShared& sh, const uint8_t* scan, int32_t nbytes, int32_t mcus, int16_t* coef, int lane, int nlanes) {
    JeReader r;
    r.src = scan;
    r.nbytes = nbytes > 0 ? nbytes : 0;
    r.base = r.staged = r.pos = r.cnt = r.fake = 0;
    r.acc = 0;
    r.status = 0;
    r.lane = lane;
    r.nlanes = nlanes;
    int32_t pred[3] = {0, 0, 0};
    bool dead = false;
    for (int32_t m = 0; m < mcus; m++) {
        for (int b = 0; b < JeSampling<S>::blocks; b++) {
            const int comp = je_comp<S>(b), t = comp ? 2 : 0;
            if (!dead) {   // DC
                je_fill(sh, r);
                const int32_t s = r.status ? -2 : je_symbol(sh, r, t);
                if (s < 0) {
                    if (s == -1) r.status |= JE_BAD_CODE;
                    dead = true;
                } else if (s > 11) {
                    r.status |= JE_DC_RANGE;
                    dead = true;
                } else {
                    const int32_t dc = pred[comp] + je_value(r, s);
                    if (r.cnt < r.fake) {
                        r.status |= JE_TRUNCATED;
                        dead = true;
                    } else if (dc < -2047 || dc > 2047) {
                        r.status |= JE_DC_RANGE;
                        dead = true;
                    } else {
                        pred[comp] = dc;
                        if (lane == 0) sh.blk[0] = (int16_t)dc;
                    }
                }
            }
            int32_t k = 1;
            while (!dead && k < 64) {   // AC: every turn consumes a code or ends
                je_fill(sh, r);
                const int32_t rs = r.status ? -2 : je_symbol(sh, r, t + 1);
                if (rs < 0) {
                    if (rs == -1) r.status |= JE_BAD_CODE;
                    dead = true;
                    break;
                }
                const int32_t run = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (r.cnt < r.fake) {
                        r.status |= JE_TRUNCATED;
                        dead = true;
                        break;
                    }
                    if (run != 15) break;   // EOB (T.81 gives the runs 1 .. 14 with size 0 no meaning in a sequential scan: as libjpeg, EOB)
                    k += 16;
                    if (k > 64) {
                        r.status |= JE_COEF_OVERRUN;
                        dead = true;
                    }
                    continue;
                }
                k += run;
                if (k > 63) {
                    r.status |= JE_COEF_OVERRUN;
                    dead = true;
                    break;
                }
                const int32_t v = je_value(r, s);
                if (r.cnt < r.fake) {
                    r.status |= JE_TRUNCATED;
                    dead = true;
                    break;
                }
                if (lane == 0) sh.blk[JE_UNI(sh.nat[k])] = (int16_t)v;
                k++;
            }
            JE_SYNC();
            int16_t* out = coef + ((int64_t)m * JeSampling<S>::blocks + b) * 64;
            for (int j = lane; j < 64; j += nlanes) {   // the block leaves as 128 contiguous bytes, and is zero again
                out[j] = sh.blk[j];
                sh.blk[j] = 0;
            }
            JE_SYNC();
        }
    }
    if (!dead) {   // what is left must be the padding: at most 7 bits, all 1
        const int32_t left = r.cnt - r.fake;
        if (r.pos < r.nbytes || left > 7 || ((uint32_t)(r.acc >> r.fake) & ((1u << left) - 1u)) != (1u << left) - 1u) r.status |= JE_LEFTOVER;
    }
    return r.status;
}

#endif  // SALVE_JPEG_ENTROPY_H
