// jpeg_encode.hip -- the entropy-coded scan of baseline 4:2:0 JPEG on gfx950 (MI355X), byte for byte what libjpeg writes with its
// defaults (opt-in: BevRasteriser.jpeg_encode, render_dataset.render_building_floor_pairs(jpeg="device")).
//
// The reference writes every BEV render as a JPEG (imageio -> Pillow -> libjpeg, quality 75; bev_rendering_utils.py:629-630).  The
// quantised coefficients come from the forward tile of jpeg_forward.h (jpeg_forward_rows / _column), the one jpeg_roundtrip.hip decodes again; behind
// them runs jchuff.c's encode_one_block with the standard tables of ITU-T T.81 Annex K (Pillow's optimize=False), one interleaved scan
// without restart intervals, MCU = Y0 Y1 Y2 Y3 Cb Cr:
//   DC      difference against the previous block of the same component in scan order (0 before the first), its category's code,
//           then the category's number of value bits (a negative value as value - 1)
//   AC      zigzag order, (run << 4 | size) symbols, 0xF0 (ZRL) for every 16 zeros before a non-zero coefficient, 0x00 (EOB) when
//           the block ends in zeros
//   bytes   most significant bit first, the last byte padded with 1-bits, a 0x00 stuffed behind every 0xFF (padding included)
//
// Launches, all per image in grid.y / grid.z and asynchronous on the caller's stream:
//   jpeg_coef_kernel        the forward tile, then quantisation; a block's 64 levels leave in zigzag order as int16, 128
//                           bytes per block in MCU-interleaved order, 16 bytes per thread.  Luma blocks of an edge MCU that lie
//                           outside the image's blocks are libjpeg's dummy blocks (jccoefct.c): zero AC, the DC of a neighbour
//   jpeg_code_kernel<false> eight threads per block, eight zigzag positions each: the block's coded length in bits.  The DC
//                           predictor is one 2-byte read of the neighbouring block: no serial chain
//   jpeg_scan_kernel<false> exclusive scan of the lengths -> every block's bit offset, and the image's bit count; one workgroup per
//                           image, looped over tiles of 1024 values with a carry
//   jpeg_zero_kernel        zeroes the words the image's bits will occupy
//   jpeg_code_kernel<true>  the same code path again, now writing: every thread assembles its bits in a register and ORs whole 32-bit
//                           words into the zeroed buffer with vector atomics (atomicOr: the result does not depend on the order)
//   jpeg_ff_kernel<false>   pads the last byte with 1-bits on the fly and counts the 0xFF bytes per chunk of 1024 bytes
//   jpeg_scan_kernel<true>  exclusive scan of those counts
//   jpeg_ff_kernel<true>    copies the bytes into the caller's slot with the stuffed zeros inserted, never past the slot, and writes
//                           the image's byte count (the NEEDED count also where the slot is too small)
// 32-bit integer arithmetic, 64-bit offsets between images, vector stores and vector atomics only, no dependence on launch or
// arrival order: the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "jpeg_forward.h"
#include "salve_common.h"

namespace {

// ITU-T T.81 Annex K.3: the number of codes of each length 1 .. 16 (BITS) and the symbols in code order (HUFFVAL)
constexpr uint8_t BITS_DC_LUMA[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t HUFFVAL_DC_LUMA[12] = {
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};

constexpr uint8_t BITS_AC_LUMA[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t HUFFVAL_AC_LUMA[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr uint8_t BITS_DC_CHROMA[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t HUFFVAL_DC_CHROMA[12] = {
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};

constexpr uint8_t BITS_AC_CHROMA[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t HUFFVAL_AC_CHROMA[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct HuffTables {
    uint32_t dc[2][12];    // [luma, chroma][category]: code << 5 | length
    uint32_t ac[2][256];   // [luma, chroma][run << 4 | size]; 0 = not a symbol of the table
};

// T.81 Annex C: codes of one length are consecutive, the first code of the next length is the successor shifted left
constexpr void derive_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}

constexpr HuffTables make_huff_tables() {
    HuffTables t{};
    derive_codes(BITS_DC_LUMA, HUFFVAL_DC_LUMA, t.dc[0]);
    derive_codes(BITS_DC_CHROMA, HUFFVAL_DC_CHROMA, t.dc[1]);
    derive_codes(BITS_AC_LUMA, HUFFVAL_AC_LUMA, t.ac[0]);
    derive_codes(BITS_AC_CHROMA, HUFFVAL_AC_CHROMA, t.ac[1]);
    return t;
}

__constant__ HuffTables c_huff = make_huff_tables();

// jpeg_natural_order: natural (row-major) index of zigzag position k
__constant__ uint8_t c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A block codes to at most 11 + 11 bits of DC (the longest DC code, category 11) and 63 x (16 + 10) bits of AC (the longest AC code,
// category 10; a ZRL's 11 bits per 16 zeros and the EOB are shorter than the coefficients they stand for): 1660 bits, 9960 bits =
// 1245 bytes per MCU of six blocks.
constexpr uint32_t MCU_MAX_BYTES = 1245;
constexpr int CHUNK_BYTES = 1024;   // bytes per stuffing chunk: one word per thread of a workgroup
constexpr int SCAN_PER_THREAD = 4;
constexpr int FF_GRID = 64, ZERO_GRID = 32;

struct Layout {   // of the workspace, per call; every section starts 16-byte aligned
    uint32_t mcus_w, mcus_h, nb, nbp, wpi, cpi;   // blocks per image (and padded to 4), words and chunks per image
    size_t coef, lens, words, counts, totals, bytes;
};

Layout layout_of(int32_t n, int32_t h, int32_t w) {
    const JpegGeometry g(h, w);
    Layout L;
    L.mcus_w = (uint32_t)g.mcus_w;
    L.mcus_h = (uint32_t)g.mcus_h;
    const uint32_t mcus = (uint32_t)g.mcus();
    L.nb = 6 * mcus;
    L.nbp = (L.nb + 3) & ~3u;
    L.wpi = ((MCU_MAX_BYTES * mcus + 3) / 4 + 2 + 3) & ~3u;
    L.cpi = ((L.wpi * 4 + CHUNK_BYTES - 1) / CHUNK_BYTES + 1 + 3) & ~3u;
    size_t at = 0;
    L.coef = at;
    at += (size_t)n * L.nb * 128;
    L.lens = at;
    at += (size_t)n * L.nbp * 4;
    L.words = at;
    at += (size_t)n * L.wpi * 4;
    L.counts = at;
    at += (size_t)n * L.cpi * 4;
    L.totals = at;   // uint32 [2][n]: bits, 0xFF bytes
    at += ((size_t)n * 8 + 15) & ~(size_t)15;
    L.bytes = at;
    return L;
}

// grid (MCU groups across, MCU rows, images)
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_coef_kernel(const uint32_t* __restrict__ in, int16_t* __restrict__ coef, int h, int w, int mcus_w,
                                                                 uint32_t nb, QTables qt) {
    __shared__ JpegTile t;
    const JpegBlockMap map = jpeg_forward_rows(in, h, w, qt, t);
    const int r = map.r, stride = map.stride;
    int* base = map.base;
    if (map.working) {   // forward pass 2 on column r, quantise
        const int* q = t.q[map.luma ? 0 : 1];
        int d[8];
        jpeg_forward_column(map, d);
#pragma unroll
        for (int k = 0; k < 8; k++) base[k * stride + r] = jpeg_quantise(d[k], q[k * 8 + r]);
    }
    __syncthreads();
    const int mcu_x = blockIdx.x * MCUS + map.m;
    if (map.working && mcu_x < mcus_w) {   // zigzag positions 8 r .. 8 r + 7 leave as one 16-byte store
        // jccoefct.c: a luma block of the MCU that lies wholly outside the image's blocks is a DUMMY block -- AC zero, DC that of the
        // block before it in the MCU (right edge), of the block before its row of blocks (bottom edge) -- not an edge-replicated one
        const int wblocks = (w + 7) >> 3, hblocks = (h + 7) >> 3;
        const bool right = map.luma && mcu_x * 2 + map.bx >= wblocks, below = map.luma && (int)blockIdx.y * 2 + map.by >= hblocks;
        const bool y1_real = mcu_x * 2 + 1 < wblocks;
        const int sby = below ? 0 : map.by, sbx = below ? (y1_real ? 1 : 0) : 0;
        const int dummy_dc = t.y[(sby * 8) * SY + map.m * 16 + sbx * 8];
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int a = c_zigzag[8 * r + 2 * k], b = c_zigzag[8 * r + 2 * k + 1];
            int va = base[(a >> 3) * stride + (a & 7)], vb = base[(b >> 3) * stride + (b & 7)];
            if (right || below) {
                va = (r == 0 && k == 0) ? dummy_dc : 0;
                vb = 0;
            }
            v[k] = ((uint32_t)va & 0xFFFFu) | ((uint32_t)vb << 16);
        }
        const uint32_t block = ((uint32_t)blockIdx.y * mcus_w + mcu_x) * 6 + map.k;
        int16_t* dst = coef + ((int64_t)blockIdx.z * nb + block) * 64 + 8 * r;
        *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// Bits of one thread, most significant first: a word leaves with one atomicOr when it is complete (or at the end)
struct BitWriter {
    uint32_t* words;
    uint32_t pos, acc;
    __device__ __forceinline__ void put(uint32_t code, uint32_t len) {   // len 1 .. 26, code < 2^len
        const uint32_t sh = pos & 31;
        const uint64_t v = (uint64_t)code << (64 - len - sh);
        acc |= (uint32_t)(v >> 32);
        pos += len;
        if (sh + len >= 32) {
            atomicOr(&words[(pos >> 5) - 1], acc);
            acc = (uint32_t)v;
        }
    }
    __device__ __forceinline__ void flush() {
        if (acc) atomicOr(&words[pos >> 5], acc);
    }
};

__device__ __forceinline__ uint32_t category(int v) { return 32 - __clz(v < 0 ? -v : v); }   // 0 for 0
__device__ __forceinline__ uint32_t value_bits(int v, uint32_t size) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1); }

// The symbols of zigzag positions 8 r .. 8 r + 7 of one block (c[0] of r == 0 is the DC DIFFERENCE); nz: the block's non-zero AC
// positions with bit 0 set as the DC's boundary.  Returns their length in bits; EMIT writes them.
template <bool EMIT>
__device__ __forceinline__ uint32_t code_chunk(const int* c, int r, uint64_t nz, const uint32_t* dc, const uint32_t* ac, BitWriter& bw) {
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int p = 8 * r + j, v = c[j];
        if (p == 0) {
            const uint32_t size = category(v), e = dc[size];
            bits += (e & 31) + size;
            if (EMIT) bw.put(((e >> 5) << size) | value_bits(v, size), (e & 31) + size);
        } else if (v != 0) {
            const uint64_t below = nz & ((1ull << p) - 1);
            const int run = p - (63 - __clzll((long long)below)) - 1;
            const uint32_t zrl = ac[0xF0];
            for (int z = run >> 4; z > 0; z--) {
                bits += zrl & 31;
                if (EMIT) bw.put(zrl >> 5, zrl & 31);
            }
            const uint32_t size = category(v), e = ac[((run & 15) << 4) | size];
            bits += (e & 31) + size;
            if (EMIT) bw.put(((e >> 5) << size) | value_bits(v, size), (e & 31) + size);
        }
    }
    if (r == 7 && !(nz >> 63)) {   // the block ends in zeros: EOB
        bits += ac[0] & 31;
        if (EMIT) bw.put(ac[0] >> 5, ac[0] & 31);
    }
    return bits;
}

// grid (blocks / 32, images): eight threads per 8 x 8 block.  EMIT false: lens[block] = coded length in bits.  EMIT true: lens holds
// the blocks' bit offsets and the codes are ORed into `words`.
template <bool EMIT>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_code_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ lens, uint32_t* __restrict__ words,
                                                                 uint32_t nb, uint32_t nbp, uint32_t wpi) {
    __shared__ uint32_t s_dc[2][12];
    __shared__ uint32_t s_ac[2][256];
    const int tid = threadIdx.x;
    s_ac[0][tid] = c_huff.ac[0][tid];
    s_ac[1][tid] = c_huff.ac[1][tid];
    if (tid < 24) s_dc[tid / 12][tid % 12] = c_huff.dc[tid / 12][tid % 12];
    __syncthreads();
    const uint32_t g = blockIdx.x * 32 + (tid >> 3);
    const int r = tid & 7;
    const bool valid = g < nb;   // (the eight threads of a block agree; all of them take part in the shuffles below)
    const int16_t* image = coef + (int64_t)blockIdx.y * nb * 64;
    int c[8];
    {
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (valid) raw = *reinterpret_cast<const uint4*>(image + (int64_t)g * 64 + 8 * r);
        const uint32_t v[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c[2 * k] = (int)(int16_t)(v[k] & 0xFFFFu);
            c[2 * k + 1] = (int)(int16_t)(v[k] >> 16);
        }
    }
    const uint32_t k6 = g % 6;   // Y0 Y1 Y2 Y3 Cb Cr
    if (valid && r == 0) {   // the DC predictor: the previous block of the same component in scan order
        const int64_t pred = k6 == 0 ? (int64_t)g - 3 : k6 <= 3 ? (int64_t)g - 1 : (int64_t)g - 6;
        if (pred >= 0) c[0] -= (int)image[pred * 64];
    }
    uint32_t m8 = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) m8 |= (uint32_t)(c[j] != 0) << j;
    if (r == 0) m8 |= 1;   // position 0 bounds the first run whatever the DC difference is
    uint32_t lo = r < 4 ? m8 << (8 * r) : 0, hi = r >= 4 ? m8 << (8 * (r - 4)) : 0;
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        lo |= __shfl_xor(lo, s, 8);
        hi |= __shfl_xor(hi, s, 8);
    }
    const uint64_t nz = ((uint64_t)hi << 32) | lo;
    const uint32_t* dc = s_dc[k6 >= 4];
    const uint32_t* ac = s_ac[k6 >= 4];
    BitWriter bw{words + (int64_t)blockIdx.y * wpi, 0, 0};
    const uint32_t mine = code_chunk<false>(c, r, nz, dc, ac, bw);
    uint32_t incl = mine;
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s, 8);
        if (r >= s) incl += up;
    }
    uint32_t* slot = lens + (int64_t)blockIdx.y * nbp + g;
    if (!EMIT) {
        if (valid && r == 7) *slot = incl;
    } else if (valid) {
        bw.pos = *slot + incl - mine;
        code_chunk<true>(c, r, nz, dc, ac, bw);
        bw.flush();
    }
}

// Exclusive prefix of v over the workgroup's 256 threads (in thread order) and the workgroup's total.  s_wave: 4 words of LDS.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s, 64);
        if (lane >= s) incl += up;
    }
    __syncthreads();   // (the previous use of s_wave is over)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t t = s_wave[k];
        if (k < wave) before += t;
        total += t;
    }
    return before + incl - v;
}

__device__ __forceinline__ uint32_t chunks_of(uint32_t bits) { return (((bits + 7) >> 3) + CHUNK_BYTES - 1) / CHUNK_BYTES; }

// grid (images): vals[image][0 .. count) becomes its exclusive prefix sum, totals[image] the sum.  CHUNKS false: count values;
// CHUNKS true: as many as the image has chunks (from its bit count in bits_total).
template <bool CHUNKS>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_scan_kernel(uint32_t* __restrict__ vals, uint32_t per_image, uint32_t count,
                                                                 const uint32_t* __restrict__ bits_total, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_wave[4];
    uint32_t* v = vals + (int64_t)blockIdx.x * per_image;
    if (CHUNKS) count = chunks_of(bits_total[blockIdx.x]);
    uint32_t carry = 0;
    for (uint32_t at = 0; at < count; at += JPEG_THREADS * SCAN_PER_THREAD) {
        const uint32_t i0 = at + threadIdx.x * SCAN_PER_THREAD;
        uint32_t x[SCAN_PER_THREAD], sum = 0;
#pragma unroll
        for (int j = 0; j < SCAN_PER_THREAD; j++) {
            x[j] = i0 + j < count ? v[i0 + j] : 0;
            sum += x[j];
        }
        uint32_t total;
        uint32_t run = carry + block_exclusive_scan(sum, s_wave, total);
#pragma unroll
        for (int j = 0; j < SCAN_PER_THREAD; j++) {
            if (i0 + j < count) v[i0 + j] = run;
            run += x[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// grid (ZERO_GRID, images): the words that the image's bits (and the padding of its last byte) will occupy
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_zero_kernel(uint32_t* __restrict__ words, uint32_t wpi, const uint32_t* __restrict__ bits_total) {
    uint32_t* w = words + (int64_t)blockIdx.y * wpi;
    const uint32_t count = min((bits_total[blockIdx.y] >> 5) + 1, wpi);
    for (uint32_t i = blockIdx.x * JPEG_THREADS + threadIdx.x; i < count; i += ZERO_GRID * JPEG_THREADS) w[i] = 0;
}

// grid (FF_GRID, images), a chunk of 1024 bytes (one word per thread) per iteration.  STUFF false: counts[chunk] = its 0xFF bytes.
// STUFF true: counts holds the exclusive prefix of those; the bytes go to the image's slot with a 0x00 behind every 0xFF.
template <bool STUFF>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_ff_kernel(const uint32_t* __restrict__ words, uint32_t wpi, uint32_t* __restrict__ counts, uint32_t cpi,
                                                               const uint32_t* __restrict__ bits_total, const uint32_t* __restrict__ ff_total,
                                                               uint8_t* __restrict__ scan, size_t scan_stride, int32_t* __restrict__ scan_bytes) {
    __shared__ uint32_t s_wave[4];
    const uint32_t bits = bits_total[blockIdx.y];
    const uint32_t nbytes = (bits + 7) >> 3, nchunks = chunks_of(bits);
    const uint32_t* w = words + (int64_t)blockIdx.y * wpi;
    uint32_t* cnt = counts + (int64_t)blockIdx.y * cpi;
    uint8_t* out = scan + (size_t)blockIdx.y * scan_stride;
    if (STUFF && blockIdx.x == 0 && threadIdx.x == 0) scan_bytes[blockIdx.y] = (int32_t)(nbytes + ff_total[blockIdx.y]);
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += FF_GRID) {
        const uint32_t wi = chunk * (CHUNK_BYTES / 4) + threadIdx.x, b0 = wi * 4;
        uint32_t word = 0;
        if (b0 < nbytes) {
            word = w[wi];
            const uint32_t pad = (8 - (bits & 7)) & 7;   // 1-bits behind the last code, up to the byte's end
            if (wi == (bits >> 5) && pad) word |= ((1u << pad) - 1) << (32 - (bits & 31) - pad);
        }
        uint32_t ff = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) ff += (b0 + j < nbytes) && ((word >> (24 - 8 * j)) & 255) == 255;
        uint32_t total;
        const uint32_t before = block_exclusive_scan(ff, s_wave, total);
        if (!STUFF) {
            if (threadIdx.x == 0) cnt[chunk] = total;
        } else {
            size_t at = (size_t)b0 + cnt[chunk] + before;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (b0 + j >= nbytes) break;
                const uint32_t byte = (word >> (24 - 8 * j)) & 255;
                if (at < scan_stride) out[at] = (uint8_t)byte;
                at++;
                if (byte == 255) {
                    if (at < scan_stride) out[at] = 0;
                    at++;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

size_t salve_bev_jpeg_encode_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!jpeg_shape_ok("salve_bev_jpeg_encode_workspace_bytes", n, h, w)) return 0;
    return layout_of(n, h, w).bytes;
}

size_t salve_bev_jpeg_encode_max_bytes(int32_t h, int32_t w) {
    if (!jpeg_shape_ok("salve_bev_jpeg_encode_max_bytes", 1, h, w)) return 0;
    const Layout L = layout_of(1, h, w);
    return ((size_t)2 * MCU_MAX_BYTES * L.mcus_w * L.mcus_h + 3) & ~(size_t)3;   // every byte may be 0xFF and get a 0x00 behind it
}

int salve_bev_jpeg_encode(const uint32_t* bev, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, uint8_t* scan, size_t scan_stride,
                          int32_t* scan_bytes, void* ws, size_t ws_bytes, void* stream) {
    const char* me = "salve_bev_jpeg_encode";
    if (!bev || !qtab || !scan || !scan_bytes || !ws) { jpeg_refuse(me, "null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!jpeg_shape_ok(me, n, h, w)) return SALVE_ERR_BAD_ARG;
    if (((uintptr_t)bev | (uintptr_t)scan_bytes) & 3) { jpeg_refuse(me, "the images and scan_bytes must be 4-byte aligned"); return SALVE_ERR_BAD_ARG; }
    if (scan_stride == 0 || (scan_stride & 3)) { jpeg_refuse(me, "scan_stride must be a positive multiple of 4"); return SALVE_ERR_BAD_ARG; }
    QTables qt;
    const Layout L = layout_of(n, h, w);
    if (!jpeg_load_qtables(me, qtab, &qt) || !jpeg_workspace_ok(me, ws, ws_bytes, L.bytes)) return SALVE_ERR_BAD_ARG;
    uint8_t* base = (uint8_t*)ws;
    int16_t* coef = (int16_t*)(base + L.coef);
    uint32_t* lens = (uint32_t*)(base + L.lens);
    uint32_t* words = (uint32_t*)(base + L.words);
    uint32_t* counts = (uint32_t*)(base + L.counts);
    uint32_t* bits_total = (uint32_t*)(base + L.totals);
    uint32_t* ff_total = bits_total + n;
    hipStream_t st = (hipStream_t)stream;
    const dim3 threads(JPEG_THREADS);
    hipLaunchKernelGGL(jpeg_coef_kernel, dim3((L.mcus_w + MCUS - 1) / MCUS, L.mcus_h, (unsigned)n), threads, 0, st, bev, coef, (int)h, (int)w,
                       (int)L.mcus_w, L.nb, qt);
    SALVE_HIP_CHECK(hipGetLastError());
    const dim3 code_grid((L.nb + 31) / 32, (unsigned)n);
    hipLaunchKernelGGL(jpeg_code_kernel<false>, code_grid, threads, 0, st, (const int16_t*)coef, lens, words, L.nb, L.nbp, L.wpi);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel<false>, dim3((unsigned)n), threads, 0, st, lens, L.nbp, L.nb, (const uint32_t*)nullptr, bits_total);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(ZERO_GRID, (unsigned)n), threads, 0, st, words, L.wpi, (const uint32_t*)bits_total);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_code_kernel<true>, code_grid, threads, 0, st, (const int16_t*)coef, lens, words, L.nb, L.nbp, L.wpi);
    SALVE_HIP_CHECK(hipGetLastError());
    const dim3 ff_grid(FF_GRID, (unsigned)n);
    hipLaunchKernelGGL(jpeg_ff_kernel<false>, ff_grid, threads, 0, st, (const uint32_t*)words, L.wpi, counts, L.cpi, (const uint32_t*)bits_total,
                       (const uint32_t*)ff_total, scan, scan_stride, scan_bytes);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel<true>, dim3((unsigned)n), threads, 0, st, counts, L.cpi, 0u, (const uint32_t*)bits_total, ff_total);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_ff_kernel<true>, ff_grid, threads, 0, st, (const uint32_t*)words, L.wpi, counts, L.cpi, (const uint32_t*)bits_total,
                       (const uint32_t*)ff_total, scan, scan_stride, scan_bytes);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
