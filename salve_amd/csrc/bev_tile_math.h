// bev_tile_math.h -- the arithmetic of the verifier's input tile, spelled out ONCE: cv2's INTER_LINEAR on uint8 (11-bit taps), the
// normalisation table, the fp16 store.  Included by bev_tiles.hip (the tile, train-tile and resize kernels) and by bev_render.hip
// (phase H of bev_densify_kernel); everything is static and inlined, neither unit exports a symbol of it.
// Reference: cv2.resize as called by transform.py:256-272 (tiles) and bev_rendering_utils.py:370-375 (panorama ingest).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static __device__ __forceinline__ uint16_t f32_to_f16(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }  // |values| < 3: no saturation needed

// One channel of one resized pixel from its four source bytes  a b  and the taps {src0, src1, w0, w1} of its row (cy) and column (cx),
//                                                              c d
// w0 + w1 = 2048: horizontal pass x2048, vertical pass with cv2's two truncating shifts, rounded and clamped to a byte.
static __device__ __forceinline__ int bilinear_u8(int a, int b, int c, int d, const int4 cy, const int4 cx) {
    const int S0 = a * cx.z + b * cx.w;
    const int S1 = c * cx.z + d * cx.w;
    const int r = (((cy.z * (S0 >> 4)) >> 16) + ((cy.w * (S1 >> 4)) >> 16) + 2) >> 2;
    return min(max(r, 0), 255);
}

// The same integers with 24-bit multiplies (full rate; the v_mul_lo_u32 of the form above are quarter rate), for the densify kernel's
// tile phase, which is bound by vector-instruction issue.  Bytes < 2^8 times weights <= 2^11 give sums S < 2^20, and the vertical
// pass multiplies a weight <= 2^11 by S >> 4 < 2^16: every product is below 2^28 of operands below 2^16, exact in a 24-bit
// multiply, and nothing is negative, so the unsigned shifts here and the signed ones above move the same bits.
static __device__ __forceinline__ int bilinear_u8_mul24(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const int4 cy, const int4 cx) {
    const int S0 = (int)(__umul24(a, cx.z) + __umul24(b, cx.w));
    const int S1 = (int)(__umul24(c, cx.z) + __umul24(d, cx.w));
    const int r = (int)(((__umul24(cy.z, S0 >> 4) >> 16) + (__umul24(cy.w, S1 >> 4) >> 16) + 2u) >> 2);
    return min(max(r, 0), 255);
}

// One tile pixel of the 0x00BBGGRR image `img` (W pixels per row): the three resized bytes through the normalisation table
// lut [3][256] (ToTensor + Normalize, evaluated in float32 on the host).
static __device__ __forceinline__ void tile_pixel(const uint32_t* __restrict__ img, int W, const int4 cy, const int4 cx, const float* __restrict__ lut, float v[3]) {
    const uint32_t p00 = img[(size_t)cy.x * W + cx.x], p01 = img[(size_t)cy.x * W + cx.y];
    const uint32_t p10 = img[(size_t)cy.y * W + cx.x], p11 = img[(size_t)cy.y * W + cx.y];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        v[ch] = lut[ch * 256 + bilinear_u8((p00 >> (8 * ch)) & 255, (p01 >> (8 * ch)) & 255, (p10 >> (8 * ch)) & 255, (p11 >> (8 * ch)) & 255, cy, cx)];
}

// The store of one early-fusion pair pixel: six halves as the three words w0 w1 w2 into the pixel px of a fp16 NHWC sample of out_c
// channels.  out_c == 8 (one surface): the whole 16-byte pixel, padding channels 6 and 7 included; otherwise three words at channel
// c0 (the first of the group's six: even, so 4-byte aligned) and, behind the sample's last group, zeros in the padding channels.
static __device__ __forceinline__ void store_pair_pixel(uint16_t* px, uint32_t w0, uint32_t w1, uint32_t w2, int c0, int out_c) {
    if (out_c == 8) {
        *reinterpret_cast<uint4*>(px) = make_uint4(w0, w1, w2, 0u);
    } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(px + c0);
        o[0] = w0; o[1] = w1; o[2] = w2;
        if (c0 + 12 > out_c)
            for (int k = c0 + 6; k < out_c; k += 2) *reinterpret_cast<uint32_t*>(px + k) = 0u;
    }
}
