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

// The three resized bytes of that pixel themselves (what tile_pixel looks up), for the kernels that work on them first.
static __device__ __forceinline__ void tile_bytes(const uint32_t* __restrict__ img, int W, const int4 cy, const int4 cx, int q[3]) {
    const uint32_t p00 = img[(size_t)cy.x * W + cx.x], p01 = img[(size_t)cy.x * W + cx.y];
    const uint32_t p10 = img[(size_t)cy.y * W + cx.x], p11 = img[(size_t)cy.y * W + cx.y];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        q[ch] = bilinear_u8((p00 >> (8 * ch)) & 255, (p01 >> (8 * ch)) & 255, (p10 >> (8 * ch)) & 255, (p11 >> (8 * ch)) & 255, cy, cx);
}

// ---- torchvision's tensor ColorJitter on uint8 pixels (functional_tensor.py of torchvision 0.11 / 0.12), float32 with
// one rounding per operation: this header's users compile with -ffp-contract=off, `/` is the correctly rounded division and float32
// denormals are kept (hipcc's defaults for gfx950).
static __device__ __forceinline__ int trunc8(float v) { return (int)fminf(fmaxf(v, 0.0f), 255.0f); }   // clamp(0, 255).to(uint8)

static __device__ __forceinline__ int jitter_grey(const int q[3]) {   // rgb_to_grayscale(...).to(uint8)
    return trunc8((0.2989f * (float)q[0] + 0.587f * (float)q[1]) + 0.114f * (float)q[2]);
}

// _blend(img, other, f) per channel: f and f_c = (float)(1.0 - (double)f) both come from the host.
static __device__ __forceinline__ void jitter_blend(int q[3], float other, float f, float f_c) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) q[ch] = trunc8(f * (float)q[ch] + f_c * other);
}

static __device__ __forceinline__ float fmod1(float a) { return a - truncf(a); }   // fmod(a, 1.0f): the fraction of a float32 is a float32

static __device__ __forceinline__ void jitter_hue(int q[3], float hue) {
    const float r = (float)q[0] / 255.0f, g = (float)q[1] / 255.0f, b = (float)q[2] / 255.0f;
    // _rgb2hsv
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float d = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    const float hr = (maxc == r) ? bc - gc : 0.0f;
    const float hg = (maxc == g && maxc != r) ? (2.0f + rc) - bc : 0.0f;
    const float hb = (maxc != g && maxc != r) ? (4.0f + gc) - rc : 0.0f;
    float hh = fmod1(((hr + hg) + hb) / 6.0f + 1.0f);
    // (h + hue_factor) % 1.0: torch's remainder -- fmod, and + 1 (one more rounding) where that is negative
    hh = fmod1(hh + hue);
    if (hh < 0.0f) hh += 1.0f;
    // _hsv2rgb
    const float h6 = hh * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const int i = (int)fl % 6;
    const float p = fminf(fmaxf(maxc * (1.0f - s), 0.0f), 1.0f);
    const float qq = fminf(fmaxf(maxc * (1.0f - s * f), 0.0f), 1.0f);
    const float t = fminf(fmaxf(maxc * (1.0f - s * (1.0f - f)), 0.0f), 1.0f);
    const float v = maxc;
    const float o0 = i == 0 ? v : i == 1 ? qq : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    const float o1 = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? qq : i == 4 ? p : p;
    const float o2 = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : qq;
    q[0] = (int)(o0 * 255.0f); q[1] = (int)(o1 * 255.0f); q[2] = (int)(o2 * 255.0f);
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
