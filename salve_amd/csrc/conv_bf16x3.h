// conv_bf16x3.h -- the bf16x3 convolution of the fp32-family verifier (resnet_f32.hip, salve_resnet_bf16x3_create): fp32 activations
// in memory, every fp32 operand split into two bf16 pieces, three bf16 MFMAs per k-step instead of one fp32 MFMA.  Included by
// resnet_f32.hip after conv_f32.h, whose argument block, tile map, gather and ReLU it uses; everything lives in an anonymous namespace.
//
//   x = hi + lo + r,   hi = bf16(x) (nearest even),   lo = bf16(x - float(hi)) (the subtraction is exact)
//   a * w ~ ah * wh + ah * wl + al * wh      (dropped: al * wl, ra * w and a * rw)
//
// bf16 keeps 8 significand bits, so |x - hi| <= 2^-8 |x| and |r| <= 2^-16 |x| in the worst case (2^-9 and 2^-18 for a typical x: the
// roundings are spread evenly over their interval); the three dropped pieces have mixed signs and average over K.  The tests hold one
// convolution output to (3 * 2^-18 + the fp32 accumulation's 4e-6) * (sum |a| |w| + |bias|); the emulated scheme reaches 0.4 of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_f32.h"

namespace {

typedef __attribute__((__ext_vector_type__(8))) __bf16 bf16x8;
typedef __attribute__((__ext_vector_type__(2))) __bf16 bf16x2;
typedef __attribute__((__ext_vector_type__(2))) float f32x2;

// The split by its rules, one element, in integer arithmetic: NaN -> (quiet NaN, 0); +-inf -> (+-inf, 0), never inf - inf; a finite x
// whose rounding would give inf -> the largest finite bf16 of its sign, and lo takes what is left.  Returns hi | lo << 16.
__host__ __device__ __forceinline__ uint32_t split_bf16_bits(float x) {
    union { float f; uint32_t u; } c, hf, d;
    c.f = x;
    const uint32_t u = c.u, a = u & 0x7FFFFFFFu;
    const bool special = a >= 0x7F800000u;   // (selects, no branches: x of a special keeps its bits below, so that x - hi is 0, not inf - inf)
    uint32_t h = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    h = (h & 0x7FFFu) == 0x7F80u ? h - 1u : h;
    h = special ? (u >> 16) | (a > 0x7F800000u ? 0x40u : 0u) : h;
    hf.u = special ? 0u : h << 16;
    c.u = special ? 0u : u;
    d.f = c.f - hf.f;   // finite, and far below the bf16 range's end: its rounding cannot overflow
    const uint32_t l = (d.u + 0x7FFFu + ((d.u >> 16) & 1u)) >> 16;
    return h | (l << 16);
}

// Two elements; hi = (hi of x0) | (hi of x1) << 16, lo likewise.  `chk` collects 0 * (x - float(hi)): it turns NaN exactly when some
// element is NaN or +-inf or rounds to inf -- the cases in which the conversion instructions do not give the rules' pieces.
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& hi, uint32_t& lo, float& chk) {
    f32x2 x = {x0, x1};
    const bf16x2 h = __builtin_convertvector(x, bf16x2);
    const f32x2 d = {x0 - (float)h[0], x1 - (float)h[1]};   // (two scalar subtractions: packed fp32 arithmetic is slow beside MFMAs)
    const bf16x2 l = __builtin_convertvector(d, bf16x2);
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
    chk = fmaf(d[0], 0.f, fmaf(d[1], 0.f, chk));
}

__device__ __forceinline__ void split_pair_slow(float x0, float x1, uint32_t& hi, uint32_t& lo) {
    const uint32_t s0 = split_bf16_bits(x0), s1 = split_bf16_bits(x1);
    hi = (s0 & 0xFFFFu) | (s1 << 16);
    lo = (s0 >> 16) | (s1 & 0xFFFF0000u);
}

// Eight fp32 values (two float4) -> their eight hi pieces and eight lo pieces, 16 bytes each.
__device__ __forceinline__ void split8(const float4& v0, const float4& v1, uint4& hi, uint4& lo) {
    float chk = 0.f;
    split_pair(v0.x, v0.y, hi.x, lo.x, chk);
    split_pair(v0.z, v0.w, hi.y, lo.y, chk);
    split_pair(v1.x, v1.y, hi.z, lo.z, chk);
    split_pair(v1.z, v1.w, hi.w, lo.w, chk);
    if (chk != chk) {
        split_pair_slow(v0.x, v0.y, hi.x, lo.x);
        split_pair_slow(v0.z, v0.w, hi.y, lo.y);
        split_pair_slow(v1.x, v1.y, hi.z, lo.z);
        split_pair_slow(v1.z, v1.w, hi.w, lo.w);
    }
}

// The weights' split, once at create: fp32 [Cout][K] -> for every row and every k-tile of 32 one 128-byte line [32 hi | 32 lo] of bf16,
// the image of a staged weight row in LDS.  A convolution's split weights take the bytes its fp32 weights took.
__global__ __launch_bounds__(256) void split_weights_bf16x3_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = split_bf16_bits(w[i]);
    uint16_t* line = out + (i >> 5) * 64 + (i & 31);
    line[0] = (uint16_t)s;
    line[32] = (uint16_t)(s >> 16);
}

// Implicit-GEMM convolution with conv_f32_kernel's block tile (128 pixels x BN channels x 32 k), waves (2 x 2, 64 x BN/2 each), tile
// map, k-table walk, second source and epilogue, on v_mfma_f32_32x32x16_bf16.
// Operand maps of the 32x32x16 form: lane l supplies A[i = l & 31][k = 8 (l >> 5) + e] and B[k = 8 (l >> 5) + e][j = l & 31] in
// element e = 0..7 of its fragment; D as in the 32x32x2 form.  A = activations (i = pixel), B = weights (j = output channel).
// LDS: a staged row is 144 bytes -- 32 hi pieces (k = 0..31), 32 lo pieces, 16 bytes of padding -- the bytes of the fp32 tile's row.
// A fragment is one 16-byte read at byte 32 s + 16 (l >> 5) of the hi or of the lo half (k-step s = 0, 1); with the 144-byte pitch the
// 16 lanes of a read group hit 16 distinct bank quads.  Per k-tile a wave reads 8 + 4 NT fragments for 12 NT MFMAs.
// Activations are split once per element between the global load's registers and the LDS store; weights arrive split.
// Per k-step and accumulator, in this order: ah * wh, ah * wl, al * wh.  No atomics and no split-K: the same input gives the same bits.
// (The v_mfma_f32_16x16x32_bf16 form at the same wave tile measured 16-19 % slower by wall clock: DESIGN.md section 4.27.)
template <int BN>
__global__ __launch_bounds__(F_THREADS, 2) void conv_bf16x3_kernel(ConvF32Args p) {
    constexpr int NT = BN / 64;                  // 32-wide n sub-tiles per wave
    constexpr int B_TPR = F_THREADS / BN;        // threads per staged weight row (2 or 4)
    constexpr int B_F4 = F_BK / 4 / B_TPR;       // 16-byte loads per thread of the weight tile (4 or 2)
    __shared__ __attribute__((aligned(16))) float As[F_BM * F_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[BN * F_LDK];

    int m_tile, n_tile;
    if (!f32_tile(blockIdx.x, p.m_tiles, p.n_tiles, m_tile, n_tile)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int m0 = m_tile * F_BM, n0 = n_tile * BN;

    // ---- this thread's staged activation row: pixel m0 + (tid >> 1), k columns [16 * (tid & 1), + 16) of every tile
    const int arow = tid >> 1, ahalf = tid & 1;
    const int m = m0 + arow;
    const bool mvalid = m < p.M;
    int iy0 = -100000, ix0 = 0;
    long long pix = 0, pix2 = 0;   // element offset of the pixel of tap (0, 0) (may lie outside the image) / of the in2 pixel
    {
        const int mm = mvalid ? m : 0;
        const int ox = mm % p.Wo, t = mm / p.Wo, oy = t % p.Ho, b = t / p.Ho;
        if (mvalid) iy0 = oy * p.stride - p.pad;
        ix0 = ox * p.stride - p.pad;
        pix = (((long long)b * p.Hi + (mvalid ? iy0 : 0)) * p.Wi + ix0) * p.Cin;
        if (p.in2) pix2 = (((long long)b * p.Hi2 + (long long)oy * p.stride2) * p.Wi2 + (long long)ox * p.stride2) * p.Cin2;
    }
    // ---- this thread's staged weight row: 128 / B_TPR bytes of the row's line of every tile (counted in floats: a line is 32 of them)
    const int brow = tid / B_TPR, bpart = tid % B_TPR;
    const float* wrow = p.w + (long long)(n0 + brow) * p.K + bpart * (F_BK / B_TPR);

    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
// global -> registers of k-tile KT
#define LOAD_TILE_X3(KT)                                                                                                       \
    {                                                                                                                          \
        if (p.in2) { /* 1 x 1 / stride 1 over [in | in2]: no table */                                                        \
            const float* src_ = nullptr;                                                                                       \
            if (mvalid) src_ = (KT) < p.nkt1 ? p.in + (long long)m * p.Cin + (KT) * F_BK + ahalf * 16                          \
                                             : p.in2 + pix2 + ((KT) - p.nkt1) * F_BK + ahalf * 16;                            \
            ra0 = ra1 = ra2 = ra3 = zero4;                                                                                     \
            if (src_) {                                                                                                        \
                ra0 = reinterpret_cast<const float4*>(src_)[0];                                                                \
                ra1 = reinterpret_cast<const float4*>(src_)[1];                                                                \
                ra2 = reinterpret_cast<const float4*>(src_)[2];                                                                \
                ra3 = reinterpret_cast<const float4*>(src_)[3];                                                                \
            }                                                                                                                  \
        } else {                                                                                                               \
            const int32_t* e_ = p.ktab + (KT) * 4 + ahalf * 2;                                                                \
            gather8(p, pix, iy0, ix0, e_[0], ra0, ra1);                                                                        \
            gather8(p, pix, iy0, ix0, e_[1], ra2, ra3);                                                                        \
        }                                                                                                                      \
        const float4* w_ = reinterpret_cast<const float4*>(wrow + (long long)(KT) * F_BK);                                    \
        rb0 = w_[0];                                                                                                           \
        rb1 = w_[1];                                                                                                           \
        if (B_F4 == 4) {                                                                                                       \
            rb2 = w_[2];                                                                                                       \
            rb3 = w_[3];                                                                                                       \
        }                                                                                                                      \
    }

    f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nkt = p.K / F_BK;
    const int frow = lane & 31, fk = (lane >> 5) * 4;   // fk in floats: 16 bytes = 8 pieces
    const float* a_frag = As + (wr * 64 + frow) * F_LDK + fk;
    const float* b_frag = Bs + (wc * (BN / 2) + frow) * F_LDK + fk;
    LOAD_TILE_X3(0);
    for (int kt = 0; kt < nkt; kt++) {
        // registers -> LDS: the activations split here, once per element
        {
            uint4 h0, l0, h1, l1;
            split8(ra0, ra1, h0, l0);
            split8(ra2, ra3, h1, l1);
            uint4* a_ = reinterpret_cast<uint4*>(As + arow * F_LDK + ahalf * 8);
            a_[0] = h0; a_[1] = h1;
            a_[4] = l0; a_[5] = l1;
            float4* b_ = reinterpret_cast<float4*>(Bs + brow * F_LDK + bpart * (F_BK / B_TPR));
            b_[0] = rb0; b_[1] = rb1;
            if (B_F4 == 4) { b_[2] = rb2; b_[3] = rb3; }
        }
        __syncthreads();
        {   // the next tile, in flight under the MFMAs below (the last iteration loads its own tile again, as in conv_f32_kernel)
            const int kn = kt + 1 < nkt ? kt + 1 : kt;
            LOAD_TILE_X3(kn);
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {
            bf16x8 ah[2], al[2], bh[NT], bl[NT];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                ah[i] = *reinterpret_cast<const bf16x8*>(a_frag + i * 32 * F_LDK + 8 * s);
                al[i] = *reinterpret_cast<const bf16x8*>(a_frag + i * 32 * F_LDK + 16 + 8 * s);
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
                bh[j] = *reinterpret_cast<const bf16x8*>(b_frag + j * 32 * F_LDK + 8 * s);
                bl[j] = *reinterpret_cast<const bf16x8*>(b_frag + j * 32 * F_LDK + 16 + 8 * s);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#undef LOAD_TILE_X3

    // ---- epilogue: + bias (+ residual), ReLU, fp32 store; a store instruction writes 32 consecutive channels of one pixel
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int n = n0 + wc * (BN / 2) + j * 32 + (lane & 31);
        const float bias = p.bias[n];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int mo = m0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (mo >= p.M) continue;
                const long long o = (long long)mo * p.Cout + n;
                float v = acc[i][j][r] + bias;
                if (p.res) v += p.res[o];
                p.out[o] = p.relu ? relu_nan(v) : v;
            }
        }
    }
}

template <int BN>
int launch_conv_bf16x3(const ConvF32Args& a, hipStream_t s) {
    const long long grid = 8ll * ((a.m_tiles + 7) / 8) * a.n_tiles;
    if (grid > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    hipLaunchKernelGGL((conv_bf16x3_kernel<BN>), dim3((unsigned)grid), dim3(F_THREADS), 0, s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace
