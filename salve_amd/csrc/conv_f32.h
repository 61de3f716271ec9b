// conv_f32.h -- the fp32 implicit-GEMM convolution of the fp32 engine (resnet_f32.hip), shared with the per-convolution training
// entries (conv_train_f32.hip).  Included by both translation units; everything lives in an anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

typedef __attribute__((__ext_vector_type__(16))) float f32x16;

constexpr int F_BM = 128;            // output pixels per workgroup
constexpr int F_BK = 32;             // k per staged tile: four ktab chunks of 8
constexpr int F_LDK = F_BK + 4;      // LDS row pitch in floats (144 B: the 16-byte fragment reads of 16 rows hit 16 distinct bank quads)
constexpr int F_THREADS = 256;       // 4 waves, 2 x 2 over the block tile

struct ConvF32Args {
    const float* in;
    const float* w;        // [Cout][K] fp32, K in the program's order
    const float* bias;
    const float* res;      // [M][Cout] or nullptr
    float* out;            // [M][Cout]
    const int32_t* ktab;   // one entry per 8 consecutive k: dy | dx << 8 | channel offset << 16; a negative entry gathers zeros
    const float* in2;      // second point-wise source (projection shortcut) or nullptr
    int Hi, Wi, Cin, Ho, Wo, Cout, stride, pad, K, M, relu;
    int Hi2, Wi2, Cin2, stride2, nkt1;   // nkt1: k-tiles of the first source
    int m_tiles, n_tiles;
};

// NaN-propagating ReLU (torch.relu(NaN) = NaN): fmaxf would return 0.
__device__ __forceinline__ float relu_nan(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }

// Workgroup -> tile: consecutive workgroup ids go round-robin to the 8 XCDs; XCD x owns a contiguous range of m-tiles and runs
// the n-tiles of one m-tile back to back, so that they share the gathered activation rows through its L2 (resnet.hip: xcd_tile).
__device__ __forceinline__ bool f32_tile(int id, int m_tiles, int n_tiles, int& m_tile, int& n_tile) {
    const int mper = (m_tiles + 7) >> 3;
    const int xcd = id & 7, s = id >> 3;
    n_tile = s % n_tiles;
    m_tile = xcd * mper + s / n_tiles;
    return s / n_tiles < mper && m_tile < m_tiles;
}

// The 8 input channels of ktab entry e (tap dy, dx; channel offset) for the pixel whose tap (0, 0) is `pix` (at iy0, ix0),
// zero outside the image.  A negative entry (bit 31: the training entries' K padding) reads nothing and gives zeros wherever
// its tap would land: the test joins the bounds test, no load and no branch of its own.
__device__ __forceinline__ void gather8(const ConvF32Args& p, long long pix, int iy0, int ix0, int32_t e, float4& v0, float4& v1) {
    const int dy = (int8_t)(e & 0xFF), dx = (int8_t)((e >> 8) & 0xFF), coff = (e >> 16) & 0xFFFF;
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e >= 0 && (unsigned)(iy0 + dy) < (unsigned)p.Hi && (unsigned)(ix0 + dx) < (unsigned)p.Wi) {
        const float4* src = reinterpret_cast<const float4*>(p.in + pix + ((long long)dy * p.Wi + dx) * p.Cin + coff);
        v0 = src[0];
        v1 = src[1];
    }
}

// Backward-data of a stride-2 convolution as a gather (conv_train_f32.hip): the kernel's output pixel (y, x) is a pixel of dx, its
// source image p.in is dy ([Hi, Wi] = the convolution's output), and ktab entry e names the forward tap (ky, kx) and a channel
// offset of dy.  (iy0, ix0) = (y + pad, x + pad); the tap reads dy[(iy0 - ky) / 2][(ix0 - kx) / 2] when both divisions are
// exact and inside dy, zero otherwise (and zero for a negative entry).  `pix` is the element offset of the sample's first dy pixel.
__device__ __forceinline__ void gather8_dgrad_s2(const ConvF32Args& p, long long pix, int iy0, int ix0, int32_t e, float4& v0, float4& v1) {
    const int ky = (int8_t)(e & 0xFF), kx = (int8_t)((e >> 8) & 0xFF), coff = (e >> 16) & 0xFFFF;
    const int ty = iy0 - ky, tx = ix0 - kx;
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e >= 0 && ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && (ty >> 1) < p.Hi && (tx >> 1) < p.Wi) {
        const float4* src = reinterpret_cast<const float4*>(p.in + pix + ((long long)(ty >> 1) * p.Wi + (tx >> 1)) * p.Cin + coff);
        v0 = src[0];
        v1 = src[1];
    }
}

// Implicit-GEMM convolution, block tile 128 pixels x BN channels x 32 k, 4 waves of 64 x BN/2, v_mfma_f32_32x32x2_f32.
// Operand maps of the 32x32x2 form: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; D[i][j] sits at
// j = lane & 31, i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of accumulator register r.  A = activations (i = pixel), B = weights
// (j = output channel), so a lane owns one output channel and the stores of a register are 32 consecutive channels.
// The k of step s (0..15) of a staged tile is h * 16 + s for lane half h: a lane reads 16 consecutive floats of its LDS row as
// four 16-byte loads.  Every output is one fp32 fma chain over all K terms (the tile's k order is a permutation of the
// program's; an fp32 chain's error bound does not depend on it).
// Staging: global -> registers one tile ahead (issued before the MFMAs of the current tile), registers -> LDS after them.
// DGRAD_S2: the activation rows are gathered by gather8_dgrad_s2 (backward-data of a stride-2 convolution; no in2, no residual).
template <int BN, bool DGRAD_S2 = false>
__global__ __launch_bounds__(F_THREADS, 2) void conv_f32_kernel(ConvF32Args p) {
    constexpr int NT = BN / 64;                  // 32-wide n sub-tiles per wave
    constexpr int B_TPR = F_THREADS / BN;        // threads per staged weight row (2 or 4)
    constexpr int B_F4 = F_BK / 4 / B_TPR;       // float4 loads per thread of the weight tile (4 or 2)
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
        if constexpr (DGRAD_S2) {
            if (mvalid) iy0 = oy + p.pad;
            ix0 = ox + p.pad;
            pix = (long long)b * p.Hi * p.Wi * p.Cin;
        } else {
            if (mvalid) iy0 = oy * p.stride - p.pad;
            ix0 = ox * p.stride - p.pad;
            pix = (((long long)b * p.Hi + (mvalid ? iy0 : 0)) * p.Wi + ix0) * p.Cin;
        }
        if (p.in2) pix2 = (((long long)b * p.Hi2 + (long long)oy * p.stride2) * p.Wi2 + (long long)ox * p.stride2) * p.Cin2;
    }
    // ---- this thread's staged weight row
    const int brow = tid / B_TPR, bpart = tid % B_TPR;
    const float* wrow = p.w + (long long)(n0 + brow) * p.K + bpart * (F_BK / B_TPR);

    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;   // (named registers: arrays indexed inside the macro's loops stayed in scratch)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
// global -> registers of k-tile KT
#define LOAD_TILE(KT)                                                                                                          \
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
            if constexpr (DGRAD_S2) {                                                                                          \
                gather8_dgrad_s2(p, pix, iy0, ix0, e_[0], ra0, ra1);                                                           \
                gather8_dgrad_s2(p, pix, iy0, ix0, e_[1], ra2, ra3);                                                           \
            } else {                                                                                                           \
                gather8(p, pix, iy0, ix0, e_[0], ra0, ra1);                                                                    \
                gather8(p, pix, iy0, ix0, e_[1], ra2, ra3);                                                                    \
            }                                                                                                                  \
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
    const int frow = lane & 31, fk = (lane >> 5) * 16;
    const float* a_frag = As + (wr * 64 + frow) * F_LDK + fk;
    const float* b_frag = Bs + (wc * (BN / 2) + frow) * F_LDK + fk;
    LOAD_TILE(0);
    for (int kt = 0; kt < nkt; kt++) {
        // registers -> LDS
        {
            float4* a_ = reinterpret_cast<float4*>(As + arow * F_LDK + ahalf * 16);
            float4* b_ = reinterpret_cast<float4*>(Bs + brow * F_LDK + bpart * (F_BK / B_TPR));
            a_[0] = ra0; a_[1] = ra1; a_[2] = ra2; a_[3] = ra3;
            b_[0] = rb0; b_[1] = rb1;
            if (B_F4 == 4) { b_[2] = rb2; b_[3] = rb3; }
        }
        __syncthreads();
        {   // the next tile, in flight under the MFMAs below (the last iteration loads its own tile again: no branch around the
            // loads, which kept the weight registers in scratch)
            const int kn = kt + 1 < nkt ? kt + 1 : kt;
            LOAD_TILE(kn);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4 af[2], bf[NT];
#pragma unroll
            for (int i = 0; i < 2; i++) af[i] = *reinterpret_cast<const float4*>(a_frag + i * 32 * F_LDK + 4 * q);
#pragma unroll
            for (int j = 0; j < NT; j++) bf[j] = *reinterpret_cast<const float4*>(b_frag + j * 32 * F_LDK + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < NT; j++)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#undef LOAD_TILE

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

template <int BN, bool DGRAD_S2 = false>
int launch_conv(const ConvF32Args& a, hipStream_t s) {
    const long long grid = 8ll * ((a.m_tiles + 7) / 8) * a.n_tiles;
    if (grid > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    hipLaunchKernelGGL((conv_f32_kernel<BN, DGRAD_S2>), dim3((unsigned)grid), dim3(F_THREADS), 0, s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace
