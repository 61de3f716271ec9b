// resnet.hip -- early-fusion ResNet verifier forward pass for gfx950 (MI355X), fp16 MFMA with fp32 accumulation.
//
// Stands behind salve/models/early_fusion.py:41-83 (EarlyFusionCEResnet.forward) with the torchvision ResNet v1.5
// trunk built by salve/models/resnet_factory.py:26-44.  The host (salve_amd/models) folds every BatchNorm into the
// preceding convolution, packs weights as [Cout][KH][KWp][Cin] fp16 and hands the network over as a small "op
// program" (salve_resnet_op_t): CONV (+bias, +residual, ReLU), MAXPOOL 3x3/2, AVGPOOL+FC.  The library just runs it.
//
// Convolution = implicit GEMM on NHWC fp16 activations:  out[m, n] = sum_k A[m, k] W[n, k],  m = (b, oy, ox),
// k = (kh, kw, ci).  Block tile 128 x BN x 64, four waves (2 x 2), v_mfma_f32_16x16x32_f16, the im2col gather of
// A staged global -> registers -> LDS one k-tile ahead of the MFMAs (issue-early / write-late), epilogue through
// LDS so that the residual read and the output store are 16-byte coalesced.  The 7x7/2 stem runs through the same
// kernel: input channels are padded to 8 (or 16) and kw to 8 so that one k-tile is one kernel row.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

#include "../../include/salve_hip.h"
#include "salve_common.h"
#include "resnet_plan.h"

namespace {

typedef __attribute__((__ext_vector_type__(8))) _Float16 act8;  // 8 activations / weights: IEEE half precision
typedef __attribute__((__ext_vector_type__(4))) float f32x4;

constexpr int BM = 128;
constexpr int BK = 64;       // one k-tile = 64 halves = one 128-byte LDS row = 8 chunks of 16 bytes
constexpr int CONV_THREADS = 256;

struct ConvArgs {
    const uint16_t* in;
    const uint16_t* w;
    const float* bias;
    const uint16_t* res;
    uint16_t* out;
    const int32_t* ktab;    // per 8-element chunk of K: dy | dx << 8 | channel offset << 16
    const uint16_t* zeros;  // >= 16 zero bytes: the source of padding taps and of rows beyond M
    int B, Hi, Wi, Cin, Ho, Wo, Cout, stride, pad, K, M, relu;
    int m_tiles, n_tiles;
    // second, point-wise source (SRC2 kernels): k-tiles from nkt1 on read Cin2 channels of in2 at (oy, ox) * stride2
    const uint16_t* in2;
    int Hi2, Wi2, Cin2, stride2, nkt1;
    int32_t* status;        // device status word (salve_hip.h) or nullptr
    int KW, cin_log2;       // conv_wide_kernel: padded kernel width, log2(Cin) (Cin is a power of two there)
    int xcd_contig;         // workgroup -> tile mapping: 1 = every XCD owns a contiguous range of m-tiles (xcd_tile below)
};

// Workgroup -> tile, XCD-aware.  Consecutive workgroup ids are dealt round-robin to the 8 XCDs (each with an L2 of its own), so
// XCD x runs ids x, x + 8, x + 16, ... in that order.  `contig`: XCD x owns the m-tiles [x * mper, (x + 1) * mper), walks them
// in order and runs the n-tiles of one m-tile back to back -- the n-tiles share their activation rows through that L2, AND
// consecutive m-tiles (the neighbouring image rows a 3x3 gather reads again) stay in the same L2.  Measured (round 3, PMC
// FETCH_SIZE at batch 4096): with m-tiles dealt round-robin instead (m_tile % 8 = XCD, the round-1 mapping) the 3x3 kernels
// fetched 1.8 - 2.1 x their input from HBM and the stride-2 3x3 of layer 2 ran AT the HBM roof (6.5 TB/s) on re-reads.
// The grid is 8 * mper * n_tiles workgroups, mper = ceil(m_tiles / 8); workgroups beyond the last m-tile leave at once.
__device__ __forceinline__ bool xcd_tile(int id, int m_tiles, int n_tiles, int contig, int& m_tile, int& n_tile) {
    if (contig) {
        const int mper = (m_tiles + 7) >> 3;
        const int xcd = id & 7, s = id >> 3;
        n_tile = s % n_tiles;
        m_tile = xcd * mper + s / n_tiles;
        return s / n_tiles < mper && m_tile < m_tiles;
    }
    const int per_group = 8 * n_tiles;
    const int g = id / per_group, r = id % per_group;
    m_tile = g * 8 + (r & 7);
    n_tile = r >> 3;
    return m_tile < m_tiles;
}
// The same for a one-dimensional list of `n` tiles (fused bottleneck blocks, stem strips): XCD x owns a contiguous range, so
// the tiles of one image -- which share halo rows -- meet in one L2.  Bijective for every n (the guide's form).
__device__ __forceinline__ int xcd_linear(int id, int n, int contig) {
    if (!contig) return id;
    const int q = n >> 3, r = n & 7, xcd = id & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// Activations and weights are IEEE half precision (fp16: 11 significand bits; the MFMA rate is that of bf16).  With bf16
// storage (8 bits) the logits of the 152-layer network missed the 1e-3 parity bound; fp16 meets it with margin.  The
// conversion saturates at the fp16 range instead of producing infinities.
__device__ __forceinline__ float act_to_f32(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ uint16_t f32_to_act(float f) {
    f = fminf(fmaxf(f, -65504.f), 65504.f);  // (v_max / v_min return the non-NaN operand: a NaN input comes out as -65504)
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}
// Saturation must not pass silently: every epilogue folds the magnitudes it stores into `amax` (v_max3_f32 with |.|
// source modifiers: half an instruction per value) and reports once per thread when the fp16 range was exceeded.
// NaN: the hardware maxima used here and in the ReLUs return their non-NaN operand, so a NaN activation is turned into 0 by
// the next ReLU instead of propagating to the logits as it does in torch -- and does NOT set the status bit.  A NaN can enter
// only through the network input or the weights (fp16 products accumulated in fp32 do not overflow): the host refuses
// non-finite weights when it packs them (hip_resnet.build_program), the rasteriser's tiles are finite by construction, and
// a caller that hands its own tensors to EarlyFusionCEResnet.forward is told so there.
__device__ __forceinline__ void track4(float& amax, float v0, float v1, float v2, float v3) {
    amax = fmaxf(amax, fmaxf(fabsf(v0), fabsf(v1)));
    amax = fmaxf(amax, fmaxf(fabsf(v2), fabsf(v3)));
}
// The epilogue arithmetic of every convolution kernel: four fp32 sums (accumulator + bias [+ residual]) -> [ReLU] -> saturate ->
// fp16, two per dword.  RELU: v_max3 (range tracking; negative sums cannot raise a maximum that starts at 0 and the ReLU stores
// 0 for them) + 2 v_med3 (ReLU and saturation in one: the median of x, 0, 65504) + v_cvt_pk_f16_f32 per PAIR -- 2 instructions
// per value where fmaxf / fminf / two conversions / or took 5 (round 3: the fused 56x56 block issued 1250 vector instructions
// per wave and tile next to its 152 MFMAs).  Same values as f32_to_act(fmaxf(v, 0)): one rounding, to nearest even; a NaN sum
// stores 0 (-65504 without ReLU), as before.
template <bool RELU>
__device__ __forceinline__ uint32_t pack2(float& amax, float a, float b) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    constexpr float lo = RELU ? 0.f : -65504.f;
    amax = RELU ? fmaxf(amax, fmaxf(a, b)) : fmaxf(amax, fmaxf(fabsf(a), fabsf(b)));
    const f2 v = {__builtin_amdgcn_fmed3f(a, lo, 65504.f), __builtin_amdgcn_fmed3f(b, lo, 65504.f)};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, h2));
}
template <bool RELU>
__device__ __forceinline__ uint2 pack4(float& amax, f32x4 v) {
    uint2 o;
    o.x = pack2<RELU>(amax, v[0], v[1]);
    o.y = pack2<RELU>(amax, v[2], v[3]);
    return o;
}
// The same for the general kernels, whose ReLU is a launch argument: `lo` = 0 (ReLU) or -65504, the low side of the range tracked
// as a minimum of its own (half an instruction more per value) -- ONE code path: two copies of the epilogue under a branch made
// hipcc spill in conv8_kernel, whose 128 accumulator registers are live there.  Report fmaxf(amax, relu ? 0 : -amin).
__device__ __forceinline__ uint2 pack4_lo(float& amax, float& amin, f32x4 v, float lo) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    amax = fmaxf(amax, fmaxf(v[0], v[1]));
    amax = fmaxf(amax, fmaxf(v[2], v[3]));
    amin = fminf(amin, fminf(v[0], v[1]));
    amin = fminf(amin, fminf(v[2], v[3]));
    const f2 a = {__builtin_amdgcn_fmed3f(v[0], lo, 65504.f), __builtin_amdgcn_fmed3f(v[1], lo, 65504.f)};
    const f2 b = {__builtin_amdgcn_fmed3f(v[2], lo, 65504.f), __builtin_amdgcn_fmed3f(v[3], lo, 65504.f)};
    uint2 o;
    o.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, h2));
    o.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(b, h2));
    return o;
}
// The sums as vector expressions, so that they become v_pk_add_f32 (two fp32 additions per instruction; same IEEE results).
__device__ __forceinline__ f32x4 vec4(float4 b) { return f32x4{b.x, b.y, b.z, b.w}; }
__device__ __forceinline__ f32x4 vec4(uint2 r) {   // four fp16 residual values
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    return __builtin_convertvector(__builtin_bit_cast(h4, r), f32x4);
}
__device__ __forceinline__ void report_range(int32_t* status, float amax) {
    if (status && !(amax <= 65504.f)) atomicOr(status, SALVE_STATUS_FP16_RANGE);
}

typedef __attribute__((address_space(1))) const void* global_cptr;
typedef __attribute__((address_space(3))) void* lds_ptr;

// LDS accesses next to LDS-DMA in flight.  hipcc (ROCm 7.2) puts an `s_waitcnt vmcnt(0)` in front of every LDS access it takes
// for a possible alias of an LDS-DMA destination -- which drains a prefetch that is meant to stay in flight -- and decides by
// the access TYPE: loads and stores of _Float16 vectors (the MFMA fragments) are left alone, the same bytes accessed as uint2 /
// uint4 / float get the wait (checked on small kernels and in the ISA of these, round 3; the fragment reads of every kernel
// here have always been exempt, which is why the counted waits of conv8_kernel work at all).  The helpers below keep an access
// typed <n x half> whatever its bits mean: the empty asm makes the value opaque, so the optimiser cannot re-type the load or
// store from its uses.  Ordering against the LDS-DMA is the caller's business (counted vmcnt + barrier), as for the fragments.
typedef __attribute__((__ext_vector_type__(4))) _Float16 half4v;
__device__ __forceinline__ uint2 lds_read8(const uint16_t* p) {
    half4v t = *reinterpret_cast<const half4v*>(p);
    asm volatile("" : "+v"(t));
    return __builtin_bit_cast(uint2, t);
}
__device__ __forceinline__ void lds_write8(uint16_t* p, uint2 v) {
    half4v t = __builtin_bit_cast(half4v, v);
    asm volatile("" : "+v"(t));
    *reinterpret_cast<half4v*>(p) = t;
}
__device__ __forceinline__ uint4 lds_read16(const uint16_t* p) {
    act8 t = *reinterpret_cast<const act8*>(p);
    asm volatile("" : "+v"(t));
    return __builtin_bit_cast(uint4, t);
}
__device__ __forceinline__ float4 lds_read_f4(const float* p) {
    act8 t = *reinterpret_cast<const act8*>(p);
    asm volatile("" : "+v"(t));
    return __builtin_bit_cast(float4, t);
}

// Staging: `global_load_lds_dwordx4` -- each lane names its own 16 source bytes (the im2col gather), the wave's 1 KiB
// lands lane-linearly in LDS without passing through VGPRs or the ds_write path.  One wave-instruction fills 8 tile
// rows of 128 bytes, so the LDS image is unpadded; bank conflicts of the 16-byte fragment reads are avoided by a swizzle
// applied on the SOURCE side: LDS slot (row r, 16-byte slot q) holds k-chunk q ^ ((r >> 1) & 7).
// One LDS stage (load, barrier, multiply, barrier; <= 35 KB): four workgroups per CU hide each other's latency.  Measured
// on every layer of ResNet-50 at batch 512, that beats two stages with the next tile's loads in flight under the MFMAs
// (64 KB, two workgroups per CU) by 25-45 %: occupancy, not explicit pipelining, is what this tile size wants.
// POINTWISE: 1x1 / stride 1 / pad 0 -- output pixel m reads input pixel m, so the im2col index arithmetic (three integer
// divisions per staged row, bounds checks per k-tile) disappears; these are 32 of ResNet-50's 53 convolutions.
// SRC2 (with POINTWISE): the GEMM runs over the concatenated channels of two tensors -- see `in2_buf` in salve_hip.h.
template <int BN, bool POINTWISE, bool SRC2 = false>
__global__ __launch_bounds__(CONV_THREADS, 2) void conv_igemm_kernel(ConvArgs p) {
    constexpr int WN = BN / 2;       // wave tile width
    constexpr int NT = WN / 16;      // 16-wide MFMA tiles per wave along n
    constexpr int B_LOADS = BN / 32; // 16-byte chunks of the weight tile per thread
    constexpr int LDC = BN + 8;
    constexpr int STAGE_ELEMS = (BM + BN) * BK;
    constexpr int C_ELEMS = BM * LDC;
    __shared__ __attribute__((aligned(1024))) uint16_t smem[STAGE_ELEMS > C_ELEMS ? STAGE_ELEMS : C_ELEMS];

    int m_tile, n_tile;
    if (!xcd_tile(blockIdx.x, p.m_tiles, p.n_tiles, p.xcd_contig, m_tile, n_tile)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: LDS-DMA bases need no per-load readfirstlane
    const int wr = wave >> 1, wc = wave & 1;
    const int m0 = m_tile * BM, n0 = n_tile * BN;
    const int row_base = tid >> 3;                           // 0..31, plus i * 32
    const int chunk = (tid & 7) ^ ((row_base >> 1) & 7);     // the k-chunk this thread fetches (source-side swizzle)

    // per-thread im2col rows (fixed for the whole K loop)
    int iy0[4], ix0[4];
    const uint16_t* rowp[4];  // POINTWISE: the input pixel's channels (or the zero page, with stride 0)
    const uint16_t* rowp2[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + row_base + i * 32;
        const bool valid = m < p.M;
        rowp2[i] = nullptr;
        if (SRC2 && valid) {
            const int ox = m % p.Wo, t = m / p.Wo, oy = t % p.Ho, b = t / p.Ho;
            rowp2[i] = p.in2 + (((long long)b * p.Hi2 + (long long)oy * p.stride2) * p.Wi2 + (long long)ox * p.stride2) * p.Cin2 + chunk * 8;
        }
        if (POINTWISE) {
            rowp[i] = valid ? p.in + (long long)m * p.Cin + chunk * 8 : nullptr;
            iy0[i] = ix0[i] = 0;
        } else {
            const int mm = valid ? m : 0;
            const int ox = mm % p.Wo, t = mm / p.Wo, oy = t % p.Ho, b = t / p.Ho;
            iy0[i] = valid ? oy * p.stride - p.pad : -100000;  // rows beyond M read zeros
            ix0[i] = ox * p.stride - p.pad;
            // the (possibly out-of-image) pixel of tap (0, 0): all 64-bit arithmetic happens here, once.  A k-tile adds one
            // 32-bit element offset (tap shift + channel offset) shared by the thread's four rows, and tests the bounds with
            // two unsigned compares -- no multiplies, no branches.  The vector instructions a k-tile spends on addresses
            // compete with the MFMAs for the SIMD's issue slot: with the full 64-bit index arithmetic per load the 3x3
            // shapes of ResNet-50 ran 6 % slower (batch 512: 887 -> 833 us over the four of them).
            rowp[i] = p.in + (((long long)b * p.Hi + (valid ? iy0[i] : 0)) * p.Wi + ix0[i]) * p.Cin;
        }
    }
    const uint16_t* wrow = p.w + (long long)(n0 + row_base) * p.K + chunk * 8;

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nkt = p.K / BK;

#define ISSUE_TILE(KT, STAGE, E)                                                                                       \
    {                                                                                                                  \
        uint16_t* As_ = smem + (STAGE) * STAGE_ELEMS + wave * 8 * BK;                                                  \
        uint16_t* Bs_ = As_ + BM * BK;                                                                                 \
        const int dy_ = (int8_t)((E) & 0xFF), dx_ = (int8_t)(((E) >> 8) & 0xFF), coff_ = ((E) >> 16) & 0xFFFF;          \
        const int delta_ = (dy_ * p.Wi + dx_) * p.Cin + coff_;                                                         \
        _Pragma("unroll") for (int i = 0; i < 4; i++) {                                                                \
            const uint16_t* src;                                                                                       \
            if (SRC2 && (KT) >= p.nkt1) {                                                                              \
                src = rowp2[i] ? rowp2[i] + ((KT) - p.nkt1) * BK : p.zeros;                                            \
            } else if (POINTWISE) {                                                                                    \
                src = rowp[i] ? rowp[i] + (KT) * BK : p.zeros;                                                         \
            } else {                                                                                                   \
                const bool ok = (unsigned)(iy0[i] + dy_) < (unsigned)p.Hi && (unsigned)(ix0[i] + dx_) < (unsigned)p.Wi; \
                src = ok ? rowp[i] + delta_ : p.zeros;                                                                 \
            }                                                                                                          \
            __builtin_amdgcn_global_load_lds((global_cptr)src, (lds_ptr)(As_ + i * 32 * BK), 16, 0, 0);                \
        }                                                                                                              \
        _Pragma("unroll") for (int j = 0; j < B_LOADS; j++)                                                            \
            __builtin_amdgcn_global_load_lds((global_cptr)(wrow + (long long)j * 32 * p.K + (KT) * BK),                \
                                             (lds_ptr)(Bs_ + j * 32 * BK), 16, 0, 0);                                  \
    }

    int32_t e_next = POINTWISE ? 0 : p.ktab[chunk];
    const int frag_row = lane & 15, frag_q = lane >> 4, frag_sw = (frag_row >> 1) & 7;
    for (int kt = 0; kt < nkt; kt++) {
        ISSUE_TILE(kt, 0, e_next);
        {   // table entry of the next tile: a plain load, first used in the next iteration
            const int k1 = kt + 1 < nkt ? kt + 1 : nkt - 1;
            if (!POINTWISE) e_next = p.ktab[k1 * 8 + chunk];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of the tile has landed
        __syncthreads();                                  // ... everyone's
        const uint16_t* As = smem;
        const uint16_t* Bs = As + BM * BK;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ks++) {
            act8 af[4], bfr[NT];
            const int slot = ((ks * 4 + frag_q) ^ frag_sw) * 8;
#pragma unroll
            for (int i = 0; i < 4; i++)
                af[i] = *reinterpret_cast<const act8*>(As + (wr * 64 + i * 16 + frag_row) * BK + slot);
#pragma unroll
            for (int j = 0; j < NT; j++)
                bfr[j] = *reinterpret_cast<const act8*>(Bs + (wc * WN + j * 16 + frag_row) * BK + slot);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < NT; j++)
                    // operands swapped: the accumulator is the TRANSPOSED tile, so a lane owns 4 consecutive output
                    // channels of one output pixel (8 bytes of the NHWC row) instead of 4 pixels of one channel
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();  // everyone is done reading the tile
    }
#undef ISSUE_TILE

    // ---- epilogue: (residual tile ->) LDS, add bias / residual / ReLU in fp32 on the accumulator's own elements,
    //      round once to fp16, then 16-byte coalesced stores.
    uint16_t* Cs = smem;
    constexpr int CH_PER_ROW = BN / 8;
    constexpr int C_ITERS = (BM * CH_PER_ROW) / CONV_THREADS;
    // (one 64-bit row offset per thread, then a scalar step per iteration: a v_mad_i64_i32 per copy otherwise)
    constexpr int ROW_STEP = CONV_THREADS / CH_PER_ROW;
    const int crow = tid / CH_PER_ROW, cch = tid % CH_PER_ROW;
    const long long coff = (long long)(m0 + crow) * p.Cout + n0 + cch * 8;
    const int cstep = ROW_STEP * p.Cout;
    if (p.res) {
#pragma unroll
        for (int it = 0; it < C_ITERS; it++) {
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (m0 + crow + it * ROW_STEP < p.M) v = *reinterpret_cast<const uint4*>(p.res + coff + it * cstep);
            *reinterpret_cast<uint4*>(Cs + (crow + it * ROW_STEP) * LDC + cch * 8) = v;
        }
        __syncthreads();
    }
    float amax = 0.f;
    float amin = 0.f;
    const float lo = p.relu ? 0.f : -65504.f;
    // (all of the lane's biases in one batch: inside the loop below -- one basic block per tile column because of the residual
    //  branch -- every column's load was followed by its own wait: NT round trips to the L2 per tile, one after the other; round 4)
    float4 bias_j[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) bias_j[j] = *reinterpret_cast<const float4*>(p.bias + n0 + wc * WN + j * 16 + 4 * (lane >> 4));
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int ncol = wc * WN + j * 16 + 4 * (lane >> 4);  // this lane's 4 consecutive channels of tile column j
        const float4 bias = bias_j[j];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int mrow = wr * 64 + i * 16 + (lane & 15);
            uint2* cell = reinterpret_cast<uint2*>(Cs + mrow * LDC + ncol);
            f32x4 v = acc[i][j] + vec4(bias);
            if (p.res) v += vec4(*cell);
            *cell = pack4_lo(amax, amin, v, lo);
        }
    }

    if (!p.relu) amax = fmaxf(amax, -amin);
    report_range(p.status, amax);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < C_ITERS; it++) {
        if (m0 + crow + it * ROW_STEP < p.M)
            *reinterpret_cast<uint4*>(p.out + coff + it * cstep) = *reinterpret_cast<const uint4*>(Cs + (crow + it * ROW_STEP) * LDC + cch * 8);
    }
}

#ifdef SALVE_BUILD_ABLATIONS   // the measured-and-rejected wide-tile kernels d / e / f: tools/probe/build_ablations.sh only
#include "../../tools/probe/ablations/conv_wide.h"
#endif
#include "conv8.h"
#include "stem_pool.h"
#include "expand_chain.h"
#include "bottleneck.h"

// 3x3 / stride 2 / pad 1 max-pool on NHWC fp16, 8 channels (16 bytes) per thread.
__global__ __launch_bounds__(256) void maxpool_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int B,
                                                      int Hi, int Wi, int C, int Ho, int Wo) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c8 = C / 8;
    const long long total = (long long)B * Ho * Wo * c8;
    if (idx >= total) return;
    const int ch = (int)(idx % c8);
    long long t = idx / c8;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float best[8];
#pragma unroll
    for (int k = 0; k < 8; k++) best[k] = -3.0e38f;
    for (int dy = 0; dy < 3; dy++) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= Hi) continue;
        for (int dx = 0; dx < 3; dx++) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= Wi) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(in + (((long long)b * Hi + iy) * Wi + ix) * C + ch * 8);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                best[2 * k] = fmaxf(best[2 * k], act_to_f32((uint16_t)(w[k] & 0xFFFFu)));
                best[2 * k + 1] = fmaxf(best[2 * k + 1], act_to_f32((uint16_t)(w[k] >> 16)));
            }
        }
    }
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (uint32_t)f32_to_act(best[2 * k]) | ((uint32_t)f32_to_act(best[2 * k + 1]) << 16);
    *reinterpret_cast<uint4*>(out + (((long long)b * Ho + oy) * Wo + ox) * C + ch * 8) = uint4{o[0], o[1], o[2], o[3]};
}

// Global average pool over HW positions + fully connected layer (fp32 weights), one block per sample.  A thread owns 8
// consecutive channels (16-byte loads, coalesced across the block) and walks the positions; the per-class partial dot
// products are then reduced across the block.
__global__ __launch_bounds__(256) void avgpool_fc_kernel(const uint16_t* __restrict__ in, int HW, int C,
                                                         const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                         int ncls, float* __restrict__ logits) {
    __shared__ float red[8][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint16_t* x = in + (long long)b * HW * C;
    float part[8];  // ncls <= 8
#pragma unroll
    for (int k = 0; k < 8; k++) part[k] = 0.f;
    const float inv = 1.0f / (float)HW;
    for (int c0 = tid * 8; c0 < C; c0 += 256 * 8) {
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; e++) s[e] = 0.f;
        for (int i = 0; i < HW; i++) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + (long long)i * C + c0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                s[2 * e] += act_to_f32((uint16_t)(w[e] & 0xFFFFu));
                s[2 * e + 1] += act_to_f32((uint16_t)(w[e] >> 16));
            }
        }
        for (int k = 0; k < ncls; k++) {
            const float* wk = fcw + (long long)k * C + c0;
#pragma unroll
            for (int e = 0; e < 8; e++) part[k] += (s[e] * inv) * wk[e];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float v = part[k];
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (tid < ncls) logits[(long long)b * ncls + tid] = ((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3])) + fcb[tid];
}

// ------------------------------------------------------------------------------------------------ the driver
// Which kernel runs which ops is decided once, by plan_resnet (resnet_plan.h, host only, pinned by tests/test_resnet_plan_host.py);
// salve_resnet_forward launches the steps of that plan, one launch_* function per step kind.
using namespace salve_plan;
static_assert(PLAN_BK == BK && PLAN_STEM_W == STEM_W && PLAN_STEM_R == STEM_R, "resnet_plan.h plans for other kernels than these");

struct ResnetHandle {
    std::vector<salve_resnet_op_t> ops;
    std::vector<Step> plan;    // the launches of a forward pass, in order (resnet_plan.h)
    uint16_t* d_weights = nullptr;
    float* d_params = nullptr;
    int32_t* d_ktab = nullptr;
    uint16_t* d_zeros = nullptr;
    size_t max_act_elems = 0;  // per sample, elements of the largest activation buffer
    int n_bufs = 0;
    int num_layers = 0, in_channels = 0, ncls = 0;
    int xcd_contig = 1;        // SALVE_RESNET_ROUND_ROBIN_TILES clears it: the round-1 mapping (m-tiles dealt round-robin to the XCDs), for A/B runs
    int n_cus = 256;
    int chain_dbg = 0;         // ablation build only (timing-only switches of expand_chain_kernel)
    int no_transposed_tiles = 0;   // SALVE_RESNET_NO_TRANSPOSED_TILES: the fused blocks' fourth, half-empty tile column instead (bit-identity tests, A/B)
};

// One forward pass: the handle, the batch and where its tensors are.
struct Pass {
    const ResnetHandle* h;
    const void* input;
    uint16_t* base;        // the activation buffers, buf_elems apart
    size_t buf_elems;
    int batch;
    float* logits;
    int32_t* status;
    hipStream_t s;
    uint16_t* buf(int i) const { return i < 0 ? const_cast<uint16_t*>(reinterpret_cast<const uint16_t*>(input)) : base + (size_t)i * buf_elems; }
    const salve_resnet_op_t& op(const Step& st, int k) const { return h->ops[(size_t)st.first + k]; }   // the step's k-th op
};

int launch_stem_pool(const Pass& p, const Step& st) {
    const ResnetHandle* h = p.h;
    const salve_resnet_op_t &o = p.op(st, 0), &pool = p.op(st, 1);
    StemArgs a;
    a.x = p.buf(o.in_buf);
    a.w = h->d_weights + o.w_off;
    a.bias = h->d_params + o.b_off;
    a.y = p.buf(pool.out_buf);
    a.zeros = h->d_zeros;
    a.B = p.batch; a.H = o.Hi; a.W = o.Wi; a.status = p.status;
    const long long strips = (long long)p.batch * ((o.Hi / 4) / STEM_R);
    const unsigned grid = (unsigned)(strips < h->n_cus ? strips : h->n_cus);   // persistent: one workgroup per CU, a contiguous range of strips each
    if (o.Cin == 24) hipLaunchKernelGGL(stem_pool_kernel<3>, dim3(grid), dim3(STEM_THREADS), 0, p.s, a);
    else if (o.Cin == 16) hipLaunchKernelGGL(stem_pool_kernel<2>, dim3(grid), dim3(STEM_THREADS), 0, p.s, a);
    else hipLaunchKernelGGL(stem_pool_kernel<1>, dim3(grid), dim3(STEM_THREADS), 0, p.s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int launch_bottleneck(const Pass& p, const Step& st) {
    const ResnetHandle* h = p.h;
    const salve_resnet_op_t &o = p.op(st, 0), &ob = p.op(st, 1), &oc = p.op(st, 2);
    BottleneckArgs a;
    a.x = p.buf(o.in_buf);
    a.y = p.buf(oc.out_buf);
    a.wa = h->d_weights + o.w_off; a.wb = h->d_weights + ob.w_off; a.wc = h->d_weights + oc.w_off;
    a.ba = h->d_params + o.b_off; a.bb = h->d_params + ob.b_off; a.bc = h->d_params + oc.b_off;
    a.zeros = h->d_zeros;
    a.B = p.batch; a.H = o.Hi; a.W = o.Wi; a.status = p.status; a.xcd_contig = h->xcd_contig;
    constexpr int th = 8;   // 64 mid channels (the only blocks the planner fuses): 8 x 16 pixel tiles
    // a strip of exactly TH columns right of the whole tile columns (56 = 3 x 16 + 8) is covered by transposed tiles of 16 rows
    const bool strip = (o.Wi % 16) == th && !h->no_transposed_tiles;
    a.tiles_x = strip ? o.Wi / 16 : (o.Wi + 15) / 16;
    a.tiles_y = o.Hi / th;
    a.tiles_t = strip ? (o.Hi + 15) / 16 : 0;
    const long long grid = (long long)p.batch * (a.tiles_x * a.tiles_y + a.tiles_t);
    if (grid > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    a.wd = nullptr; a.bd = nullptr; a.t1n = nullptr; a.y_even = 0;
    if (st.form == BLOCK_NEXT) {
        const salve_resnet_op_t& on = p.op(st, 3);
        a.wd = h->d_weights + on.w_off; a.bd = h->d_params + on.b_off; a.t1n = p.buf(on.out_buf); a.y_even = st.y_even;
    }
    if (st.form == BLOCK_PROJ) hipLaunchKernelGGL((bottleneck_kernel<64, th, true>), dim3((unsigned)grid), dim3(BN_THREADS), 0, p.s, a);
    else if (st.form == BLOCK_NEXT) hipLaunchKernelGGL((bottleneck_kernel<64, th, false, true>), dim3((unsigned)grid), dim3(BN_THREADS), 0, p.s, a);
    else hipLaunchKernelGGL((bottleneck_kernel<64, th>), dim3((unsigned)grid), dim3(BN_THREADS), 0, p.s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

// One instantiation of expand_chain_kernel: its tile is ROWS = 16 NW / NSPLIT pixels, its workgroup NW waves.
template <int MID, int MIDN, int R, bool CHAIN, int AHEAD = 2, int NW = 8, int NSPLIT = 1>
void launch_chain_form(const Pass& p, ChainArgs& a) {
    constexpr int rows = NW * 16 / NSPLIT;
    a.n_tiles = (int)(((long long)a.M + rows - 1) / rows);
    const unsigned grid = (unsigned)(a.n_tiles < p.h->n_cus ? a.n_tiles : p.h->n_cus);   // persistent: one workgroup per CU
    hipLaunchKernelGGL((expand_chain_kernel<MID, MIDN, R, CHAIN, AHEAD, NW, NSPLIT>), dim3(grid), dim3(NW * 64), 0, p.s, a);
}

int launch_expand_chain(const Pass& p, const Step& st) {
    const ResnetHandle* h = p.h;
    const salve_resnet_op_t &o = p.op(st, 0), &on = p.op(st, st.chained ? 1 : 0);
    ChainArgs a;
    a.t2 = p.buf(o.in_buf); a.x = p.buf(o.res_buf); a.y = p.buf(o.out_buf);
    a.wc = h->d_weights + o.w_off; a.bc = h->d_params + o.b_off;
    a.t1n = st.chained ? p.buf(on.out_buf) : nullptr;
    a.wa = st.chained ? h->d_weights + on.w_off : nullptr;
    a.ba = st.chained ? h->d_params + on.b_off : nullptr;
    a.zeros = h->d_zeros;
    const long long M = (long long)p.batch * o.Ho * o.Wo;
    if (M > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    a.M = (int)M;
    a.status = p.status;
    a.y_even_w = st.y_even ? o.Wo : 0;
    a.dbg = h->chain_dbg;
    switch (st.form) {
    case CHAIN_X128: launch_chain_form<128, 128, 14, false>(p, a); break;
    case CHAIN_X256: launch_chain_form<256, 256, 12, false>(p, a); break;
    case CHAIN_C128_128: launch_chain_form<128, 128, 12, true>(p, a); break;
    case CHAIN_C128_256: launch_chain_form<128, 256, 8, true>(p, a); break;
    case CHAIN_C256_256: launch_chain_form<256, 256, 5, true>(p, a); break;
    case CHAIN_X256_SPLIT: launch_chain_form<256, 256, 12, false, 2, 16, 2>(p, a); break;
    case CHAIN_C128_256_SPLIT: launch_chain_form<128, 256, 8, true, 2, 16, 2>(p, a); break;
    case CHAIN_C256_256_SPLIT: launch_chain_form<256, 256, 5, true, 2, 16, 2>(p, a); break;
    case CHAIN_X128_W16: launch_chain_form<128, 128, 7, false, 2, 16>(p, a); break;
    case CHAIN_C128_128_W16: launch_chain_form<128, 128, 6, true, 2, 16>(p, a); break;
    }
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int launch_conv(const Pass& p, const Step& st) {
    const ResnetHandle* h = p.h;
    const salve_resnet_op_t& o = p.op(st, 0);
    hipStream_t s = p.s;
    ConvArgs a;
    a.in = p.buf(o.in_buf);
    a.w = h->d_weights + o.w_off;
    a.bias = h->d_params + o.b_off;
    a.res = o.res_buf != SALVE_NO_BUF ? p.buf(o.res_buf) : nullptr;
    a.out = p.buf(o.out_buf);
    a.ktab = h->d_ktab + o.ktab_off;
    a.zeros = h->d_zeros;
    a.status = p.status;
    a.xcd_contig = h->xcd_contig;
    a.B = p.batch; a.Hi = o.Hi; a.Wi = o.Wi; a.Cin = o.Cin; a.Ho = o.Ho; a.Wo = o.Wo; a.Cout = o.Cout;
    a.stride = o.stride; a.pad = o.pad; a.K = o.KH * o.KW * o.Cin; a.relu = o.relu;
    const bool src2 = o.in2_buf != SALVE_NO_BUF;
    a.in2 = src2 ? p.buf(o.in2_buf) : nullptr;
    a.Hi2 = o.Hi2; a.Wi2 = o.Wi2; a.Cin2 = o.Cin2; a.stride2 = o.stride2;
    a.nkt1 = a.K / BK;
    if (src2) a.K += o.Cin2;
    const long long M = (long long)p.batch * o.Ho * o.Wo;
    if (M > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    a.M = (int)M;
    a.KW = o.KW;
    a.cin_log2 = 0;
    while ((1 << a.cin_log2) < o.Cin) a.cin_log2++;
    const bool pw = pointwise(o);
    if (conv_runs_wide(st, o, p.batch)) {
        const int cfg = st.form;
        const int bn = (cfg == WIDE_256_K64_S2 || cfg == WIDE_8PHASE) ? 256 : 128;
        a.m_tiles = (int)((M + C8_BM - 1) / C8_BM);
        a.n_tiles = o.Cout / bn;
        const unsigned grid = (unsigned)(((a.m_tiles + 7) / 8) * 8 * a.n_tiles);
#ifdef SALVE_BUILD_ABLATIONS
#define WIDE_LAUNCH(BN_, KS_, NS_)                                                                                                  \
    {                                                                                                                               \
        if (src2) hipLaunchKernelGGL((conv_wide_kernel<BN_, KS_, NS_, true, true>), dim3(grid), dim3(WIDE_THREADS), 0, s, a);       \
        else if (pw) hipLaunchKernelGGL((conv_wide_kernel<BN_, KS_, NS_, true, false>), dim3(grid), dim3(WIDE_THREADS), 0, s, a);   \
        else hipLaunchKernelGGL((conv_wide_kernel<BN_, KS_, NS_, false, false>), dim3(grid), dim3(WIDE_THREADS), 0, s, a);          \
    }
#endif
        if (cfg == WIDE_8PHASE) {
            if (src2) hipLaunchKernelGGL((conv8_kernel<true, true>), dim3(grid), dim3(C8_THREADS), 0, s, a);
            else if (pw) hipLaunchKernelGGL((conv8_kernel<true, false>), dim3(grid), dim3(C8_THREADS), 0, s, a);
            else hipLaunchKernelGGL((conv8_kernel<false, false>), dim3(grid), dim3(C8_THREADS), 0, s, a);
        }
#ifdef SALVE_BUILD_ABLATIONS
        else if (cfg == WIDE_PC_128) {
            if (src2) hipLaunchKernelGGL((conv_pc_kernel<true, true>), dim3(grid), dim3(PC_THREADS), 0, s, a);
            else if (pw) hipLaunchKernelGGL((conv_pc_kernel<true, false>), dim3(grid), dim3(PC_THREADS), 0, s, a);
            else hipLaunchKernelGGL((conv_pc_kernel<false, false>), dim3(grid), dim3(PC_THREADS), 0, s, a);
        } else if (cfg == WIDE_256_K64_S2) WIDE_LAUNCH(256, 64, 2)
        else WIDE_LAUNCH(128, 64, 1)
#undef WIDE_LAUNCH
#endif
        SALVE_HIP_CHECK(hipGetLastError());
        return SALVE_OK;
    }
    a.m_tiles = (int)((M + BM - 1) / BM);
    const int bn = (o.Cout % 128 == 0) ? 128 : 64;
    a.n_tiles = o.Cout / bn;
    const unsigned grid = (unsigned)(((a.m_tiles + 7) / 8) * 8 * a.n_tiles);
    if (src2 && bn == 128) hipLaunchKernelGGL((conv_igemm_kernel<128, true, true>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    else if (src2) hipLaunchKernelGGL((conv_igemm_kernel<64, true, true>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    else if (bn == 128 && pw) hipLaunchKernelGGL((conv_igemm_kernel<128, true>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    else if (bn == 128) hipLaunchKernelGGL((conv_igemm_kernel<128, false>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    else if (pw) hipLaunchKernelGGL((conv_igemm_kernel<64, true>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    else hipLaunchKernelGGL((conv_igemm_kernel<64, false>), dim3(grid), dim3(CONV_THREADS), 0, s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int launch_maxpool(const Pass& p, const Step& st) {
    const salve_resnet_op_t& o = p.op(st, 0);
    const long long total = (long long)p.batch * o.Ho * o.Wo * (o.Cin / 8);
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p.s, p.buf(o.in_buf), p.buf(o.out_buf),
                       p.batch, o.Hi, o.Wi, o.Cin, o.Ho, o.Wo);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int launch_avgpool_fc(const Pass& p, const Step& st) {
    const salve_resnet_op_t& o = p.op(st, 0);
    hipLaunchKernelGGL(avgpool_fc_kernel, dim3(p.batch), dim3(256), 0, p.s, p.buf(o.in_buf), o.Hi * o.Wi,
                       o.Cin, p.h->d_params + o.w_off, p.h->d_params + o.b_off, o.Cout, p.logits);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace

extern "C" {

void* salve_resnet_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                          const void* weights_f16, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                          const int32_t* ktab, size_t ktab_entries, int32_t flags) {
    if (!ops || n_ops <= 0 || !weights_f16 || !params_f32 || !ktab) {
        salve_fail("salve_resnet_create: null argument");
        return nullptr;
    }
    if (flags & ~SALVE_RESNET_ALL_FLAGS) {
        salve_fail("salve_resnet_create: unknown bit in flags (SALVE_RESNET_*): a caller written for another ABI version");
        return nullptr;
    }
    int conv_wide = -1;
#ifdef SALVE_BUILD_ABLATIONS   // development build only: the rejected wide-tile kernels d / e / f of tools/probe/ablations/conv_wide.h
    if (const char* e = getenv("SALVE_CONV_WIDE")) conv_wide = e[0] == 'd' ? WIDE_256_K64_S2 : (e[0] == 'e' ? WIDE_128_K64_S1 : (e[0] == 'f' ? WIDE_PC_128 : -1));
#endif
    std::vector<Step> plan = plan_resnet(ops, n_ops, ktab, ktab_entries, flags, conv_wide);
    if (plan.empty()) return nullptr;   // an op was refused (check_op)
    ResnetHandle* h = new ResnetHandle();
    h->num_layers = num_layers;
    h->in_channels = in_channels;
    h->plan.swap(plan);
    for (int i = 0; i < n_ops; i++) {
        const salve_resnet_op_t& o = ops[i];
        h->ops.push_back(o);
        if (o.op != SALVE_OP_AVGPOOL_FC) {
            const size_t e = (size_t)o.Ho * o.Wo * o.Cout;
            if (e > h->max_act_elems) h->max_act_elems = e;
            if (o.out_buf + 1 > h->n_bufs) h->n_bufs = o.out_buf + 1;
        } else {
            h->ncls = o.Cout;
        }
    }
    h->xcd_contig = (flags & SALVE_RESNET_ROUND_ROBIN_TILES) ? 0 : 1;
    h->no_transposed_tiles = (flags & SALVE_RESNET_NO_TRANSPOSED_TILES) ? 1 : 0;
#ifdef SALVE_BUILD_ABLATIONS   // development build only: timing-only switches of expand_chain_kernel (they compute WRONG results)
    if (const char* d = getenv("SALVE_CHAIN_DBG")) h->chain_dbg = atoi(d);
#endif
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        h->n_cus = cus;
    if (hipMalloc(&h->d_weights, weights_bytes) != hipSuccess || hipMalloc(&h->d_params, params_bytes) != hipSuccess ||
        hipMalloc(&h->d_ktab, ktab_entries * sizeof(int32_t)) != hipSuccess || hipMalloc(&h->d_zeros, 256) != hipSuccess) {
        salve_fail("salve_resnet_create: hipMalloc failed");
        salve_resnet_destroy(h);
        return nullptr;
    }
    if (hipMemcpy(h->d_weights, weights_f16, weights_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_params, params_f32, params_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_ktab, ktab, ktab_entries * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->d_zeros, 0, 256) != hipSuccess) {
        salve_fail("salve_resnet_create: hipMemcpy failed");
        salve_resnet_destroy(h);
        return nullptr;
    }
    return h;
}

void salve_resnet_destroy(void* handle) {
    ResnetHandle* h = reinterpret_cast<ResnetHandle*>(handle);
    if (!h) return;
    if (h->d_weights) (void)hipFree(h->d_weights);
    if (h->d_params) (void)hipFree(h->d_params);
    if (h->d_ktab) (void)hipFree(h->d_ktab);
    if (h->d_zeros) (void)hipFree(h->d_zeros);
    delete h;
}

int salve_resnet_num_layers(void* handle) { return handle ? reinterpret_cast<ResnetHandle*>(handle)->num_layers : 0; }

size_t salve_resnet_workspace_bytes(void* handle, int32_t batch) {
    ResnetHandle* h = reinterpret_cast<ResnetHandle*>(handle);
    if (!h || batch <= 0) return 0;
    return (size_t)h->n_bufs * (size_t)batch * h->max_act_elems * sizeof(uint16_t) + 256;
}

int salve_resnet_forward(void* handle, const void* input, int32_t batch, float* logits, void* workspace,
                         size_t workspace_bytes, int32_t* status, void* stream) {
    ResnetHandle* h = reinterpret_cast<ResnetHandle*>(handle);
    if (!h || !input || !logits || !workspace || batch <= 0) {
        salve_fail("salve_resnet_forward: null argument or bad batch");
        return SALVE_ERR_BAD_ARG;
    }
    if (workspace_bytes < salve_resnet_workspace_bytes(handle, batch)) {
        salve_fail("salve_resnet_forward: workspace too small");
        return SALVE_ERR_WORKSPACE;
    }
    const Pass p = {h, input, reinterpret_cast<uint16_t*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255), (size_t)batch * h->max_act_elems,
                    batch, logits, status, (hipStream_t)stream};
    for (const Step& st : h->plan) {
        int rc = SALVE_OK;
        switch (st.kind) {
        case STEM_POOL: rc = launch_stem_pool(p, st); break;
        case BOTTLENECK: rc = launch_bottleneck(p, st); break;
        case EXPAND_CHAIN: rc = launch_expand_chain(p, st); break;
        case CONV: rc = launch_conv(p, st); break;
        case MAXPOOL: rc = launch_maxpool(p, st); break;
        case AVGPOOL_FC: rc = launch_avgpool_fc(p, st); break;
        }
        if (rc != SALVE_OK) return rc;
    }
    return SALVE_OK;
}

}  // extern "C"
