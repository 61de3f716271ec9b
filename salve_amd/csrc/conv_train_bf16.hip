// conv_train_bf16.hip -- per-convolution bf16 entries for opt-in mixed-precision training of the verifier on gfx950 (MI355X):
// forward, backward-data (dgrad) and backward-weight (wgrad) of one convolution, bf16 operands on the bf16 matrix cores with fp32
// accumulation.  The same descriptors, layouts and refusals as the fp32 entries: both run conv_train.h's shape contract
// (check_desc) and host drivers; this file holds the bf16 kernels and the bf16 precision policy.  The caller keeps fp32 master
// weights and passes their bf16 copy (salve_amd/models/trainable.py: Conv2dBF16Function).
//
//   forward  conv_bf16_kernel: implicit GEMM, M = batch * Ho * Wo pixels, N = Cout, K = KH * KW * Cin, block tile 128 pixels x
//            BN channels x 64 k, 4 waves, v_mfma_f32_16x16x32_bf16.  The staging is conv_igemm_kernel's (resnet.hip): each lane
//            names the 16 source bytes of one k-table entry (8 channels of one tap) and global_load_lds_dwordx4 drops them into
//            LDS, swizzled on the source side; taps outside the image read a zero page.  fp32 accumulation, ONE rounding to
//            bf16 per output in the epilogue (a plain conversion: v_cvt_pk_bf16_f32, NaN stays NaN), no bias, no activation.
//            The stems' K = 49 * Cin is padded to a multiple of 64 with zero weight columns whose table entries are negative:
//            they read the zero page and no pixel.
//   dgrad    stride 1: conv_bf16_kernel over dy with the weights transposed ([Cin][KH][KW][Cout]) and rotated by 180 degrees on the
//            device, pad' = KH - 1 - pad.  Stride 2: the DGRAD_S2 gather of conv_f32.h -- the tap (ky, kx) of dx pixel (iy, ix)
//            reads dy[(iy + pad - ky) / 2][(ix + pad - kx) / 2] when both divisions are exact, the zero page otherwise (the
//            zero terms are multiplied).  The stem's dgrad is refused (SALVE_ERR_UNSUPPORTED).
//   wgrad    wgrad_bf16_kernel: dW[Cout, K] = sum over the batch * Ho * Wo pixels of dy (x) x_patch with the pixels as the MFMA
//            reduction; bf16 x bf16 products are exact in fp32.  The pixel range is split over workgroups into fp32 partial slabs
//            that wgrad_combine_kernel sums in split order: no atomics, the same inputs give bit-identical dW, which stays
//            fp32 throughout.  Both operands are transposed on their way into LDS (pixels along the LDS row), 4 pixels x 8
//            channels per thread.
#include "conv_train.h"

namespace {

typedef __attribute__((__ext_vector_type__(8))) __bf16 bf16x8;
typedef __attribute__((__ext_vector_type__(4))) __bf16 bf16x4;
typedef __attribute__((__ext_vector_type__(4))) float f32x4;
typedef __attribute__((address_space(1))) const void* global_cptr;
typedef __attribute__((address_space(3))) void* lds_ptr;

constexpr int G_BM = 128;        // output pixels per forward / dgrad workgroup
constexpr int G_BK = 64;         // k per staged tile: 8 table entries of 8 channels = one 128-byte LDS row
constexpr int G_THREADS = 256;   // 4 waves, 2 x 2 over the block tile
constexpr int ZERO_BYTES = 256;  // the zero page of padding taps and of rows beyond M (>= 16 bytes)

constexpr int W_BK = 128;           // k columns per wgrad workgroup
constexpr int W_LDP = W_BP + 8;     // LDS row pitch in bf16 (80 B: the 16-byte fragment reads of 16 rows hit 16 distinct slots)
constexpr int W_MIN_TILES = 16;     // staged pixel tiles per split at least

struct ConvBf16Args {
    const uint16_t* in;     // NHWC [.., Hi, Wi, Cin] bf16
    const uint16_t* w;      // [Cout][K] bf16
    uint16_t* out;          // [M][Cout] bf16
    const int32_t* ktab;    // one entry per 8 consecutive k: dy | dx << 8 | channel offset << 16; a negative entry reads the zero page
    const uint16_t* zeros;  // ZERO_BYTES of zeros
    int Hi, Wi, Cin, Ho, Wo, Cout, stride, pad, K, M;
    int m_tiles, n_tiles;
};

// Workgroup -> tile: consecutive ids go round-robin to the 8 XCDs; XCD x owns a contiguous range of m-tiles and runs the n-tiles
// of one m-tile back to back, so that they share the gathered activation rows through its L2 (resnet.hip: xcd_tile).
__device__ __forceinline__ bool bf16_tile(int id, int m_tiles, int n_tiles, int& m_tile, int& n_tile) {
    const int mper = (m_tiles + 7) >> 3;
    const int xcd = id & 7, s = id >> 3;
    n_tile = s % n_tiles;
    m_tile = xcd * mper + s / n_tiles;
    return s / n_tiles < mper && m_tile < m_tiles;
}

// Implicit-GEMM convolution (conv_igemm_kernel's structure and staging).  One LDS stage: issue the tile's LDS-DMA loads, wait,
// barrier, 2 x 4 x NT MFMAs per wave, barrier.  LDS slot (row r, 16-byte slot q) holds k-chunk q ^ ((r >> 1) & 7).
// Operands swapped in the MFMA: the accumulator is the transposed tile, so a lane owns 4 consecutive output channels of one pixel.
template <int BN, int MODE>
__global__ __launch_bounds__(G_THREADS, 2) void conv_bf16_kernel(ConvBf16Args p) {
    constexpr int WN = BN / 2;
    constexpr int NT = WN / 16;
    constexpr int B_LOADS = BN / 32;
    constexpr int LDC = BN + 8;
    constexpr int STAGE_ELEMS = (G_BM + BN) * G_BK;
    constexpr int C_ELEMS = G_BM * LDC;
    __shared__ __attribute__((aligned(1024))) uint16_t smem[STAGE_ELEMS > C_ELEMS ? STAGE_ELEMS : C_ELEMS];

    int m_tile, n_tile;
    if (!bf16_tile(blockIdx.x, p.m_tiles, p.n_tiles, m_tile, n_tile)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int m0 = m_tile * G_BM, n0 = n_tile * BN;
    const int row_base = tid >> 3;
    const int chunk = (tid & 7) ^ ((row_base >> 1) & 7);

    // per-thread rows (fixed for the whole K loop)
    int iy0[4], ix0[4];
    const uint16_t* rowp[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + row_base + i * 32;
        const bool valid = m < p.M;
        const int mm = valid ? m : 0;
        const int ox = mm % p.Wo, t = mm / p.Wo, oy = t % p.Ho, b = t / p.Ho;
        if (MODE == POINTWISE) {
            rowp[i] = valid ? p.in + (long long)m * p.Cin + chunk * 8 : nullptr;
            iy0[i] = ix0[i] = 0;
        } else if (MODE == DGRAD_S2) {
            iy0[i] = valid ? oy + p.pad : -100000;
            ix0[i] = ox + p.pad;
            rowp[i] = p.in + (long long)b * p.Hi * p.Wi * p.Cin;
        } else {
            iy0[i] = valid ? oy * p.stride - p.pad : -100000;
            ix0[i] = ox * p.stride - p.pad;
            rowp[i] = p.in + (((long long)b * p.Hi + (valid ? iy0[i] : 0)) * p.Wi + ix0[i]) * p.Cin;
        }
    }
    const uint16_t* wrow = p.w + (long long)(n0 + row_base) * p.K + chunk * 8;

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nkt = p.K / G_BK;
    int32_t e_next = MODE == POINTWISE ? 0 : p.ktab[chunk];
    const int frag_row = lane & 15, frag_q = lane >> 4, frag_sw = (frag_row >> 1) & 7;
    for (int kt = 0; kt < nkt; kt++) {
        {
            uint16_t* As_ = smem + wave * 8 * G_BK;
            uint16_t* Bs_ = As_ + G_BM * G_BK;
            const int32_t e = e_next;
            const int ky = (int8_t)(e & 0xFF), kx = (int8_t)((e >> 8) & 0xFF), coff = (e >> 16) & 0xFFFF;
            const int delta = (ky * p.Wi + kx) * p.Cin + coff;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint16_t* src;
                if (MODE == POINTWISE) {
                    src = rowp[i] ? rowp[i] + kt * G_BK : p.zeros;
                } else if (MODE == DGRAD_S2) {
                    const int ty = iy0[i] - ky, tx = ix0[i] - kx;
                    const bool ok = e >= 0 && !((ty | tx) & 1) && (unsigned)(ty >> 1) < (unsigned)p.Hi && (unsigned)(tx >> 1) < (unsigned)p.Wi;
                    src = ok ? rowp[i] + ((long long)(ty >> 1) * p.Wi + (tx >> 1)) * p.Cin + coff : p.zeros;
                } else {
                    const bool ok = e >= 0 && (unsigned)(iy0[i] + ky) < (unsigned)p.Hi && (unsigned)(ix0[i] + kx) < (unsigned)p.Wi;
                    src = ok ? rowp[i] + delta : p.zeros;
                }
                __builtin_amdgcn_global_load_lds((global_cptr)src, (lds_ptr)(As_ + i * 32 * G_BK), 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < B_LOADS; j++)
                __builtin_amdgcn_global_load_lds((global_cptr)(wrow + (long long)j * 32 * p.K + kt * G_BK), (lds_ptr)(Bs_ + j * 32 * G_BK),
                                                 16, 0, 0);
        }
        if (MODE != POINTWISE) {   // table entry of the next tile: a plain load, first used in the next iteration
            const int k1 = kt + 1 < nkt ? kt + 1 : nkt - 1;
            e_next = p.ktab[k1 * 8 + chunk];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of the tile has landed
        __syncthreads();                                  // ... everyone's
        const uint16_t* As = smem;
        const uint16_t* Bs = As + G_BM * G_BK;
#pragma unroll
        for (int ks = 0; ks < G_BK / 32; ks++) {
            bf16x8 af[4], bfr[NT];
            const int slot = ((ks * 4 + frag_q) ^ frag_sw) * 8;
#pragma unroll
            for (int i = 0; i < 4; i++) af[i] = *reinterpret_cast<const bf16x8*>(As + (wr * 64 + i * 16 + frag_row) * G_BK + slot);
#pragma unroll
            for (int j = 0; j < NT; j++) bfr[j] = *reinterpret_cast<const bf16x8*>(Bs + (wc * WN + j * 16 + frag_row) * G_BK + slot);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();   // everyone is done reading the tile
    }

    // ---- epilogue: round once to bf16 into LDS, then 16-byte coalesced stores of whole 8-channel chunks
    uint16_t* Cs = smem;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int ncol = wc * WN + j * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int mrow = wr * 64 + i * 16 + (lane & 15);
            *reinterpret_cast<uint2*>(Cs + mrow * LDC + ncol) = __builtin_bit_cast(uint2, __builtin_convertvector(acc[i][j], bf16x4));
        }
    }
    __syncthreads();
    constexpr int CH_PER_ROW = BN / 8;
    constexpr int ROW_STEP = G_THREADS / CH_PER_ROW;
    constexpr int C_ITERS = G_BM / ROW_STEP;
    const int crow = tid / CH_PER_ROW, cch = tid % CH_PER_ROW;
#pragma unroll
    for (int it = 0; it < C_ITERS; it++) {
        const int r = crow + it * ROW_STEP;
        if (m0 + r < p.M)
            *reinterpret_cast<uint4*>(p.out + (long long)(m0 + r) * p.Cout + n0 + cch * 8) = *reinterpret_cast<const uint4*>(Cs + r * LDC + cch * 8);
    }
}

struct WgradBf16Args {
    const uint16_t* x;    // NHWC [B, Hi, Wi, Cin]
    const uint16_t* dy;   // NHWC [B, Ho, Wo, Cout]
    float* out;           // [splits][Cout][K] fp32 partial slabs (or dW itself when there is one split)
    int Hi, Wi, Cin, Ho, Wo, Cout, KW, stride, pad, K, P;
    int n_ptiles, tiles_per_split, co_tiles;
};

// Four pixels x 8 channels (four 16-byte rows) -> 8 channels x 4 pixels (eight 8-byte rows).
__device__ __forceinline__ void transpose4x8(const uint4 (&v)[4], uint2 (&o)[8]) {
    const uint32_t a[4][4] = {{v[0].x, v[0].y, v[0].z, v[0].w}, {v[1].x, v[1].y, v[1].z, v[1].w},
                              {v[2].x, v[2].y, v[2].z, v[2].w}, {v[3].x, v[3].y, v[3].z, v[3].w}};
#pragma unroll
    for (int d = 0; d < 4; d++) {
        o[2 * d].x = (a[0][d] & 0xFFFFu) | (a[1][d] << 16);
        o[2 * d].y = (a[2][d] & 0xFFFFu) | (a[3][d] << 16);
        o[2 * d + 1].x = (a[0][d] >> 16) | (a[1][d] & 0xFFFF0000u);
        o[2 * d + 1].y = (a[2][d] >> 16) | (a[3][d] & 0xFFFF0000u);
    }
}

// wgrad: block tile W_BK k columns x BCO output channels over the pixel tiles [t0, t1) of its split, 4 waves of 64 x BCO / 2.
// MFMA operands: A = x_patch^T (row = k column, reduction = pixel), B = dy (reduction = pixel, column = output channel), so a
// lane's accumulator holds 4 consecutive k columns of one dW row: one 16-byte store.  LDS holds both operands [row][pixel].
// Staging: threads 0..127 load the x tile (chunk c = 8 k columns of one tap, pixels 4g .. 4g + 3), threads 128..255 the dy tile
// (chunk c = 8 output channels; BCO = 64 leaves half of them idle); the next tile's loads are in flight under the MFMAs.
template <int BCO>
__global__ __launch_bounds__(G_THREADS, 2) void wgrad_bf16_kernel(WgradBf16Args p) {
    constexpr int NT = BCO / 32;   // 16-wide co tiles per wave
    __shared__ __attribute__((aligned(16))) uint16_t Xs[W_BK * W_LDP];
    __shared__ __attribute__((aligned(16))) uint16_t Ds[BCO * W_LDP];
    const int co_tile = blockIdx.x % p.co_tiles, k_tile = blockIdx.x / p.co_tiles, split = blockIdx.y;
    const int co0 = co_tile * BCO, k0 = k_tile * W_BK;
    const int t0 = split * p.tiles_per_split;
    const int t1 = min(t0 + p.tiles_per_split, p.n_ptiles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    const bool is_x = tid < 128;
    const int c = tid & 15, g = (tid >> 4) & 7;
    // x chunk: tap and channel offset of k columns k0 + 8c .. + 8 (zeros beyond K); dy chunk: channels co0 + 8c .. + 8
    const int q = (k0 >> 3) + c;
    const bool active = is_x ? q * 8 < p.K : c < BCO / 8;
    const int coff = (q % (p.Cin / 8)) * 8, kx = (q / (p.Cin / 8)) % p.KW, ky = q / ((p.Cin / 8) * p.KW);
    uint16_t* dst = (is_x ? Xs + (c * 8) * W_LDP : Ds + (c * 8) * W_LDP) + g * 4;

    // coordinates of pixel m = t * W_BP + 4g (the first of the thread's four), advanced by W_BP per tile
    int m = t0 * W_BP + 4 * g;
    int ox = m % p.Wo, oy = (m / p.Wo) % p.Ho, b = m / (p.Wo * p.Ho);
    uint4 r[4];
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    auto load = [&]() {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            r[u] = zero;
            int x_ = ox + u, y_ = oy, b_ = b;
            while (x_ >= p.Wo) { x_ -= p.Wo; if (++y_ == p.Ho) { y_ = 0; ++b_; } }
            if (!active || m + u >= p.P) continue;
            if (is_x) {
                const int iy = y_ * p.stride - p.pad + ky, ix = x_ * p.stride - p.pad + kx;
                if ((unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi)
                    r[u] = *reinterpret_cast<const uint4*>(p.x + (((long long)b_ * p.Hi + iy) * p.Wi + ix) * p.Cin + coff);
            } else {
                r[u] = *reinterpret_cast<const uint4*>(p.dy + (long long)(m + u) * p.Cout + co0 + c * 8);
            }
        }
    };
    auto advance = [&]() {
        m += W_BP;
        ox += W_BP;
        while (ox >= p.Wo) { ox -= p.Wo; if (++oy == p.Ho) { oy = 0; ++b; } }
    };

    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fk = (lane >> 4) * 8;
    const uint16_t* a_frag = Xs + (wr * 64 + frow) * W_LDP + fk;
    const uint16_t* b_frag = Ds + (wc * (BCO / 2) + frow) * W_LDP + fk;
    if (t0 < t1) load();
    for (int t = t0; t < t1; t++) {
        {   // registers -> LDS, transposed: row = k column / output channel, 4 consecutive pixels per 8-byte write
            uint2 o[8];
            transpose4x8(r, o);
            if (is_x || c < BCO / 8) {
#pragma unroll
                for (int e = 0; e < 8; e++) *reinterpret_cast<uint2*>(dst + e * W_LDP) = o[e];
            }
        }
        __syncthreads();
        if (t + 1 < t1) {
            advance();
            load();
        }
        bf16x8 af[4], bfr[NT];
#pragma unroll
        for (int i = 0; i < 4; i++) af[i] = *reinterpret_cast<const bf16x8*>(a_frag + i * 16 * W_LDP);
#pragma unroll
        for (int j = 0; j < NT; j++) bfr[j] = *reinterpret_cast<const bf16x8*>(b_frag + j * 16 * W_LDP);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    // D[i = k column][j = co]: column = lane & 15, rows 4 (lane >> 4) .. + 3 -> 4 consecutive k columns of dW row co
    float* o = p.out + (long long)split * p.Cout * p.K;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int kcol = k0 + wr * 64 + i * 16 + 4 * (lane >> 4);
        if (kcol >= p.K) continue;   // K is a multiple of 8: a group of 4 is all in or all out
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int co = co0 + wc * (BCO / 2) + j * 16 + (lane & 15);
            *reinterpret_cast<float4*>(o + (long long)co * p.K + kcol) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
    }
}

template <int BN, int MODE>
int launch_bf16(const ConvBf16Args& a, hipStream_t s) {
    const long long grid = 8ll * ((a.m_tiles + 7) / 8) * a.n_tiles;
    if (grid > 0x7FFFFFFFll) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
    hipLaunchKernelGGL((conv_bf16_kernel<BN, MODE>), dim3((unsigned)grid), dim3(G_THREADS), 0, s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

struct BF16 {
    typedef uint16_t T;
    typedef ConvBf16Args Args;
    typedef WgradBf16Args WgradArgs;
    static constexpr int BK = G_BK;
    static constexpr bool POINTWISE = true;   // a 1x1 / stride-1 pass reads its rows directly: no k table
    static size_t head_bytes(int) { return ZERO_BYTES; }   // the zero page

    static int launch_gemm(ConvBf16Args& a, void* head, int mode, hipStream_t s) {
        a.zeros = static_cast<const uint16_t*>(head);
        a.m_tiles = (int)(((long long)a.M + G_BM - 1) / G_BM);
        const bool wide = a.Cout % 128 == 0;
        a.n_tiles = a.Cout / (wide ? 128 : 64);
        if (mode == POINTWISE) return wide ? launch_bf16<128, POINTWISE>(a, s) : launch_bf16<64, POINTWISE>(a, s);
        if (mode == DGRAD_S2) return wide ? launch_bf16<128, DGRAD_S2>(a, s) : launch_bf16<64, DGRAD_S2>(a, s);
        return wide ? launch_bf16<128, GATHER>(a, s) : launch_bf16<64, GATHER>(a, s);
    }

    static WgradTile wgrad_tile(const salve_conv_desc_t* d) { return {d->Cout % 128 == 0 ? 128 : 64, W_BK, W_MIN_TILES}; }
    static void launch_wgrad(const WgradBf16Args& a, const WgradTile& t, dim3 grid, hipStream_t s) {
        if (t.bco == 128) hipLaunchKernelGGL(wgrad_bf16_kernel<128>, grid, dim3(G_THREADS), 0, s, a);
        else hipLaunchKernelGGL(wgrad_bf16_kernel<64>, grid, dim3(G_THREADS), 0, s, a);
    }
};

}  // namespace

extern "C" {

size_t salve_conv_bf16_workspace_bytes(const salve_conv_desc_t* d, int32_t pass) {
    return conv_workspace_bytes<BF16>("salve_conv_bf16_workspace_bytes: null descriptor", d, pass);
}

int salve_conv_bf16_forward(const salve_conv_desc_t* d, const uint16_t* x, const uint16_t* w, uint16_t* y, void* ws, size_t ws_bytes,
                            void* stream) {
    return conv_forward<BF16>("salve_conv_bf16_forward: null descriptor", d, x, w, y, ws, ws_bytes, stream);
}

int salve_conv_bf16_backward_data(const salve_conv_desc_t* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx, void* ws, size_t ws_bytes,
                                  void* stream) {
    return conv_backward_data<BF16>("salve_conv_bf16_backward_data: null descriptor", d, dy, w, dx, ws, ws_bytes, stream);
}

int salve_conv_bf16_backward_weight(const salve_conv_desc_t* d, const uint16_t* x, const uint16_t* dy, float* dw, void* ws, size_t ws_bytes,
                                    void* stream) {
    return conv_backward_weight<BF16>("salve_conv_bf16_backward_weight: null descriptor", d, x, dy, dw, ws, ws_bytes, stream);
}

}  // extern "C"
