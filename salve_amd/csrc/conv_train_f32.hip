// conv_train_f32.hip -- per-convolution fp32 entries for training the verifier on gfx950 (MI355X): forward, backward-data
// (dgrad) and backward-weight (wgrad) of one convolution of the early-fusion ResNet, in the reference's precision
// (salve/configs/*.yaml train in fp32; scripts/train.py).  The autograd plumbing (BatchNorm, ReLU, pooling, loss, Adam) is
// torch's (salve_amd/models/trainable.py); every convolution of a training step runs here.
//
//   forward  conv_f32_kernel (conv_f32.h, the fp32 engine's implicit GEMM) with a zero bias, no residual, no ReLU.  The k table
//            is built on the device from the descriptor; the stems' K = 49 * Cin (not a multiple of 32) is padded with zero
//            weight columns whose table entries are negative: they gather zeros and read no pixel.
//   dgrad    stride 1: conv_f32_kernel over dy with the weights transposed ([Cin][KH][KW][Cout]) and rotated by 180 degrees,
//            pad' = KH - 1 - pad.  Stride 2: conv_f32_kernel<.., DGRAD_S2> -- the tap (ky, kx) of dx pixel (iy, ix) reads
//            dy[(iy + pad - ky) / 2][(ix + pad - kx) / 2] when both divisions are exact, zero otherwise (3/4 of its K terms are zero
//            for a 3 x 3 / 2 convolution: the gather does not skip them).  The stem's dgrad is refused (SALVE_ERR_UNSUPPORTED):
//            the network input needs no gradient.
//   wgrad    wgrad_f32_kernel: dW[Cout, KH*KW*Cin] = sum over the batch * Ho * Wo pixels of dy (x) x_patch, v_mfma_f32_32x32x2_f32
//            with the pixels as the reduction.  The pixel range is split over workgroups into fp32 partial slabs that
//            wgrad_combine_kernel sums in split order: no float atomics, the same inputs give bit-identical dW.  The split count
//            depends on the shape only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"
#include "conv_f32.h"

namespace {

constexpr int W_BM = 64;     // output channels per wgrad workgroup
constexpr int W_BN = 128;    // k columns (tap, input channel) per wgrad workgroup: 4 waves of 32
constexpr int W_BP = 32;     // pixels per staged tile (the MFMA reduction)
constexpr int W_TARGET_WG = 1024;   // workgroups a wgrad launch aims at (4 per CU); fixed, so the split is a function of the shape
constexpr int W_MIN_TILES = 8;      // staged pixel tiles per split at least

constexpr int32_t KTAB_PAD = INT32_MIN;   // a padding entry of the k table: negative (conv_f32.h: gather8)

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// One table entry per 8 consecutive k of a [rows][KH][KW][C] weight row: tap (ky, kx) | channel offset << 16.  Entries at and
// beyond n_valid pad K to a multiple of 32 (the stems): they are negative, which gather8 answers with zeros without reading the
// image.  (A far tap is no padding: dy = -128 lies INSIDE an image of 129 rows or more, and 0 * inf is NaN.)
__global__ __launch_bounds__(256) void ktab_kernel(int32_t* __restrict__ tab, int n_valid, int n_total, int C, int KW) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_total) return;
    if (q >= n_valid) { tab[q] = KTAB_PAD; return; }
    const int c8 = q % (C / 8), kx = (q / (C / 8)) % KW, ky = q / ((C / 8) * KW);
    tab[q] = ky | (kx << 8) | ((c8 * 8) << 16);
}

// [Cout][K] -> [Cout][Kp] (columns K..Kp-1 zero): the stems' padded weight rows.
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ w, float* __restrict__ out, int rows, int K, int Kp) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * Kp) return;
    const int k = (int)(idx % Kp);
    const long long r = idx / Kp;
    out[idx] = k < K ? w[r * K + k] : 0.f;
}

// w [Cout][KH][KW][Cin] -> out [Cin][KH][KW][Cout], taps rotated by 180 degrees when rot (stride-1 dgrad) or kept (stride-2 gather).
__global__ __launch_bounds__(256) void transpose_weights_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int KH, int KW,
                                                                int Cin, int rot) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)Cout * KH * KW * Cin) return;
    const int co = (int)(idx % Cout);
    long long t = idx / Cout;
    const int kx = (int)(t % KW);
    t /= KW;
    const int ky = (int)(t % KH);
    const int ci = (int)(t / KH);
    const int sy = rot ? KH - 1 - ky : ky, sx = rot ? KW - 1 - kx : kx;
    out[idx] = w[(((long long)co * KH + sy) * KW + sx) * Cin + ci];
}

struct WgradArgs {
    const float* x;    // NHWC [B, Hi, Wi, Cin]
    const float* dy;   // NHWC [B, Ho, Wo, Cout]
    float* out;        // [splits][Cout][K] partial slabs (or dW itself when there is one split)
    int Hi, Wi, Cin, Ho, Wo, Cout, KW, stride, pad, K, P;
    int n_ptiles, tiles_per_split, co_tiles;
};

// wgrad: block tile 64 output channels x 128 k columns, 4 waves of 64 x 32, over the pixel tiles [t0, t1) of its split.
// MFMA operands (conv_f32_kernel's maps): A = dy^T (i = output channel, k = pixel), B = x_patch (k = pixel, j = k column); a lane
// owns one k column, so the stores of a register are 32 consecutive columns of one dW row.  LDS holds both operands transposed,
// [row][pixel], so that the fragment reads are conv_f32_kernel's 16-byte reads along the reduction.
__global__ __launch_bounds__(F_THREADS, 2) void wgrad_f32_kernel(WgradArgs p) {
    __shared__ __attribute__((aligned(16))) float As[W_BM * F_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[W_BN * F_LDK];
    const int co_tile = blockIdx.x % p.co_tiles, k_tile = blockIdx.x / p.co_tiles, split = blockIdx.y;
    const int co0 = co_tile * W_BM, k0 = k_tile * W_BN;
    const int t0 = split * p.tiles_per_split;
    const int t1 = min(t0 + p.tiles_per_split, p.n_ptiles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- staging: pixel sp of the tile; dy channels co0 + 8 seg .. + 8; k columns k0 + 16 seg .. + 16 (two chunks of 8 channels)
    const int sp = tid & 31, seg = tid >> 5;
    int cky[2], ckx[2], ccoff[2];
    bool cvalid[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int q = (k0 >> 3) + seg * 2 + h;
        cvalid[h] = q * 8 < p.K;
        ccoff[h] = (q % (p.Cin / 8)) * 8;
        ckx[h] = (q / (p.Cin / 8)) % p.KW;
        cky[h] = q / ((p.Cin / 8) * p.KW);
    }
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rd0, rd1, rx0, rx1, rx2, rx3;
#define WG_LOAD(T)                                                                                                             \
    {                                                                                                                          \
        const int m_ = (T) * W_BP + sp;                                                                                        \
        rd0 = rd1 = rx0 = rx1 = rx2 = rx3 = zero4;                                                                             \
        if (m_ < p.P) {                                                                                                        \
            const int ox_ = m_ % p.Wo, t_ = m_ / p.Wo, oy_ = t_ % p.Ho, b_ = t_ / p.Ho;                                         \
            const float4* d_ = reinterpret_cast<const float4*>(p.dy + (long long)m_ * p.Cout + co0 + seg * 8);                 \
            rd0 = d_[0];                                                                                                       \
            rd1 = d_[1];                                                                                                       \
            const int iy_ = oy_ * p.stride - p.pad, ix_ = ox_ * p.stride - p.pad;                                             \
            if (cvalid[0] && (unsigned)(iy_ + cky[0]) < (unsigned)p.Hi && (unsigned)(ix_ + ckx[0]) < (unsigned)p.Wi) {          \
                const float4* s_ = reinterpret_cast<const float4*>(                                                           \
                    p.x + (((long long)b_ * p.Hi + iy_ + cky[0]) * p.Wi + ix_ + ckx[0]) * p.Cin + ccoff[0]);                   \
                rx0 = s_[0];                                                                                                   \
                rx1 = s_[1];                                                                                                   \
            }                                                                                                                  \
            if (cvalid[1] && (unsigned)(iy_ + cky[1]) < (unsigned)p.Hi && (unsigned)(ix_ + ckx[1]) < (unsigned)p.Wi) {          \
                const float4* s_ = reinterpret_cast<const float4*>(                                                           \
                    p.x + (((long long)b_ * p.Hi + iy_ + cky[1]) * p.Wi + ix_ + ckx[1]) * p.Cin + ccoff[1]);                   \
                rx2 = s_[0];                                                                                                   \
                rx3 = s_[1];                                                                                                   \
            }                                                                                                                  \
        }                                                                                                                      \
    }

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;

    const int frow = lane & 31, fk = (lane >> 5) * 16;
    const float* a_frag = As + frow * F_LDK + fk;
    const float* b_frag = Bs + (wave * 32 + frow) * F_LDK + fk;
    if (t0 < t1) WG_LOAD(t0);
    for (int t = t0; t < t1; t++) {
        {   // registers -> LDS, transposed: row = channel / k column, column = pixel
            const float d[8] = {rd0.x, rd0.y, rd0.z, rd0.w, rd1.x, rd1.y, rd1.z, rd1.w};
            const float xv[16] = {rx0.x, rx0.y, rx0.z, rx0.w, rx1.x, rx1.y, rx1.z, rx1.w,
                                  rx2.x, rx2.y, rx2.z, rx2.w, rx3.x, rx3.y, rx3.z, rx3.w};
#pragma unroll
            for (int e = 0; e < 8; e++) As[(seg * 8 + e) * F_LDK + sp] = d[e];
#pragma unroll
            for (int e = 0; e < 16; e++) Bs[(seg * 16 + e) * F_LDK + sp] = xv[e];
        }
        __syncthreads();
        if (t + 1 < t1) WG_LOAD(t + 1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4 af[2], bf;
#pragma unroll
            for (int i = 0; i < 2; i++) af[i] = *reinterpret_cast<const float4*>(a_frag + i * 32 * F_LDK + 4 * q);
            bf = *reinterpret_cast<const float4*>(b_frag + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < 2; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[s], acc[i], 0, 0, 0);
        }
        __syncthreads();
    }
#undef WG_LOAD

    const int kcol = k0 + wave * 32 + (lane & 31);
    if (kcol >= p.K) return;
    float* o = p.out + (long long)split * p.Cout * p.K + kcol;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(long long)co * p.K] = acc[i][r];
        }
}

// dW = slab 0 + slab 1 + ... in split order (one fixed fp32 summation order per element).
__global__ __launch_bounds__(256) void wgrad_combine_kernel(const float* __restrict__ slabs, float* __restrict__ dw, long long n4, int splits) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n4) return;
    const float4* s = reinterpret_cast<const float4*>(slabs) + idx;
    float4 a = s[0];
    for (int k = 1; k < splits; k++) {
        const float4 v = s[(long long)k * n4];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    reinterpret_cast<float4*>(dw)[idx] = a;
}

// The shapes of every convolution of ResNet-18/34/50/101/152 (v1.5) with an early-fusion stem; anything else is refused.
int check_desc(const salve_conv_desc_t* d, const char* who) {
    if (!d) { salve_fail(who); return SALVE_ERR_BAD_ARG; }
    const bool k1 = d->KH == 1 && d->KW == 1 && d->pad == 0 && (d->stride == 1 || d->stride == 2);
    const bool k3 = d->KH == 3 && d->KW == 3 && d->pad == 1 && (d->stride == 1 || d->stride == 2);
    const bool k7 = d->KH == 7 && d->KW == 7 && d->pad == 3 && d->stride == 2;
    if (!k1 && !k3 && !k7) { salve_fail("conv: only 1x1 (pad 0), 3x3 (pad 1) with stride 1 or 2 and the 7x7 / 2 / pad 3 stem are supported"); return SALVE_ERR_BAD_ARG; }
    if (k7 ? (d->Cin != 8 && d->Cin != 16 && d->Cin != 24) : (d->Cin < 64 || d->Cin > 2048 || d->Cin % 64 != 0)) {
        salve_fail("conv: Cin must be 64..2048 in steps of 64 (the 7x7 stem: 8, 16 or 24, the zero-padded 6 / 12 / 18 channels)");
        return SALVE_ERR_BAD_ARG;
    }
    if (d->Cout < 64 || d->Cout > 2048 || d->Cout % 64 != 0) { salve_fail("conv: Cout must be 64..2048 in steps of 64"); return SALVE_ERR_BAD_ARG; }
    if (d->batch <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Hi > 4096 || d->Wi > 4096) { salve_fail("conv: bad batch or input size"); return SALVE_ERR_BAD_ARG; }
    if (d->Ho != (d->Hi + 2 * d->pad - d->KH) / d->stride + 1 || d->Wo != (d->Wi + 2 * d->pad - d->KW) / d->stride + 1 || d->Ho <= 0 || d->Wo <= 0) {
        salve_fail("conv: Ho / Wo do not match the input size, kernel, stride and padding");
        return SALVE_ERR_BAD_ARG;
    }
    const long long px = (long long)d->batch * (d->Hi > d->Ho ? (long long)d->Hi * d->Wi : (long long)d->Ho * d->Wo);
    if (px > 0x7FFFFFFFll - 1024) { salve_fail("conv: batch too large"); return SALVE_ERR_BAD_ARG; }
    return SALVE_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

void wgrad_split(const salve_conv_desc_t* d, int& n_ptiles, int& tiles_per_split, int& splits, int& co_tiles, int& k_tiles) {
    const long long P = (long long)d->batch * d->Ho * d->Wo;
    const int K = d->KH * d->KW * d->Cin;
    n_ptiles = (int)((P + W_BP - 1) / W_BP);
    co_tiles = d->Cout / W_BM;
    k_tiles = (K + W_BN - 1) / W_BN;
    int want = (W_TARGET_WG + co_tiles * k_tiles - 1) / (co_tiles * k_tiles);
    const int most = (n_ptiles + W_MIN_TILES - 1) / W_MIN_TILES;
    if (want > most) want = most;
    if (want < 1) want = 1;
    tiles_per_split = (n_ptiles + want - 1) / want;
    splits = (n_ptiles + tiles_per_split - 1) / tiles_per_split;
}

// Workspace sections of the forward / dgrad passes: zero bias | k table | packed weights.
struct GemmWs {
    size_t bias, ktab, w, total;
};

GemmWs gemm_ws(int n_out, int K, bool packed_w) {
    const int Kp = (K + F_BK - 1) / F_BK * F_BK;
    GemmWs g;
    g.bias = 0;
    g.ktab = align256((size_t)n_out * sizeof(float));
    g.w = g.ktab + align256((size_t)(Kp / 8) * sizeof(int32_t));
    g.total = g.w + (packed_w ? align256((size_t)n_out * Kp * sizeof(float)) : 0) + 256;   // + 256: the caller's pointer is aligned here
    return g;
}

int launch_gemm(ConvF32Args& a, bool dgrad_s2, hipStream_t s) {
    const long long M = (long long)a.M;
    a.m_tiles = (int)((M + F_BM - 1) / F_BM);
    if (a.Cout % 128 == 0) {
        a.n_tiles = a.Cout / 128;
        return dgrad_s2 ? launch_conv<128, true>(a, s) : launch_conv<128>(a, s);
    }
    a.n_tiles = a.Cout / 64;
    return dgrad_s2 ? launch_conv<64, true>(a, s) : launch_conv<64>(a, s);
}

unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

size_t salve_conv_f32_workspace_bytes(const salve_conv_desc_t* d, int32_t pass) {
    if (check_desc(d, "salve_conv_f32_workspace_bytes: null descriptor") != SALVE_OK) return 0;
    const int K = d->KH * d->KW * d->Cin;
    if (pass == SALVE_CONV_FWD) return gemm_ws(d->Cout, K, K % F_BK != 0).total;
    if (pass == SALVE_CONV_DGRAD) {
        if (d->KH == 7) { salve_fail("salve_conv_f32: the stem's dgrad is not supported (the network input needs no gradient)"); return 0; }
        return gemm_ws(d->Cin, d->KH * d->KW * d->Cout, true).total;
    }
    if (pass == SALVE_CONV_WGRAD) {
        int n_ptiles, tps, splits, co_tiles, k_tiles;
        wgrad_split(d, n_ptiles, tps, splits, co_tiles, k_tiles);
        return (splits > 1 ? align256((size_t)splits * d->Cout * K * sizeof(float)) : 0) + 256;
    }
    salve_fail("salve_conv_f32_workspace_bytes: pass must be SALVE_CONV_FWD, _DGRAD or _WGRAD");
    return 0;
}

int salve_conv_f32_forward(const salve_conv_desc_t* d, const float* x, const float* w, float* y, void* ws, size_t ws_bytes, void* stream) {
    int st = check_desc(d, "salve_conv_f32_forward: null descriptor");
    if (st != SALVE_OK) return st;
    if (!x || !w || !y || !ws || !aligned16(x) || !aligned16(w) || !aligned16(y)) {
        salve_fail("salve_conv_f32_forward: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    const int K = d->KH * d->KW * d->Cin, Kp = (K + F_BK - 1) / F_BK * F_BK;
    const GemmWs g = gemm_ws(d->Cout, K, K != Kp);
    if (ws_bytes < g.total) { salve_fail("salve_conv_f32_forward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* bias = reinterpret_cast<float*>(base + g.bias);
    int32_t* ktab = reinterpret_cast<int32_t*>(base + g.ktab);
    SALVE_HIP_CHECK(hipMemsetAsync(bias, 0, (size_t)d->Cout * sizeof(float), s));
    hipLaunchKernelGGL(ktab_kernel, dim3(blocks256(Kp / 8)), dim3(256), 0, s, ktab, K / 8, Kp / 8, d->Cin, d->KW);
    SALVE_HIP_CHECK(hipGetLastError());
    const float* wk = w;
    if (K != Kp) {
        float* wp = reinterpret_cast<float*>(base + g.w);
        hipLaunchKernelGGL(pad_rows_kernel, dim3(blocks256((long long)d->Cout * Kp)), dim3(256), 0, s, w, wp, d->Cout, K, Kp);
        SALVE_HIP_CHECK(hipGetLastError());
        wk = wp;
    }
    ConvF32Args a = {};
    a.in = x; a.w = wk; a.bias = bias; a.res = nullptr; a.out = y; a.ktab = ktab; a.in2 = nullptr;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
    a.stride = d->stride; a.pad = d->pad; a.K = Kp; a.M = (int)((long long)d->batch * d->Ho * d->Wo); a.relu = 0;
    a.nkt1 = Kp / F_BK;
    return launch_gemm(a, false, s);
}

int salve_conv_f32_backward_data(const salve_conv_desc_t* d, const float* dy, const float* w, float* dx, void* ws, size_t ws_bytes,
                                 void* stream) {
    int st = check_desc(d, "salve_conv_f32_backward_data: null descriptor");
    if (st != SALVE_OK) return st;
    if (d->KH == 7) { salve_fail("salve_conv_f32_backward_data: the stem's dgrad is not supported (the network input needs no gradient)"); return SALVE_ERR_UNSUPPORTED; }
    if (!dy || !w || !dx || !ws || !aligned16(dy) || !aligned16(w) || !aligned16(dx)) {
        salve_fail("salve_conv_f32_backward_data: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    const int K = d->KH * d->KW * d->Cout;   // a multiple of 64: Cout is
    const GemmWs g = gemm_ws(d->Cin, K, true);
    if (ws_bytes < g.total) { salve_fail("salve_conv_f32_backward_data: workspace too small"); return SALVE_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* bias = reinterpret_cast<float*>(base + g.bias);
    int32_t* ktab = reinterpret_cast<int32_t*>(base + g.ktab);
    float* wt = reinterpret_cast<float*>(base + g.w);
    const bool s2 = d->stride == 2;
    SALVE_HIP_CHECK(hipMemsetAsync(bias, 0, (size_t)d->Cin * sizeof(float), s));
    hipLaunchKernelGGL(ktab_kernel, dim3(blocks256(K / 8)), dim3(256), 0, s, ktab, K / 8, K / 8, d->Cout, d->KW);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(transpose_weights_kernel, dim3(blocks256((long long)K * d->Cin)), dim3(256), 0, s, w, wt, d->Cout,
                       d->KH, d->KW, d->Cin, s2 ? 0 : 1);
    SALVE_HIP_CHECK(hipGetLastError());
    ConvF32Args a = {};
    a.in = dy; a.w = wt; a.bias = bias; a.res = nullptr; a.out = dx; a.ktab = ktab; a.in2 = nullptr;
    a.Hi = d->Ho; a.Wi = d->Wo; a.Cin = d->Cout; a.Ho = d->Hi; a.Wo = d->Wi; a.Cout = d->Cin;
    a.stride = 1; a.pad = s2 ? d->pad : d->KH - 1 - d->pad;
    a.K = K; a.M = (int)((long long)d->batch * d->Hi * d->Wi); a.relu = 0;
    a.nkt1 = K / F_BK;
    return launch_gemm(a, s2, s);
}

int salve_conv_f32_backward_weight(const salve_conv_desc_t* d, const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes,
                                   void* stream) {
    int st = check_desc(d, "salve_conv_f32_backward_weight: null descriptor");
    if (st != SALVE_OK) return st;
    if (!x || !dy || !dw || !ws || !aligned16(x) || !aligned16(dy) || !aligned16(dw)) {
        salve_fail("salve_conv_f32_backward_weight: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (ws_bytes < salve_conv_f32_workspace_bytes(d, SALVE_CONV_WGRAD)) { salve_fail("salve_conv_f32_backward_weight: workspace too small"); return SALVE_ERR_WORKSPACE; }
    int n_ptiles, tps, splits, co_tiles, k_tiles;
    wgrad_split(d, n_ptiles, tps, splits, co_tiles, k_tiles);
    const int K = d->KH * d->KW * d->Cin;
    hipStream_t s = (hipStream_t)stream;
    float* slabs = reinterpret_cast<float*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    WgradArgs a;
    a.x = x; a.dy = dy; a.out = splits > 1 ? slabs : dw;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout; a.KW = d->KW;
    a.stride = d->stride; a.pad = d->pad; a.K = K; a.P = (int)((long long)d->batch * d->Ho * d->Wo);
    a.n_ptiles = n_ptiles; a.tiles_per_split = tps; a.co_tiles = co_tiles;
    hipLaunchKernelGGL(wgrad_f32_kernel, dim3((unsigned)(co_tiles * k_tiles), (unsigned)splits), dim3(F_THREADS), 0, s, a);
    SALVE_HIP_CHECK(hipGetLastError());
    if (splits > 1) {
        const long long n4 = (long long)d->Cout * K / 4;
        hipLaunchKernelGGL(wgrad_combine_kernel, dim3(blocks256(n4)), dim3(256), 0, s, slabs, dw, n4, splits);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    return SALVE_OK;
}

}  // extern "C"
