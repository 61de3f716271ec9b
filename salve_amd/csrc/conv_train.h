// conv_train.h -- what the fp32 and the bf16 training convolutions (conv_train_f32.hip, conv_train_bf16.hip) share: the shape
// contract, the k table, the weight repacking kernels, the wgrad split and combine, the workspace layout and the four host drivers
// behind the salve_conv_{f32,bf16}_* entries.  Included by both translation units; everything lives in an anonymous namespace.
//
// A translation unit supplies its compute kernels and a precision policy P:
//   T, Args, WgradArgs       element type (float / uint16_t bf16 bits), the kernels' argument structs
//   BK                       K granule of the forward / dgrad kernel: K is padded to a multiple of it
//   POINTWISE                a 1x1 / stride-1 pass takes a pointwise kernel and builds no k table
//   head_bytes(n_out)        bytes of zeros at the head of the workspace (a zero bias / the zero page)
//   launch_gemm(a, head, mode, stream), wgrad_tile(d), launch_wgrad(a, tile, grid, stream)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int W_BP = 32;            // pixels per staged wgrad tile (the MFMA reduction)
constexpr int W_TARGET_WG = 1024;   // workgroups a wgrad launch aims at (4 per CU); fixed, so the split is a function of the shape

constexpr int32_t KTAB_PAD = INT32_MIN;   // a padding entry of the k table: negative, gathers zeros

enum GemmMode { GATHER = 0, POINTWISE = 1, DGRAD_S2 = 2 };

// One table entry per 8 consecutive k of a [rows][KH][KW][C] weight row: tap (ky, kx) | channel offset << 16.  Entries at and
// beyond n_valid pad K to a multiple of the K granule (the stems): they are negative, which the kernels answer with zeros without
// reading the image.  (A far tap is no padding: dy = -128 lies INSIDE an image of 129 rows or more, and 0 * inf is NaN.)
__global__ __launch_bounds__(256) void ktab_kernel(int32_t* __restrict__ tab, int n_valid, int n_total, int C, int KW) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_total) return;
    if (q >= n_valid) { tab[q] = KTAB_PAD; return; }
    const int c8 = q % (C / 8), kx = (q / (C / 8)) % KW, ky = q / ((C / 8) * KW);
    tab[q] = ky | (kx << 8) | ((c8 * 8) << 16);
}

// [Cout][K] -> [Cout][Kp] (columns K..Kp-1 zero): the stems' padded weight rows.
template <typename T>
__global__ __launch_bounds__(256) void pad_rows_kernel(const T* __restrict__ w, T* __restrict__ out, int rows, int K, int Kp) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * Kp) return;
    const int k = (int)(idx % Kp);
    const long long r = idx / Kp;
    out[idx] = k < K ? w[r * K + k] : (T)0;
}

// w [Cout][KH][KW][Cin] -> out [Cin][KH][KW][Cout], taps rotated by 180 degrees when rot (stride-1 dgrad) or kept (stride-2 gather).
template <typename T>
__global__ __launch_bounds__(256) void transpose_weights_kernel(const T* __restrict__ w, T* __restrict__ out, int Cout, int KH, int KW, int Cin,
                                                                int rot) {
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

// The shapes of every convolution of ResNet-18/34/50/101/152 (v1.5) with an early-fusion stem; anything else is refused.  The
// one shape contract of both precisions.
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

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool usable(const void* a, const void* b, const void* c, const void* ws) { return a && b && c && ws && aligned16(a) && aligned16(b) && aligned16(c); }
unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }
char* ws_base(void* ws) { return reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255); }   // (every workspace size counts these 256 bytes)

struct WgradTile {
    int bco, bk, min_tiles;   // output channels and k columns per workgroup; staged pixel tiles per split at least
};

struct WgradSplit {
    int n_ptiles, tiles_per_split, splits, co_tiles, k_tiles;
};

// The pixel range of a wgrad is cut into `splits` runs of `tiles_per_split` tiles: a function of the shape only.
WgradSplit wgrad_split(const salve_conv_desc_t* d, const WgradTile& t) {
    const long long P = (long long)d->batch * d->Ho * d->Wo;
    const int K = d->KH * d->KW * d->Cin;
    WgradSplit w;
    w.n_ptiles = (int)((P + W_BP - 1) / W_BP);
    w.co_tiles = d->Cout / t.bco;
    w.k_tiles = (K + t.bk - 1) / t.bk;
    int want = (W_TARGET_WG + w.co_tiles * w.k_tiles - 1) / (w.co_tiles * w.k_tiles);
    const int most = (w.n_ptiles + t.min_tiles - 1) / t.min_tiles;
    if (want > most) want = most;
    if (want < 1) want = 1;
    w.tiles_per_split = (w.n_ptiles + want - 1) / want;
    w.splits = (w.n_ptiles + w.tiles_per_split - 1) / w.tiles_per_split;
    return w;
}

size_t wgrad_ws(const salve_conv_desc_t* d, const WgradSplit& w) {
    const int K = d->KH * d->KW * d->Cin;
    return (w.splits > 1 ? align256((size_t)w.splits * d->Cout * K * sizeof(float)) : 0) + 256;
}

// Workspace sections of the forward / dgrad passes: head (zeros) | k table | packed weights.
struct GemmWs {
    size_t ktab, w, total;
    int Kp;
};

template <typename P>
GemmWs gemm_ws(int n_out, int K, bool packed_w) {
    GemmWs g;
    g.Kp = (K + P::BK - 1) / P::BK * P::BK;
    g.ktab = align256(P::head_bytes(n_out));
    g.w = g.ktab + align256((size_t)(g.Kp / 8) * sizeof(int32_t));
    g.total = g.w + (packed_w ? align256((size_t)n_out * g.Kp * sizeof(typename P::T)) : 0) + 256;
    return g;
}

template <typename P>
size_t conv_workspace_bytes(const char* who, const salve_conv_desc_t* d, int32_t pass) {
    if (check_desc(d, who) != SALVE_OK) return 0;
    const int K = d->KH * d->KW * d->Cin;
    if (pass == SALVE_CONV_FWD) return gemm_ws<P>(d->Cout, K, K % P::BK != 0).total;
    if (pass == SALVE_CONV_DGRAD) {
        if (d->KH == 7) { salve_fail("salve_conv_*: the stem's dgrad is not supported (the network input needs no gradient)"); return 0; }
        return gemm_ws<P>(d->Cin, d->KH * d->KW * d->Cout, true).total;
    }
    if (pass == SALVE_CONV_WGRAD) return wgrad_ws(d, wgrad_split(d, P::wgrad_tile(d)));
    salve_fail("salve_conv_*_workspace_bytes: pass must be SALVE_CONV_FWD, _DGRAD or _WGRAD");
    return 0;
}

template <typename P, typename T = typename P::T>
int conv_forward(const char* who, const salve_conv_desc_t* d, const T* x, const T* w, T* y, void* ws, size_t ws_bytes, void* stream) {
    int st = check_desc(d, who);
    if (st != SALVE_OK) return st;
    if (!usable(x, w, y, ws)) { salve_fail("salve_conv_*_forward: null or not 16-byte aligned pointer"); return SALVE_ERR_BAD_ARG; }
    const int K = d->KH * d->KW * d->Cin;
    const GemmWs g = gemm_ws<P>(d->Cout, K, K % P::BK != 0);
    const int Kp = g.Kp;   // K, padded with zero weight columns (the stems)
    if (ws_bytes < g.total) { salve_fail("salve_conv_*_forward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = ws_base(ws);
    int32_t* ktab = reinterpret_cast<int32_t*>(base + g.ktab);
    SALVE_HIP_CHECK(hipMemsetAsync(base, 0, P::head_bytes(d->Cout), s));
    const bool pointwise = P::POINTWISE && d->KH == 1 && d->stride == 1;
    if (!pointwise) {
        hipLaunchKernelGGL(ktab_kernel, dim3(blocks256(Kp / 8)), dim3(256), 0, s, ktab, K / 8, Kp / 8, d->Cin, d->KW);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    const T* wk = w;
    if (K != Kp) {
        T* wp = reinterpret_cast<T*>(base + g.w);
        hipLaunchKernelGGL(pad_rows_kernel<T>, dim3(blocks256((long long)d->Cout * Kp)), dim3(256), 0, s, w, wp, d->Cout, K, Kp);
        SALVE_HIP_CHECK(hipGetLastError());
        wk = wp;
    }
    typename P::Args a = {};
    a.in = x; a.w = wk; a.out = y; a.ktab = ktab;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
    a.stride = d->stride; a.pad = d->pad; a.K = Kp; a.M = (int)((long long)d->batch * d->Ho * d->Wo);
    return P::launch_gemm(a, base, pointwise ? POINTWISE : GATHER, s);
}

// dx as a convolution over dy: the weights transposed on the device, stride 1 rotated by 180 degrees with pad' = KH - 1 - pad,
// stride 2 through the DGRAD_S2 gather with the forward taps and padding.
template <typename P, typename T = typename P::T>
int conv_backward_data(const char* who, const salve_conv_desc_t* d, const T* dy, const T* w, T* dx, void* ws, size_t ws_bytes, void* stream) {
    int st = check_desc(d, who);
    if (st != SALVE_OK) return st;
    if (d->KH == 7) { salve_fail("salve_conv_*_backward_data: the stem's dgrad is not supported (the network input needs no gradient)"); return SALVE_ERR_UNSUPPORTED; }
    if (!usable(dy, w, dx, ws)) { salve_fail("salve_conv_*_backward_data: null or not 16-byte aligned pointer"); return SALVE_ERR_BAD_ARG; }
    const int K = d->KH * d->KW * d->Cout;   // a multiple of 64: Cout is
    const GemmWs g = gemm_ws<P>(d->Cin, K, true);
    if (ws_bytes < g.total) { salve_fail("salve_conv_*_backward_data: workspace too small"); return SALVE_ERR_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* base = ws_base(ws);
    int32_t* ktab = reinterpret_cast<int32_t*>(base + g.ktab);
    T* wt = reinterpret_cast<T*>(base + g.w);
    const bool s2 = d->stride == 2, pointwise = P::POINTWISE && d->KH == 1 && !s2;
    SALVE_HIP_CHECK(hipMemsetAsync(base, 0, P::head_bytes(d->Cin), s));
    if (!pointwise) {
        hipLaunchKernelGGL(ktab_kernel, dim3(blocks256(K / 8)), dim3(256), 0, s, ktab, K / 8, K / 8, d->Cout, d->KW);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(transpose_weights_kernel<T>, dim3(blocks256((long long)K * d->Cin)), dim3(256), 0, s, w, wt, d->Cout, d->KH, d->KW, d->Cin,
                       s2 ? 0 : 1);
    SALVE_HIP_CHECK(hipGetLastError());
    typename P::Args a = {};
    a.in = dy; a.w = wt; a.out = dx; a.ktab = ktab;
    a.Hi = d->Ho; a.Wi = d->Wo; a.Cin = d->Cout; a.Ho = d->Hi; a.Wo = d->Wi; a.Cout = d->Cin;
    a.stride = 1; a.pad = s2 ? d->pad : d->KH - 1 - d->pad;
    a.K = K; a.M = (int)((long long)d->batch * d->Hi * d->Wi);
    return P::launch_gemm(a, base, s2 ? DGRAD_S2 : (pointwise ? POINTWISE : GATHER), s);
}

template <typename P, typename T = typename P::T>
int conv_backward_weight(const char* who, const salve_conv_desc_t* d, const T* x, const T* dy, float* dw, void* ws, size_t ws_bytes, void* stream) {
    int st = check_desc(d, who);
    if (st != SALVE_OK) return st;
    if (!usable(x, dy, dw, ws)) { salve_fail("salve_conv_*_backward_weight: null or not 16-byte aligned pointer"); return SALVE_ERR_BAD_ARG; }
    const WgradTile tile = P::wgrad_tile(d);
    const WgradSplit sp = wgrad_split(d, tile);
    if (ws_bytes < wgrad_ws(d, sp)) { salve_fail("salve_conv_*_backward_weight: workspace too small"); return SALVE_ERR_WORKSPACE; }
    const int K = d->KH * d->KW * d->Cin;
    hipStream_t s = (hipStream_t)stream;
    float* slabs = reinterpret_cast<float*>(ws_base(ws));
    typename P::WgradArgs a;
    a.x = x; a.dy = dy; a.out = sp.splits > 1 ? slabs : dw;
    a.Hi = d->Hi; a.Wi = d->Wi; a.Cin = d->Cin; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout; a.KW = d->KW;
    a.stride = d->stride; a.pad = d->pad; a.K = K; a.P = (int)((long long)d->batch * d->Ho * d->Wo);
    a.n_ptiles = sp.n_ptiles; a.tiles_per_split = sp.tiles_per_split; a.co_tiles = sp.co_tiles;
    P::launch_wgrad(a, tile, dim3((unsigned)(sp.co_tiles * sp.k_tiles), (unsigned)sp.splits), s);
    SALVE_HIP_CHECK(hipGetLastError());
    if (sp.splits > 1) {
        const long long n4 = (long long)d->Cout * K / 4;
        hipLaunchKernelGGL(wgrad_combine_kernel, dim3(blocks256(n4)), dim3(256), 0, s, slabs, dw, n4, sp.splits);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    return SALVE_OK;
}

}  // namespace
