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
//
// This file holds the fp32 wgrad kernel and the fp32 precision policy.  The shape contract (check_desc), the k table, the weight
// repacking, the wgrad split and combine, the workspace layout and the host drivers of the four entries are conv_train.h's, shared
// with the bf16 entries (conv_train_bf16.hip).
#include "conv_f32.h"
#include "conv_train.h"

namespace {

constexpr int W_BM = 64;          // output channels per wgrad workgroup
constexpr int W_BN = 128;         // k columns (tap, input channel) per wgrad workgroup: 4 waves of 32
constexpr int W_MIN_TILES = 8;   // staged pixel tiles per split at least

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

struct F32 {
    typedef float T;
    typedef ConvF32Args Args;
    typedef ::WgradArgs WgradArgs;
    static constexpr int BK = F_BK;
    static constexpr bool POINTWISE = false;   // a 1x1 convolution gathers through the k table like any other
    static size_t head_bytes(int n_out) { return (size_t)n_out * sizeof(float); }   // the zero bias of conv_f32_kernel's epilogue

    static int launch_gemm(ConvF32Args& a, void* head, int mode, hipStream_t s) {
        a.bias = static_cast<const float*>(head);
        a.nkt1 = a.K / F_BK;
        a.m_tiles = (int)(((long long)a.M + F_BM - 1) / F_BM);
        const bool dgrad_s2 = mode == DGRAD_S2;
        if (a.Cout % 128 == 0) {
            a.n_tiles = a.Cout / 128;
            return dgrad_s2 ? launch_conv<128, true>(a, s) : launch_conv<128>(a, s);
        }
        a.n_tiles = a.Cout / 64;
        return dgrad_s2 ? launch_conv<64, true>(a, s) : launch_conv<64>(a, s);
    }

    static WgradTile wgrad_tile(const salve_conv_desc_t*) { return {W_BM, W_BN, W_MIN_TILES}; }
    static void launch_wgrad(const WgradArgs& a, const WgradTile&, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(wgrad_f32_kernel, grid, dim3(F_THREADS), 0, s, a);
    }
};

}  // namespace

extern "C" {

size_t salve_conv_f32_workspace_bytes(const salve_conv_desc_t* d, int32_t pass) {
    return conv_workspace_bytes<F32>("salve_conv_f32_workspace_bytes: null descriptor", d, pass);
}

int salve_conv_f32_forward(const salve_conv_desc_t* d, const float* x, const float* w, float* y, void* ws, size_t ws_bytes, void* stream) {
    return conv_forward<F32>("salve_conv_f32_forward: null descriptor", d, x, w, y, ws, ws_bytes, stream);
}

int salve_conv_f32_backward_data(const salve_conv_desc_t* d, const float* dy, const float* w, float* dx, void* ws, size_t ws_bytes,
                                 void* stream) {
    return conv_backward_data<F32>("salve_conv_f32_backward_data: null descriptor", d, dy, w, dx, ws, ws_bytes, stream);
}

int salve_conv_f32_backward_weight(const salve_conv_desc_t* d, const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes,
                                   void* stream) {
    return conv_backward_weight<F32>("salve_conv_f32_backward_weight: null descriptor", d, x, dy, dw, ws, ws_bytes, stream);
}

}  // extern "C"
