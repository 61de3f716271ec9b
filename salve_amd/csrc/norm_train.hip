// norm_train.hip -- training BatchNorm for gfx950 (MI355X) on NHWC activations in fp32 and bf16, with ReLU and the residual add
// fused in, forward and backward (opt-in: salve_amd/models/trainable.py: BatchNormHipFunction, set_train_norm("hip")).
//
// The activation is [rows, C], rows = batch * H * W, the channel innermost (what the training convolutions write).  These are
// bandwidth kernels: every thread owns ONE 16-byte group of channels (4 fp32 or 8 bf16) and walks rows, so every load and store
// is 16 bytes per lane and the per-channel constants live in registers.  A workgroup of 256 threads is GX channel groups wide
// (GX a power of two, at most 64) and RY = 256 / GX rows high; grid = (row chunks, channel tiles).  All arithmetic is fp32.
//
//   forward, train   bn_stats_kernel:  per thread Welford (count, mean, M2) over its rows, the RY threads of a channel group are
//                                      combined with Chan's formula in a fixed tree through LDS, one partial per workgroup and
//                                      channel goes to the workspace.  Never E[x^2] - E[x]^2.
//                    bn_stats_finalise_kernel: one wave per channel; lane l combines the partials l, l + 64, ... in that order,
//                                      then the 64 lanes in a fixed shuffle tree (Chan again).  Writes save_mean, save_invstd =
//                                      1 / sqrt(M2 / rows + eps) and updates the running statistics (unbiased variance).
//                    bn_apply_kernel:  y = (x - mean) * (gamma * invstd) + beta, + residual, max(0, .), one rounding for bf16.
//   forward, eval    bn_apply_kernel alone on the running statistics (invstd = 1 / sqrt(running_var + eps) per thread).
//   backward, train  bn_bwd_reduce_kernel: g = dy (where y > 0 if ReLU was fused); per thread sums of g and g * xhat, the same
//                                      LDS tree, one partial per workgroup and channel.
//                    bn_bwd_finalise_kernel: one wave per channel, the same fixed order: dbeta, dgamma.
//                    bn_bwd_dx_kernel: dx = gamma * invstd * (g - dbeta / rows - xhat * dgamma / rows); dres = g with a residual.
//
//   synchronised (data-parallel ranks; salve_amd/models/trainable.py: SyncBatchNormHipFunction) -- the same kernels behind split
//   entries, with room between the phases for the other ranks' results, and no further pass over x:
//                    salve_bn_*_stats            bn_stats_kernel + bn_stats_finalise_kernel writing the rows' (mean, M2) instead
//                                                of finishing them
//                    salve_bn_combine            bn_combine_kernel: the ranks' (mean, M2) by Chan in rank order, then the same finish
//                    salve_bn_*_apply            bn_apply_kernel
//                    salve_bn_*_backward_reduce  bn_bwd_reduce_kernel + bn_bwd_finalise_kernel
//                    salve_bn_*_backward_apply   bn_bwd_dx_kernel, which adds the ranks' sums in rank order itself
//
// No atomics anywhere; the split of rows over workgroups is a function of (rows, C, dtype) only, so the same inputs give
// bit-identical results.  Element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_GX = 64;           // channel groups per workgroup at most (1 KiB of a row)
constexpr int BN_TARGET_WG = 2048;      // workgroups a reduction launch aims at: 8 per CU.  Fixed: the split depends on the shape only
constexpr int BN_MIN_ROWS = 16;         // rows per thread of a reduction workgroup at least (keeps the partials below 10 % of x)
constexpr int BN_APPLY_ROWS = 8;        // rows per thread of an element-wise workgroup
constexpr int BN_ALL_FLAGS = SALVE_BN_RELU | SALVE_BN_ADD | SALVE_BN_EVAL;

// ---- 16-byte channel groups -----------------------------------------------------------------------------------------------
template <typename T> struct Group;
template <> struct Group<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct Group<uint16_t> {
    static constexpr int N = 8;
    typedef __attribute__((__ext_vector_type__(8))) __bf16 bf16x8;
    typedef __attribute__((__ext_vector_type__(8))) float f32x8;
    static __device__ __forceinline__ void load(const uint16_t* p, float (&v)[8]) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {   // bf16 = the upper half of the fp32 bits
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
    static __device__ __forceinline__ void store(uint16_t* p, const float (&v)[8]) {
        f32x8 f;
#pragma unroll
        for (int i = 0; i < 8; i++) f[i] = v[i];
        // one rounding to nearest even, NaN stays NaN (v_cvt_pk_bf16_f32)
        *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, __builtin_convertvector(f, bf16x8));
    }
};

// ---- launch geometry (host and device agree through these numbers) --------------------------------------------------------
struct Geom {
    int G;        // 16-byte channel groups per row
    int gx;       // channel groups per workgroup (power of two)
    int ry;       // rows a workgroup reads at once = BN_THREADS / gx
    int ctiles;   // workgroups across the channels
    int rpc;      // rows per reduction chunk (a multiple of ry)
    int S;        // reduction chunks = partials per channel
    int apply_rpc, apply_chunks;
};

Geom geometry(int rows, int C, int vec) {
    Geom g;
    g.G = C / vec;
    g.gx = 1;
    while (g.gx < g.G && g.gx < BN_MAX_GX) g.gx <<= 1;
    g.ry = BN_THREADS / g.gx;
    g.ctiles = (g.G + g.gx - 1) / g.gx;
    const long long min_chunk = (long long)g.ry * BN_MIN_ROWS;
    long long s = (rows + min_chunk - 1) / min_chunk;
    const long long cap = BN_TARGET_WG / g.ctiles > 0 ? BN_TARGET_WG / g.ctiles : 1;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    long long rpc = (rows + s - 1) / s;
    rpc = (rpc + g.ry - 1) / g.ry * g.ry;
    g.rpc = (int)rpc;
    g.S = (int)((rows + rpc - 1) / rpc);
    g.apply_rpc = g.ry * BN_APPLY_ROWS;
    g.apply_chunks = (int)(((long long)rows + g.apply_rpc - 1) / g.apply_rpc);
    return g;
}

// Chan, Golub, LeVeque: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb).  An empty side leaves the other unchanged.
__device__ __forceinline__ void chan(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    const float n = na + nb;
    if (nb == 0.f) return;
    const float f = nb / n;
    const float d = mb - ma;
    ma = na == 0.f ? mb : __builtin_fmaf(d, f, ma);
    qa = qa + qb + d * d * (na * f);
    na = n;
}

// ---- forward: statistics ---------------------------------------------------------------------------------------------------
// partial layout: float [S][3][C] = count, mean, M2
template <typename T>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ partial, int rows, int C, int G,
                                                              int gx, int rpc) {
    constexpr int N = Group<T>::N;
    __shared__ float red[BN_THREADS * (2 * N + 1)];
    const int ry = BN_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    const bool live = g < G;
    const long long r0 = (long long)blockIdx.x * rpc;
    const long long r1 = r0 + rpc < rows ? r0 + rpc : rows;
    float mean[N], m2[N], cnt = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) mean[i] = m2[i] = 0.f;
    if (live) {
        const T* px = x + (size_t)g * N;
        long long r = r0 + ty;
        for (; r + 3ll * ry < r1; r += 4ll * ry) {   // four rows in flight
            float v[4][N];
#pragma unroll
            for (int u = 0; u < 4; u++) Group<T>::load(px + (size_t)(r + (long long)u * ry) * C, v[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cnt += 1.f;
                const float inv = 1.f / cnt;
#pragma unroll
                for (int i = 0; i < N; i++) {
                    const float d = v[u][i] - mean[i];
                    mean[i] = __builtin_fmaf(d, inv, mean[i]);
                    m2[i] = __builtin_fmaf(d, v[u][i] - mean[i], m2[i]);
                }
            }
        }
        for (; r < r1; r += ry) {
            float v[N];
            Group<T>::load(px + (size_t)r * C, v);
            cnt += 1.f;
            const float inv = 1.f / cnt;
#pragma unroll
            for (int i = 0; i < N; i++) {
                const float d = v[i] - mean[i];
                mean[i] = __builtin_fmaf(d, inv, mean[i]);
                m2[i] = __builtin_fmaf(d, v[i] - mean[i], m2[i]);
            }
        }
    }
    // the ry threads of a channel group: a fixed tree over ty
    float* mine = red + threadIdx.x * (2 * N + 1);
    mine[0] = cnt;
#pragma unroll
    for (int i = 0; i < N; i++) { mine[1 + i] = mean[i]; mine[1 + N + i] = m2[i]; }
    __syncthreads();
    for (int s = ry >> 1; s > 0; s >>= 1) {
        if (ty < s) {
            const float* other = red + (threadIdx.x + s * gx) * (2 * N + 1);
            const float nb = other[0];
            float na = cnt;
#pragma unroll
            for (int i = 0; i < N; i++) {
                na = cnt;
                chan(na, mean[i], m2[i], nb, other[1 + i], other[1 + N + i]);
            }
            cnt = na;
            mine[0] = cnt;
#pragma unroll
            for (int i = 0; i < N; i++) { mine[1 + i] = mean[i]; mine[1 + N + i] = m2[i]; }
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        float* out = partial + (size_t)blockIdx.x * 3 * C + (size_t)g * N;
#pragma unroll
        for (int i = 0; i < N; i++) { out[i] = cnt; out[C + i] = mean[i]; out[2 * C + i] = m2[i]; }
    }
}

// channel c's (mean, M2) over `rows` rows -> save_mean, save_invstd and the momentum update of the running statistics
__device__ __forceinline__ void bn_finish(int c, float m, float q, long long rows, float eps, float momentum, float* __restrict__ save_mean,
                                          float* __restrict__ save_invstd, float* __restrict__ running_mean, float* __restrict__ running_var) {
    const float var = q / (float)rows;
    save_mean[c] = m;
    save_invstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (q / (float)(rows - 1));
}

// one wave per channel: lane l takes the partials l, l + 64, ... in order, then a fixed shuffle tree over the lanes.
// local: float [2][C], or NULL.  Given, the channel's (mean, M2) go there and nothing is finished (salve_bn_*_stats: the ranks'
// statistics are combined first, bn_combine_kernel).
__global__ __launch_bounds__(BN_THREADS) void bn_stats_finalise_kernel(const float* __restrict__ partial, int S, int C, int rows, float eps,
                                                                       float momentum, float* __restrict__ save_mean,
                                                                       float* __restrict__ save_invstd, float* __restrict__ running_mean,
                                                                       float* __restrict__ running_var, float* __restrict__ local) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= C) return;   // whole waves leave together
    float n = 0.f, m = 0.f, q = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float* p = partial + (size_t)s * 3 * C + c;
        chan(n, m, q, p[0], p[C], p[2 * C]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float nb = __shfl_down(n, off, 64), mb = __shfl_down(m, off, 64), qb = __shfl_down(q, off, 64);
        chan(n, m, q, nb, mb, qb);
    }
    if (lane == 0) {
        if (local) {
            local[c] = m;
            local[C + c] = q;
        } else {
            bn_finish(c, m, q, rows, eps, momentum, save_mean, save_invstd, running_mean, running_var);
        }
    }
}

// The ranks' statistics, float [world][2][C] = (mean, M2) of rank r's counts.n[r] rows, combined with Chan's formula in rank order
// (a rank without rows is skipped), then finished over the `rows` rows of all ranks.  One thread per channel; with one rank the
// result is the fused forward's.
struct BnCounts { float n[SALVE_BN_MAX_WORLD]; };

__global__ __launch_bounds__(BN_THREADS) void bn_combine_kernel(const float* __restrict__ partials, BnCounts counts, int world, int C, long long rows,
                                                                float eps, float momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                                float* __restrict__ running_mean, float* __restrict__ running_var) {
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c >= C) return;
    float n = 0.f, m = 0.f, q = 0.f;
    for (int r = 0; r < world; r++) {
        const float* p = partials + (size_t)r * 2 * C + c;
        const float nb = counts.n[r];
        if (nb == 0.f) continue;
        if (n == 0.f) { n = nb; m = p[0]; q = p[C]; }   // the first rank with rows: its statistics as they are
        else chan(n, m, q, nb, p[0], p[C]);
    }
    bn_finish(c, m, q, rows, eps, momentum, mean, invstd, running_mean, running_var);
}

// ---- forward: apply --------------------------------------------------------------------------------------------------------
template <bool RELU, bool ADD>
__device__ __forceinline__ float bn_out(float x, float mean, float a, float b, float res) {
    float t = __builtin_fmaf(x - mean, a, b);
    if (ADD) t += res;
    if (RELU) t = (t > 0.f || t != t) ? t : 0.f;   // NaN stays NaN, as torch's ReLU
    return t;
}

// scale_is_var: `scale` holds a variance (eval mode: the running variance), else 1 / sqrt(var + eps)
template <typename T, bool RELU, bool ADD>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                              const float* __restrict__ mean_p, const float* __restrict__ scale_p,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, int scale_is_var,
                                                              float eps, int rows, int C, int G, int gx, int rpc) {
    constexpr int N = Group<T>::N;
    const int ry = BN_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    if (g >= G) return;
    const long long r0 = (long long)blockIdx.x * rpc;
    const long long r1 = r0 + rpc < rows ? r0 + rpc : rows;
    float mean[N], a[N], b[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int c = g * N + i;
        const float s = scale_p[c];
        mean[i] = mean_p[c];
        a[i] = gamma[c] * (scale_is_var ? 1.f / sqrtf(s + eps) : s);
        b[i] = beta[c];
    }
    long long r = r0 + ty;
    for (; r + 3ll * ry < r1; r += 4ll * ry) {   // four rows in flight
        float v[4][N], o[4][N] = {};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t off = (size_t)(r + (long long)u * ry) * C + (size_t)g * N;
            Group<T>::load(x + off, v[u]);
            if (ADD) Group<T>::load(res + off, o[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < N; i++) v[u][i] = bn_out<RELU, ADD>(v[u][i], mean[i], a[i], b[i], o[u][i]);
            Group<T>::store(y + (size_t)(r + (long long)u * ry) * C + (size_t)g * N, v[u]);
        }
    }
    for (; r < r1; r += ry) {
        const size_t off = (size_t)r * C + (size_t)g * N;
        float v[N], o[N] = {};
        Group<T>::load(x + off, v);
        if (ADD) Group<T>::load(res + off, o);
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = bn_out<RELU, ADD>(v[i], mean[i], a[i], b[i], o[i]);
        Group<T>::store(y + off, v);
    }
}

// ---- backward: reduce ------------------------------------------------------------------------------------------------------
// partial layout: float [S][2][C] = sum g, sum g * xhat
template <typename T, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
                                                                   const float* __restrict__ mean_p, const float* __restrict__ invstd_p,
                                                                   float* __restrict__ partial, int rows, int C, int G, int gx, int rpc) {
    constexpr int N = Group<T>::N;
    __shared__ float red[BN_THREADS * (2 * N + 1)];   // odd pitch: no bank conflicts
    const int ry = BN_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    const bool live = g < G;
    const long long r0 = (long long)blockIdx.x * rpc;
    const long long r1 = r0 + rpc < rows ? r0 + rpc : rows;
    float sg[N], sgx[N];
#pragma unroll
    for (int i = 0; i < N; i++) sg[i] = sgx[i] = 0.f;
    if (live) {
        float mean[N], invstd[N];
#pragma unroll
        for (int i = 0; i < N; i++) { mean[i] = mean_p[g * N + i]; invstd[i] = invstd_p[g * N + i]; }
        long long r = r0 + ty;
        for (; r + ry < r1; r += 2ll * ry) {   // two rows in flight (up to six 16-byte loads)
            float gv[2][N], xv[2][N], yv[2][N];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const size_t off = (size_t)(r + (long long)u * ry) * C + (size_t)g * N;
                Group<T>::load(dy + off, gv[u]);
                Group<T>::load(x + off, xv[u]);
                if (RELU) Group<T>::load(y + off, yv[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int i = 0; i < N; i++) {
                    const float gg = RELU ? (yv[u][i] > 0.f ? gv[u][i] : 0.f) : gv[u][i];
                    sg[i] += gg;
                    sgx[i] = __builtin_fmaf(gg, (xv[u][i] - mean[i]) * invstd[i], sgx[i]);
                }
        }
        for (; r < r1; r += ry) {
            const size_t off = (size_t)r * C + (size_t)g * N;
            float gv[N], xv[N], yv[N];
            Group<T>::load(dy + off, gv);
            Group<T>::load(x + off, xv);
            if (RELU) Group<T>::load(y + off, yv);
#pragma unroll
            for (int i = 0; i < N; i++) {
                const float gg = RELU ? (yv[i] > 0.f ? gv[i] : 0.f) : gv[i];
                sg[i] += gg;
                sgx[i] = __builtin_fmaf(gg, (xv[i] - mean[i]) * invstd[i], sgx[i]);
            }
        }
    }
    float* mine = red + threadIdx.x * (2 * N + 1);
#pragma unroll
    for (int i = 0; i < N; i++) { mine[i] = sg[i]; mine[N + i] = sgx[i]; }
    __syncthreads();
    for (int s = ry >> 1; s > 0; s >>= 1) {
        if (ty < s) {
            const float* other = red + (threadIdx.x + s * gx) * (2 * N + 1);
#pragma unroll
            for (int i = 0; i < N; i++) {
                sg[i] += other[i];
                sgx[i] += other[N + i];
                mine[i] = sg[i];
                mine[N + i] = sgx[i];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        float* out = partial + (size_t)blockIdx.x * 2 * C + (size_t)g * N;
#pragma unroll
        for (int i = 0; i < N; i++) { out[i] = sg[i]; out[C + i] = sgx[i]; }
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_finalise_kernel(const float* __restrict__ partial, int S, int C, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float* p = partial + (size_t)s * 2 * C + c;
        a += p[0];
        b += p[C];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    if (lane == 0) { dbeta[c] = a; dgamma[c] = b; }
}

// ---- backward: dx ----------------------------------------------------------------------------------------------------------
// dbeta, dgamma: `world` ranks' sums of g and of g * xhat, rank r's at [r * rank_stride + c], added here in rank order (the fused
// backward: world 1, its own dbeta and dgamma); total_rows: the rows of all ranks, `rows` this launch's.
template <typename T, bool RELU, bool ADD>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
                                                               const float* __restrict__ mean_p, const float* __restrict__ invstd_p,
                                                               const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, int world, long long rank_stride,
                                                               long long total_rows, T* __restrict__ dx, T* __restrict__ dres, int rows, int C,
                                                               int G, int gx, int rpc) {
    constexpr int N = Group<T>::N;
    const int ry = BN_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    if (g >= G) return;
    const long long r0 = (long long)blockIdx.x * rpc;
    const long long r1 = r0 + rpc < rows ? r0 + rpc : rows;
    const float inv_rows = 1.f / (float)total_rows;
    float mean[N], invstd[N], a[N], k1[N], k2[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int c = g * N + i;
        mean[i] = mean_p[c];
        invstd[i] = invstd_p[c];
        a[i] = gamma[c] * invstd[i];
        float sb = dbeta[c], sg = dgamma[c];
        for (int r = 1; r < world; r++) {
            sb += dbeta[(size_t)r * rank_stride + c];
            sg += dgamma[(size_t)r * rank_stride + c];
        }
        k1[i] = sb * inv_rows;
        k2[i] = sg * inv_rows;
    }
    long long r = r0 + ty;
    for (; r + ry < r1; r += 2ll * ry) {   // two rows in flight (up to six 16-byte loads)
        float gv[2][N], xv[2][N], yv[2][N];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const size_t off = (size_t)(r + (long long)u * ry) * C + (size_t)g * N;
            Group<T>::load(dy + off, gv[u]);
            Group<T>::load(x + off, xv[u]);
            if (RELU) Group<T>::load(y + off, yv[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const size_t off = (size_t)(r + (long long)u * ry) * C + (size_t)g * N;
#pragma unroll
            for (int i = 0; i < N; i++) {
                if (RELU) gv[u][i] = yv[u][i] > 0.f ? gv[u][i] : 0.f;
                const float xhat = (xv[u][i] - mean[i]) * invstd[i];
                xv[u][i] = a[i] * (gv[u][i] - k1[i] - xhat * k2[i]);
            }
            Group<T>::store(dx + off, xv[u]);
            if (ADD) Group<T>::store(dres + off, gv[u]);
        }
    }
    for (; r < r1; r += ry) {
        const size_t off = (size_t)r * C + (size_t)g * N;
        float gv[N], xv[N], yv[N];
        Group<T>::load(dy + off, gv);
        Group<T>::load(x + off, xv);
        if (RELU) Group<T>::load(y + off, yv);
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (RELU) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
            const float xhat = (xv[i] - mean[i]) * invstd[i];
            xv[i] = a[i] * (gv[i] - k1[i] - xhat * k2[i]);
        }
        Group<T>::store(dx + off, xv);
        if (ADD) Group<T>::store(dres + off, gv);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// min_rows: 2 for the fused entries; 0 for the split ones, whose rows are one rank's (the ranks' total is checked where it is known)
int check_bn_desc(const salve_bn_desc_t* d, const char* who, int min_rows = 2) {
    if (!d) { salve_fail(who); return SALVE_ERR_BAD_ARG; }
    if (d->C < 8 || d->C > 4096 || d->C % 8 != 0) { salve_fail("bn: C must be a multiple of 8 from 8 to 4096"); return SALVE_ERR_BAD_ARG; }
    if (d->rows < min_rows) { salve_fail(min_rows == 2 ? "bn: rows must be at least 2" : "bn: a rank's rows must not be negative"); return SALVE_ERR_BAD_ARG; }
    if (d->flags & ~BN_ALL_FLAGS) { salve_fail("bn: unknown flag bit"); return SALVE_ERR_BAD_ARG; }
    if (!(d->eps >= 0.f) || !(d->momentum >= 0.f && d->momentum <= 1.f)) { salve_fail("bn: eps must be >= 0 and momentum in [0, 1]"); return SALVE_ERR_BAD_ARG; }
    return SALVE_OK;
}

// the split entries: train mode only (the eval form reads no batch statistics: salve_bn_*_forward alone serves it)
int check_split_desc(const salve_bn_desc_t* d, const char* who) {
    const int st = check_bn_desc(d, who, 0);
    if (st != SALVE_OK) return st;
    if (d->flags & SALVE_BN_EVAL) { salve_fail("bn: the split entries synchronise batch statistics; the eval form has none"); return SALVE_ERR_UNSUPPORTED; }
    return SALVE_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The workspace serves both dtypes: sized for the fp32 split, which is never smaller than the bf16 one.
size_t bn_ws(const salve_bn_desc_t* d, int pass) {
    if (pass == SALVE_BN_FWD && (d->flags & SALVE_BN_EVAL)) return 256;
    if (d->rows == 0) return 256;   // (a split pass of a rank without rows launches nothing)
    const bool fwd = pass == SALVE_BN_FWD || pass == SALVE_BN_STATS;
    const Geom g4 = geometry(d->rows, d->C, 4), g8 = geometry(d->rows, d->C, 8);
    const size_t S = (size_t)(g4.S > g8.S ? g4.S : g8.S);
    return align256(S * (fwd ? 3 : 2) * d->C * sizeof(float)) + 256;
}

template <typename T, bool RELU, bool ADD>
void launch_apply(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* x, const T* res, T* y, const float* mean, const float* scale,
                  const float* gamma, const float* beta, int scale_is_var) {
    hipLaunchKernelGGL((bn_apply_kernel<T, RELU, ADD>), dim3((unsigned)g.apply_chunks, (unsigned)g.ctiles), dim3(BN_THREADS), 0, s, x, res, y, mean,
                       scale, gamma, beta, scale_is_var, d->eps, d->rows, d->C, g.G, g.gx, g.apply_rpc);
}

template <typename T>
void dispatch_apply(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* x, const T* residual, T* y, const float* mean, const float* scale,
                    const float* gamma, const float* beta, int scale_is_var) {
    const bool relu = d->flags & SALVE_BN_RELU, add = d->flags & SALVE_BN_ADD;
    if (relu && add) launch_apply<T, true, true>(g, s, d, x, residual, y, mean, scale, gamma, beta, scale_is_var);
    else if (relu) launch_apply<T, true, false>(g, s, d, x, residual, y, mean, scale, gamma, beta, scale_is_var);
    else if (add) launch_apply<T, false, true>(g, s, d, x, residual, y, mean, scale, gamma, beta, scale_is_var);
    else launch_apply<T, false, false>(g, s, d, x, residual, y, mean, scale, gamma, beta, scale_is_var);
}

// The statistics pass and its finalise.  local NULL: save_mean, save_invstd and the running update over d->rows (the fused forward);
// local given: the rows' (mean, M2) go there and nothing else is written (salve_bn_*_stats).
template <typename T>
int launch_stats(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* x, void* ws, float* save_mean, float* save_invstd,
                 float* running_mean, float* running_var, float* local) {
    float* partial = reinterpret_cast<float*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    hipLaunchKernelGGL(bn_stats_kernel<T>, dim3((unsigned)g.S, (unsigned)g.ctiles), dim3(BN_THREADS), 0, s, x, partial, d->rows, d->C, g.G, g.gx, g.rpc);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bn_stats_finalise_kernel, dim3((unsigned)((d->C + 3) / 4)), dim3(BN_THREADS), 0, s, partial, g.S, d->C, d->rows, d->eps,
                       d->momentum, save_mean, save_invstd, running_mean, running_var, local);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

template <typename T>
int bn_forward(const char* who, const salve_bn_desc_t* d, const T* x, const T* residual, const float* gamma, const float* beta, float* running_mean,
               float* running_var, T* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, void* stream) {
    int st = check_bn_desc(d, who);
    if (st != SALVE_OK) return st;
    const bool add = d->flags & SALVE_BN_ADD, eval = d->flags & SALVE_BN_EVAL;
    if (!x || !gamma || !beta || !y || !ws || (add && !residual) || (eval ? (!running_mean || !running_var) : (!save_mean || !save_invstd)) ||
        !aligned16(x) || !aligned16(y) || !aligned16(residual)) {
        salve_fail("salve_bn_*_forward: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (ws_bytes < bn_ws(d, SALVE_BN_FWD)) { salve_fail("salve_bn_*_forward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    const Geom g = geometry(d->rows, d->C, Group<T>::N);
    hipStream_t s = (hipStream_t)stream;
    const float *mean = running_mean, *scale = running_var;
    if (!eval) {
        st = launch_stats<T>(g, s, d, x, ws, save_mean, save_invstd, running_mean, running_var, nullptr);
        if (st != SALVE_OK) return st;
        mean = save_mean;
        scale = save_invstd;
    }
    dispatch_apply<T>(g, s, d, x, residual, y, mean, scale, gamma, beta, eval ? 1 : 0);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

// ---- the split forward: statistics | combine (salve_bn_combine) | apply ----------------------------------------------------------
template <typename T>
int bn_stats(const char* who, const salve_bn_desc_t* d, const T* x, float* partial, void* ws, size_t ws_bytes, void* stream) {
    const int st = check_split_desc(d, who);
    if (st != SALVE_OK) return st;
    if (!partial || (d->rows > 0 && (!x || !ws || !aligned16(x)))) {
        salve_fail("salve_bn_*_stats: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (d->rows == 0) {   // a rank that got none of a short batch: zeros, which salve_bn_combine skips
        SALVE_HIP_CHECK(hipMemsetAsync(partial, 0, (size_t)2 * d->C * sizeof(float), s));
        return SALVE_OK;
    }
    if (ws_bytes < bn_ws(d, SALVE_BN_STATS)) { salve_fail("salve_bn_*_stats: workspace too small"); return SALVE_ERR_WORKSPACE; }
    return launch_stats<T>(geometry(d->rows, d->C, Group<T>::N), s, d, x, ws, nullptr, nullptr, nullptr, nullptr, partial);
}

template <typename T>
int bn_apply(const char* who, const salve_bn_desc_t* d, const T* x, const T* residual, const float* gamma, const float* beta, const float* mean,
             const float* invstd, T* y, void* stream) {
    const int st = check_split_desc(d, who);
    if (st != SALVE_OK) return st;
    const bool add = d->flags & SALVE_BN_ADD;
    if (!gamma || !beta || !mean || !invstd || (d->rows > 0 && (!x || !y || (add && !residual))) || !aligned16(x) || !aligned16(y) ||
        !aligned16(residual)) {
        salve_fail("salve_bn_*_apply: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (d->rows == 0) return SALVE_OK;
    dispatch_apply<T>(geometry(d->rows, d->C, Group<T>::N), (hipStream_t)stream, d, x, residual, y, mean, invstd, gamma, beta, 0);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

template <typename T, bool RELU, bool ADD>
void launch_dx(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
               const float* gamma, const float* dgamma, const float* dbeta, int world, long long rank_stride, long long total_rows, T* dx, T* dres) {
    hipLaunchKernelGGL((bn_bwd_dx_kernel<T, RELU, ADD>), dim3((unsigned)g.apply_chunks, (unsigned)g.ctiles), dim3(BN_THREADS), 0, s, dy, x, y, mean,
                       invstd, gamma, dgamma, dbeta, world, rank_stride, total_rows, dx, dres, d->rows, d->C, g.G, g.gx, g.apply_rpc);
}

template <typename T>
void dispatch_dx(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                 const float* gamma, const float* dgamma, const float* dbeta, int world, long long rank_stride, long long total_rows, T* dx, T* dres) {
    const bool relu = d->flags & SALVE_BN_RELU, add = d->flags & SALVE_BN_ADD;
    if (relu && add) launch_dx<T, true, true>(g, s, d, dy, x, y, mean, invstd, gamma, dgamma, dbeta, world, rank_stride, total_rows, dx, dres);
    else if (relu) launch_dx<T, true, false>(g, s, d, dy, x, y, mean, invstd, gamma, dgamma, dbeta, world, rank_stride, total_rows, dx, dres);
    else if (add) launch_dx<T, false, true>(g, s, d, dy, x, y, mean, invstd, gamma, dgamma, dbeta, world, rank_stride, total_rows, dx, dres);
    else launch_dx<T, false, false>(g, s, d, dy, x, y, mean, invstd, gamma, dgamma, dbeta, world, rank_stride, total_rows, dx, dres);
}

// The reduce pass and its finalise: dbeta = sum g, dgamma = sum g * xhat over d->rows.
template <typename T>
int launch_reduce(const Geom& g, hipStream_t s, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                  void* ws, float* dgamma, float* dbeta) {
    float* partial = reinterpret_cast<float*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    const dim3 grid((unsigned)g.S, (unsigned)g.ctiles);
    if (d->flags & SALVE_BN_RELU) hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, true>), grid, dim3(BN_THREADS), 0, s, dy, x, y, mean, invstd, partial, d->rows, d->C, g.G, g.gx, g.rpc);
    else hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, false>), grid, dim3(BN_THREADS), 0, s, dy, x, y, mean, invstd, partial, d->rows, d->C, g.G, g.gx, g.rpc);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bn_bwd_finalise_kernel, dim3((unsigned)((d->C + 3) / 4)), dim3(BN_THREADS), 0, s, partial, g.S, d->C, dgamma, dbeta);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

template <typename T>
int bn_backward(const char* who, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* gamma, const float* save_mean,
                const float* save_invstd, T* dx, T* dres, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    int st = check_bn_desc(d, who);
    if (st != SALVE_OK) return st;
    if (d->flags & SALVE_BN_EVAL) { salve_fail("salve_bn_*_backward: the eval form has no backward pass"); return SALVE_ERR_UNSUPPORTED; }
    const bool relu = d->flags & SALVE_BN_RELU, add = d->flags & SALVE_BN_ADD;
    if (!dy || !x || !gamma || !save_mean || !save_invstd || !dx || !dgamma || !dbeta || !ws || (relu && !y) || (add && !dres) || !aligned16(dy) ||
        !aligned16(x) || !aligned16(y) || !aligned16(dx) || !aligned16(dres)) {
        salve_fail("salve_bn_*_backward: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (ws_bytes < bn_ws(d, SALVE_BN_BWD)) { salve_fail("salve_bn_*_backward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    const Geom g = geometry(d->rows, d->C, Group<T>::N);
    hipStream_t s = (hipStream_t)stream;
    st = launch_reduce<T>(g, s, d, dy, x, y, save_mean, save_invstd, ws, dgamma, dbeta);
    if (st != SALVE_OK) return st;
    dispatch_dx<T>(g, s, d, dy, x, y, save_mean, save_invstd, gamma, dgamma, dbeta, 1, 0, d->rows, dx, dres);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

// ---- the split backward: reduce | (the ranks' sums gathered) | apply ---------------------------------------------------------------
template <typename T>
int bn_backward_reduce(const char* who, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* mean, const float* invstd,
                       float* sums, void* ws, size_t ws_bytes, void* stream) {
    const int st = check_split_desc(d, who);
    if (st != SALVE_OK) return st;
    const bool relu = d->flags & SALVE_BN_RELU;
    if (!sums || !mean || !invstd || (d->rows > 0 && (!dy || !x || !ws || (relu && !y))) || !aligned16(dy) || !aligned16(x) || !aligned16(y)) {
        salve_fail("salve_bn_*_backward_reduce: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (d->rows == 0) {
        SALVE_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)2 * d->C * sizeof(float), s));
        return SALVE_OK;
    }
    if (ws_bytes < bn_ws(d, SALVE_BN_BWD_REDUCE)) { salve_fail("salve_bn_*_backward_reduce: workspace too small"); return SALVE_ERR_WORKSPACE; }
    return launch_reduce<T>(geometry(d->rows, d->C, Group<T>::N), s, d, dy, x, y, mean, invstd, ws, sums + d->C, sums);
}

template <typename T>
int bn_backward_apply(const char* who, const salve_bn_desc_t* d, const T* dy, const T* x, const T* y, const float* gamma, const float* mean,
                      const float* invstd, const float* sums, int world, long long total_rows, T* dx, T* dres, void* stream) {
    const int st = check_split_desc(d, who);
    if (st != SALVE_OK) return st;
    if (world < 1 || world > SALVE_BN_MAX_WORLD) { salve_fail("bn: world must be 1 .. SALVE_BN_MAX_WORLD"); return SALVE_ERR_BAD_ARG; }
    if (total_rows < 2 || total_rows < d->rows) { salve_fail("bn: the ranks' rows must be at least 2 together, and no fewer than this rank's"); return SALVE_ERR_BAD_ARG; }
    const bool relu = d->flags & SALVE_BN_RELU, add = d->flags & SALVE_BN_ADD;
    if (!gamma || !mean || !invstd || !sums || (d->rows > 0 && (!dy || !x || !dx || (relu && !y) || (add && !dres))) || !aligned16(dy) ||
        !aligned16(x) || !aligned16(y) || !aligned16(dx) || !aligned16(dres)) {
        salve_fail("salve_bn_*_backward_apply: null or not 16-byte aligned pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (d->rows == 0) return SALVE_OK;
    dispatch_dx<T>(geometry(d->rows, d->C, Group<T>::N), (hipStream_t)stream, d, dy, x, y, mean, invstd, gamma, sums + d->C, sums, world,
                   2ll * d->C, total_rows, dx, dres);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace

extern "C" {

size_t salve_bn_workspace_bytes(const salve_bn_desc_t* d, int32_t pass) {
    if (pass == SALVE_BN_STATS || pass == SALVE_BN_BWD_REDUCE)   // the split passes: the rows are one rank's, which may have none
        return check_split_desc(d, "salve_bn_workspace_bytes: null descriptor") == SALVE_OK ? bn_ws(d, pass) : 0;
    if (check_bn_desc(d, "salve_bn_workspace_bytes: null descriptor") != SALVE_OK) return 0;
    if (pass != SALVE_BN_FWD && pass != SALVE_BN_BWD) { salve_fail("salve_bn_workspace_bytes: pass must be one of SALVE_BN_FWD, _BWD, _STATS, _BWD_REDUCE"); return 0; }
    if (pass == SALVE_BN_BWD && (d->flags & SALVE_BN_EVAL)) { salve_fail("salve_bn_workspace_bytes: the eval form has no backward pass"); return 0; }
    return bn_ws(d, pass);
}

int salve_bn_f32_forward(const salve_bn_desc_t* d, const float* x, const float* residual, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                         void* stream) {
    return bn_forward<float>("salve_bn_f32_forward: null descriptor", d, x, residual, gamma, beta, running_mean, running_var, y, save_mean,
                             save_invstd, ws, ws_bytes, stream);
}

int salve_bn_f32_backward(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean,
                          const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    return bn_backward<float>("salve_bn_f32_backward: null descriptor", d, dy, x, y, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, ws,
                              ws_bytes, stream);
}

int salve_bn_bf16_forward(const salve_bn_desc_t* d, const uint16_t* x, const uint16_t* residual, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, uint16_t* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                          void* stream) {
    return bn_forward<uint16_t>("salve_bn_bf16_forward: null descriptor", d, x, residual, gamma, beta, running_mean, running_var, y, save_mean,
                                save_invstd, ws, ws_bytes, stream);
}

int salve_bn_bf16_backward(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* gamma,
                           const float* save_mean, const float* save_invstd, uint16_t* dx, uint16_t* dres, float* dgamma, float* dbeta, void* ws,
                           size_t ws_bytes, void* stream) {
    return bn_backward<uint16_t>("salve_bn_bf16_backward: null descriptor", d, dy, x, y, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, ws,
                                 ws_bytes, stream);
}

int salve_bn_f32_stats(const salve_bn_desc_t* d, const float* x, float* partial, void* ws, size_t ws_bytes, void* stream) {
    return bn_stats<float>("salve_bn_f32_stats: null descriptor", d, x, partial, ws, ws_bytes, stream);
}

int salve_bn_bf16_stats(const salve_bn_desc_t* d, const uint16_t* x, float* partial, void* ws, size_t ws_bytes, void* stream) {
    return bn_stats<uint16_t>("salve_bn_bf16_stats: null descriptor", d, x, partial, ws, ws_bytes, stream);
}

int salve_bn_combine(const salve_bn_desc_t* d, const float* partials, const int64_t* rows, int32_t world, float* running_mean, float* running_var,
                     float* mean, float* invstd, void* stream) {
    const int st = check_split_desc(d, "salve_bn_combine: null descriptor");
    if (st != SALVE_OK) return st;
    if (world < 1 || world > SALVE_BN_MAX_WORLD) { salve_fail("bn: world must be 1 .. SALVE_BN_MAX_WORLD"); return SALVE_ERR_BAD_ARG; }
    if (!partials || !rows || !mean || !invstd) { salve_fail("salve_bn_combine: null pointer"); return SALVE_ERR_BAD_ARG; }
    BnCounts counts = {};
    long long total = 0;
    for (int r = 0; r < world; r++) {
        if (rows[r] < 0 || rows[r] > INT32_MAX) { salve_fail("salve_bn_combine: a rank's rows must be 0 .. 2^31 - 1"); return SALVE_ERR_BAD_ARG; }
        counts.n[r] = (float)rows[r];
        total += rows[r];
    }
    if (total < 2) { salve_fail("bn: rows must be at least 2"); return SALVE_ERR_BAD_ARG; }
    hipLaunchKernelGGL(bn_combine_kernel, dim3((unsigned)((d->C + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0, (hipStream_t)stream, partials,
                       counts, world, d->C, total, d->eps, d->momentum, mean, invstd, running_mean, running_var);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_bn_f32_apply(const salve_bn_desc_t* d, const float* x, const float* residual, const float* gamma, const float* beta, const float* mean,
                       const float* invstd, float* y, void* stream) {
    return bn_apply<float>("salve_bn_f32_apply: null descriptor", d, x, residual, gamma, beta, mean, invstd, y, stream);
}

int salve_bn_bf16_apply(const salve_bn_desc_t* d, const uint16_t* x, const uint16_t* residual, const float* gamma, const float* beta,
                        const float* mean, const float* invstd, uint16_t* y, void* stream) {
    return bn_apply<uint16_t>("salve_bn_bf16_apply: null descriptor", d, x, residual, gamma, beta, mean, invstd, y, stream);
}

int salve_bn_f32_backward_reduce(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                                 float* sums, void* ws, size_t ws_bytes, void* stream) {
    return bn_backward_reduce<float>("salve_bn_f32_backward_reduce: null descriptor", d, dy, x, y, mean, invstd, sums, ws, ws_bytes, stream);
}

int salve_bn_bf16_backward_reduce(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* mean,
                                  const float* invstd, float* sums, void* ws, size_t ws_bytes, void* stream) {
    return bn_backward_reduce<uint16_t>("salve_bn_bf16_backward_reduce: null descriptor", d, dy, x, y, mean, invstd, sums, ws, ws_bytes, stream);
}

int salve_bn_f32_backward_apply(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* gamma, const float* mean,
                                const float* invstd, const float* sums, int32_t world, int64_t total_rows, float* dx, float* dres, void* stream) {
    return bn_backward_apply<float>("salve_bn_f32_backward_apply: null descriptor", d, dy, x, y, gamma, mean, invstd, sums, world, total_rows, dx,
                                    dres, stream);
}

int salve_bn_bf16_backward_apply(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* gamma,
                                 const float* mean, const float* invstd, const float* sums, int32_t world, int64_t total_rows, uint16_t* dx,
                                 uint16_t* dres, void* stream) {
    return bn_backward_apply<uint16_t>("salve_bn_bf16_backward_apply: null descriptor", d, dy, x, y, gamma, mean, invstd, sums, world, total_rows,
                                       dx, dres, stream);
}

}  // extern "C"
