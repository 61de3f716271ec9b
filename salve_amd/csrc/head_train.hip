// head_train.hip -- the classifier head of a training step for gfx950 (MI355X): average pool + fc + softmax + cross-entropy +
// arg-max accuracy counts in one fused forward, and the matching fused backward, on NHWC activations in fp32 and bf16 (opt-in:
// salve_amd/models/trainable.py: ClassifierHeadHipFunction, set_train_head("hip")).
//
// The last block's output is x [B, HW, C], the channel innermost.  Only two kernels touch it, and they are bandwidth kernels in the
// form of norm_train.hip: a thread owns ONE 16-byte group of channels (4 fp32 or 8 bf16) and walks the HW rows of one sample, a
// workgroup of 256 threads is GX channel groups wide (a power of two, at most 64) and RY = 256 / GX rows high, grid = (B, channel
// tiles).  Everything else is a few kilobytes.
//
//   forward   head_pool_kernel:    per thread the fp32 sum of its rows (r = ty, ty + RY, ...), the RY threads of a channel group
//                                  added in a fixed tree through LDS, divided by HW once: pooled [B, C].
//             head_logits_kernel:  one workgroup per sample: per thread fused multiply-adds over its 16-byte groups of C for each of
//                                  the K classes, a fixed shuffle tree per wave, the four waves added in order, + bias; lane 0 then
//                                  forms the max-subtracted softmax and the row's -log_softmax[target] (K values: in double,
//                                  each result rounded to fp32 once) and the arg-max of the probabilities it has just written
//                                  (first index wins a tie).  Per-row loss (double) and (target, hit) go to the workspace.
//             head_finish_kernel:  ONE workgroup: the per-row losses summed in a fixed order (thread t takes rows t, t + 256, ...,
//                                  then the same tree) and divided by B; the per-class counts; the meter record updated with plain
//                                  stores, every word by one owner thread.
//   backward  head_dw_kernel:      dW [K, C] and db [K]: a thread owns one column of [pooled | 1], four threads share it over the
//                                  samples (b = ty, ty + 4, ...), added in a fixed order through LDS.
//             head_dx_kernel:      dx [B, HW, C] = (dlogits . W) / HW broadcast over the rows, rounded once; also writes dlogits.
//   dlogits = (probs - onehot) * (g / B) is recomputed from probs wherever it is needed by one function: the same bits everywhere.
//   The few scalars per row (softmax, row loss, dlogits) and the sum of the row losses are formed in double and rounded once; the
//   sums over HW, C and B for pooled, logits, dW, db and dx are fp32 fused multiply-adds.
//
// No atomics on floating-point values anywhere (the per-class counts are integers, added in LDS); the split of the work is a function
// of the shape and the dtype only, so the same inputs give bit-identical results.  Element offsets are 64-bit.  A row whose target
// lies outside [0, K) indexes nothing: no loss, no gradient, no count, one more in bad_targets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_WAVES = HEAD_THREADS / 64;
constexpr int HEAD_MAX_GX = 64;                       // channel groups per workgroup at most (1 KiB of a row)
constexpr int HEAD_MAX_K = SALVE_HEAD_MAX_CLASSES;
constexpr int HEAD_DW_COLS = 64, HEAD_DW_PHASES = HEAD_THREADS / HEAD_DW_COLS;
static_assert(sizeof(salve_head_meter_t) == (2 * SALVE_HEAD_MAX_CLASSES + 3) * 8, "the meter record salve_hip.h documents");
static_assert(HEAD_MAX_K <= 64 && HEAD_DW_PHASES == 4, "one wave finishes the classes; head_dw_kernel adds four phases");

// ---- 16-byte channel groups (as norm_train.hip) ---------------------------------------------------------------------------
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

struct Geom {
    int G;        // 16-byte channel groups per row
    int gx;       // channel groups per workgroup (power of two)
    int ctiles;   // workgroups across the channels
};

Geom geometry(int C, int vec) {
    Geom g;
    g.G = C / vec;
    g.gx = 1;
    while (g.gx < g.G && g.gx < HEAD_MAX_GX) g.gx <<= 1;
    g.ctiles = (g.G + g.gx - 1) / g.gx;
    return g;
}

// ---- forward: average pool -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(HEAD_THREADS) void head_pool_kernel(const T* __restrict__ x, float* __restrict__ pooled, int HW, int C, int G, int gx) {
    constexpr int N = Group<T>::N;
    __shared__ float red[HEAD_THREADS * (N + 1)];   // odd pitch: no bank conflicts
    const int ry = HEAD_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    const bool live = g < G;
    const int b = blockIdx.x;
    float s[N];
#pragma unroll
    for (int i = 0; i < N; i++) s[i] = 0.f;
    if (live) {
        const T* px = x + (size_t)b * HW * C + (size_t)g * N;
        int r = ty;
        for (; r + 3 * ry < HW; r += 4 * ry) {   // four rows in flight
            float v[4][N];
#pragma unroll
            for (int u = 0; u < 4; u++) Group<T>::load(px + (size_t)(r + u * ry) * C, v[u]);
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int i = 0; i < N; i++) s[i] += v[u][i];
        }
        for (; r < HW; r += ry) {
            float v[N];
            Group<T>::load(px + (size_t)r * C, v);
#pragma unroll
            for (int i = 0; i < N; i++) s[i] += v[i];
        }
    }
    float* mine = red + threadIdx.x * (N + 1);
#pragma unroll
    for (int i = 0; i < N; i++) mine[i] = s[i];
    __syncthreads();
    for (int h = ry >> 1; h > 0; h >>= 1) {   // the ry threads of a channel group: a fixed tree over ty
        if (ty < h) {
            const float* other = red + (threadIdx.x + h * gx) * (N + 1);
#pragma unroll
            for (int i = 0; i < N; i++) {
                s[i] += other[i];
                mine[i] = s[i];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        const float hw = (float)HW;
        float o[4];
        float* out = pooled + (size_t)b * C + (size_t)g * N;
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = s[4 * q + i] / hw;
            Group<float>::store(out + 4 * q, o);
        }
    }
}

// a fixed shuffle tree over the 64 lanes; lane 0 holds the sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- forward: fc + softmax + loss + arg-max, one workgroup per sample -----------------------------------------------------------
// rowinfo: -1 for a target outside [0, K), else target | 256 when the prediction equals it
__global__ __launch_bounds__(HEAD_THREADS) void head_logits_kernel(const float* __restrict__ pooled, const float* __restrict__ weight,
                                                                   const float* __restrict__ bias, const int64_t* __restrict__ target,
                                                                   float* __restrict__ logits, float* __restrict__ probs,
                                                                   double* __restrict__ rowloss, int32_t* __restrict__ rowinfo, int C, int K) {
    __shared__ float part[HEAD_WAVES][HEAD_MAX_K];
    __shared__ float lg[HEAD_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float acc[HEAD_MAX_K];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) acc[k] = 0.f;
    const float4* p4 = reinterpret_cast<const float4*>(pooled + (size_t)b * C);
    const int nv = C >> 2;
    for (int v = tid; v < nv; v += HEAD_THREADS) {
        const float4 p = p4[v];
#pragma unroll
        for (int k = 0; k < HEAD_MAX_K; k++) {
            if (k < K) {   // (uniform)
                const float4 w = reinterpret_cast<const float4*>(weight + (size_t)k * C)[v];
                float a = acc[k];
                a = __builtin_fmaf(p.x, w.x, a);
                a = __builtin_fmaf(p.y, w.y, a);
                a = __builtin_fmaf(p.z, w.z, a);
                a = __builtin_fmaf(p.w, w.w, a);
                acc[k] = a;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) {
        if (k < K) {
            const float s = wave_sum(acc[k]);
            if (lane == 0) part[wave][k] = s;
        }
    }
    __syncthreads();
    if (tid < K) lg[tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + bias[tid];
    __syncthreads();
    if (tid != 0) return;
    float m = lg[0];
    for (int k = 1; k < K; k++) m = lg[k] > m ? lg[k] : m;
    // K values per row on one lane: in double, so that a probability and the row's loss are each rounded to fp32 once
    double e[HEAD_MAX_K], sum = 0.0;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) {
        e[k] = k < K ? exp((double)lg[k] - (double)m) : 0.0;   // a NaN logit makes the sum, every probability and the loss NaN
        sum += e[k];
    }
    float best = 0.f;
    int pred = 0;
    float* pr = probs + (size_t)b * K;
    float* lo = logits + (size_t)b * K;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) {
        if (k < K) {
            const float p = (float)(e[k] / sum);
            pr[k] = p;
            lo[k] = lg[k];
            if (k == 0 || p > best) { best = p; pred = k; }   // the first index wins a tie
        }
    }
    const int64_t t = target[b];
    const bool valid = t >= 0 && t < K;
    rowloss[b] = valid ? log(sum) - ((double)lg[(int)t] - (double)m) : 0.0;
    rowinfo[b] = valid ? ((int32_t)t | (pred == (int)t ? 256 : 0)) : -1;
}

// ---- forward: the batch's loss and the meter record, ONE workgroup --------------------------------------------------------------
__global__ __launch_bounds__(HEAD_THREADS) void head_finish_kernel(const double* __restrict__ rowloss, const int32_t* __restrict__ rowinfo, int B,
                                                                   int K, int accumulate, float* __restrict__ loss, salve_head_meter_t* meter) {
    __shared__ double part[HEAD_WAVES];
    __shared__ int n_total[HEAD_MAX_K], n_correct[HEAD_MAX_K], n_bad;
    const int tid = threadIdx.x;
    if (tid < HEAD_MAX_K) n_total[tid] = n_correct[tid] = 0;
    if (tid == 0) n_bad = 0;
    __syncthreads();
    double s = 0.0;
    for (int b = tid; b < B; b += HEAD_THREADS) {
        s += rowloss[b];
        const int32_t info = rowinfo[b];
        if (info < 0) {
            atomicAdd(&n_bad, 1);   // integers in LDS: the order does not matter
        } else {
            atomicAdd(&n_total[info & 255], 1);
            if (info & 256) atomicAdd(&n_correct[info & 255], 1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);   // the same fixed tree as wave_sum
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const float l = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)B);   // rounded once
        *loss = l;
        if (meter) {
            if (accumulate) {   // run_epoch's `loss_sum += float(loss.item()) * n`, in double
                meter->loss_sum = meter->loss_sum + (double)l * (double)B;
                meter->loss_rows = meter->loss_rows + B;
            }
            meter->bad_targets = meter->bad_targets + n_bad;
        }
    }
    if (meter && tid < K) {   // every counter has one owner
        meter->total[tid] = meter->total[tid] + n_total[tid];
        meter->correct[tid] = meter->correct[tid] + n_correct[tid];
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// dlogits[b][k] of a row with target t (0 for a target outside [0, K)); scale = g / B.  Formed in double and rounded once.
__device__ __forceinline__ float head_dlogit(const float* __restrict__ probs, int64_t t, int b, int k, int K, double scale) {
    if (t < 0 || t >= K) return 0.f;
    return (float)(((double)probs[(size_t)b * K + k] - (t == k ? 1.0 : 0.0)) * scale);
}

// column c < C of [pooled | 1] gives dW[:, c], column C gives db
__global__ __launch_bounds__(HEAD_THREADS) void head_dw_kernel(const float* __restrict__ pooled, const float* __restrict__ probs,
                                                               const int64_t* __restrict__ target, const float* __restrict__ grad_loss,
                                                               float* __restrict__ dw, float* __restrict__ db, int B, int C, int K) {
    __shared__ float red[HEAD_DW_PHASES][HEAD_MAX_K][HEAD_DW_COLS];
    const int tx = threadIdx.x & (HEAD_DW_COLS - 1), ty = threadIdx.x / HEAD_DW_COLS;   // (a wave is one ty: its rows are uniform)
    const int col = blockIdx.x * HEAD_DW_COLS + tx;
    const bool live = col <= C;
    const double scale = (double)*grad_loss / (double)B;
    float acc[HEAD_MAX_K];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) acc[k] = 0.f;
    if (live) {
        for (int b = ty; b < B; b += HEAD_DW_PHASES) {
            const int64_t t = target[b];
            if (t < 0 || t >= K) continue;
            const float pv = col < C ? pooled[(size_t)b * C + col] : 1.f;
#pragma unroll
            for (int k = 0; k < HEAD_MAX_K; k++)
                if (k < K) acc[k] = __builtin_fmaf(head_dlogit(probs, t, b, k, K, scale), pv, acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < HEAD_MAX_K; k++) red[ty][k][tx] = acc[k];
    __syncthreads();
    if (ty == 0 && live) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_K; k++) {
            if (k < K) {
                const float s = (red[0][k][tx] + red[1][k][tx]) + (red[2][k][tx] + red[3][k][tx]);
                if (col < C) dw[(size_t)k * C + col] = s;
                else db[k] = s;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(HEAD_THREADS) void head_dx_kernel(const float* __restrict__ probs, const int64_t* __restrict__ target,
                                                               const float* __restrict__ weight, const float* __restrict__ grad_loss,
                                                               float* __restrict__ dlogits, T* __restrict__ dx, int B, int HW, int C, int K, int G,
                                                               int gx) {
    constexpr int N = Group<T>::N;
    const int ry = HEAD_THREADS / gx;
    const int tx = threadIdx.x & (gx - 1), ty = threadIdx.x / gx;
    const int g = blockIdx.y * gx + tx;
    const int b = blockIdx.x;
    const double scale = (double)*grad_loss / (double)B;
    const int64_t t = target[b];
    if (blockIdx.y == 0 && threadIdx.x < K) dlogits[(size_t)b * K + threadIdx.x] = head_dlogit(probs, t, b, threadIdx.x, K, scale);
    if (g >= G) return;
    float v[N];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = 0.f;
    for (int k = 0; k < K; k++) {
        const float d = head_dlogit(probs, t, b, k, K, scale);
        const float* w = weight + (size_t)k * C + (size_t)g * N;
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            float wv[4];
            Group<float>::load(w + 4 * q, wv);
#pragma unroll
            for (int i = 0; i < 4; i++) v[4 * q + i] = __builtin_fmaf(d, wv[i], v[4 * q + i]);
        }
    }
    const float hw = (float)HW;
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = v[i] / hw;
    T* out = dx + (size_t)b * HW * C + (size_t)g * N;
    for (int r = ty; r < HW; r += ry) Group<T>::store(out + (size_t)r * C, v);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int check_head_desc(const salve_head_desc_t* d, const char* who) {
    if (!d) { salve_fail(who); return SALVE_ERR_BAD_ARG; }
    if (d->B < 1 || d->B > 65535) { salve_fail("head: B must be from 1 to 65535"); return SALVE_ERR_BAD_ARG; }
    if (d->HW < 1 || d->HW > 1024) { salve_fail("head: HW must be from 1 to 1024"); return SALVE_ERR_BAD_ARG; }
    if (d->C < 8 || d->C > 4096 || d->C % 8 != 0) { salve_fail("head: C must be a multiple of 8 from 8 to 4096"); return SALVE_ERR_BAD_ARG; }
    if (d->K < 2 || d->K > HEAD_MAX_K) { salve_fail("head: K must be from 2 to 16"); return SALVE_ERR_BAD_ARG; }
    if (d->flags & ~SALVE_HEAD_ACCUMULATE_LOSS) { salve_fail("head: unknown flag bit"); return SALVE_ERR_BAD_ARG; }
    return SALVE_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

size_t head_ws(const salve_head_desc_t* d, int pass) {
    if (pass == SALVE_HEAD_BWD) return 256;   // (nothing is kept there; 0 means refused)
    return align256((size_t)d->B * 8) + align256((size_t)d->B * 4) + 256;
}

template <typename T>
int head_forward(const char* who, const salve_head_desc_t* d, const T* x, const float* weight, const float* bias, const int64_t* target,
                 float* pooled, float* logits, float* probs, float* loss, salve_head_meter_t* meter, void* ws, size_t ws_bytes, void* stream) {
    int st = check_head_desc(d, who);
    if (st != SALVE_OK) return st;
    if (!x || !weight || !bias || !target || !pooled || !logits || !probs || !loss || !ws) { salve_fail("salve_head_*_forward: null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!aligned(x, 16) || !aligned(weight, 16) || !aligned(pooled, 16) || !aligned(target, 8) || !aligned(meter, 8) || !aligned(bias, 4) ||
        !aligned(logits, 4) || !aligned(probs, 4) || !aligned(loss, 4)) {
        salve_fail("salve_head_*_forward: x, weight and pooled must be 16-byte aligned, target and the meter record 8-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    if (ws_bytes < head_ws(d, SALVE_HEAD_FWD)) { salve_fail("salve_head_*_forward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    const Geom g = geometry(d->C, Group<T>::N);
    hipStream_t s = (hipStream_t)stream;
    double* rowloss = reinterpret_cast<double*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    int32_t* rowinfo = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(rowloss) + align256((size_t)d->B * 8));
    hipLaunchKernelGGL(head_pool_kernel<T>, dim3((unsigned)d->B, (unsigned)g.ctiles), dim3(HEAD_THREADS), 0, s, x, pooled, d->HW, d->C, g.G, g.gx);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_logits_kernel, dim3((unsigned)d->B), dim3(HEAD_THREADS), 0, s, pooled, weight, bias, target, logits, probs, rowloss, rowinfo,
                       d->C, d->K);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_finish_kernel, dim3(1), dim3(HEAD_THREADS), 0, s, rowloss, rowinfo, d->B, d->K, d->flags & SALVE_HEAD_ACCUMULATE_LOSS, loss, meter);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

template <typename T>
int head_backward(const char* who, const salve_head_desc_t* d, const float* pooled, const float* probs, const int64_t* target, const float* weight,
                  const float* grad_loss, float* dlogits, float* dw, float* db, T* dx, void* ws, size_t ws_bytes, void* stream) {
    int st = check_head_desc(d, who);
    if (st != SALVE_OK) return st;
    if (!pooled || !probs || !target || !weight || !grad_loss || !dlogits || !dw || !db || !dx || !ws) { salve_fail("salve_head_*_backward: null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!aligned(dx, 16) || !aligned(weight, 16) || !aligned(target, 8) || !aligned(pooled, 4) || !aligned(probs, 4) || !aligned(grad_loss, 4) ||
        !aligned(dlogits, 4) || !aligned(dw, 4) || !aligned(db, 4)) {
        salve_fail("salve_head_*_backward: dx and weight must be 16-byte aligned, target 8-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    if (ws_bytes < head_ws(d, SALVE_HEAD_BWD)) { salve_fail("salve_head_*_backward: workspace too small"); return SALVE_ERR_WORKSPACE; }
    const Geom g = geometry(d->C, Group<T>::N);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(head_dw_kernel, dim3((unsigned)((d->C + 1 + HEAD_DW_COLS - 1) / HEAD_DW_COLS)), dim3(HEAD_THREADS), 0, s, pooled, probs, target,
                       grad_loss, dw, db, d->B, d->C, d->K);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(head_dx_kernel<T>, dim3((unsigned)d->B, (unsigned)g.ctiles), dim3(HEAD_THREADS), 0, s, probs, target, weight, grad_loss, dlogits, dx,
                       d->B, d->HW, d->C, d->K, g.G, g.gx);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace

extern "C" {

size_t salve_head_workspace_bytes(const salve_head_desc_t* d, int32_t pass) {
    if (check_head_desc(d, "salve_head_workspace_bytes: null descriptor") != SALVE_OK) return 0;
    if (pass != SALVE_HEAD_FWD && pass != SALVE_HEAD_BWD) { salve_fail("salve_head_workspace_bytes: pass must be SALVE_HEAD_FWD or SALVE_HEAD_BWD"); return 0; }
    return head_ws(d, pass);
}

int salve_head_f32_forward(const salve_head_desc_t* d, const float* x, const float* weight, const float* bias, const int64_t* target, float* pooled,
                           float* logits, float* probs, float* loss, salve_head_meter_t* meter, void* ws, size_t ws_bytes, void* stream) {
    return head_forward<float>("salve_head_f32_forward: null descriptor", d, x, weight, bias, target, pooled, logits, probs, loss, meter, ws, ws_bytes,
                               stream);
}

int salve_head_bf16_forward(const salve_head_desc_t* d, const uint16_t* x, const float* weight, const float* bias, const int64_t* target, float* pooled,
                            float* logits, float* probs, float* loss, salve_head_meter_t* meter, void* ws, size_t ws_bytes, void* stream) {
    return head_forward<uint16_t>("salve_head_bf16_forward: null descriptor", d, x, weight, bias, target, pooled, logits, probs, loss, meter, ws,
                                  ws_bytes, stream);
}

int salve_head_f32_backward(const salve_head_desc_t* d, const float* pooled, const float* probs, const int64_t* target, const float* weight,
                            const float* grad_loss, float* dlogits, float* dw, float* db, float* dx, void* ws, size_t ws_bytes, void* stream) {
    return head_backward<float>("salve_head_f32_backward: null descriptor", d, pooled, probs, target, weight, grad_loss, dlogits, dw, db, dx, ws,
                                ws_bytes, stream);
}

int salve_head_bf16_backward(const salve_head_desc_t* d, const float* pooled, const float* probs, const int64_t* target, const float* weight,
                             const float* grad_loss, float* dlogits, float* dw, float* db, uint16_t* dx, void* ws, size_t ws_bytes, void* stream) {
    return head_backward<uint16_t>("salve_head_bf16_backward: null descriptor", d, pooled, probs, target, weight, grad_loss, dlogits, dw, db, dx, ws,
                                   ws_bytes, stream);
}

}  // extern "C"
