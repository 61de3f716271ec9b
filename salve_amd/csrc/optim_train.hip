// optim_train.hip -- Adam for gfx950 (MI355X) over every parameter tensor of a model in ONE launch, writing the bf16 copy of a
// weight that the bf16 training convolutions read while the new value is still in registers (opt-in: salve_amd/optim.py: HipAdam,
// `--optim hip`).
//
// A table-driven multi-tensor kernel: the device table holds one salve_adam_segment_t per parameter tensor (pointers, length and
// the step's scalars), the chunk map one (segment, offset) per workgroup.  A workgroup of 256 threads owns SALVE_ADAM_CHUNK
// consecutive elements of one segment.  This is a bandwidth kernel: where the segment's four fp32 pointers are 16-byte aligned
// at the chunk's offset (and the bf16 copy 8-byte aligned) every lane moves 16 bytes per load and store, and a full chunk has
// all of its sixteen loads per lane in flight before the first store; otherwise, and for the last n % 4 elements, elements
// go one by one.  No atomics, no LDS, every element is touched by exactly one thread: the same inputs give bit-identical outputs.
// Element offsets are 64-bit.
//
// The arithmetic is torch.optim.Adam's (amsgrad=False, maximize=False, L2 weight decay), all fp32.  The operation order and the
// three fused multiply-adds are those of torch's own fp32 kernels on the CPU (add with alpha, lerp, addcmul, addcdiv), so the
// two round alike; the file is built with -ffp-contract=off and every fma below is spelled out, nothing else is contracted:
//     g   = fma(weight_decay, p, g)                    (skipped when weight_decay == 0, so a non-finite p is not multiplied by 0)
//     m   = fma(1 - beta1, g - m, m)                   (the first moment, torch's lerp)
//     v   = fma((1 - beta2) * g, g, v * beta2)         (the second moment)
//     den = sqrt(v) / sqrt(1 - beta2^t) + eps
//     p   = p - (step_size * m) / den                  (step_size = lr / (1 - beta1^t))
// sqrt and the divisions are correctly rounded (a bandwidth kernel has the cycles).  The host computes step_size,
// sqrt(1 - beta2^t), 1 - beta1 and 1 - beta2 in double and rounds them to fp32 once (1 - beta2 formed in fp32 from the rounded
// beta2 would be wrong by 6e-5 relative).
// The bf16 copy is the new p rounded to nearest even, infinities kept, a NaN stored as 0x7FC0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC_PER_THREAD = SALVE_ADAM_CHUNK / (4 * ADAM_THREADS);   // 16-byte groups a lane owns in a full chunk
static_assert(SALVE_ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a full chunk is a whole number of 16-byte groups per lane");
static_assert(sizeof(salve_adam_segment_t) == 80 && sizeof(salve_adam_chunk_t) == 16, "the table layout salve_hip.h documents");

struct Scalars {
    float step_size, sqrt_bc2, beta2, w1, w2, eps, wd;
};

// the operation order of the header comment
__device__ __forceinline__ float adam_update(float p, float g, float& m, float& v, const Scalars& s) {
    if (s.wd != 0.f) g = __builtin_fmaf(s.wd, p, g);
    m = __builtin_fmaf(s.w1, g - m, m);
    v = __builtin_fmaf(s.w2 * g, g, v * s.beta2);
    const float den = sqrtf(v) / s.sqrt_bc2 + s.eps;
    return p - (s.step_size * m) / den;
}

// fp32 -> bf16 bits, round to nearest even in integers (denormals included, whatever the wave's denormal mode); +-inf unchanged
__device__ __forceinline__ uint32_t bf16_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void adam_group(float4& p, const float4& g, float4& m, float4& v, const Scalars& s) {
    p.x = adam_update(p.x, g.x, m.x, v.x, s);
    p.y = adam_update(p.y, g.y, m.y, v.y, s);
    p.z = adam_update(p.z, g.z, m.z, v.z, s);
    p.w = adam_update(p.w, g.w, m.w, v.w, s);
}

__device__ __forceinline__ uint2 bf16_group(const float4& p) {
    return make_uint2(bf16_bits(p.x) | (bf16_bits(p.y) << 16), bf16_bits(p.z) | (bf16_bits(p.w) << 16));
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(const salve_adam_segment_t* __restrict__ table, int n_segments,
                                                            const salve_adam_chunk_t* __restrict__ chunk_map) {
    const salve_adam_chunk_t c = chunk_map[blockIdx.x];
    if (c.segment < 0 || c.segment >= n_segments) return;   // (uniform: the whole workgroup leaves)
    const salve_adam_segment_t seg = table[c.segment];
    if (c.offset < 0 || c.offset >= seg.n) return;
    const int64_t left = seg.n - c.offset;
    const int len = left < SALVE_ADAM_CHUNK ? (int)left : SALVE_ADAM_CHUNK;
    float* __restrict__ p = seg.param + c.offset;
    const float* __restrict__ g = seg.grad + c.offset;
    float* __restrict__ m = seg.exp_avg + c.offset;
    float* __restrict__ v = seg.exp_avg_sq + c.offset;
    uint16_t* __restrict__ sh = seg.shadow_bf16 ? seg.shadow_bf16 + c.offset : nullptr;
    const Scalars s = {seg.step_size, seg.sqrt_bc2, seg.beta2, seg.one_minus_beta1, seg.one_minus_beta2, seg.eps, seg.weight_decay};
    const int tid = threadIdx.x;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && ((uintptr_t)sh & 7) == 0;
    if (!vec) {   // 4-byte aligned only: one element per lane and pass
        for (int i = tid; i < len; i += ADAM_THREADS) {
            float mi = m[i], vi = v[i];
            const float pi = adam_update(p[i], g[i], mi, vi, s);
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
            if (sh) sh[i] = (uint16_t)bf16_bits(pi);
        }
        return;
    }
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    uint2* s2 = reinterpret_cast<uint2*>(sh);
    if (len == SALVE_ADAM_CHUNK) {   // a full chunk: every load of the lane is issued before its first store
        float4 pv[ADAM_VEC_PER_THREAD], gv[ADAM_VEC_PER_THREAD], mv[ADAM_VEC_PER_THREAD], vv[ADAM_VEC_PER_THREAD];
#pragma unroll
        for (int u = 0; u < ADAM_VEC_PER_THREAD; u++) {
            const int i = tid + u * ADAM_THREADS;
            pv[u] = p4[i];
            gv[u] = g4[i];
            mv[u] = m4[i];
            vv[u] = v4[i];
        }
#pragma unroll
        for (int u = 0; u < ADAM_VEC_PER_THREAD; u++) {
            const int i = tid + u * ADAM_THREADS;
            adam_group(pv[u], gv[u], mv[u], vv[u], s);
            p4[i] = pv[u];
            m4[i] = mv[u];
            v4[i] = vv[u];
            if (s2) s2[i] = bf16_group(pv[u]);
        }
        return;
    }
    const int nv = len >> 2;
    for (int i = tid; i < nv; i += ADAM_THREADS) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i];
        const float4 gv = g4[i];
        adam_group(pv, gv, mv, vv, s);
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
        if (s2) s2[i] = bf16_group(pv);
    }
    const int i = (nv << 2) + tid;   // the last len % 4 elements
    if (i < len) {
        float mi = m[i], vi = v[i];
        const float pi = adam_update(p[i], g[i], mi, vi, s);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (sh) sh[i] = (uint16_t)bf16_bits(pi);
    }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int salve_adam_step(const salve_adam_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                    const salve_adam_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, void* stream) {
    if (!table || n_segments < 0 || n_chunks < 0 || (n_chunks > 0 && (!chunk_map || n_segments == 0))) {
        salve_fail("salve_adam_step: null table or chunk map, or a negative count");
        return SALVE_ERR_BAD_ARG;
    }
    if (!aligned(table, 8) || !aligned(chunk_map, 8)) { salve_fail("salve_adam_step: the table and the chunk map must be 8-byte aligned"); return SALVE_ERR_BAD_ARG; }
    if (host_table) {
        for (int32_t i = 0; i < n_segments; i++) {
            const salve_adam_segment_t& s = host_table[i];
            if (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq || s.n < 0 || !aligned(s.param, 4) || !aligned(s.grad, 4) ||
                !aligned(s.exp_avg, 4) || !aligned(s.exp_avg_sq, 4) || !aligned(s.shadow_bf16, 2)) {
                salve_fail("salve_adam_step: a segment with a null or misaligned pointer or a negative length");
                return SALVE_ERR_BAD_ARG;
            }
        }
        if (host_chunk_map) {
            for (int32_t i = 0; i < n_chunks; i++) {
                const salve_adam_chunk_t& c = host_chunk_map[i];
                if (c.segment < 0 || c.segment >= n_segments || c.offset < 0 || c.offset % SALVE_ADAM_CHUNK != 0 || c.offset >= host_table[c.segment].n) {
                    salve_fail("salve_adam_step: a chunk names a segment outside the table or an offset outside its segment");
                    return SALVE_ERR_BAD_ARG;
                }
            }
        }
    }
    if (n_chunks == 0) return SALVE_OK;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, table, (int)n_segments, chunk_map);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
