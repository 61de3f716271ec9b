// flat_bucket.hip -- gather any number of fp32 tensors into one flat buffer, or scatter the buffer back, in ONE launch (gfx950):
// the bucket of data-parallel training (salve_amd/dist_train.py: FlatBucket).  Every step's gradients -- some hundred tensors from
// 64 to 2.4 M elements -- are packed, scaled by 1 / world, into the buffer that the one all-reduce of the step then sums.
//
// Table-driven like optim_train.hip, whose chunk map it shares: the device table holds one salve_flat_segment_t per tensor
// (address, length, first element inside the flat buffer), the chunk map one (segment, offset) per workgroup.  A workgroup of 256
// threads owns SALVE_ADAM_CHUNK consecutive elements of one segment.  A streaming copy: the flat side of a chunk is 16-byte aligned
// by contract (the buffer is, segment offsets are multiples of 4 elements, chunk offsets multiples of the chunk), so where the
// tensor's address at the chunk is 16-byte aligned too every lane moves 16 bytes per load and store, and a full chunk has its four
// loads per lane in flight before the first store; a tensor that is only 4-byte aligned, and the last n % 4 elements, go element by
// element.  Every element is moved by exactly one thread; the padding between segments is never read or written.  Element offsets
// are 64-bit.
//
// scale == 1: the elements move as 32-bit words and no arithmetic touches them -- NaN payloads, infinities, -0 and denormals arrive
// as they left.  Any other scale: one fp32 multiply per element (the file is built with -ffp-contract=off; there is nothing to
// contract).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int FLAT_THREADS = 256;
constexpr int FLAT_VEC_PER_THREAD = SALVE_ADAM_CHUNK / (4 * FLAT_THREADS);   // 16-byte groups a lane owns in a full chunk
static_assert(SALVE_ADAM_CHUNK % (4 * FLAT_THREADS) == 0, "a full chunk is a whole number of 16-byte groups per lane");
static_assert(sizeof(salve_flat_segment_t) == 24 && sizeof(salve_adam_chunk_t) == 16, "the table layout salve_hip.h documents");

template <bool SCALED>
__device__ __forceinline__ uint32_t move(uint32_t bits, float scale) {
    if (!SCALED) return bits;
    return __float_as_uint(__uint_as_float(bits) * scale);
}

template <bool SCALED>
__device__ __forceinline__ uint4 move4(uint4 v, float scale) {
    return make_uint4(move<SCALED>(v.x, scale), move<SCALED>(v.y, scale), move<SCALED>(v.z, scale), move<SCALED>(v.w, scale));
}

// PACK: tensor -> flat; otherwise flat -> tensor
template <bool PACK, bool SCALED>
__global__ __launch_bounds__(FLAT_THREADS) void flat_kernel(const salve_flat_segment_t* __restrict__ table, int n_segments,
                                                            const salve_adam_chunk_t* __restrict__ chunk_map, uint32_t* flat,
                                                            int64_t flat_elems, float scale) {
    const salve_adam_chunk_t c = chunk_map[blockIdx.x];
    if (c.segment < 0 || c.segment >= n_segments) return;   // (uniform: the whole workgroup leaves)
    const salve_flat_segment_t seg = table[c.segment];
    if (c.offset < 0 || c.offset >= seg.n || seg.offset < 0 || seg.offset > flat_elems || seg.n > flat_elems - seg.offset) return;
    const int64_t left = seg.n - c.offset;
    const int len = left < SALVE_ADAM_CHUNK ? (int)left : SALVE_ADAM_CHUNK;
    uint32_t* t = reinterpret_cast<uint32_t*>(seg.tensor) + c.offset;
    uint32_t* f = flat + seg.offset + c.offset;
    const uint32_t* src = PACK ? t : f;   // (no __restrict__: a tensor may be its own view of the buffer -- then every element moves onto itself)
    uint32_t* dst = PACK ? f : t;
    const int tid = threadIdx.x;
    if ((((uintptr_t)t | (uintptr_t)f) & 15) != 0) {   // 4-byte aligned only: one element per lane and pass
        for (int i = tid; i < len; i += FLAT_THREADS) dst[i] = move<SCALED>(src[i], scale);
        return;
    }
    const uint4* src4 = reinterpret_cast<const uint4*>(src);
    uint4* dst4 = reinterpret_cast<uint4*>(dst);
    if (len == SALVE_ADAM_CHUNK) {   // a full chunk: every load of the lane is issued before its first store
        uint4 v[FLAT_VEC_PER_THREAD];
#pragma unroll
        for (int u = 0; u < FLAT_VEC_PER_THREAD; u++) v[u] = src4[tid + u * FLAT_THREADS];
#pragma unroll
        for (int u = 0; u < FLAT_VEC_PER_THREAD; u++) dst4[tid + u * FLAT_THREADS] = move4<SCALED>(v[u], scale);
        return;
    }
    const int nv = len >> 2;
    for (int i = tid; i < nv; i += FLAT_THREADS) dst4[i] = move4<SCALED>(src4[i], scale);
    const int i = (nv << 2) + tid;   // the last len % 4 elements
    if (i < len) dst[i] = move<SCALED>(src[i], scale);
}

// Every refusal, from the host copies of the tables; nothing is launched before all of them have passed.
int validate(const char* who, const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
             const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, const float* flat, int64_t flat_elems) {
    char msg[160];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof(msg), "%s: %s", who, what);
        salve_fail(msg);
        return (int)SALVE_ERR_BAD_ARG;
    };
    if (n_segments < 0 || n_chunks < 0 || flat_elems < 0) return fail("a negative count");
    if (n_segments == 0) return n_chunks == 0 ? (int)SALVE_OK : fail("chunks without a segment");
    if (!table || !host_table) return fail("null table (the device table and its host copy are both required)");
    if (n_chunks > 0 && (!chunk_map || !host_chunk_map)) return fail("null chunk map (the device map and its host copy are both required)");
    if (((uintptr_t)table & 7) != 0 || ((uintptr_t)chunk_map & 7) != 0) return fail("the table and the chunk map must be 8-byte aligned");
    if (((uintptr_t)flat & 15) != 0) return fail("the flat buffer must be 16-byte aligned");
    int64_t end = 0;      // one past the last element of the segments so far
    int64_t chunk = 0;    // the next chunk of the map
    for (int32_t i = 0; i < n_segments; i++) {
        const salve_flat_segment_t& s = host_table[i];
        if (s.n < 0) return fail("a segment with a negative length");
        if (s.offset < 0 || s.offset % 4 != 0) return fail("a segment offset that is negative or not a multiple of 4");
        if (s.offset < end) return fail("segment offsets descend or segments overlap");
        if (s.offset > flat_elems || s.n > flat_elems - s.offset) return fail("a segment reaches past the end of the flat buffer");
        if (s.n > 0 && (!s.tensor || !flat)) return fail("a null pointer for a segment that has elements");
        if ((s.tensor & 3) != 0) return fail("a tensor address that is not 4-byte aligned");
        end = s.offset + s.n;
        for (int64_t o = 0; o < s.n; o += SALVE_ADAM_CHUNK, chunk++) {   // the map is the segments' chunks in table order, each once
            if (chunk >= n_chunks || host_chunk_map[chunk].segment != i || host_chunk_map[chunk].offset != o)
                return fail("the chunk map does not match the table");
        }
    }
    if (chunk != n_chunks) return fail("the chunk map does not match the table");
    return SALVE_OK;
}

template <bool PACK>
int launch(const char* who, const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
           const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, float* flat, int64_t flat_elems, float scale,
           void* stream) {
    const int st = validate(who, table, n_segments, chunk_map, n_chunks, host_table, host_chunk_map, flat, flat_elems);
    if (st != SALVE_OK) return st;
    if (n_segments == 0 || n_chunks == 0) return SALVE_OK;
    uint32_t* words = reinterpret_cast<uint32_t*>(flat);
    if (scale == 1.0f)
        hipLaunchKernelGGL((flat_kernel<PACK, false>), dim3((unsigned)n_chunks), dim3(FLAT_THREADS), 0, (hipStream_t)stream, table, (int)n_segments,
                           chunk_map, words, flat_elems, scale);
    else
        hipLaunchKernelGGL((flat_kernel<PACK, true>), dim3((unsigned)n_chunks), dim3(FLAT_THREADS), 0, (hipStream_t)stream, table, (int)n_segments,
                           chunk_map, words, flat_elems, scale);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace

extern "C" {

int salve_flat_pack(const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                    const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, float* flat, int64_t flat_elems, float scale,
                    void* stream) {
    return launch<true>("salve_flat_pack", table, n_segments, chunk_map, n_chunks, host_table, host_chunk_map, flat, flat_elems, scale, stream);
}

int salve_flat_unpack(const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                      const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, float* flat, int64_t flat_elems, float scale,
                      void* stream) {
    return launch<false>("salve_flat_unpack", table, n_segments, chunk_map, n_chunks, host_table, host_chunk_map, flat, flat_elems, scale, stream);
}

}  // extern "C"
