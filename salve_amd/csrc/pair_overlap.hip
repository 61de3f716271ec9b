// pair_overlap.hip -- the visual overlap of BEV image pairs for gfx950 (MI355X): per job the number of pixels occupied in both images, in
// either, in the first and in the second.  Compile with -ffp-contract=off -fno-slp-vectorize (integers only; the flags are the default of
// the exact-arithmetic files).
//
// The reference computes this on the host from the two tile FILES of a scored pair: scripts/measure_acc_vs_overlap.py:77-80 reads them back
// and calls salve/utils/iou_utils.py:14-37 -- occupied = np.amax(f, axis=2) > 0, IoU = |and| / (|or| + 1e-12).  Here both images are still in
// device memory as 0x00BBGGRR words, so occupied is (pixel & 0x00FFFFFF) != 0 and the four counts are exact integers; the division stays
// with the caller (salve_amd/overlap.py).
//
//   pair_overlap_kernel   salve_bev_pair_overlap: one workgroup of 256 threads per job
//
// Bound: reading 2 * h * w * 4 bytes per job, once (a posed render from HBM, the identity render it is compared with usually from the L2 or
// the Infinity Cache: many jobs share it).  One workgroup per job: a launch of the fused path has thousands of jobs, so the CUs are full
// without splitting a job, and a job's four counts are summed in ONE fixed order -- lane, wave (shuffles), workgroup (LDS) -- with no atomic
// and no second launch: the same bytes on every run.
//
// Alignment: an image is only 4-byte aligned (501 * 501 is odd: image k starts at k * 1 004 004 bytes), and the two images of a job have
// different residues mod 16.  Each image is therefore cut into 16-byte CHUNKS on its OWN grid: chunk k of an image whose first aligned pixel
// is pixel `head` (0..3) holds pixels head + 4 k .. head + 4 k + 3; chunk -1 is the partial head, the last chunk the partial tail.  Whole
// chunks are one aligned 16-byte load, partial ones are read pixel by pixel, and a pixel outside [0, h * w) is never read and counts as
// empty.  A chunk becomes a 4-bit occupancy mask.  The job is walked on a's grid; the pixels of a's chunk k lie in b's chunks m = k + s and
// m + 1 at bit offset d, with d = (head_a - head_b) mod 4 and s = floor((head_a - head_b) / 4): b's aligned masks are brought onto a's grid
// by ((mask_b(m) | mask_b(m + 1) << 4) >> d) & 15, where mask_b(m + 1) is the next lane's mask (a shuffle), not a second load.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int OVERLAP_THREADS = 256;                       // 4 waves
constexpr int OVERLAP_UNROLL = 4;                          // chunks per lane and step: 2 * 4 16-byte loads in flight before the first compare
constexpr int OVERLAP_WAVE_SPAN = 64 * OVERLAP_UNROLL;     // consecutive chunks one wave takes per step

__device__ __forceinline__ uint32_t occupied4(const uint4 v) {
    return ((v.x & 0x00FFFFFFu) ? 1u : 0u) | ((v.y & 0x00FFFFFFu) ? 2u : 0u) | ((v.z & 0x00FFFFFFu) ? 4u : 0u) | ((v.w & 0x00FFFFFFu) ? 8u : 0u);
}

// The occupancy mask of chunk k of an image with `head` pixels in front of its first 16-byte boundary: bit i = pixel head + 4 k + i.  A whole
// chunk is one aligned load; a partial one (the head, the tail, or a chunk outside the image altogether) reads only its pixels inside [0, HW).
__device__ __forceinline__ uint32_t chunk_mask(const uint32_t* __restrict__ img, int head, int k, long long HW) {
    const long long p0 = (long long)head + 4LL * k;
    if (p0 >= 0 && p0 + 3 < HW) return occupied4(*reinterpret_cast<const uint4*>(img + p0));
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const long long p = p0 + i;
        if (p >= 0 && p < HW && (img[p] & 0x00FFFFFFu)) m |= 1u << i;
    }
    return m;
}

__global__ __launch_bounds__(OVERLAP_THREADS) void pair_overlap_kernel(const uint32_t* __restrict__ bev_a, int n_bev_a, const uint32_t* __restrict__ bev_b,
                                                                       int n_bev_b, long long HW, const salve_overlap_job_t* __restrict__ jobs,
                                                                       int4* __restrict__ out, int32_t* __restrict__ status) {
    const int job = blockIdx.x;
    const salve_overlap_job_t jb = jobs[job];
    // the table is device memory: checked here, before any address is formed (workgroup-uniform)
    if (jb.a < 0 || jb.a >= n_bev_a || jb.b < 0 || jb.b >= n_bev_b) {
        if (threadIdx.x == 0) {
            out[job] = make_int4(-1, -1, -1, -1);
            if (status) atomicOr(status, SALVE_STATUS_BAD_TILE_JOB);
        }
        return;
    }
    const uint32_t* __restrict__ a = bev_a + (size_t)jb.a * (size_t)HW;
    const uint32_t* __restrict__ b = bev_b + (size_t)jb.b * (size_t)HW;
    // pixels in front of each image's first 16-byte boundary (the arrays are 4-byte aligned: checked on the host)
    const int head_a = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u) >> 2);
    const int head_b = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(b) & 15u)) & 15u) >> 2);
    const int d = (head_a - head_b) & 3, s = (head_a - head_b - d) / 4;   // s = -1 or 0
    const int k_first = head_a > 0 ? -1 : 0;                               // a's chunks: k_first .. k_last, the whole ones 0 .. k_whole_*
    const int k_last = (int)((HW - 1 - head_a) >> 2);                      // (arithmetic shift: -1 for an image that ends inside its head)
    const int k_whole_a = (int)((HW - head_a - 4) >> 2), k_whole_b = (int)((HW - head_b - 4) >> 2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t n_and = 0, n_a = 0, n_b = 0;
    for (int base = k_first + wave * OVERLAP_WAVE_SPAN; base <= k_last; base += (OVERLAP_THREADS / 64) * OVERLAP_WAVE_SPAN) {
        uint32_t ma[OVERLAP_UNROLL], mb[OVERLAP_UNROLL], mb_next[OVERLAP_UNROLL];
        // (wave-uniform) every chunk of the step, b's one-past-the-span included, is a whole chunk: plain aligned loads, all issued first
        if (base >= 0 && base + OVERLAP_WAVE_SPAN - 1 <= k_whole_a && base + s >= 0 && base + s + OVERLAP_WAVE_SPAN <= k_whole_b) {
            uint4 va[OVERLAP_UNROLL], vb[OVERLAP_UNROLL];
            const uint4* pa = reinterpret_cast<const uint4*>(a + head_a) + base + lane;
            const uint4* pb = reinterpret_cast<const uint4*>(b + head_b) + (base + s) + lane;
#pragma unroll
            for (int u = 0; u < OVERLAP_UNROLL; u++) va[u] = pa[u * 64];
#pragma unroll
            for (int u = 0; u < OVERLAP_UNROLL; u++) vb[u] = pb[u * 64];
            uint32_t beyond = 0;   // b's chunk behind the wave's span: lane 63 of the last row has no next lane to ask
            if (d != 0 && lane == 63) beyond = occupied4(pb[OVERLAP_UNROLL * 64 - 63]);
#pragma unroll
            for (int u = 0; u < OVERLAP_UNROLL; u++) {
                ma[u] = occupied4(va[u]);
                mb[u] = occupied4(vb[u]);
            }
#pragma unroll
            for (int u = 0; u < OVERLAP_UNROLL; u++) {
                const uint32_t right = __shfl_down(mb[u], 1, 64);                                                 // chunk m + 1 for lanes 0 .. 62
                const uint32_t wrap = u + 1 < OVERLAP_UNROLL ? __shfl(mb[(u + 1) % OVERLAP_UNROLL], 0, 64) : beyond;   // for lane 63: lane 0 of the next row
                mb_next[u] = lane < 63 ? right : wrap;
            }
        } else {   // a step that touches a partial chunk or the end of an image: guarded reads
#pragma unroll
            for (int u = 0; u < OVERLAP_UNROLL; u++) {
                const int k = base + u * 64 + lane;
                ma[u] = chunk_mask(a, head_a, k, HW);
                mb[u] = chunk_mask(b, head_b, k + s, HW);
                mb_next[u] = d != 0 ? chunk_mask(b, head_b, k + s + 1, HW) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < OVERLAP_UNROLL; u++) {
            const uint32_t on_a_grid = ((mb[u] | (mb_next[u] << 4)) >> d) & 15u;
            n_and += __popc(ma[u] & on_a_grid);
            n_a += __popc(ma[u]);
            n_b += __popc(on_a_grid);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_and += __shfl_down(n_and, o, 64);
        n_a += __shfl_down(n_a, o, 64);
        n_b += __shfl_down(n_b, o, 64);
    }
    __shared__ uint32_t part[OVERLAP_THREADS / 64][3];
    if (lane == 0) {
        part[wave][0] = n_and;
        part[wave][1] = n_a;
        part[wave][2] = n_b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t_and = 0, t_a = 0, t_b = 0;
#pragma unroll
        for (int w = 0; w < OVERLAP_THREADS / 64; w++) {
            t_and += part[w][0];
            t_a += part[w][1];
            t_b += part[w][2];
        }
        out[job] = make_int4((int)t_and, (int)(t_a + t_b - t_and), (int)t_a, (int)t_b);   // ONE 16-byte store per row
    }
}

}  // namespace

extern "C" {

int salve_bev_pair_overlap(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                           const salve_overlap_job_t* jobs, int32_t n_jobs, int32_t* out, int32_t* status, void* stream) {
    if (bev_h < 1 || bev_w < 1) { salve_fail("salve_bev_pair_overlap: bev_h and bev_w must be at least 1"); return SALVE_ERR_BAD_ARG; }
    if ((long long)bev_h * bev_w >= (1LL << 31)) { salve_fail("salve_bev_pair_overlap: bev_h * bev_w must stay below 2^31 (the counts are int32)"); return SALVE_ERR_BAD_ARG; }
    if (n_bev_a < 0 || n_bev_b < 0 || n_jobs < 0) { salve_fail("salve_bev_pair_overlap: negative count"); return SALVE_ERR_BAD_ARG; }
    if (n_jobs == 0) return SALVE_OK;
    if (!jobs || !out || !bev_a || !bev_b) { salve_fail("salve_bev_pair_overlap: null pointer"); return SALVE_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0 || reinterpret_cast<uintptr_t>(bev_a) % 4 != 0 || reinterpret_cast<uintptr_t>(bev_b) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(jobs) % 4 != 0) {
        salve_fail("salve_bev_pair_overlap: out must be 16-byte aligned, the images and the job table 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(pair_overlap_kernel, dim3((unsigned)n_jobs), dim3(OVERLAP_THREADS), 0, (hipStream_t)stream, bev_a, n_bev_a, bev_b, n_bev_b,
                       (long long)bev_h * bev_w, jobs, reinterpret_cast<int4*>(out), status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
