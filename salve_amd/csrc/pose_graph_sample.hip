// pose_graph_sample.hip -- RANSAC over random spanning trees for gfx950 (MI355X): every hypothesis (a subset of a floor's thresholded
// measurements, drawn on the host) -> its edges -> the largest component -> a BFS tree and one Sim(2) pose per panorama -> the mean
// disagreement of those poses with ALL thresholded measurements of the floor; then per floor the reference's scan for the best hypothesis.
// Any number of floors and hypotheses in ONE call of two launches.  Compile with -ffp-contract=off -fno-slp-vectorize (pose_graph_common.h).
//
// The reference does this per floor on the host, in salve/algorithms/spanning_tree.py (method `random_spanning_trees` of scripts/run_sfm.py):
//   :179-334  ransac_spanning_trees                    the hypotheses' edges (phase A'), the scan (launch 2)
//   :73-141   greedily_construct_st_Sim2               phases C, D (pose_graph_common.h, shared with pose_graph.hip)
//   :337-384  compute_hypothesis_errors                phase E
//   :144-176  compute_objective_function_improvement   launch 2
// include/salve_hip.h (salve_pose_graph_sample_trees) states the rules; this file states how they run.
//
//   sample_trees_kernel   launch 1: one workgroup of 256 threads per hypothesis, the hypothesis's graph in LDS (pose_graph.hip's layout, of which
//                         `adj` lies idle, and 256 doubles behind it for the sums: 161 312 bytes of the 160 KiB at max_nodes = 256)
//   sample_pick_kernel    launch 2: one workgroup per floor; one thread scans the floor's hypotheses in order, all copy the winner out
//
// A workgroup finds its floor by itself: hypothesis h belongs to the LOWEST floor f whose extent hyp_start[f] .. hyp_start[f + 1] - 1 is well
// formed and holds h (a scan of hyp_start by the 256 threads and an integer LDS minimum -- a binary search would trust a table that a malformed
// floor may have broken for its sound neighbours).  Launch 2 verifies every table again for its floor, and that launch 1 evaluated each of the
// floor's hypotheses for THIS floor: a floor whose extent overlaps a lower floor's is malformed.
//
// The sums of phase E are float64 in one stated order -- thread t adds its rows lo + t, lo + t + 256, ... ascending from 0.0, the 256 partial
// sums are folded by halving (p[t] += p[t + 128], then 64, ... 1) -- and no floating-point atomic exists anywhere, so every output is the same
// bytes on every run.  A NaN average is written as the one quiet NaN 0x7FF8000000000000.
//
// Bound: one floor's hundred hypotheses are latency-bound per workgroup, as pose_graph.hip -- the chains of barriers of phases C and D, then
// one pass over the floor's rows (48 bytes each, L2-resident after the floor's first hypothesis) with two atan2f and one float64 fmod per
// measured row, and the 8 + 8 barriers of the two folds: 0.09 ms for 100 hypotheses on 64 panoramas and 2048 rows, beside 0.07 ms for
// pose_graph_kernel's one workgroup on the same rows (profiles/r20_pose_graph_sample.txt).  What differs is the width: hypotheses x floors
// independent workgroups fill the CUs that one workgroup per floor leaves idle.  512 such floors, 51 200 workgroups of 39 VGPRs and 14 KiB of
// LDS (eleven per CU at max_nodes = 64; one per CU at 256, where the pair table takes the CU's LDS), are throughput-bound instead: 2.7 ms,
// 52 ns per hypothesis, each of which reads its floor's 96 KiB of rows three times from the L2 (contract, phase A', phase E) -- 15 GB per
// call.  The contract pass repeats per hypothesis what launch 2 verifies once per floor; it stays because launch 1 forms LDS addresses from
// the rows' indices and no address is formed from an unverified table.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/salve_hip.h"
#include "pose_graph_common.h"
#include "salve_common.h"

namespace {

constexpr float RAD2DEG_QUOT_F32 = 180.0f / 3.14159274101257324f;   // the float32 QUOTIENT 180.0f / (float)pi = 57.295776: numpy's float32 rad2deg
static_assert(RAD2DEG_QUOT_F32 == 57.295776f, "not (float)(180 / pi) = 57.29578");
constexpr unsigned long long F64_QNAN_BITS = 0x7FF8000000000000ull;
enum { SCAL_EDGES = SCAL_CHOSEN, SCAL_MEASURED = SCAL_TRIPLETS };   // this kernel's use of the workgroup's scalars

__host__ __device__ inline size_t sample_lds_bytes(int M) { return graph_lds_bytes(M) + GRAPH_THREADS * sizeof(double); }

__device__ __forceinline__ double canonical_nan(double x) { return x != x ? __longlong_as_double((long long)F64_QNAN_BITS) : x; }

__device__ __forceinline__ salve_graph_tree_out_t empty_tree_out(int floor) {
    salve_graph_tree_out_t o;
    o.avg_rot_err = o.avg_trans_err = __longlong_as_double((long long)F64_QNAN_BITS);
    o.n_localized = o.n_measured = o.n_edges = 0;
    o.origin = -1;
    o.floor = floor;
    o.reserved = 0;
    return o;
}

__device__ __forceinline__ bool is_candidate(const salve_graph_row_t* __restrict__ row, float conf_thr) {
    return row->y_hat == 1 && row->prob >= conf_thr;   // (false for a NaN prob)
}

// bit k of a hypothesis's mask; a bit beyond the mask's words is not set
__device__ __forceinline__ bool mask_bit(const uint32_t* __restrict__ mask, int mask_words, int k) {
    const int w = k >> 5;
    return w < mask_words && ((mask[w] >> (k & 31)) & 1u) != 0;
}

// halving fold of the 256 partial sums, in the stated order; the total is part[0] behind the last barrier
__device__ __forceinline__ double fold_partials(double* part, int tid, double mine) {
    __syncthreads();   // (the previous fold's readers are done)
    part[tid] = mine;
    __syncthreads();
    for (int s = GRAPH_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] = part[tid] + part[tid + s];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(GRAPH_THREADS) void sample_trees_kernel(const salve_graph_row_t* __restrict__ rows, int n_rows,
                                                                     const int32_t* __restrict__ floor_start, const int32_t* __restrict__ n_nodes,
                                                                     int n_floors, int max_nodes, float conf_thr, const int32_t* __restrict__ hyp_start,
                                                                     const uint32_t* __restrict__ hyp_mask, int n_hyps, int mask_words,
                                                                     salve_graph_tree_out_t* __restrict__ out_trees,
                                                                     salve_graph_node_out_t* __restrict__ ws_nodes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_floor;
    const int h = blockIdx.x, tid = threadIdx.x;
    const GraphLds g = graph_lds(smem, max_nodes);
    double* const part = reinterpret_cast<double*>(smem + graph_lds_bytes(max_nodes));

    // the hypothesis's floor: the lowest one whose well-formed extent holds h
    if (tid == 0) s_floor = INT_MAX;
    __syncthreads();
    for (int f = tid; f < n_floors; f += GRAPH_THREADS) {
        const int hs = hyp_start[f], he = hyp_start[f + 1];
        if (hs >= 0 && hs <= he && he <= n_hyps && hs <= h && h < he) atomicMin(&s_floor, f);
    }
    __syncthreads();
    const int floor = s_floor;
    if (floor == INT_MAX) {   // (workgroup-uniform) no floor names it
        if (tid == 0) out_trees[h] = empty_tree_out(-1);
        return;
    }

    // the floor's tables, verified before any address is formed from them (workgroup-uniform)
    int lo = floor_start[floor], hi = floor_start[floor + 1], n = n_nodes[floor];
    const bool bad_extent = lo < 0 || hi < lo || hi > n_rows;
    const bool bad_nodes = n < 0 || n > max_nodes;
    if (bad_extent) lo = hi = 0;
    if (bad_nodes) n = 0;
    const int W = (max_nodes + 31) / 32;
    graph_clear(g, n, W, tid);
    __syncthreads();
    if (graph_rows_malformed(rows, lo, hi, n, tid)) g.scal[SCAL_BAD] = 1;
    __syncthreads();
    if (g.scal[SCAL_BAD] || bad_extent || bad_nodes) {   // launch 2 writes the floor empty and raises the status bit
        if (tid == 0) out_trees[h] = empty_tree_out(floor);
        return;
    }
    const uint32_t* __restrict__ const mask = hyp_mask + (size_t)h * (size_t)mask_words;

    // ---- A': the thread of a pair's FIRST row walks the pair's rows and keeps the LAST candidate whose mask bit is set
    int my_edges = 0;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const int a = rows[r].i1, b = rows[r].i2;
        if (r > lo && rows[r - 1].i1 == a && rows[r - 1].i2 == b) continue;
        int last = -1;
        for (int q = r; q < hi && rows[q].i1 == a && rows[q].i2 == b; q++)
            if (is_candidate(rows + q, conf_thr) && mask_bit(mask, mask_words, q - lo)) last = q;
        if (last >= 0) {
            g.pair[tri_index(a, b, n)] = last;
            atomicOr(&g.adj2[a * W + (b >> 5)], 1u << (b & 31));
            atomicOr(&g.adj2[b * W + (a >> 5)], 1u << (a & 31));
            my_edges++;
        }
    }
    if (my_edges) atomicAdd(&g.scal[SCAL_EDGES], my_edges);
    __syncthreads();

    // ---- C, D (pose_graph_common.h)
    const int origin = graph_component(g, g.adj2, n, W, tid);
    const bool placed = graph_tree(g, g.adj2, rows, n, W, tid, origin);
    if (tid < n) ws_nodes[(size_t)h * (size_t)max_nodes + tid] = graph_node_out(g, tid, placed);

    // ---- E: every candidate row of the floor, masked or not, whose two ends are localized, against the pose the tree implies for it
    double sum_rot = 0.0, sum_trans = 0.0;
    int my_measured = 0;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const salve_graph_row_t* __restrict__ const row = rows + r;
        if (!is_candidate(row, conf_thr)) continue;
        const int a = row->i1, b = row->i2;
        if (g.depth[a] < 0 || g.depth[b] < 0) continue;
        Sim2 W1, W2;   // wS_i1, wS_i2
        W1.R00 = g.R[4 * a + 0]; W1.R01 = g.R[4 * a + 1]; W1.R10 = g.R[4 * a + 2]; W1.R11 = g.R[4 * a + 3];
        W1.tx = g.t[2 * a + 0]; W1.ty = g.t[2 * a + 1]; W1.s = g.s[a];
        W2.R00 = g.R[4 * b + 0]; W2.R01 = g.R[4 * b + 1]; W2.R10 = g.R[4 * b + 2]; W2.R11 = g.R[4 * b + 3];
        W2.tx = g.t[2 * b + 0]; W2.ty = g.t[2 * b + 1]; W2.s = g.s[b];
        const Sim2 Z = sim2_compose(sim2_inverse(W2), W1);
        const double th_sim = (double)(atan2f(Z.R10, Z.R00) * RAD2DEG_QUOT_F32);
        const double th_m = (double)(atan2f(row->R[2], row->R[0]) * RAD2DEG_QUOT_F32);
        double d = fmod(th_m - th_sim + 180.0, 360.0);   // Python's %: the sign of the divisor
        if (d < 0.0) d += 360.0;
        const double rot_err = fabs(d - 180.0);
        const float dx = Z.tx - row->t[0], dy = Z.ty - row->t[1];
        const double trans_err = (double)sqrtf(dx * dx + dy * dy);
        sum_rot = sum_rot + rot_err;
        sum_trans = sum_trans + trans_err;
        my_measured++;
    }
    if (my_measured) atomicAdd(&g.scal[SCAL_MEASURED], my_measured);
    const double total_rot = fold_partials(part, tid, sum_rot);
    const double total_trans = fold_partials(part, tid, sum_trans);   // (its barriers also order the integer sum above)
    if (tid == 0) {
        salve_graph_tree_out_t o;
        const int n_measured = g.scal[SCAL_MEASURED];
        o.avg_rot_err = canonical_nan(total_rot / (double)n_measured);   // 0 measured rows: NaN, as np.mean([])
        o.avg_trans_err = canonical_nan(total_trans / (double)n_measured);
        o.n_localized = origin >= 0 ? g.count[origin] : 0;
        o.n_measured = n_measured;
        o.n_edges = g.scal[SCAL_EDGES];
        o.origin = origin;
        o.floor = floor;
        o.reserved = 0;
        out_trees[h] = o;
    }
}

__global__ __launch_bounds__(GRAPH_THREADS) void sample_pick_kernel(const salve_graph_row_t* __restrict__ rows, int n_rows,
                                                                    const int32_t* __restrict__ floor_start, const int32_t* __restrict__ n_nodes,
                                                                    int max_nodes, float conf_thr, const int32_t* __restrict__ hyp_start,
                                                                    const uint32_t* __restrict__ hyp_mask, int n_hyps, int mask_words,
                                                                    const salve_graph_tree_out_t* __restrict__ trees,
                                                                    const salve_graph_node_out_t* __restrict__ ws_nodes, int32_t* __restrict__ out_inlier,
                                                                    salve_graph_node_out_t* __restrict__ out_nodes,
                                                                    salve_graph_sample_floor_out_t* __restrict__ out_floors,
                                                                    int32_t* __restrict__ status) {
    __shared__ int s_bad, s_candidates, s_best;
    const int floor = blockIdx.x, tid = threadIdx.x;
    int lo = floor_start[floor], hi = floor_start[floor + 1], n = n_nodes[floor];
    int hs = hyp_start[floor], he = hyp_start[floor + 1];
    const bool bad_extent = lo < 0 || hi < lo || hi > n_rows;
    const bool bad_nodes = n < 0 || n > max_nodes;
    const bool bad_hyps = hs < 0 || he < hs || he > n_hyps;
    if (bad_extent) lo = hi = 0;
    if (bad_nodes) n = 0;
    if (bad_hyps) hs = he = 0;
    salve_graph_node_out_t* __restrict__ const nodes = out_nodes + (size_t)floor * (size_t)max_nodes;
    if (tid == 0) { s_bad = 0; s_candidates = 0; s_best = -1; }
    __syncthreads();
    bool bad = graph_rows_malformed(rows, lo, hi, n, tid);
    for (int h = hs + tid; h < he; h += GRAPH_THREADS)
        if (trees[h].floor != floor) bad = true;   // a lower floor's extent holds it too
    if (bad) s_bad = 1;
    __syncthreads();
    const double qnan = __longlong_as_double((long long)F64_QNAN_BITS);
    if (s_bad || bad_extent || bad_nodes || bad_hyps) {   // (workgroup-uniform) the floor is written empty
        for (int r = lo + tid; r < hi; r += GRAPH_THREADS) out_inlier[r] = 0;
        if (tid < n) nodes[tid] = empty_node_out();
        if (tid == 0) {
            salve_graph_sample_floor_out_t fo;
            fo.best = -1; fo.n_candidates = 0; fo.n_hyps = 0; fo.n_improvements = 0;
            fo.avg_rot_err = fo.avg_trans_err = qnan;
            out_floors[floor] = fo;
            if (status) atomicOr(status, SALVE_STATUS_BAD_GRAPH_ROW);
        }
        return;
    }
    int my_candidates = 0;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) my_candidates += is_candidate(rows + r, conf_thr);
    if (my_candidates) atomicAdd(&s_candidates, my_candidates);
    __syncthreads();

    // the reference's scan (spanning_tree.py:215-300), float64, the additions left to right; a NaN objective never replaces the best
    if (tid == 0) {
        double best_rot = __longlong_as_double(0x7FF0000000000000ll), best_trans = best_rot;
        int best_n = 0, best = -1, n_improvements = 0;
        for (int k = 0; k < he - hs; k++) {
            const double rot = trees[hs + k].avg_rot_err, trans = trees[hs + k].avg_trans_err;
            const int nl = trees[hs + k].n_localized;
            const double rot_win = (best_rot - rot) / 5.0;
            const double trans_win = (best_trans - trans) / 1.0;
            const double loc_win = (double)(-(best_n - nl)) / ((double)best_n + 1e-10);
            const double obj = (rot_win + trans_win) + 1.33 * loc_win;
            if (obj > 0.0) { best_rot = rot; best_trans = trans; best_n = nl; best = k; n_improvements++; }
        }
        s_best = best;
        salve_graph_sample_floor_out_t fo;
        fo.best = best; fo.n_hyps = he - hs; fo.n_improvements = n_improvements;
        fo.n_candidates = s_candidates;
        fo.avg_rot_err = best >= 0 ? best_rot : qnan;
        fo.avg_trans_err = best >= 0 ? best_trans : qnan;
        out_floors[floor] = fo;
    }
    __syncthreads();
    const int best = s_best;
    if (tid < n) nodes[tid] = best >= 0 ? ws_nodes[(size_t)(hs + best) * (size_t)max_nodes + tid] : empty_node_out();
    const uint32_t* __restrict__ const mask = hyp_mask + (size_t)(hs + (best >= 0 ? best : 0)) * (size_t)mask_words;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS)
        out_inlier[r] = best >= 0 && is_candidate(rows + r, conf_thr) && mask_bit(mask, mask_words, r - lo);
}

std::mutex g_sample_lds_mu;
size_t g_sample_lds_attr[64];

}  // namespace

extern "C" {

size_t salve_pose_graph_sample_workspace_bytes(int32_t n_hyps, int32_t max_nodes) {
    if (n_hyps <= 0 || max_nodes <= 0) return 0;
    return (size_t)n_hyps * (size_t)max_nodes * sizeof(salve_graph_node_out_t);   // every hypothesis's node records
}

int salve_pose_graph_sample_trees(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes,
                                  int32_t n_floors, int32_t max_nodes, float confidence_threshold, const int32_t* hyp_start,
                                  const uint32_t* hyp_mask, int32_t n_hyps, int32_t mask_words, salve_graph_tree_out_t* out_trees,
                                  int32_t* out_inlier, salve_graph_node_out_t* out_nodes, salve_graph_sample_floor_out_t* out_floors,
                                  void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    if (n_rows < 0 || n_floors < 0 || n_hyps < 0 || mask_words < 0) {
        salve_fail("salve_pose_graph_sample_trees: negative count");
        return SALVE_ERR_BAD_ARG;
    }
    if (max_nodes < 1 || max_nodes > SALVE_GRAPH_MAX_NODES) {
        salve_fail("salve_pose_graph_sample_trees: max_nodes must lie in 1 .. 256 (a floor of more panoramas is not supported)");
        return SALVE_ERR_BAD_ARG;
    }
    if (confidence_threshold != confidence_threshold) { salve_fail("salve_pose_graph_sample_trees: the threshold is NaN"); return SALVE_ERR_BAD_ARG; }
    if (n_floors == 0 || n_hyps == 0) return SALVE_OK;
    if (!floor_start || !n_nodes || !hyp_start || !out_trees || !out_nodes || !out_floors || !workspace || (n_rows > 0 && (!rows || !out_inlier)) ||
        (mask_words > 0 && !hyp_mask)) {
        salve_fail("salve_pose_graph_sample_trees: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    const auto misaligned = [](const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (misaligned(rows, 8) || misaligned(out_trees, 8) || misaligned(out_nodes, 8) || misaligned(out_floors, 8) || misaligned(workspace, 8) ||
        misaligned(floor_start, 4) || misaligned(n_nodes, 4) || misaligned(hyp_start, 4) || misaligned(hyp_mask, 4) || misaligned(out_inlier, 4) ||
        misaligned(status, 4)) {
        salve_fail("salve_pose_graph_sample_trees: rows, out_trees, out_nodes, out_floors and the workspace must be 8-byte aligned, the other "
                   "tables 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    if (workspace_bytes < salve_pose_graph_sample_workspace_bytes(n_hyps, max_nodes)) {
        salve_fail("salve_pose_graph_sample_trees: the workspace is shorter than salve_pose_graph_sample_workspace_bytes");
        return SALVE_ERR_WORKSPACE;
    }
    const size_t lds = sample_lds_bytes(max_nodes);
    if (lds > 64 * 1024) {   // opt in to more than 64 KB of dynamic LDS, per device
        std::lock_guard<std::mutex> lock(g_sample_lds_mu);
        int dev = 0;
        SALVE_HIP_CHECK(hipGetDevice(&dev));
        const int slot = (dev >= 0 && dev < 64) ? dev : 0;
        if (dev != slot || lds > g_sample_lds_attr[slot]) {
            SALVE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(sample_trees_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g_sample_lds_attr[slot] = lds;
        }
    }
    salve_graph_node_out_t* const ws_nodes = static_cast<salve_graph_node_out_t*>(workspace);
    hipLaunchKernelGGL(sample_trees_kernel, dim3((unsigned)n_hyps), dim3(GRAPH_THREADS), lds, (hipStream_t)stream, rows, n_rows, floor_start, n_nodes,
                       n_floors, max_nodes, confidence_threshold, hyp_start, hyp_mask, n_hyps, mask_words, out_trees, ws_nodes);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sample_pick_kernel, dim3((unsigned)n_floors), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, rows, n_rows, floor_start, n_nodes,
                       max_nodes, confidence_threshold, hyp_start, hyp_mask, n_hyps, mask_words, out_trees, ws_nodes, out_inlier, out_nodes, out_floors,
                       status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
