// pose_graph.hip -- the floor pose graph for gfx950 (MI355X): scored alignment hypotheses -> the best row per panorama pair -> the edges that
// lie in a consistent 3-cycle -> the largest connected component -> a BFS spanning tree and one global Sim(2) pose per panorama.  Any number
// of floors in ONE launch.  Compile with -ffp-contract=off -fno-slp-vectorize: the Sim(2) arithmetic below is the reference's float32 /
// float64 arithmetic operation by operation, and no product may be fused into a sum.
//
// The reference does this per floor on the host, in scripts/run_sfm.py:112-152 and :440-446 (method `spanning_tree`):
//   salve/common/edge_classification.py:213-251   get_conf_thresholded_edge_measurements    phase A
//   salve/common/edge_classification.py:254-311   get_most_likely_relative_pose_per_edge    phase A
//   salve/algorithms/cycle_consistency.py:26-91    extract_triplets, create_adjacency_list   phase B
//   salve/algorithms/cycle_consistency.py:172-222  compute_SE2_cycle_error                   phase B
//   salve/algorithms/cycle_consistency.py:225-303  filter_to_SE2_cycle_consistent_edges      phase B
//   salve/algorithms/spanning_tree.py:73-141       greedily_construct_st_Sim2                phases C, D
// include/salve_hip.h (salve_pose_graph_solve) states the rules of the four phases; this file states how they run.  The Sim(2) arithmetic, the
// LDS layout below and phases C and D are in pose_graph_common.h, shared with pose_graph_sample.hip (salve_pose_graph_sample_trees).
//
//   pose_graph_kernel   salve_pose_graph_solve: one workgroup of 256 threads per floor, the floor's graph in LDS
//
// LDS, for max_nodes = M and W = ceil(M / 32) words per bitmask row (graph_lds_bytes; 159 264 bytes of the 160 KiB at M = 256, 12 192 at
// M = 64, so small floors share a CU):
//   pair      int32 [M (M - 1) / 2]   the chosen row of pair (a, b), a < b, at a (2 n - a - 1) / 2 + b - a - 1; -1 = no chosen row   130 560
//   adj       uint32 [M][W]           adjacency of the CHOSEN edges (phase B reads it)                                                   8 192
//   adj2      uint32 [M][W]           adjacency of the graph of phases C and D: the consistent edges, or the chosen ones                 8 192
//   R, t, s   float [M][4], float [M][2], double [M]   wS_v of the localized nodes                                                      8 192
//   label, count, depth, parent   int32 [M] each                                                                                         4 096
//   scalars   int32 [8]               bad-row flag, progress flag, origin, the floor's four counts                                          32
// The pair table is the large item.  It stays in LDS and not in a per-floor global workspace: phase B looks two pairs up per 3-cycle and
// phase D one per node, all dependent reads, and a launch of hundreds of floors would need hundreds of 128 KiB workspaces.
//
// Per-edge statistics are NOT accumulated with atomics, one visit per cycle: four words for each of 32 640 pairs (510 KiB) do not fit next to
// the pair table.  The thread that owns a chosen edge (a, b) walks ALL its cycles -- the set bits of adj[a] & adj[b], below, between and
// above a and b -- sorts each (a, b, c) and evaluates the cycle itself, statistics in registers.  A cycle is evaluated by its three edges, from
// the same three rows in the same order, hence with equal bits; the floor's cycle count is the sum over the edges / 3.  Only integer LDS
// atomics remain (bit sets, counts), so no output depends on an arrival order: the same bytes on every run.
//
// Deviations from the reference (all three are choices it leaves to an unspecified iteration order):
//   - among rows of a pair with equal prob (fp32 softmax saturates at exactly 1.0: the normal case) the FIRST in row order is chosen;
//   - among equally large components the one holding the lowest node wins;
//   - among several shortest paths to a node, the one through the lowest-index neighbour of the previous BFS level, level by level.
// Limit: 256 panoramas per floor (SALVE_GRAPH_MAX_NODES): the bitmask rows and the pair table are sized for it.
//
// Bound: latency, not bandwidth or arithmetic.  A floor reads its rows once (48 bytes each) and writes 24 bytes per row; a ZInD-sized floor
// (tens of panoramas, hundreds of chosen edges, thousands of cycles at ~150 float operations and two float64 divisions each) is microseconds
// of arithmetic on one CU.  What a floor costs is its chain of workgroup barriers: one label-propagation step per hop of the graph's diameter,
// one BFS level per hop of the tree's depth, each a barrier and a few dependent LDS reads.  Floors are independent, so a launch of F floors
// fills F workgroup slots and the chains overlap; one workgroup per floor keeps every atomic and every barrier inside a CU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/salve_hip.h"
#include "pose_graph_common.h"
#include "salve_common.h"

namespace {

constexpr uint32_t F32_INF_BITS = 0x7F800000u;
constexpr float RAD2DEG_F32 = 57.29577951308232f;   // (float)(180 / pi)

__device__ __forceinline__ salve_graph_row_out_t empty_row_out() {
    salve_graph_row_out_t o;
    o.chosen = 0; o.consistent = 0; o.n_triplets = 0; o.n_consistent = 0;
    o.min_rot_err = __uint_as_float(F32_INF_BITS); o.min_trans_err = __uint_as_float(F32_INF_BITS);
    return o;
}

// The error of the 3-cycle i0 < i1 < i2 from the rows of its three edges: (inverse(S_02).compose(S_12)).compose(S_01)
__device__ __forceinline__ void cycle_error(const salve_graph_row_t* __restrict__ r01, const salve_graph_row_t* __restrict__ r12,
                                            const salve_graph_row_t* __restrict__ r02, float* rot_deg, float* trans) {
    const Sim2 Z = sim2_compose(sim2_compose(sim2_inverse(sim2_load(r02)), sim2_load(r12)), sim2_load(r01));
    *rot_deg = fabsf(atan2f(Z.R10, Z.R00)) * RAD2DEG_F32;
    *trans = sqrtf(Z.tx * Z.tx + Z.ty * Z.ty);   // correctly rounded (hipcc's default for sqrtf; __fsqrt_rn is the approximate instruction here)
}

__global__ __launch_bounds__(GRAPH_THREADS) void pose_graph_kernel(const salve_graph_row_t* __restrict__ rows, int n_rows,
                                                                   const int32_t* __restrict__ floor_start, const int32_t* __restrict__ n_nodes,
                                                                   int max_nodes, float conf_thr, float rot_thr, float trans_thr, int cycle_filter,
                                                                   salve_graph_row_out_t* __restrict__ out_rows,
                                                                   salve_graph_node_out_t* __restrict__ out_nodes,
                                                                   salve_graph_floor_out_t* __restrict__ out_floors, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int floor = blockIdx.x, tid = threadIdx.x;
    const GraphLds g = graph_lds(smem, max_nodes);
    // the tables are device memory: verified before any address is formed from them (workgroup-uniform)
    int lo = floor_start[floor], hi = floor_start[floor + 1], n = n_nodes[floor];
    const bool bad_extent = lo < 0 || hi < lo || hi > n_rows;
    const bool bad_nodes = n < 0 || n > max_nodes;
    if (bad_extent) lo = hi = 0;   // no row of such a floor can be named: none is read or written
    if (bad_nodes) n = 0;          // (and no node record)
    const int W = (max_nodes + 31) / 32;
    salve_graph_node_out_t* __restrict__ const nodes = out_nodes + (size_t)floor * (size_t)max_nodes;

    graph_clear(g, n, W, tid);
    __syncthreads();

    // the row contract: sorted by (i1, i2), 0 <= i1 < i2 < n
    const bool bad = graph_rows_malformed(rows, lo, hi, n, tid);
    if (bad) g.scal[SCAL_BAD] = 1;
    __syncthreads();
    if (g.scal[SCAL_BAD] || bad_extent || bad_nodes) {   // (workgroup-uniform) the floor is written empty
        for (int r = lo + tid; r < hi; r += GRAPH_THREADS) out_rows[r] = empty_row_out();
        if (tid < n) nodes[tid] = empty_node_out();
        if (tid == 0) {
            salve_graph_floor_out_t fo;
            fo.n_chosen = fo.n_triplets = fo.n_consistent_triplets = fo.n_consistent_edges = fo.n_localized = 0;
            fo.origin = -1;
            out_floors[floor] = fo;
            if (status) atomicOr(status, SALVE_STATUS_BAD_GRAPH_ROW);
        }
        return;
    }

    // ---- A: the thread of a pair's FIRST row walks the pair's rows (they are contiguous) and keeps the first candidate of largest prob
    int my_chosen = 0;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const int a = rows[r].i1, b = rows[r].i2;
        if (r > lo && rows[r - 1].i1 == a && rows[r - 1].i2 == b) continue;
        int best = -1;
        float best_p = 0.0f;
        for (int q = r; q < hi && rows[q].i1 == a && rows[q].i2 == b; q++) {
            const float p = rows[q].prob;
            if (rows[q].y_hat == 1 && p >= conf_thr && (best < 0 || p > best_p)) { best = q; best_p = p; }
        }
        if (best >= 0) {
            g.pair[tri_index(a, b, n)] = best;
            atomicOr(&g.adj[a * W + (b >> 5)], 1u << (b & 31));
            atomicOr(&g.adj[b * W + (a >> 5)], 1u << (a & 31));
            my_chosen++;
        }
    }
    __syncthreads();

    // ---- B: the thread of a chosen row owns that edge: all its 3-cycles, statistics in registers, its row record written once
    int my_trip = 0, my_cons_trip = 0, my_cons_edges = 0;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const int a = rows[r].i1, b = rows[r].i2;
        salve_graph_row_out_t o = empty_row_out();
        if (g.pair[tri_index(a, b, n)] == r) {
            uint32_t min_rot = F32_INF_BITS, min_trans = F32_INF_BITS;
            int trip = 0, cons = 0;
            for (int w = 0; w < W; w++) {
                uint32_t m = g.adj[a * W + w] & g.adj[b * W + w];
                while (m) {
                    const int c = w * 32 + __builtin_ctz(m);
                    m &= m - 1;
                    int i0 = a, i1 = b, i2 = c;             // a < b; bring c to its place
                    if (c < a) { i0 = c; i1 = a; i2 = b; }
                    else if (c < b) { i1 = c; i2 = b; }
                    float rot, trans;
                    cycle_error(rows + g.pair[tri_index(i0, i1, n)], rows + g.pair[tri_index(i1, i2, n)], rows + g.pair[tri_index(i0, i2, n)], &rot,
                                &trans);
                    trip++;
                    if (rot < rot_thr && trans < trans_thr) cons++;   // (false for a NaN error)
                    // min on the bit patterns of the non-negative floats: a NaN (above +inf's pattern) never lowers it
                    const uint32_t rb = __float_as_uint(rot), tb = __float_as_uint(trans);
                    if (rb < min_rot) min_rot = rb;
                    if (tb < min_trans) min_trans = tb;
                }
            }
            o.chosen = 1;
            o.consistent = cons > 0;
            o.n_triplets = trip;
            o.n_consistent = cons;
            o.min_rot_err = __uint_as_float(min_rot);
            o.min_trans_err = __uint_as_float(min_trans);
            my_trip += trip;
            my_cons_trip += cons;
            my_cons_edges += cons > 0;
            if (!cycle_filter || cons > 0) {
                atomicOr(&g.adj2[a * W + (b >> 5)], 1u << (b & 31));
                atomicOr(&g.adj2[b * W + (a >> 5)], 1u << (a & 31));
            }
        }
        out_rows[r] = o;
    }
    // the floor's counts: integer sums, so their order does not matter; every cycle was counted by its three edges
    if (my_chosen) atomicAdd(&g.scal[SCAL_CHOSEN], my_chosen);
    if (my_trip) atomicAdd(&g.scal[SCAL_TRIPLETS], my_trip);
    if (my_cons_trip) atomicAdd(&g.scal[SCAL_CONSISTENT_TRIPLETS], my_cons_trip);
    if (my_cons_edges) atomicAdd(&g.scal[SCAL_CONSISTENT_EDGES], my_cons_edges);
    __syncthreads();

    // ---- C, D (pose_graph_common.h): the largest component of adj2, its BFS tree, one pose per node
    const int origin = graph_component(g, g.adj2, n, W, tid);
    const bool placed = graph_tree(g, g.adj2, rows, n, W, tid, origin);

    if (tid < n) nodes[tid] = graph_node_out(g, tid, placed);
    if (tid == 0) {
        salve_graph_floor_out_t fo;
        fo.n_chosen = g.scal[SCAL_CHOSEN];
        fo.n_triplets = g.scal[SCAL_TRIPLETS] / 3;
        fo.n_consistent_triplets = g.scal[SCAL_CONSISTENT_TRIPLETS] / 3;
        fo.n_consistent_edges = g.scal[SCAL_CONSISTENT_EDGES];
        fo.n_localized = origin >= 0 ? g.count[origin] : 0;
        fo.origin = origin;
        out_floors[floor] = fo;
    }
}

std::mutex g_lds_mu;
size_t g_lds_attr[64];

}  // namespace

extern "C" {

size_t salve_pose_graph_workspace_bytes(int32_t n_floors, int32_t max_nodes) {
    (void)n_floors;
    (void)max_nodes;
    return 0;   // the floor's graph lives in LDS
}

int salve_pose_graph_solve(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                           int32_t max_nodes, float confidence_threshold, float rot_threshold_deg, float trans_threshold, int32_t cycle_filter,
                           salve_graph_row_out_t* out_rows, salve_graph_node_out_t* out_nodes, salve_graph_floor_out_t* out_floors,
                           void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    if (n_rows < 0 || n_floors < 0) { salve_fail("salve_pose_graph_solve: negative count"); return SALVE_ERR_BAD_ARG; }
    if (max_nodes < 1 || max_nodes > SALVE_GRAPH_MAX_NODES) {
        salve_fail("salve_pose_graph_solve: max_nodes must lie in 1 .. 256 (a floor of more panoramas is not supported)");
        return SALVE_ERR_BAD_ARG;
    }
    if (cycle_filter != 0 && cycle_filter != 1) { salve_fail("salve_pose_graph_solve: cycle_filter must be 0 or 1"); return SALVE_ERR_BAD_ARG; }
    if (confidence_threshold != confidence_threshold || rot_threshold_deg != rot_threshold_deg || trans_threshold != trans_threshold) {
        salve_fail("salve_pose_graph_solve: a threshold is NaN");
        return SALVE_ERR_BAD_ARG;
    }
    if (n_floors == 0) return SALVE_OK;
    if (!floor_start || !n_nodes || !out_nodes || !out_floors || (n_rows > 0 && (!rows || !out_rows))) {
        salve_fail("salve_pose_graph_solve: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(rows) % 8 != 0 || reinterpret_cast<uintptr_t>(out_rows) % 8 != 0 || reinterpret_cast<uintptr_t>(out_nodes) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(out_floors) % 4 != 0 || reinterpret_cast<uintptr_t>(floor_start) % 4 != 0 ||
        reinterpret_cast<uintptr_t>(n_nodes) % 4 != 0 || reinterpret_cast<uintptr_t>(status) % 4 != 0) {
        salve_fail("salve_pose_graph_solve: rows, out_rows and out_nodes must be 8-byte aligned, the other tables 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    const size_t lds = graph_lds_bytes(max_nodes);
    if (lds > 64 * 1024) {   // opt in to more than 64 KB of dynamic LDS, per device
        std::lock_guard<std::mutex> lock(g_lds_mu);
        int dev = 0;
        SALVE_HIP_CHECK(hipGetDevice(&dev));
        const int slot = (dev >= 0 && dev < 64) ? dev : 0;
        if (dev != slot || lds > g_lds_attr[slot]) {
            SALVE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pose_graph_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g_lds_attr[slot] = lds;
        }
    }
    hipLaunchKernelGGL(pose_graph_kernel, dim3((unsigned)n_floors), dim3(GRAPH_THREADS), lds, (hipStream_t)stream, rows, n_rows, floor_start, n_nodes,
                       max_nodes, confidence_threshold, rot_threshold_deg, trans_threshold, cycle_filter, out_rows, out_nodes, out_floors, status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
