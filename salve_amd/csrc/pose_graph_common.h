// pose_graph_common.h -- what the pose-graph kernels share (pose_graph.hip: salve_pose_graph_solve; pose_graph_sample.hip:
// salve_pose_graph_sample_trees): the reference's Sim(2) arithmetic operation by operation, the floor's graph in LDS, and the two phases both
// kernels end with -- C, the largest connected component and its origin, and D, the level-synchronous BFS tree with one pose per node.
// Compile every file that includes this with -ffp-contract=off -fno-slp-vectorize: no product below may be fused into a sum.
// include/salve_hip.h states the rules of the phases and their three tie rules; pose_graph.hip's head states the LDS layout.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/salve_hip.h"

namespace {

constexpr int GRAPH_THREADS = 256;   // 4 waves; also the node limit: phases C and D give every node its own thread
static_assert(GRAPH_THREADS == SALVE_GRAPH_MAX_NODES, "one thread per node");

struct Sim2 {
    float R00, R01, R10, R11, tx, ty;
    double s;
};

__device__ __forceinline__ Sim2 sim2_load(const salve_graph_row_t* __restrict__ row) {
    Sim2 S;
    S.R00 = row->R[0]; S.R01 = row->R[1]; S.R10 = row->R[2]; S.R11 = row->R[3];
    S.tx = row->t[0]; S.ty = row->t[1];
    S.s = row->s;
    return S;
}

// Sim2.inverse: Rt = R.T; t = -Rt @ ((float)s * t); s = 1.0 / s
__device__ __forceinline__ Sim2 sim2_inverse(const Sim2& A) {
    const float sf = (float)A.s;
    const float ux = sf * A.tx, uy = sf * A.ty;
    Sim2 S;
    S.R00 = A.R00; S.R01 = A.R10; S.R10 = A.R01; S.R11 = A.R11;
    S.tx = (-S.R00) * ux + (-S.R01) * uy;
    S.ty = (-S.R10) * ux + (-S.R11) * uy;
    S.s = 1.0 / A.s;
    return S;
}

// A.compose(B): R = A.R @ B.R; t = A.R @ B.t + (float)(1.0 / B.s) * A.t; s = A.s * B.s
__device__ __forceinline__ Sim2 sim2_compose(const Sim2& A, const Sim2& B) {
    const float inv = (float)(1.0 / B.s);
    Sim2 S;
    S.R00 = A.R00 * B.R00 + A.R01 * B.R10;
    S.R01 = A.R00 * B.R01 + A.R01 * B.R11;
    S.R10 = A.R10 * B.R00 + A.R11 * B.R10;
    S.R11 = A.R10 * B.R01 + A.R11 * B.R11;
    S.tx = (A.R00 * B.tx + A.R01 * B.ty) + inv * A.tx;
    S.ty = (A.R10 * B.tx + A.R11 * B.ty) + inv * A.ty;
    S.s = A.s * B.s;
    return S;
}

__device__ __forceinline__ int tri_index(int a, int b, int n) { return a * (2 * n - a - 1) / 2 + (b - a - 1); }   // a < b < n <= 256

struct GraphLds {
    int32_t* pair;
    uint32_t *adj, *adj2;
    float *R, *t;
    double* s;
    int32_t *label, *count, *depth, *parent, *scal;
};

__host__ __device__ inline size_t graph_lds_bytes(int M) {
    const size_t W = (size_t)(M + 31) / 32;
    size_t pairs = (size_t)M * (M - 1) / 2;
    pairs = (pairs + 1) & ~(size_t)1;   // keeps what follows 8-byte aligned
    return pairs * 4 + 2 * (size_t)M * W * 4 + (size_t)M * (16 + 8 + 8) + 4 * (size_t)M * 4 + 32;
}

__device__ __forceinline__ GraphLds graph_lds(unsigned char* smem, int M) {
    const size_t W = (size_t)(M + 31) / 32;
    size_t pairs = (size_t)M * (M - 1) / 2;
    pairs = (pairs + 1) & ~(size_t)1;
    GraphLds g;
    g.s = reinterpret_cast<double*>(smem);                       // the 8-byte items first
    g.pair = reinterpret_cast<int32_t*>(g.s + M);
    g.adj = reinterpret_cast<uint32_t*>(g.pair + pairs);
    g.adj2 = g.adj + (size_t)M * W;
    g.R = reinterpret_cast<float*>(g.adj2 + (size_t)M * W);
    g.t = g.R + 4 * (size_t)M;
    g.label = reinterpret_cast<int32_t*>(g.t + 2 * (size_t)M);
    g.count = g.label + M;
    g.depth = g.count + M;
    g.parent = g.depth + M;
    g.scal = g.parent + M;
    return g;
}

// the scalars of a workgroup; the first three belong to the shared phases, the rest to the kernel
enum { SCAL_BAD = 0, SCAL_PROGRESS, SCAL_ORIGIN, SCAL_CHOSEN, SCAL_TRIPLETS, SCAL_CONSISTENT_TRIPLETS, SCAL_CONSISTENT_EDGES, SCAL_COUNT = 8 };

// Clears the floor's graph: no chosen row, no edge, every node its own label and outside the tree.  The caller's barrier follows.
__device__ __forceinline__ void graph_clear(const GraphLds& g, int n, int W, int tid) {
    const int n_pairs = n * (n - 1) / 2;
    for (int i = tid; i < n_pairs; i += GRAPH_THREADS) g.pair[i] = -1;
    for (int i = tid; i < n * W; i += GRAPH_THREADS) { g.adj[i] = 0u; g.adj2[i] = 0u; }
    if (tid < n) { g.label[tid] = tid; g.count[tid] = 0; g.depth[tid] = -1; g.parent[tid] = -1; }
    if (tid < SCAL_COUNT) g.scal[tid] = tid == SCAL_ORIGIN ? -1 : 0;
}

// The row contract of rows lo .. hi - 1: sorted by (i1, i2), 0 <= i1 < i2 < n.  This thread's share; true when a row of it breaks the contract.
__device__ __forceinline__ bool graph_rows_malformed(const salve_graph_row_t* __restrict__ rows, int lo, int hi, int n, int tid) {
    bool bad = false;
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const int a = rows[r].i1, b = rows[r].i2;
        if (a < 0 || a >= b || b >= n) bad = true;
        if (r > lo) {
            const int pa = rows[r - 1].i1, pb = rows[r - 1].i2;
            if (pa > a || (pa == a && pb > b)) bad = true;
        }
    }
    return bad;
}

__device__ __forceinline__ salve_graph_node_out_t empty_node_out() {
    salve_graph_node_out_t o;
    o.localized = 0; o.parent = -1; o.depth = -1; o.reserved = 0;
    o.R[0] = o.R[1] = o.R[2] = o.R[3] = 0.0f;
    o.t[0] = o.t[1] = 0.0f;
    o.s = 0.0;
    return o;
}

// ---- C: label propagation over `adj` to the component's lowest node, then the largest component, the lowest label among equals.  A label
// only falls and never below that node, so a stale read of a neighbour's label costs a step at worst; the loop ends with the step in which
// no label fell.  Called by the whole workgroup behind a barrier; returns the origin (-1: the graph has no edge) behind one.  g.count[origin]
// is the component's size.
__device__ __forceinline__ int graph_component(const GraphLds& g, const uint32_t* adj, int n, int W, int tid) {
    for (;;) {
        bool fell = false;
        if (tid < n) {
            int best = g.label[tid];
            for (int w = 0; w < W; w++) {
                uint32_t m = adj[tid * W + w];
                while (m) {
                    const int u = w * 32 + __builtin_ctz(m);
                    m &= m - 1;
                    const int lu = __atomic_load_n(&g.label[u], __ATOMIC_RELAXED);
                    if (lu < best) best = lu;
                }
            }
            if (best < g.label[tid]) { __atomic_store_n(&g.label[tid], best, __ATOMIC_RELAXED); fell = true; }
        }
        if (fell) g.scal[SCAL_PROGRESS] = 1;
        __syncthreads();
        const bool progress = g.scal[SCAL_PROGRESS] != 0;
        __syncthreads();
        if (!progress) break;
        if (tid == 0) g.scal[SCAL_PROGRESS] = 0;
        __syncthreads();
    }
    if (tid < n) atomicAdd(&g.count[g.label[tid]], 1);
    __syncthreads();
    if (tid == 0) {   // the largest component, the lowest label among equals; a component of one node has no edge
        int best = -1, best_n = 1;
        for (int v = 0; v < n; v++)
            if (g.count[v] > best_n) { best = v; best_n = g.count[v]; }
        g.scal[SCAL_ORIGIN] = best;
    }
    __syncthreads();
    return g.scal[SCAL_ORIGIN];
}

// ---- D: level-synchronous BFS over `adj` from the origin; a node joins level L through its lowest-index neighbour of level L - 1, by the
// row g.pair names for that edge.  Leaves wS_v in g.R, g.t, g.s and the tree in g.parent, g.depth (-1: not in the tree); returns whether
// this thread's node was placed.  Called by the whole workgroup; ends behind a barrier.
__device__ __forceinline__ bool graph_tree(const GraphLds& g, const uint32_t* adj, const salve_graph_row_t* __restrict__ rows, int n, int W, int tid,
                                           int origin) {
    const bool member = tid < n && origin >= 0 && g.label[tid] == origin;
    if (member && tid == origin) {
        g.depth[tid] = 0;
        g.R[4 * tid + 0] = 1.0f; g.R[4 * tid + 1] = 0.0f; g.R[4 * tid + 2] = 0.0f; g.R[4 * tid + 3] = 1.0f;
        g.t[2 * tid + 0] = 0.0f; g.t[2 * tid + 1] = 0.0f;
        g.s[tid] = 1.0;
    }
    __syncthreads();
    bool placed = member && tid == origin;
    for (int level = 1; origin >= 0 && level < n; level++) {
        bool joined = false;
        if (member && !placed) {
            int p = -1;
            for (int w = 0; w < W && p < 0; w++) {
                uint32_t m = adj[tid * W + w];
                while (m) {
                    const int u = w * 32 + __builtin_ctz(m);
                    m &= m - 1;
                    if (__atomic_load_n(&g.depth[u], __ATOMIC_RELAXED) == level - 1) { p = u; break; }   // (a node of THIS level holds `level`)
                }
            }
            if (p >= 0) {
                Sim2 P;
                P.R00 = g.R[4 * p + 0]; P.R01 = g.R[4 * p + 1]; P.R10 = g.R[4 * p + 2]; P.R11 = g.R[4 * p + 3];
                P.tx = g.t[2 * p + 0]; P.ty = g.t[2 * p + 1];
                P.s = g.s[p];
                const int v = tid;
                const Sim2 E = p < v ? sim2_inverse(sim2_load(rows + g.pair[tri_index(p, v, n)])) : sim2_load(rows + g.pair[tri_index(v, p, n)]);
                const Sim2 S = sim2_compose(P, E);
                g.R[4 * v + 0] = S.R00; g.R[4 * v + 1] = S.R01; g.R[4 * v + 2] = S.R10; g.R[4 * v + 3] = S.R11;
                g.t[2 * v + 0] = S.tx; g.t[2 * v + 1] = S.ty;
                g.s[v] = S.s;
                g.parent[v] = p;
                __atomic_store_n(&g.depth[v], level, __ATOMIC_RELAXED);
                placed = joined = true;
            }
        }
        if (joined) g.scal[SCAL_PROGRESS] = 1;
        __syncthreads();
        const bool progress = g.scal[SCAL_PROGRESS] != 0;
        __syncthreads();
        if (!progress) break;
        if (tid == 0) g.scal[SCAL_PROGRESS] = 0;
        __syncthreads();
    }
    return placed;
}

// the node record of this thread's node, from the tree in LDS
__device__ __forceinline__ salve_graph_node_out_t graph_node_out(const GraphLds& g, int tid, bool placed) {
    salve_graph_node_out_t o = empty_node_out();
    if (placed) {
        o.localized = 1;
        o.parent = g.parent[tid];
        o.depth = g.depth[tid];
        o.R[0] = g.R[4 * tid + 0]; o.R[1] = g.R[4 * tid + 1]; o.R[2] = g.R[4 * tid + 2]; o.R[3] = g.R[4 * tid + 3];
        o.t[0] = g.t[2 * tid + 0]; o.t[1] = g.t[2 * tid + 1];
        o.s = g.s[tid];
    }
    return o;
}

}  // namespace
