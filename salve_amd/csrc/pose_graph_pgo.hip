// pose_graph_pgo.hip -- pose-graph optimisation for gfx950 (MI355X): the spanning tree's poses of a floor refined by a robust
// Levenberg-Marquardt over ALL the floor's thresholded predictions (the reference's `--method pgo`, salve/algorithms/pose2_slam.py:57-286 with
// optimize_poses_only and without axis alignment).  Any number of floors in ONE launch.  Compile with -ffp-contract=off -fno-slp-vectorize:
// the sums below are float64 in one stated order and no product may be fused into a sum.  include/salve_hip.h (salve_pose_graph_optimise)
// states the problem, the step, the loop and the order of every sum; this file states how they run.
//
//   pgo_kernel   one workgroup of 256 threads per floor; the LM control flow is uniform over the workgroup (every decision is taken on a value
//                all threads read from LDS behind a barrier)
//
// LDS for max_nodes = M (pgo_lds_bytes; 155 584 bytes of the 160 KiB at M = 256, 44 320 at M = 32, so small floors share a CU):
//   H        double [N (N + 1) / 2], N = 3 min(M, SALVE_PGO_LDS_NODES)   the packed lower triangle of J^T J + lambda I, factorised in place
//   X, XT    double [M][5] each     x, y, theta, cos, sin of the current and of the trial estimate, by node
//   g, y, d  double [3 M] each      -J^T r, the forward substitution's result, the step
//   partial  double [256]           the cost's partial sums
//   idx      int32 [M]              the unknown's index of a node (-1: not localized);  scalars int32 [8]
// A floor of more than SALVE_PGO_LDS_NODES localized nodes keeps H in its slice of the workspace instead (up to 768 x 769 / 2 doubles, 2.4 MB):
// the same code through the same pointer, decided per floor from its localized count.  H is not kept twice: a rejected step rebuilds the
// linearisation (the same values in the same order) before it is factorised with the next lambda.  Rejections are rare.
//
// Parallel parts: the blocks of H (one owner per block, see the header), the factorisation (per column: the pivot, the column scaled and
// copied to LDS, then the trailing update with a wave per row and its lanes along the row, so that both storages are read and written in
// consecutive addresses; three barriers per column), the two substitutions (two barriers per column), the cost (a thread per row, folded by
// halving).
// Bound: latency.  A ZInD-sized floor (3 L ~ 100) is ~700 barriers and a few thousand LDS operations per thread and linearisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/salve_hip.h"
#include "pose_graph_common.h"
#include "salve_common.h"

namespace {

constexpr double PGO_PI = 3.141592653589793, PGO_TWO_PI = 6.283185307179586;
constexpr double PGO_LAMBDA_INITIAL = 1e-5, PGO_LAMBDA_FACTOR = 10.0, PGO_LAMBDA_UPPER = 1e5;
constexpr uint64_t F64_QNAN_BITS = 0x7FF8000000000000ull;

struct PgoParams {
    double sig_odo[3], sig_prior[3], k, rel_tol, abs_tol;
    int32_t robust, max_iterations;
    float conf_thr;
};

__host__ __device__ inline int pgo_lds_nodes(int M) { return M < SALVE_PGO_LDS_NODES ? M : SALVE_PGO_LDS_NODES; }
__host__ __device__ inline size_t pgo_tri(int N) { return (size_t)N * (size_t)(N + 1) / 2; }
__host__ __device__ inline size_t pgo_lds_bytes(int M) { return 8 * (pgo_tri(3 * pgo_lds_nodes(M)) + 19 * (size_t)M + 256) + 4 * ((size_t)M + 8); }
__host__ __device__ inline size_t pgo_floor_workspace_doubles(int M) { return M > SALVE_PGO_LDS_NODES ? pgo_tri(3 * M) : 0; }

enum { PS_BAD = 0, PS_NONFINITE, PS_FACTORS, PS_DOWN, PS_COUNT = 8 };

__device__ __forceinline__ double wrap_pi(double a) { return a - PGO_TWO_PI * ceil((a - PGO_PI) / PGO_TWO_PI); }
__device__ __forceinline__ double qnan() { return __longlong_as_double((long long)F64_QNAN_BITS); }
__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

struct Meas { double x, y, th, c, s; };

__device__ __forceinline__ Meas meas_load(const salve_graph_row_t* __restrict__ row) {
    Meas m;
    m.x = (double)row->t[0]; m.y = (double)row->t[1];
    m.th = atan2((double)row->R[2], (double)row->R[0]);
    m.c = cos(m.th); m.s = sin(m.th);
    return m;
}

// One factor at an estimate: the whitened residual r scaled by sqrt(w), the sum of squares ss of the unscaled one, rho, and what its Jacobians need
struct Factor {
    double r[3], rho, sw;
    int down;
    double J1[3][3], J2[3][3];   // whitened, scaled by sqrt(w): wrt the local coordinates of x_i1 and of x_i2 (the prior: J1 only)
};

__device__ __forceinline__ void robust_weight(const PgoParams& P, const double* r, Factor& f) {
    const double ss = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    const double n = sqrt(ss);
    double w = 1.0;
    f.down = 0;
    if (P.robust && n > P.k) { f.rho = P.k * (n - 0.5 * P.k); w = P.k / n; f.down = 1; }
    else f.rho = 0.5 * ss;
    f.sw = sqrt(w);
    f.r[0] = f.sw * r[0]; f.r[1] = f.sw * r[1]; f.r[2] = f.sw * r[2];
}

// BetweenFactorPose2(X(i2), X(i1), m) at X1 = x_i1, X2 = x_i2 (x, y, theta, cos, sin each)
__device__ __forceinline__ void between_factor(const PgoParams& P, const double* X1, const double* X2, const Meas& m, bool jac, Factor& f) {
    const double vx = X1[0] - X2[0], vy = X1[1] - X2[1];
    const double dx = X2[3] * vx + X2[4] * vy, dy = X2[3] * vy - X2[4] * vx;   // delta = R(theta2)^T (p1 - p2)
    const double ux = dx - m.x, uy = dy - m.y;
    double r[3];
    r[0] = (m.c * ux + m.s * uy) / P.sig_odo[0];
    r[1] = (m.c * uy - m.s * ux) / P.sig_odo[1];
    r[2] = wrap_pi((X1[2] - X2[2]) - m.th) / P.sig_odo[2];
    robust_weight(P, r, f);
    if (!jac) return;
    const double cd = X1[3] * X2[3] + X1[4] * X2[4], sd = X1[4] * X2[3] - X1[3] * X2[4];   // cos, sin of theta1 - theta2
    const double ce = m.c * cd + m.s * sd, se = m.c * sd - m.s * cd;                       // ... of theta1 - theta2 - m_theta
    const double a0 = f.sw / P.sig_odo[0], a1 = f.sw / P.sig_odo[1], a2 = f.sw / P.sig_odo[2];
    f.J1[0][0] = a0 * ce; f.J1[0][1] = a0 * -se; f.J1[0][2] = 0.0;
    f.J1[1][0] = a1 * se; f.J1[1][1] = a1 * ce;  f.J1[1][2] = 0.0;
    f.J1[2][0] = 0.0;     f.J1[2][1] = 0.0;      f.J1[2][2] = a2;
    f.J2[0][0] = a0 * -m.c; f.J2[0][1] = a0 * -m.s; f.J2[0][2] = a0 * (m.c * dy - m.s * dx);
    f.J2[1][0] = a1 * m.s;  f.J2[1][1] = a1 * -m.c; f.J2[1][2] = a1 * (-(m.s * dy) - m.c * dx);
    f.J2[2][0] = 0.0;       f.J2[2][1] = 0.0;       f.J2[2][2] = -a2;
}

__device__ __forceinline__ void prior_factor(const PgoParams& P, const double* X, bool jac, Factor& f) {
    double r[3];
    r[0] = X[0] / P.sig_prior[0]; r[1] = X[1] / P.sig_prior[1]; r[2] = wrap_pi(X[2]) / P.sig_prior[2];
    robust_weight(P, r, f);
    if (!jac) return;
    const double a0 = f.sw / P.sig_prior[0], a1 = f.sw / P.sig_prior[1], a2 = f.sw / P.sig_prior[2];
    f.J1[0][0] = a0 * X[3]; f.J1[0][1] = a0 * -X[4]; f.J1[0][2] = 0.0;
    f.J1[1][0] = a1 * X[4]; f.J1[1][1] = a1 * X[3];  f.J1[1][2] = 0.0;
    f.J1[2][0] = 0.0;       f.J1[2][1] = 0.0;        f.J1[2][2] = a2;
}

// acc[p][q] += sum_i A[i][p] * B[i][q], the three products summed in order of i
__device__ __forceinline__ void add_JtJ(double (*acc)[3], const double (*A)[3], const double (*B)[3]) {
    for (int p = 0; p < 3; p++)
        for (int q = 0; q < 3; q++) acc[p][q] += (A[0][p] * B[0][q] + A[1][p] * B[1][q]) + A[2][p] * B[2][q];
}
__device__ __forceinline__ void add_Jtr(double* acc, const double (*A)[3], const double* r) {
    for (int p = 0; p < 3; p++) acc[p] += (A[0][p] * r[0] + A[1][p] * r[1]) + A[2][p] * r[2];
}

struct PgoLds {
    double *H, *X, *XT, *g, *y, *d, *partial;
    int32_t *idx, *scal;
};

__device__ __forceinline__ bool row_is_factor(const salve_graph_row_t* __restrict__ row, const PgoLds& L, float thr) {
    return row->y_hat == 1 && row->prob >= thr && L.idx[row->i1] >= 0 && L.idx[row->i2] >= 0;
}

// E at the estimate X: the header's order.  Also counts the down-weighted factors into scal[PS_DOWN].  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ double pgo_cost(const PgoParams& P, const PgoLds& L, const double* X, const salve_graph_row_t* __restrict__ rows, int lo,
                                           int hi, int origin, int tid) {
    double sum = 0.0;
    int down = 0;
    Factor f;
    if (tid == 0) { prior_factor(P, X + 5 * origin, false, f); sum = f.rho; down = f.down; }
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        if (!row_is_factor(rows + r, L, P.conf_thr)) continue;
        between_factor(P, X + 5 * rows[r].i1, X + 5 * rows[r].i2, meas_load(rows + r), false, f);
        sum += f.rho;
        down += f.down;
    }
    L.partial[tid] = sum;
    if (tid == 0) L.scal[PS_DOWN] = 0;
    __syncthreads();
    if (down) atomicAdd(&L.scal[PS_DOWN], down);
    for (int h = GRAPH_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) L.partial[tid] += L.partial[tid + h];
        __syncthreads();
    }
    const double E = L.partial[0];
    __syncthreads();
    return E;
}

// H = J^T J (packed lower triangle), g = -J^T r at the estimate L.X.  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ void pgo_linearise(const PgoParams& P, const PgoLds& L, const salve_graph_row_t* __restrict__ rows, int lo, int hi, int n,
                                              int N, int origin, int tid) {
    const size_t tri = pgo_tri(N);
    for (size_t i = tid; i < tri; i += GRAPH_THREADS) L.H[i] = 0.0;
    __syncthreads();
    // the block of a pair: the thread of the pair's first row, over the pair's rows in row order
    for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
        const int a = rows[r].i1, b = rows[r].i2;
        if (r > lo && rows[r - 1].i1 == a && rows[r - 1].i2 == b) continue;
        if (L.idx[a] < 0 || L.idx[b] < 0) continue;
        double B[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        bool any = false;
        Factor f;
        for (int q = r; q < hi && rows[q].i1 == a && rows[q].i2 == b; q++) {
            if (!row_is_factor(rows + q, L, P.conf_thr)) continue;
            between_factor(P, L.X + 5 * a, L.X + 5 * b, meas_load(rows + q), true, f);
            add_JtJ(B, f.J2, f.J1);   // row block: x_i2 (the higher unknown), column block: x_i1
            any = true;
        }
        if (any) {
            const int ub = 3 * L.idx[b], ua = 3 * L.idx[a];
            for (int p = 0; p < 3; p++)
                for (int q = 0; q < 3; q++) L.H[pgo_tri(ub + p) + (size_t)(ua + q)] = B[p][q];
        }
    }
    // a node's diagonal block and gradient segment: the node's thread, over all rows that touch it in row order, the prior first
    if (tid < n && L.idx[tid] >= 0) {
        const int v = tid;
        double D[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        double gs[3] = {0.0, 0.0, 0.0};
        Factor f;
        if (v == origin) {
            prior_factor(P, L.X + 5 * v, true, f);
            add_JtJ(D, f.J1, f.J1);
            add_Jtr(gs, f.J1, f.r);
        }
        for (int r = lo; r < hi; r++) {
            const int a = rows[r].i1, b = rows[r].i2;
            if ((a != v && b != v) || !row_is_factor(rows + r, L, P.conf_thr)) continue;
            between_factor(P, L.X + 5 * a, L.X + 5 * b, meas_load(rows + r), true, f);
            if (a == v) { add_JtJ(D, f.J1, f.J1); add_Jtr(gs, f.J1, f.r); }
            else        { add_JtJ(D, f.J2, f.J2); add_Jtr(gs, f.J2, f.r); }
        }
        const int u = 3 * L.idx[v];
        for (int p = 0; p < 3; p++) {
            for (int q = 0; q <= p; q++) L.H[pgo_tri(u + p) + (size_t)(u + q)] = D[p][q];
            L.g[u + p] = -gs[p];
        }
    }
    __syncthreads();
}

// (H + lambda I) d = g: Cholesky in place, forward and backward substitution.  False (workgroup-uniform) for a pivot that is not finite and
// positive.  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ bool pgo_solve(const PgoLds& L, int N, double lambda, int tid) {
    double* __restrict__ const H = L.H;
    for (int i = tid; i < N; i += GRAPH_THREADS) { H[pgo_tri(i) + i] += lambda; L.y[i] = L.g[i]; }
    for (int j = 0; j < N; j++) {
        __syncthreads();
        const double piv = H[pgo_tri(j) + j];
        if (!(piv > 0.0) || !finite_d(piv)) { __syncthreads(); return false; }
        const double ljj = sqrt(piv);
        __syncthreads();
        for (int i = j + 1 + tid; i < N; i += GRAPH_THREADS) {   // the column, scaled, and a copy of it in LDS (d is free until the substitutions end)
            const double lij = H[pgo_tri(i) + j] / ljj;
            H[pgo_tri(i) + j] = lij;
            L.d[i] = lij;
        }
        if (tid == 0) H[pgo_tri(j) + j] = ljj;
        __syncthreads();
        // the trailing update: a wave per row, its lanes along the row (consecutive addresses in either storage); every entry takes the same
        // one product and one difference per column whichever thread holds it
        for (int i = j + 1 + (tid >> 6); i < N; i += GRAPH_THREADS / 64) {
            const double lij = L.d[i];
            double* __restrict__ const Hi = H + pgo_tri(i);
            for (int k = j + 1 + (tid & 63); k <= i; k += 64) Hi[k] -= lij * L.d[k];
        }
    }
    // L y = g (y starts as g)
    for (int j = 0; j < N; j++) {
        __syncthreads();
        const double yj = L.y[j] / H[pgo_tri(j) + j];
        for (int i = j + 1 + ((tid - (j + 1)) & (GRAPH_THREADS - 1)); i < N; i += GRAPH_THREADS) L.y[i] -= H[pgo_tri(i) + j] * yj;
        __syncthreads();
        if (tid == 0) L.y[j] = yj;
    }
    // L^T d = y (in y, then copied)
    for (int j = N - 1; j >= 0; j--) {
        __syncthreads();
        const double dj = L.y[j] / H[pgo_tri(j) + j];
        for (int i = tid; i < j; i += GRAPH_THREADS) L.y[i] -= H[pgo_tri(j) + i] * dj;
        __syncthreads();
        if (tid == 0) L.y[j] = dj;
    }
    __syncthreads();
    for (int i = tid; i < N; i += GRAPH_THREADS) L.d[i] = L.y[i];
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(GRAPH_THREADS) void pgo_kernel(const salve_graph_row_t* __restrict__ rows, int n_rows, const int32_t* __restrict__ floor_start,
                                                            const int32_t* __restrict__ n_nodes, int max_nodes,
                                                            const salve_graph_node_out_t* __restrict__ init, PgoParams P,
                                                            salve_graph_node_out_t* __restrict__ out_nodes, double* __restrict__ out_pose,
                                                            salve_graph_pgo_floor_out_t* __restrict__ out_floors, double* __restrict__ workspace,
                                                            int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int floor = blockIdx.x, tid = threadIdx.x, M = max_nodes;
    PgoLds L;
    L.H = reinterpret_cast<double*>(smem);
    L.X = L.H + pgo_tri(3 * pgo_lds_nodes(M));
    L.XT = L.X + 5 * (size_t)M;
    L.g = L.XT + 5 * (size_t)M;
    L.y = L.g + 3 * (size_t)M;
    L.d = L.y + 3 * (size_t)M;
    L.partial = L.d + 3 * (size_t)M;
    L.idx = reinterpret_cast<int32_t*>(L.partial + GRAPH_THREADS);
    L.scal = L.idx + M;

    int lo = floor_start[floor], hi = floor_start[floor + 1], n = n_nodes[floor];
    const bool bad_extent = lo < 0 || hi < lo || hi > n_rows;
    const bool bad_nodes = n < 0 || n > max_nodes;
    if (bad_extent) lo = hi = 0;
    if (bad_nodes) n = 0;
    const salve_graph_node_out_t* __restrict__ const in = init + (size_t)floor * (size_t)M;
    salve_graph_node_out_t* __restrict__ const nodes = out_nodes + (size_t)floor * (size_t)M;
    double* __restrict__ const pose = out_pose + 3 * (size_t)floor * (size_t)M;

    if (tid < PS_COUNT) L.scal[tid] = 0;
    __syncthreads();
    bool bad = graph_rows_malformed(rows, lo, hi, n, tid);
    bool localized = false;
    if (tid < n) {
        const int parent = in[tid].parent;
        if (parent < -1 || parent >= n) bad = true;
        localized = in[tid].localized != 0;
        L.idx[tid] = localized ? 0 : -1;
    }
    if (bad) L.scal[PS_BAD] = 1;
    __syncthreads();
    int origin = -1, n_unknown = 0;
    if (!(L.scal[PS_BAD] || bad_extent || bad_nodes)) {
        int before = 0;
        for (int v = 0; v < n; v++) {
            if (L.idx[v] < 0) continue;
            if (origin < 0) origin = v;
            if (v < tid) before++;
            n_unknown++;
        }
        __syncthreads();
        if (tid < n && localized) L.idx[tid] = before;
    }
    salve_graph_pgo_floor_out_t fo;
    fo.n_unknown_nodes = fo.n_factors = fo.n_iterations = fo.n_rejected = fo.n_downweighted = 0;
    fo.stop_reason = SALVE_PGO_STOP_EMPTY;
    fo.lambda = PGO_LAMBDA_INITIAL;
    fo.cost_initial = fo.cost_final = qnan();
    if (origin < 0) {   // (workgroup-uniform) malformed, or nothing localized: the floor is written empty
        if (tid < n) {
            nodes[tid] = empty_node_out();
            pose[3 * tid + 0] = pose[3 * tid + 1] = pose[3 * tid + 2] = qnan();
        }
        if (tid == 0) {
            out_floors[floor] = fo;
            if (status && (L.scal[PS_BAD] || bad_extent || bad_nodes)) atomicOr(status, SALVE_STATUS_BAD_GRAPH_ROW);
        }
        return;
    }
    const int N = 3 * n_unknown;
    if (n_unknown > pgo_lds_nodes(M)) L.H = workspace + (size_t)floor * pgo_floor_workspace_doubles(M);   // (only when M > SALVE_PGO_LDS_NODES)

    // the initial estimate; the factors counted and their inputs checked
    if (tid < n && localized) {
        double* X = L.X + 5 * tid;
        X[0] = (double)in[tid].t[0]; X[1] = (double)in[tid].t[1];
        X[2] = atan2((double)in[tid].R[2], (double)in[tid].R[0]);
        X[3] = cos(X[2]); X[4] = sin(X[2]);
        if (!finite_d(((X[0] + X[1]) + (double)in[tid].R[0]) + (double)in[tid].R[2])) L.scal[PS_NONFINITE] = 1;
    }
    __syncthreads();
    {
        int mine = 0;
        bool nonfinite = false;
        for (int r = lo + tid; r < hi; r += GRAPH_THREADS) {
            if (!row_is_factor(rows + r, L, P.conf_thr)) continue;
            mine++;
            const double sum = (((double)rows[r].t[0] + (double)rows[r].t[1]) + (double)rows[r].R[0]) + (double)rows[r].R[2];
            if (!finite_d(sum)) nonfinite = true;
        }
        if (mine) atomicAdd(&L.scal[PS_FACTORS], mine);
        if (nonfinite) L.scal[PS_NONFINITE] = 1;
    }
    __syncthreads();
    fo.n_unknown_nodes = n_unknown;
    fo.n_factors = 1 + L.scal[PS_FACTORS];

    double lambda = PGO_LAMBDA_INITIAL;
    int stop = 0, iterations = 0, rejected = 0;
    if (L.scal[PS_NONFINITE]) {
        stop = SALVE_PGO_STOP_NON_FINITE;
    } else {
        double E = pgo_cost(P, L, L.X, rows, lo, hi, origin, tid);
        fo.n_downweighted = L.scal[PS_DOWN];
        fo.cost_initial = fo.cost_final = E;
        while (!stop) {
            if (iterations >= P.max_iterations) { stop = SALVE_PGO_STOP_MAX_ITERATIONS; break; }
            iterations++;
            double En = 0.0;
            int down = 0;
            for (;;) {
                pgo_linearise(P, L, rows, lo, hi, n, N, origin, tid);
                bool accepted = false;
                if (pgo_solve(L, N, lambda, tid)) {
                    if (tid < n && localized) {   // the retraction
                        const double* X = L.X + 5 * tid;
                        double* T = L.XT + 5 * tid;
                        const double* d = L.d + 3 * L.idx[tid];
                        T[0] = X[0] + (X[3] * d[0] - X[4] * d[1]);
                        T[1] = X[1] + (X[4] * d[0] + X[3] * d[1]);
                        T[2] = X[2] + d[2];
                        T[3] = cos(T[2]); T[4] = sin(T[2]);
                    }
                    __syncthreads();
                    En = pgo_cost(P, L, L.XT, rows, lo, hi, origin, tid);
                    down = L.scal[PS_DOWN];
                    accepted = finite_d(En) && En <= E;
                }
                if (accepted) break;
                rejected++;
                lambda *= PGO_LAMBDA_FACTOR;
                if (lambda > PGO_LAMBDA_UPPER) { stop = SALVE_PGO_STOP_LAMBDA; break; }
            }
            if (stop) break;
            __syncthreads();
            if (tid < n && localized)
                for (int k = 0; k < 5; k++) L.X[5 * tid + k] = L.XT[5 * tid + k];
            __syncthreads();
            const double decrease = E - En, E_old = E;
            E = En;
            fo.cost_final = E;
            fo.n_downweighted = down;
            lambda /= PGO_LAMBDA_FACTOR;
            if (decrease <= P.abs_tol) stop = SALVE_PGO_STOP_ABSOLUTE;
            else if (decrease / E_old <= P.rel_tol) stop = SALVE_PGO_STOP_RELATIVE;
        }
    }
    fo.n_iterations = iterations;
    fo.n_rejected = rejected;
    fo.stop_reason = stop;
    fo.lambda = lambda;

    if (tid < n) {
        salve_graph_node_out_t o = empty_node_out();
        double px = qnan(), py = qnan(), pth = qnan();
        if (localized) {
            const double* X = L.X + 5 * tid;
            px = X[0]; py = X[1]; pth = X[2];
            o.localized = 1; o.parent = in[tid].parent; o.depth = in[tid].depth;
            o.R[0] = (float)X[3]; o.R[1] = (float)-X[4]; o.R[2] = (float)X[4]; o.R[3] = (float)X[3];
            o.t[0] = (float)px; o.t[1] = (float)py;
            o.s = 1.0;
        }
        nodes[tid] = o;
        pose[3 * tid + 0] = px; pose[3 * tid + 1] = py; pose[3 * tid + 2] = pth;
    }
    if (tid == 0) out_floors[floor] = fo;
}

std::mutex g_pgo_mu;
size_t g_pgo_lds_attr[64];

bool positive(double v) { return v > 0.0 && v == v; }

}  // namespace

extern "C" {

size_t salve_pose_graph_optimise_workspace_bytes(int32_t n_floors, int32_t max_nodes) {
    if (n_floors <= 0 || max_nodes < 1 || max_nodes > SALVE_GRAPH_MAX_NODES) return 0;
    return (size_t)n_floors * pgo_floor_workspace_doubles(max_nodes) * sizeof(double);
}

int salve_pose_graph_optimise(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                              int32_t max_nodes, float confidence_threshold, const salve_graph_node_out_t* init, int32_t robust, double huber_k,
                              const double* odometry_sigmas, const double* prior_sigmas, int32_t max_iterations, double relative_error_tol,
                              double absolute_error_tol, salve_graph_node_out_t* out_nodes, double* out_pose,
                              salve_graph_pgo_floor_out_t* out_floors, void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    if (n_rows < 0 || n_floors < 0) { salve_fail("salve_pose_graph_optimise: negative count"); return SALVE_ERR_BAD_ARG; }
    if (max_nodes < 1 || max_nodes > SALVE_GRAPH_MAX_NODES) {
        salve_fail("salve_pose_graph_optimise: max_nodes must lie in 1 .. 256 (a floor of more panoramas is not supported)");
        return SALVE_ERR_BAD_ARG;
    }
    if (confidence_threshold != confidence_threshold) { salve_fail("salve_pose_graph_optimise: the threshold is NaN"); return SALVE_ERR_BAD_ARG; }
    if (robust != 0 && robust != 1) { salve_fail("salve_pose_graph_optimise: robust must be 0 or 1"); return SALVE_ERR_BAD_ARG; }
    if (!odometry_sigmas || !prior_sigmas) { salve_fail("salve_pose_graph_optimise: null sigmas"); return SALVE_ERR_BAD_ARG; }
    for (int i = 0; i < 3; i++)
        if (!positive(odometry_sigmas[i]) || !positive(prior_sigmas[i])) {
            salve_fail("salve_pose_graph_optimise: a sigma is NaN or not positive");
            return SALVE_ERR_BAD_ARG;
        }
    if (!positive(huber_k) || !positive(relative_error_tol) || !positive(absolute_error_tol)) {
        salve_fail("salve_pose_graph_optimise: huber_k or a tolerance is NaN or not positive");
        return SALVE_ERR_BAD_ARG;
    }
    if (max_iterations < 0) { salve_fail("salve_pose_graph_optimise: negative max_iterations"); return SALVE_ERR_BAD_ARG; }
    if (n_floors == 0) return SALVE_OK;
    if (!floor_start || !n_nodes || !init || !out_nodes || !out_pose || !out_floors || (n_rows > 0 && !rows)) {
        salve_fail("salve_pose_graph_optimise: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    const auto mis = [](const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (mis(rows, 8) || mis(init, 8) || mis(out_nodes, 8) || mis(out_pose, 8) || mis(out_floors, 8) || mis(workspace, 8) || mis(floor_start, 4) ||
        mis(n_nodes, 4) || mis(status, 4)) {
        salve_fail("salve_pose_graph_optimise: rows, init, out_nodes, out_pose, out_floors and the workspace must be 8-byte aligned, the other "
                   "tables 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    const size_t need = salve_pose_graph_optimise_workspace_bytes(n_floors, max_nodes);
    if (need > 0 && (!workspace || workspace_bytes < need)) { salve_fail("salve_pose_graph_optimise: workspace too small"); return SALVE_ERR_WORKSPACE; }
    PgoParams P;
    for (int i = 0; i < 3; i++) { P.sig_odo[i] = odometry_sigmas[i]; P.sig_prior[i] = prior_sigmas[i]; }
    P.k = huber_k; P.rel_tol = relative_error_tol; P.abs_tol = absolute_error_tol;
    P.robust = robust; P.max_iterations = max_iterations; P.conf_thr = confidence_threshold;
    const size_t lds = pgo_lds_bytes(max_nodes);
    if (lds > 64 * 1024) {   // opt in to more than 64 KB of dynamic LDS, per device
        std::lock_guard<std::mutex> lock(g_pgo_mu);
        int dev = 0;
        SALVE_HIP_CHECK(hipGetDevice(&dev));
        const int slot = (dev >= 0 && dev < 64) ? dev : 0;
        if (dev != slot || lds > g_pgo_lds_attr[slot]) {
            SALVE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pgo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g_pgo_lds_attr[slot] = lds;
        }
    }
    hipLaunchKernelGGL(pgo_kernel, dim3((unsigned)n_floors), dim3(GRAPH_THREADS), lds, (hipStream_t)stream, rows, n_rows, floor_start, n_nodes, max_nodes,
                       init, P, out_nodes, out_pose, out_floors, static_cast<double*>(workspace), status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
