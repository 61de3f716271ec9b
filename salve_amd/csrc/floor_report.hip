// floor_report.hip -- the floor reconstruction report for gfx950 (MI355X): the Sim(3) alignment of a floor's estimated poses to the truth over
// many RANSAC subsets, the pick, the aligned poses, the pose errors, and the raster IoU of the two floor plans.  Any number of floors per call.
// Compile with -ffp-contract=off -fno-slp-vectorize (pose_graph_common.h): no product below may be fused into a sum.
//
// The reference does this per floor on the host:
//   salve/common/floor_reconstruction_report.py:50-149   from_est_floor_pose_graph       (the report)
//   salve/common/posegraph2d.py:326-383                  align_by_Sim3_to_ref_pose_graph, apply_Sim3   (launch 2)
//   salve/utils/ransac.py:14-129                         ransac_align_poses_sim3_ignore_missing, compute_pose_errors_3d   (launches 1, 2)
//   salve/common/floor_reconstruction_report.py:271-338  render_raster_occupancy, rasterize_room   (salve_floor_iou)
// include/salve_hip.h (salve_floor_align, salve_floor_iou) states the rules; this file states how they run.
//
//   floor_align_kernel    launch 1: one wavefront per hypothesis, four hypotheses per workgroup of 256 threads.  The floor's two pose tables are
//                         widened to float64 into LDS (24 KiB + 256 flags) once per DISTINCT floor among the four: once when they share it.
//   floor_pick_kernel     launch 2: one workgroup per floor; thread 0 scans the hypotheses, every thread applies the winner to its panorama.
//   floor_rooms_check_kernel  salve_floor_iou, launch 0: one workgroup verifies that the rooms' vertex extents ascend.
//   floor_pose_kernel     launch 1: one workgroup per floor and table; a thread poses its panorama's room to int32 pixels and takes the
//                         bounding box.
//   floor_raster_kernel   launch 2: one workgroup per 16 x 16 pixel tile of one floor; the polygons whose box meets the tile are staged in LDS
//                         1024 edges at a time (20 KiB), every thread evaluates the fill rule for its pixel; wave ballots, one integer atomic
//                         per wave and counter.
//   floor_iou_kernel      launch 3: one thread per floor divides.
//
// Sums: float64, one order, no floating-point atomic.  Launch 1: lane l of the wavefront adds the values of its indices l, l + 64, l + 128,
// l + 192 ascending from 0.0; the 64 partial sums fold by halving (p[l] += p[l + 32], then 16, ... 1).  Launch 2: thread t holds panorama t's
// value (0.0 without one); the 256 values fold by halving (128, 64, ... 1).  A NaN mean is written as the one quiet NaN 0x7FF8000000000000.
//
// Bound: launch 1 is latency-bound per wavefront -- ten folds of six shuffles, two atan2 per pair and Karcher step, one sin and cos per step --
// and throughput-bound over a thousand hypotheses per floor; the raster is bound by the per-pixel edge loop over the tile's survivors.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "pose_graph_common.h"
#include "salve_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int HYPS_PER_WG = GRAPH_THREADS / WAVE;
constexpr int MASK_WORDS = SALVE_FLOOR_MASK_WORDS;
static_assert(MASK_WORDS * 32 == SALVE_GRAPH_MAX_NODES, "one mask bit per panorama");
constexpr double RAD2DEG = 57.29577951308232;   // 180 / pi, numpy's rad2deg factor
constexpr unsigned long long QNAN_BITS = 0x7FF8000000000000ull;

__device__ __forceinline__ double qnan() { return __longlong_as_double((long long)QNAN_BITS); }
__device__ __forceinline__ double canonical(double x) { return x != x ? qnan() : x; }

// the 64 partial sums folded by halving; the total in every lane
__device__ __forceinline__ double wave_fold(double v) {
    for (int s = WAVE / 2; s > 0; s >>= 1) {
        const double o = __shfl_down(v, s, WAVE);
        v = v + o;
    }
    return __shfl(v, 0, WAVE);
}

struct FloorPoses {   // a floor's two tables, widened
    double aR[SALVE_GRAPH_MAX_NODES][4], at[SALVE_GRAPH_MAX_NODES][2];   // truth
    double bR[SALVE_GRAPH_MAX_NODES][4], bt[SALVE_GRAPH_MAX_NODES][2];   // estimate
    unsigned char both[SALVE_GRAPH_MAX_NODES];
};

struct Mat2 {
    double m00, m01, m10, m11;
};

// aRb_i = Ra_i * Rb_i^T
__device__ __forceinline__ Mat2 rel_rot(const FloorPoses& P, int i) {
    Mat2 X;
    X.m00 = P.aR[i][0] * P.bR[i][0] + P.aR[i][1] * P.bR[i][1];
    X.m01 = P.aR[i][0] * P.bR[i][2] + P.aR[i][1] * P.bR[i][3];
    X.m10 = P.aR[i][2] * P.bR[i][0] + P.aR[i][3] * P.bR[i][1];
    X.m11 = P.aR[i][2] * P.bR[i][2] + P.aR[i][3] * P.bR[i][3];
    return X;
}

__device__ __forceinline__ salve_floor_hyp_out_t empty_hyp_out(int floor) {
    salve_floor_hyp_out_t o;
    o.R[0] = 1.0; o.R[1] = 0.0; o.R[2] = 0.0; o.R[3] = 1.0;
    o.t[0] = o.t[1] = 0.0;
    o.s = 1.0;
    o.rot_err = o.trans_err = qnan();
    o.n_pairs = 0;
    o.floor = floor;
    return o;
}

// rot_i and trans_i of one panorama under (R, t, s): the rules of step 8
__device__ __forceinline__ void pose_errors(const double* aR, const double* at, const double* bR, const double* bt, const Mat2& R, double tx, double ty,
                                            double s, double& rot, double& trans) {
    const double p00 = R.m00 * bR[0] + R.m01 * bR[2], p10 = R.m10 * bR[0] + R.m11 * bR[2];
    const double e00 = aR[0] * p00 + aR[2] * p10, e10 = aR[1] * p00 + aR[3] * p10;
    rot = fabs(atan2(e10, e00)) * RAD2DEG;
    const double ux = s * ((R.m00 * bt[0] + R.m01 * bt[1]) + tx), uy = s * ((R.m10 * bt[0] + R.m11 * bt[1]) + ty);
    const double dx = at[0] - ux, dy = at[1] - uy;
    trans = sqrt(dx * dx + dy * dy);
}

// One hypothesis by one wavefront over the floor in LDS.
__device__ salve_floor_hyp_out_t align_wave(const FloorPoses& P, int n, const uint32_t* __restrict__ mask, int lane, int floor) {
    bool pr[4];
    int n_pairs = 0, first = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = lane + WAVE * k;
        pr[k] = i < n && ((mask[i >> 5] >> (i & 31)) & 1u) != 0 && P.both[i] != 0;
        const unsigned long long b = __ballot(pr[k]);
        n_pairs += __popcll(b);
        if (first < 0 && b) first = WAVE * k + __builtin_ctzll(b);
    }
    const double dn = (double)n_pairs;
    Mat2 R = {1.0, 0.0, 0.0, 1.0};
    double tx = 0.0, ty = 0.0, s = 1.0;
    if (n_pairs >= 2) {   // (wave-uniform)
        R = rel_rot(P, first);
        for (int step = 0; step < 2; step++) {   // two Karcher steps
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!pr[k]) continue;
                const Mat2 X = rel_rot(P, lane + WAVE * k);
                const double m00 = R.m00 * X.m00 + R.m10 * X.m10, m10 = R.m01 * X.m00 + R.m11 * X.m10;
                acc = acc + atan2(m10, m00);
            }
            const double m = wave_fold(acc) / dn;
            const double c = cos(m), sn = sin(m);
            Mat2 Q;
            Q.m00 = R.m00 * c + R.m01 * sn;
            Q.m01 = R.m00 * (-sn) + R.m01 * c;
            Q.m10 = R.m10 * c + R.m11 * sn;
            Q.m11 = R.m10 * (-sn) + R.m11 * c;
            R = Q;
        }
        double sax = 0.0, say = 0.0, sbx = 0.0, sby = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!pr[k]) continue;
            const int i = lane + WAVE * k;
            sax = sax + P.at[i][0]; say = say + P.at[i][1];
            sbx = sbx + P.bt[i][0]; sby = sby + P.bt[i][1];
        }
        const double cax = wave_fold(sax) / dn, cay = wave_fold(say) / dn, cbx = wave_fold(sbx) / dn, cby = wave_fold(sby) / dn;
        double sy = 0.0, sx = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!pr[k]) continue;
            const int i = lane + WAVE * k;
            const double dbx = P.bt[i][0] - cbx, dby = P.bt[i][1] - cby;
            const double rbx = R.m00 * dbx + R.m01 * dby, rby = R.m10 * dbx + R.m11 * dby;
            const double dax = P.at[i][0] - cax, day = P.at[i][1] - cay;
            sy = sy + (dax * rbx + day * rby);
            sx = sx + (rbx * rbx + rby * rby);
        }
        const double y = wave_fold(sy), x = wave_fold(sx);
        s = y / x;
        const double rcx = R.m00 * cbx + R.m01 * cby, rcy = R.m10 * cbx + R.m11 * cby;
        if (s != s || s == 0.0) {   // this project's own fallback (salve_hip.h)
            s = 1.0;
            tx = cax - rcx; ty = cay - rcy;
        } else {
            tx = (cax - s * rcx) / s; ty = (cay - s * rcy) / s;
        }
    }
    double srot = 0.0, strans = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!pr[k]) continue;
        const int i = lane + WAVE * k;
        double rot, trans;
        pose_errors(P.aR[i], P.at[i], P.bR[i], P.bt[i], R, tx, ty, s, rot, trans);
        srot = srot + rot;
        strans = strans + trans;
    }
    salve_floor_hyp_out_t o;
    o.R[0] = canonical(R.m00); o.R[1] = canonical(R.m01); o.R[2] = canonical(R.m10); o.R[3] = canonical(R.m11);   // (a NaN pose: the one quiet NaN)
    o.t[0] = canonical(tx); o.t[1] = canonical(ty);
    o.s = canonical(s);
    o.rot_err = canonical(wave_fold(srot) / dn);   // no pair: NaN, as np.mean([])
    o.trans_err = canonical(wave_fold(strans) / dn);
    o.n_pairs = n_pairs;
    o.floor = floor;
    return o;
}

__device__ __forceinline__ bool node_extent_ok(int lo, int hi, int n_nodes) {
    return lo >= 0 && hi >= lo && hi <= n_nodes && hi - lo <= SALVE_GRAPH_MAX_NODES;
}

__global__ __launch_bounds__(GRAPH_THREADS) void floor_align_kernel(const int32_t* __restrict__ node_start, int n_floors, int n_nodes,
                                                                    const salve_graph_node_out_t* __restrict__ truth,
                                                                    const salve_graph_node_out_t* __restrict__ est,
                                                                    const int32_t* __restrict__ hyp_start, const uint32_t* __restrict__ hyp_mask,
                                                                    int n_hyps, salve_floor_hyp_out_t* __restrict__ out_hyps) {
    __shared__ FloorPoses P;
    __shared__ int s_floor[HYPS_PER_WG];
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int h0 = blockIdx.x * HYPS_PER_WG, h = h0 + wave;

    // every hypothesis's floor: the lowest one whose well-formed extent holds it
    if (tid < HYPS_PER_WG) s_floor[tid] = INT_MAX;
    __syncthreads();
    for (int f = tid; f < n_floors; f += GRAPH_THREADS) {
        const int hs = hyp_start[f], he = hyp_start[f + 1];
        if (hs < 0 || hs > he || he > n_hyps) continue;
        for (int w = 0; w < HYPS_PER_WG; w++)
            if (hs <= h0 + w && h0 + w < he) atomicMin(&s_floor[w], f);
    }
    __syncthreads();
    const int floor = s_floor[wave];
    bool done = h >= n_hyps;
    if (!done && floor == INT_MAX) {   // (wave-uniform) no floor names it
        if (lane == 0) out_hyps[h] = empty_hyp_out(-1);
        done = true;
    }
    // one pass per DISTINCT floor among the four (workgroup-uniform loop: s_floor is shared)
    for (int w = 0; w < HYPS_PER_WG; w++) {
        const int f = s_floor[w];
        bool seen = f == INT_MAX || h0 + w >= n_hyps;
        for (int v = 0; v < w; v++) seen = seen || s_floor[v] == f;
        if (seen) continue;
        const int lo = node_start[f], hi = node_start[f + 1];
        const bool ok = node_extent_ok(lo, hi, n_nodes);   // verified before an address is formed from it
        const int n = ok ? hi - lo : 0;
        __syncthreads();   // the previous floor's readers are done
        if (tid < n) {
            const salve_graph_node_out_t a = truth[lo + tid], b = est[lo + tid];
            for (int k = 0; k < 4; k++) { P.aR[tid][k] = (double)a.R[k]; P.bR[tid][k] = (double)b.R[k]; }
            for (int k = 0; k < 2; k++) { P.at[tid][k] = (double)a.t[k]; P.bt[tid][k] = (double)b.t[k]; }
            P.both[tid] = a.localized != 0 && b.localized != 0;
        }
        __syncthreads();
        if (!done && floor == f) {   // (wave-uniform)
            const salve_floor_hyp_out_t o = ok ? align_wave(P, n, hyp_mask + (size_t)h * MASK_WORDS, lane, f) : empty_hyp_out(f);
            if (lane == 0) out_hyps[h] = o;
            done = true;
        }
    }
}

__global__ __launch_bounds__(GRAPH_THREADS) void floor_pick_kernel(const int32_t* __restrict__ node_start, int n_nodes,
                                                                   const salve_graph_node_out_t* __restrict__ truth,
                                                                   const salve_graph_node_out_t* __restrict__ est,
                                                                   const int32_t* __restrict__ hyp_start, int n_hyps,
                                                                   const double* __restrict__ gt_scale, const double* __restrict__ metres,
                                                                   const salve_floor_hyp_out_t* __restrict__ hyps,
                                                                   salve_graph_node_out_t* __restrict__ out_nodes, double* __restrict__ out_rot_err,
                                                                   double* __restrict__ out_trans_err, salve_floor_align_out_t* __restrict__ out_floors,
                                                                   int32_t* __restrict__ status) {
    __shared__ double part[GRAPH_THREADS];
    __shared__ int s_bad, s_best;
    const int floor = blockIdx.x, tid = threadIdx.x;
    int lo = node_start[floor], hi = node_start[floor + 1];
    int hs = hyp_start[floor], he = hyp_start[floor + 1];
    const bool bad_nodes = !node_extent_ok(lo, hi, n_nodes);
    const bool bad_hyps = hs < 0 || he < hs || he > n_hyps;
    if (bad_nodes) lo = hi = 0;
    if (bad_hyps) hs = he = 0;
    const int n = hi - lo;
    if (tid == 0) { s_bad = 0; s_best = -1; }
    __syncthreads();
    bool bad = false;
    for (int h = hs + tid; h < he; h += GRAPH_THREADS)
        if (hyps[h].floor != floor) bad = true;   // a lower floor's extent holds it too
    if (bad) s_bad = 1;
    __syncthreads();
    salve_floor_align_out_t fo;
    fo.best = -1; fo.n_hyps = 0; fo.n_est = 0; fo.n_gt = 0;
    fo.avg_rot_err = fo.avg_trans_err = fo.percent_localized = qnan();
    fo.R[0] = fo.R[1] = fo.R[2] = fo.R[3] = fo.t[0] = fo.t[1] = fo.s = qnan();
    if (s_bad || bad_nodes || bad_hyps) {   // (workgroup-uniform) the floor is written empty
        if (tid < n) { out_nodes[lo + tid] = empty_node_out(); out_rot_err[lo + tid] = qnan(); out_trans_err[lo + tid] = qnan(); }
        if (tid == 0) {
            out_floors[floor] = fo;
            if (status) atomicOr(status, SALVE_STATUS_BAD_FLOOR_TABLE);
        }
        return;
    }
    // the pick (ransac.py:36-77): in order from +inf, +inf; a NaN never replaces the best
    if (tid == 0) {
        double best_rot = __longlong_as_double(0x7FF0000000000000ll), best_trans = best_rot;
        int best = -1;
        for (int k = 0; k < he - hs; k++) {
            const double rot = hyps[hs + k].rot_err, trans = hyps[hs + k].trans_err;
            if (trans <= best_trans && rot <= best_rot) { best = k; best_rot = rot; best_trans = trans; }
        }
        s_best = best;
    }
    salve_graph_node_out_t a = empty_node_out(), b = empty_node_out();
    if (tid < n) { a = truth[lo + tid]; b = est[lo + tid]; }
    const int n_gt = __syncthreads_count(a.localized != 0);
    const int n_est = __syncthreads_count(b.localized != 0);   // (its barrier also publishes s_best)
    const int best = s_best;
    salve_floor_hyp_out_t w = empty_hyp_out(floor);
    if (best >= 0) w = hyps[hs + best];

    // apply (posegraph2d.py:351-383): a_Sim2_b.compose(b_Sim2_i) under the float32 rules, then (R, t * (float)scale, gt_scale)
    salve_graph_node_out_t o = empty_node_out();
    double rot = qnan(), trans = qnan();
    bool measured = false;
    if (best >= 0 && b.localized != 0) {
        Sim2 A, B;
        A.R00 = (float)w.R[0]; A.R01 = (float)w.R[1]; A.R10 = (float)w.R[2]; A.R11 = (float)w.R[3];
        A.tx = (float)w.t[0]; A.ty = (float)w.t[1]; A.s = w.s;
        B.R00 = b.R[0]; B.R01 = b.R[1]; B.R10 = b.R[2]; B.R11 = b.R[3];
        B.tx = b.t[0]; B.ty = b.t[1]; B.s = 1.0;
        const Sim2 S = sim2_compose(A, B);
        const float sf = (float)S.s;
        o.localized = 1;
        o.R[0] = S.R00; o.R[1] = S.R01; o.R[2] = S.R10; o.R[3] = S.R11;
        o.t[0] = S.tx * sf; o.t[1] = S.ty * sf;
        o.s = gt_scale[floor];
        if (a.localized != 0) {   // the floor's errors: the aligned float32 pose, widened, against the truth
            const double aR[4] = {(double)a.R[0], (double)a.R[1], (double)a.R[2], (double)a.R[3]}, at[2] = {(double)a.t[0], (double)a.t[1]};
            const double bR[4] = {(double)o.R[0], (double)o.R[1], (double)o.R[2], (double)o.R[3]}, bt[2] = {(double)o.t[0], (double)o.t[1]};
            const Mat2 I = {1.0, 0.0, 0.0, 1.0};
            pose_errors(aR, at, bR, bt, I, 0.0, 0.0, 1.0, rot, trans);
            measured = true;
        }
    }
    if (tid < n) { out_nodes[lo + tid] = o; out_rot_err[lo + tid] = canonical(rot); out_trans_err[lo + tid] = canonical(trans); }
    const int n_both = __syncthreads_count(measured);
    double total[2];
    for (int q = 0; q < 2; q++) {
        __syncthreads();   // the previous fold's readers are done
        part[tid] = measured ? (q == 0 ? rot : trans) : 0.0;
        __syncthreads();
        for (int s = GRAPH_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) part[tid] = part[tid] + part[tid + s];
            __syncthreads();
        }
        total[q] = part[0];
    }
    if (tid == 0) {
        fo.best = best; fo.n_hyps = he - hs; fo.n_est = n_est; fo.n_gt = n_gt;
        fo.percent_localized = canonical((double)n_est / (double)n_gt * 100.0);
        if (best >= 0) {
            fo.avg_rot_err = canonical(total[0] / (double)n_both);
            fo.avg_trans_err = canonical(total[1] / (double)n_both * metres[floor]);
            for (int k = 0; k < 4; k++) fo.R[k] = w.R[k];
            fo.t[0] = w.t[0]; fo.t[1] = w.t[1]; fo.s = w.s;
        }
        out_floors[floor] = fo;
    }
}

// ------------------------------------------------------------------------------------------------ salve_floor_iou
constexpr int TILE = 16;
constexpr int EDGE_CAP = 1024;
constexpr double PIXEL_LIMIT = 16777216.0;   // 2^24 pixels: pack_layouts' limit

// floor division (Python's `//`) for a positive divisor
__device__ __forceinline__ long long floordiv(long long a, long long b) {
    long long q = a / b;
    if ((a % b != 0) && (a < 0)) q--;
    return q;
}

// oracle.layout_oracle.on_line8: is (x, y) a pixel of the 8-connected line from (x1, y1) to (x2, y2)?  (layout.hip's, restated)
__device__ __forceinline__ bool on_line8(int x, int y, int x1, int y1, int x2, int y2) {
    const int dx = abs(x2 - x1), dy = abs(y2 - y1);
    const int sx = x2 >= x1 ? 1 : -1, sy = y2 >= y1 ? 1 : -1;
    if (dy > dx) {
        const int j = (y - y1) * sy;
        if (j < 0 || j > dy) return false;
        const long long m = j == 0 ? 0 : max(0ll, -floordiv(-(2ll * dx * j - dy), 2ll * dy));
        return (long long)((x - x1) * sx) == m;
    }
    const int j = (x - x1) * sx;
    if (j < 0 || j > dx) return false;
    if (dx == 0) return y == y1;
    const long long m = j == 0 ? 0 : max(0ll, -floordiv(-(2ll * dy * j - dx), 2ll * dx));
    return (long long)((y - y1) * sy) == m;
}

// The vertex extents of ALL panoramas, sound or not: the posed pixels live in the workspace by vertex index, so two panoramas that claim one
// vertex would overwrite each other's pixels across floors.  One workgroup; *flag = 1 unless room_off ascends within [0, n_room_xy].
__global__ __launch_bounds__(GRAPH_THREADS) void floor_rooms_check_kernel(const int64_t* __restrict__ room_off, int n_nodes, long long n_room_xy,
                                                                          int32_t* __restrict__ flag) {
    int bad = 0;
    for (int i = threadIdx.x; i < n_nodes; i += GRAPH_THREADS) {
        const long long v0 = room_off[i], v1 = room_off[i + 1];
        if (v0 < 0 || v1 < v0 || v1 > n_room_xy) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) *flag = bad;
}

__global__ __launch_bounds__(GRAPH_THREADS) void floor_pose_kernel(const int32_t* __restrict__ rooms_bad, const double* __restrict__ room_xy,
                                                                   const int64_t* __restrict__ room_off,
                                                                   long long n_room_xy, const int32_t* __restrict__ node_start, int n_nodes,
                                                                   const salve_graph_node_out_t* __restrict__ est,
                                                                   const salve_graph_node_out_t* __restrict__ truth,
                                                                   const double* __restrict__ metres, double off_x, double off_y, double px_per_m,
                                                                   int4* __restrict__ ws_box, int2* __restrict__ ws_px,
                                                                   salve_floor_iou_out_t* __restrict__ out) {
    const int floor = blockIdx.x, tb = blockIdx.y, tid = threadIdx.x;
    const int lo = node_start[floor], hi = node_start[floor + 1];
    if (!node_extent_ok(lo, hi, n_nodes) || *rooms_bad != 0) {   // (workgroup-uniform)
        if (tid == 0) atomicOr(&out[floor].bad, 1);
        return;
    }
    const salve_graph_node_out_t* __restrict__ const table = tb ? truth : est;
    const double m = metres[floor];
    int bad = 0;
    if (tid < hi - lo) {
        const int i = lo + tid;
        long long v0 = room_off[i], v1 = room_off[i + 1];
        if (v0 < 0 || v1 < v0 || v1 > n_room_xy) { bad = 1; v0 = v1 = 0; }
        const salve_graph_node_out_t p = table[i];
        int4 box = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);   // x0, y0, x1, y1: empty
        if (p.localized != 0 && !bad) {
            const double r00 = (double)p.R[0], r01 = (double)p.R[1], r10 = (double)p.R[2], r11 = (double)p.R[3];
            const double tx = (double)p.t[0], ty = (double)p.t[1];
            for (long long k = v0; k < v1; k++) {
                const double x = room_xy[2 * k], y = room_xy[2 * k + 1];
                double px = x * r00 + y * r01, py = x * r10 + y * r11;   // v @ R.T, un-fused
                px = px + tx; py = py + ty;
                px = px * p.s; py = py * p.s;
                px = px * m; py = py * m;
                px = px + off_x; py = py + off_y;                        // bevimg_Sim2_world: rotation I, + t, * s
                px = px * px_per_m; py = py * px_per_m;
                px = rint(px); py = rint(py);                            // np.round: half to even
                const bool ok = fabs(px) <= PIXEL_LIMIT && fabs(py) <= PIXEL_LIMIT;   // (false for NaN)
                const int2 q = ok ? make_int2((int)px, (int)py) : make_int2(0, 0);
                if (!ok) bad = 1;
                ws_px[(size_t)tb * (size_t)n_room_xy + (size_t)k] = q;
                box.x = min(box.x, q.x); box.y = min(box.y, q.y); box.z = max(box.z, q.x); box.w = max(box.w, q.y);
            }
        }
        ws_box[(size_t)tb * (size_t)n_nodes + i] = box;
    }
    if (__syncthreads_or(bad) && tid == 0) atomicOr(&out[floor].bad, 1);
}

__global__ __launch_bounds__(GRAPH_THREADS) void floor_raster_kernel(const int64_t* __restrict__ room_off, long long n_room_xy,
                                                                     const int32_t* __restrict__ node_start, int n_nodes, int H, int W, int tiles_x,
                                                                     int tiles, const int4* __restrict__ ws_box, const int2* __restrict__ ws_px,
                                                                     salve_floor_iou_out_t* __restrict__ out, uint32_t* __restrict__ out_masks) {
    __shared__ int4 s_edge[EDGE_CAP];
    __shared__ int s_eid[EDGE_CAP];
    __shared__ int s_total;
    const int floor = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x;
    const int lo = node_start[floor], hi = node_start[floor + 1];
    if (!node_extent_ok(lo, hi, n_nodes) || out[floor].bad != 0) return;   // (workgroup-uniform; the pose launch raised it)
    const int tx0 = (tile % tiles_x) * TILE, ty0 = (tile / tiles_x) * TILE;
    const int x = tx0 + (tid & (TILE - 1)), y = ty0 + (tid >> 4);
    const bool in_img = x < W && y < H;
    const long long xf = (long long)x << 16;
    bool cov[2] = {false, false};
    for (int tb = 0; tb < 2; tb++) {
        __syncthreads();   // the previous table's readers are done
        if (tid == 0) s_total = 0;
        __syncthreads();
        // cull: this thread's panorama survives iff its box meets the tile; a survivor takes a contiguous range of the table's edge list
        long long v0 = 0;
        int nv = 0, base = 0;
        if (tid < hi - lo) {
            const int4 box = ws_box[(size_t)tb * (size_t)n_nodes + lo + tid];
            if (box.x <= tx0 + TILE - 1 && box.z >= tx0 && box.y <= ty0 + TILE - 1 && box.w >= ty0) {   // (false for the empty box)
                v0 = room_off[lo + tid];   // (a non-empty box: the pose launch verified the extent)
                nv = (int)min(room_off[lo + tid + 1] - v0, (long long)INT_MAX / 2);
                base = atomicAdd(&s_total, nv);
            }
        }
        __syncthreads();
        const int total = s_total;
        const int2* __restrict__ const px = ws_px + (size_t)tb * (size_t)n_room_xy;
        int le = 0, lt = 0, cur = -1;
        bool c = false;
        for (int c0 = 0; c0 < total; c0 += EDGE_CAP) {
            const int cnt = min(EDGE_CAP, total - c0);
            __syncthreads();   // the previous chunk's readers are done
            for (int j = max(0, c0 - base); j < nv && base + j < c0 + cnt; j++) {   // the owner stages its edges of this chunk
                const int2 p = px[v0 + j], q = px[v0 + (j + 1 == nv ? 0 : j + 1)];
                s_edge[base + j - c0] = make_int4(p.x, p.y, q.x, q.y);
                s_eid[base + j - c0] = tid;
            }
            __syncthreads();
            for (int e = 0; e < cnt; e++) {
                const int id = s_eid[e];
                if (id != cur) { c = c || ((le | lt) & 1); le = lt = 0; cur = id; }   // even-odd PER polygon
                int4 E = s_edge[e];
                c = c || on_line8(x, y, E.x, E.y, E.z, E.w);
                if (E.y == E.w) continue;
                if (E.y > E.w) E = make_int4(E.z, E.w, E.x, E.y);
                if (E.y <= y && y < E.w) {
                    const long long num = (long long)(E.z - E.x) << 16;
                    const long long slope = num / (E.w - E.y);                       // C division truncates toward zero
                    const long long cr = ((long long)E.x << 16) + (long long)(y - E.y) * slope;
                    le += cr <= xf;
                    lt += cr < xf;
                }
            }
        }
        cov[tb] = in_img && (c || ((le | lt) & 1));
    }
    const int lane = tid % WAVE;
    const unsigned long long be = __ballot(cov[0]), bg = __ballot(cov[1]);
    if (lane == 0) {   // ONE integer atomic per wave and counter
        if (be) atomicAdd(&out[floor].n_est, (int)__popcll(be));
        if (bg) atomicAdd(&out[floor].n_gt, (int)__popcll(bg));
        if (be & bg) atomicAdd(&out[floor].inter, (int)__popcll(be & bg));
        if (be | bg) atomicAdd(&out[floor].uni, (int)__popcll(be | bg));
    }
    if (out_masks && (lane & (TILE - 1)) == 0 && y < H) {   // the lane that starts a row of the tile writes the row's 16 bits
        const int words = (W + 31) / 32;
        for (int tb = 0; tb < 2; tb++) {
            const uint32_t bits = (uint32_t)(((tb ? bg : be) >> lane) & 0xFFFFull);
            if (bits) atomicOr(&out_masks[(((size_t)floor * 2 + tb) * (size_t)H + (size_t)y) * (size_t)words + (size_t)(tx0 >> 5)], bits << (tx0 & 31));
        }
    }
}

__global__ void floor_iou_kernel(int n_floors, salve_floor_iou_out_t* __restrict__ out, int32_t* __restrict__ status) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_floors) return;
    if (out[f].bad != 0) {
        out[f].n_est = out[f].n_gt = out[f].inter = out[f].uni = 0;
        out[f].iou = qnan();
        if (status) atomicOr(status, SALVE_STATUS_BAD_FLOOR_TABLE);
    } else {
        out[f].iou = (double)out[f].inter / ((double)out[f].uni + 1e-12);
    }
}

bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

extern "C" {

int salve_floor_align(const int32_t* node_start, int32_t n_floors, int32_t n_nodes, const salve_graph_node_out_t* truth,
                      const salve_graph_node_out_t* est, const int32_t* hyp_start, const uint32_t* hyp_mask, int32_t n_hyps, const double* gt_scale,
                      const double* metres_per_coordinate, salve_floor_hyp_out_t* out_hyps, salve_graph_node_out_t* out_nodes, double* out_rot_err,
                      double* out_trans_err, salve_floor_align_out_t* out_floors, int32_t* status, void* stream) {
    if (n_floors < 0 || n_nodes < 0 || n_hyps < 0) {
        salve_fail("salve_floor_align: negative count");
        return SALVE_ERR_BAD_ARG;
    }
    if (n_floors == 0) return SALVE_OK;
    if (!node_start || !hyp_start || !gt_scale || !metres_per_coordinate || !out_floors ||
        (n_nodes > 0 && (!truth || !est || !out_nodes || !out_rot_err || !out_trans_err)) || (n_hyps > 0 && (!hyp_mask || !out_hyps))) {
        salve_fail("salve_floor_align: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (misaligned(truth, 8) || misaligned(est, 8) || misaligned(gt_scale, 8) || misaligned(metres_per_coordinate, 8) || misaligned(out_hyps, 8) ||
        misaligned(out_nodes, 8) || misaligned(out_rot_err, 8) || misaligned(out_trans_err, 8) || misaligned(out_floors, 8) ||
        misaligned(node_start, 4) || misaligned(hyp_start, 4) || misaligned(hyp_mask, 4) || misaligned(status, 4)) {
        salve_fail("salve_floor_align: the pose tables, the float64 tables and the output records must be 8-byte aligned, the other tables 4-byte "
                   "aligned");
        return SALVE_ERR_BAD_ARG;
    }
    if (n_hyps > 0) {
        hipLaunchKernelGGL(floor_align_kernel, dim3((unsigned)((n_hyps + HYPS_PER_WG - 1) / HYPS_PER_WG)), dim3(GRAPH_THREADS), 0, (hipStream_t)stream,
                           node_start, n_floors, n_nodes, truth, est, hyp_start, hyp_mask, n_hyps, out_hyps);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(floor_pick_kernel, dim3((unsigned)n_floors), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, node_start, n_nodes, truth, est,
                       hyp_start, n_hyps, gt_scale, metres_per_coordinate, out_hyps, out_nodes, out_rot_err, out_trans_err, out_floors, status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

size_t salve_floor_iou_workspace_bytes(int64_t n_room_xy, int32_t n_nodes) {
    if (n_room_xy < 0 || n_nodes < 0) return 0;
    return 16 + 2 * ((size_t)n_nodes * sizeof(int4) + (size_t)n_room_xy * sizeof(int2));   // a flag; both tables: a box per panorama, a pixel per vertex
}

int salve_floor_iou(const double* room_xy, const int64_t* room_off, int64_t n_room_xy, const int32_t* node_start, int32_t n_floors, int32_t n_nodes,
                    const salve_graph_node_out_t* est, const salve_graph_node_out_t* truth, const double* metres_per_coordinate, int32_t img_h,
                    int32_t img_w, float offset_x, float offset_y, double pixels_per_metre, salve_floor_iou_out_t* out, uint32_t* out_masks,
                    void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const auto finite = [](double v) { return v - v == 0.0; };   // false for NaN and the infinities
    if (n_floors < 0 || n_nodes < 0 || n_room_xy < 0) {
        salve_fail("salve_floor_iou: negative count");
        return SALVE_ERR_BAD_ARG;
    }
    if (img_h < 1 || img_w < 1 || img_h > 32000 || img_w > 32000 || !finite((double)offset_x) || !finite((double)offset_y) || !finite(pixels_per_metre)) {
        salve_fail("salve_floor_iou: image size outside 1 .. 32000 or a non-finite raster parameter");
        return SALVE_ERR_BAD_ARG;
    }
    if (n_floors == 0) return SALVE_OK;
    const int tiles_x = (img_w + TILE - 1) / TILE, tiles = tiles_x * ((img_h + TILE - 1) / TILE);
    if ((long long)tiles * n_floors > (long long)INT_MAX) {
        salve_fail("salve_floor_iou: more than 2^31 - 1 tiles in one call");
        return SALVE_ERR_BAD_ARG;
    }
    if (!room_off || !node_start || !metres_per_coordinate || !out || !workspace || (n_room_xy > 0 && !room_xy) || (n_nodes > 0 && (!est || !truth))) {
        salve_fail("salve_floor_iou: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (misaligned(room_xy, 8) || misaligned(room_off, 8) || misaligned(est, 8) || misaligned(truth, 8) || misaligned(metres_per_coordinate, 8) ||
        misaligned(out, 8) || misaligned(workspace, 16) || misaligned(node_start, 4) || misaligned(out_masks, 4) || misaligned(status, 4)) {
        salve_fail("salve_floor_iou: the workspace must be 16-byte aligned, the float64, int64 and record tables 8-byte aligned, the other tables "
                   "4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    if (workspace_bytes < salve_floor_iou_workspace_bytes(n_room_xy, n_nodes)) {
        salve_fail("salve_floor_iou: the workspace is shorter than salve_floor_iou_workspace_bytes");
        return SALVE_ERR_WORKSPACE;
    }
    int32_t* const ws_flag = static_cast<int32_t*>(workspace);
    int4* const ws_box = static_cast<int4*>(workspace) + 1;
    int2* const ws_px = reinterpret_cast<int2*>(ws_box + 2 * (size_t)n_nodes);
    SALVE_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_floors * sizeof(salve_floor_iou_out_t), (hipStream_t)stream));   // the counters and `bad`
    if (out_masks)
        SALVE_HIP_CHECK(hipMemsetAsync(out_masks, 0, (size_t)n_floors * 2 * (size_t)img_h * (size_t)((img_w + 31) / 32) * sizeof(uint32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(floor_rooms_check_kernel, dim3(1), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, room_off, n_nodes, (long long)n_room_xy, ws_flag);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(floor_pose_kernel, dim3((unsigned)n_floors, 2), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, ws_flag, room_xy, room_off,
                       (long long)n_room_xy, node_start, n_nodes, est, truth, metres_per_coordinate, (double)offset_x, (double)offset_y,
                       pixels_per_metre, ws_box, ws_px, out);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(floor_raster_kernel, dim3((unsigned)(tiles * n_floors)), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, room_off,
                       (long long)n_room_xy, node_start, n_nodes, img_h, img_w, tiles_x, tiles, ws_box, ws_px, out, out_masks);
    SALVE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(floor_iou_kernel, dim3((unsigned)((n_floors + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_floors, out, status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
