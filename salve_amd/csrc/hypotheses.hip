// hypotheses.hip -- the alignment hypotheses of every panorama pair for gfx950 (MI355X): all W/D/O alignments of a pair fitted, accepted by
// width ratio, pruned to unique Sim(2)s, labelled against the ground truth, counted, and the pair's visual adjacency -- any number of floors in
// ONE launch.  Compile with -ffp-contract=off -fno-slp-vectorize: the fit is float64 operation by operation (the numpy emulator of
// tests/hypotheses_cases.py gives the same bits), the truth of a pair is the reference's float32 Sim(2) arithmetic (pose_graph_common.h).
//
// The reference does this per pair on the host with one Python object and one JSON file per hypothesis (scripts/export_alignment_hypotheses.py
// :93-273, salve/utils/wdo_alignment.py:107-284); include/salve_hip.h (salve_hypotheses_generate) states the rules; this file states how they run.
//
//   hypotheses_kernel   one workgroup of ONE wavefront per panorama pair
//
// Why a wavefront per pair: a pair has 2 d1 d2 + w1 w2 + 2 o1 o2 candidates -- a handful to a few dozen on MHNet's predictions, 5120 at the
// limit of 32 objects per type -- each a closed-form fit of ~60 float64 operations, one square root and two divisions.  The fits are
// independent; the pruning is NOT: candidate c is kept unless it equals one KEPT before it, which is a chain through the candidate order.
// So the wave takes the candidates 64 at a time, one per lane:
//   1. every lane fits its candidate and tests the width ratio (independent);
//   2. every lane compares its candidate with the rows kept by EARLIER chunks (LDS, 24 bytes each, broadcast reads);
//   3. the chain inside the chunk is resolved with ballots: the lowest lane still alive is kept, its R and t are broadcast by shuffles, the
//      higher lanes that equal it die; repeated once per KEPT row of the chunk, not per candidate;
//   4. a kept lane labels its row and writes it at row_offset + (its rank among the kept) -- the rank is the order of the candidates, so the
//      output needs no atomic append and is the same bytes on every run; the host drops the gap behind n_kept.
// The kept list lives in LDS because step 2 re-reads every kept row once per chunk; 24 bytes x max_capacity (the host passes the launch's
// largest pair) are 1.5 KiB for 64 candidates -- tens of pairs share a CU -- and 120 KiB at the 5120 limit, one pair per CU.
//
// LDS (dynamic, 16-byte aligned base):
//   idx    uint8 [2][3][32]   the position within its panorama of the r-th object of type T, for pano1 and pano2            192 bytes
//   kept   float [max_capacity][6]   R00 R01 R10 R11 tx ty of the rows kept so far
//
// Bound: latency.  A pair reads a few hundred bytes (L2-resident tables) and writes 48 bytes per kept row; its time is the dependent chain
// table offsets -> types -> vertices -> square root and divisions -> (per kept row) one ballot and six shuffles.  Pairs are independent, a
// split has millions: the chains overlap across the 32 wave slots of every CU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/salve_hip.h"
#include "pose_graph_common.h"
#include "salve_common.h"

namespace {

constexpr int HYP_THREADS = 64;                                // one wavefront
constexpr int HYP_PER_TYPE = SALVE_HYP_MAX_WDO_PER_TYPE;       // 32
constexpr int HYP_IDX_BYTES = 2 * 3 * HYP_PER_TYPE;            // 192: a multiple of 16, so `kept` stays 16-byte aligned
constexpr double RAD2DEG_F64 = 57.29577951308232;             // 180 / pi
static_assert(HYP_IDX_BYTES % 16 == 0, "the kept list follows the index table");

__host__ __device__ inline size_t hyp_lds_bytes(int max_capacity) {
    return (size_t)HYP_IDX_BYTES + (((size_t)(max_capacity > 0 ? max_capacity : 1) * 24 + 15) & ~(size_t)15);
}

struct Fit {
    float R00, R01, R10, R11, tx, ty;
};

// |x - k| <= 1e-8 + 1e-5 |k|: np.allclose with the kept row on the right-hand side; false for a NaN
__device__ __forceinline__ bool close1(float x, float k) {
    const double d = fabs((double)x - (double)k);
    return d <= 1e-8 + 1e-5 * fabs((double)k);
}

__device__ __forceinline__ bool fit_equal(const Fit& x, const Fit& k) {
    return close1(x.R00, k.R00) && close1(x.R01, k.R01) && close1(x.R10, k.R10) && close1(x.R11, k.R11) && close1(x.tx, k.tx) && close1(x.ty, k.ty);
}

// gtsam's Pose2::Align over the five-point polygons [p1, p1, p2, p2, p1] of both objects: a* is pano2's, b* pano1's.  p1 counts three times
// and p2 twice: the rotation equals the two-point fit's, the translation does not when the widths differ.
__device__ __forceinline__ Fit fit_se2(double a1x, double a1y, double a2x, double a2y, double b1x, double b1y, double b2x, double b2y) {
    const double cax = ((((a1x + a1x) + a2x) + a2x) + a1x) / 5.0, cay = ((((a1y + a1y) + a2y) + a2y) + a1y) / 5.0;
    const double cbx = ((((b1x + b1x) + b2x) + b2x) + b1x) / 5.0, cby = ((((b1y + b1y) + b2y) + b2y) + b1y) / 5.0;
    const double da1x = a1x - cax, da1y = a1y - cay, da2x = a2x - cax, da2y = a2y - cay;
    const double db1x = b1x - cbx, db1y = b1y - cby, db2x = b2x - cbx, db2y = b2y - cby;
    const double c1 = db1x * da1x + db1y * da1y, c2 = db2x * da2x + db2y * da2y;
    const double s1 = (-db1y) * da1x + db1x * da1y, s2 = (-db2y) * da2x + db2x * da2y;
    const double c = ((((0.0 + c1) + c1) + c2) + c2) + c1;
    const double s = ((((0.0 + s1) + s1) + s2) + s2) + s1;
    const double h = sqrt(c * c + s * s);
    double r_c = 1.0, r_s = 0.0;
    if (h != 0.0) { r_c = c / h; r_s = s / h; }
    Fit f;
    f.R00 = (float)r_c; f.R01 = (float)(-r_s); f.R10 = (float)r_s; f.R11 = (float)r_c;
    f.tx = (float)(cax - (r_c * cbx + (-r_s) * cby));
    f.ty = (float)(cay - (r_s * cbx + r_c * cby));
    return f;
}

__device__ __forceinline__ double seg_width(double x1, double y1, double x2, double y2) {
    const double dx = x1 - x2, dy = y1 - y2;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ double point_distance(double px, double py, double qx, double qy) {
    const double dx = px - qx, dy = py - qy;
    return sqrt(dx * dx + dy * dy);
}

// GEOS' Distance::pointToSegment
__device__ __forceinline__ double point_segment_distance(double px, double py, double ax, double ay, double bx, double by) {
    if (ax == bx && ay == by) return point_distance(px, py, ax, ay);
    const double len2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay);
    const double r = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / len2;
    if (r <= 0.0) return point_distance(px, py, ax, ay);
    if (r >= 1.0) return point_distance(px, py, bx, by);
    const double s = ((ay - py) * (bx - ax) - (ax - px) * (by - ay)) / len2;
    return fabs(s) * sqrt(len2);
}

// the discrete Hausdorff distance of two segments (for segments the exact one): the larger of the two directed maxima over endpoints
__device__ __forceinline__ double segment_hausdorff(const double* __restrict__ a, const double* __restrict__ b) {
    const double d0 = point_segment_distance(a[0], a[1], b[0], b[1], b[2], b[3]), d1 = point_segment_distance(a[2], a[3], b[0], b[1], b[2], b[3]);
    const double d2 = point_segment_distance(b[0], b[1], a[0], a[1], a[2], a[3]), d3 = point_segment_distance(b[2], b[3], a[0], a[1], a[2], a[3]);
    return fmax(fmax(d0, d1), fmax(d2, d3));
}

// obj_almost_equal(hypothesis, G, object): see include/salve_hip.h
__device__ __forceinline__ int label_of(const Fit& f, const Sim2& G, int type) {
    const double gtx = (double)G.tx, gty = (double)G.ty;
    if (!(fabs((double)f.tx - gtx) <= 0.35 + 1e-5 * fabs(gtx))) return 0;
    if (!(fabs((double)f.ty - gty) <= 0.35 + 1e-5 * fabs(gty))) return 0;
    if (!(fabs(1.0 - G.s) <= 0.35 + 1e-5 * fabs(G.s))) return 0;
    const double th = atan2((double)f.R10, (double)f.R00) * RAD2DEG_F64, th_g = atan2((double)G.R10, (double)G.R00) * RAD2DEG_F64;
    double m = fmod((th_g - th) + 180.0, 360.0);   // Python's %: the sign of the modulus
    if (m < 0.0) m += 360.0;
    double d = m - 180.0;
    if (d < -180.0) d += 360.0;
    return fabs(d) <= (type == 2 ? 9.0 : 7.0) ? 1 : 0;
}

__device__ __forceinline__ Sim2 pose_load(const salve_graph_node_out_t* __restrict__ p) {
    Sim2 S;
    S.R00 = p->R[0]; S.R01 = p->R[1]; S.R10 = p->R[2]; S.R11 = p->R[3];
    S.tx = p->t[0]; S.ty = p->t[1];
    S.s = p->s;
    return S;
}

__global__ __launch_bounds__(HYP_THREADS) void hypotheses_kernel(const double* __restrict__ wdo_xy, const uint8_t* __restrict__ wdo_type,
                                                                 const int64_t* __restrict__ wdo_off, int64_t n_wdo, const double* __restrict__ gt_xy,
                                                                 const int64_t* __restrict__ gt_off, int64_t n_gt,
                                                                 const salve_graph_node_out_t* __restrict__ poses, int n_panos,
                                                                 const salve_hyp_pair_t* __restrict__ pairs, int max_capacity, double min_ratio,
                                                                 salve_hyp_row_t* __restrict__ out_rows, int64_t n_rows,
                                                                 salve_hyp_pair_out_t* __restrict__ out_pairs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint8_t* const idx = smem;                                            // [2][3][32]
    float* const kept = reinterpret_cast<float*>(smem + HYP_IDX_BYTES);   // [max_capacity][6]
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;

    // ---- the pair's record and tables, verified before any address is formed from them (everything here is wave-uniform)
    const salve_hyp_pair_t pr = pairs[p];
    bool bad = pr.pano1 < 0 || pr.pano1 >= n_panos || pr.pano2 < 0 || pr.pano2 >= n_panos || pr.capacity < 0 || pr.capacity > max_capacity ||
               pr.row_offset < 0 || pr.row_offset > n_rows || (int64_t)pr.capacity > n_rows - pr.row_offset;
    int64_t lo[2] = {0, 0}, glo[2] = {0, 0};
    int n_obj[2] = {0, 0}, n_gobj[2] = {0, 0};
    if (!bad) {
        for (int s = 0; s < 2; s++) {
            const int pano = s ? pr.pano2 : pr.pano1;
            const int64_t a = wdo_off[pano], b = wdo_off[pano + 1], ga = gt_off[pano], gb = gt_off[pano + 1];
            if (a < 0 || b < a || b > n_wdo || b - a > 3 * HYP_PER_TYPE || ga < 0 || gb < ga || gb > n_gt || gb - ga > (int64_t)1 << 20) { bad = true; break; }
            lo[s] = a; n_obj[s] = (int)(b - a);
            glo[s] = ga; n_gobj[s] = (int)(gb - ga);
        }
    }
    // the r-th object of each type: ranks by ballot, 64 objects at a time
    int cnt[2][3] = {{0, 0, 0}, {0, 0, 0}};
    if (!bad) {
        for (int s = 0; s < 2; s++) {
            for (int base = 0; base < n_obj[s]; base += HYP_THREADS) {
                const int k = base + lane;
                const int ty = k < n_obj[s] ? (int)wdo_type[lo[s] + k] : -1;
                if (__ballot(ty > 2)) bad = true;
                for (int T = 0; T < 3; T++) {
                    const unsigned long long m = __ballot(ty == T);
                    const int r = cnt[s][T] + __popcll(m & below);
                    if (ty == T && r < HYP_PER_TYPE) idx[(s * 3 + T) * HYP_PER_TYPE + r] = (uint8_t)k;
                    cnt[s][T] += __popcll(m);
                }
            }
            for (int T = 0; T < 3; T++)
                if (cnt[s][T] > HYP_PER_TYPE) bad = true;
        }
    }
    // doors (1), windows (0), openings (2): align_rooms_by_wd's order
    const int d1 = cnt[0][1], d2 = cnt[1][1], w1 = cnt[0][0], w2 = cnt[1][0], o1 = cnt[0][2], o2 = cnt[1][2];
    const int n_door = 2 * d1 * d2, n_window = w1 * w2, n_opening = 2 * o1 * o2;
    if (!bad && n_door + n_window + n_opening != pr.capacity) bad = true;
    if (bad) {
        if (lane == 0) {
            salve_hyp_pair_out_t o;
            o.n_kept = -1; o.n_valid = 0; o.n_rejected = 0; o.visibly_adjacent = 0;
            o.R[0] = o.R[1] = o.R[2] = o.R[3] = 0.0f; o.t[0] = o.t[1] = 0.0f; o.s = 0.0;
            out_pairs[p] = o;
        }
        return;
    }
    __syncthreads();   // idx is written

    // ---- the truth of the pair: i2Ti1_gt = wTi2.inverse().compose(wTi1)
    const Sim2 G = sim2_compose(sim2_inverse(pose_load(poses + pr.pano2)), pose_load(poses + pr.pano1));

    // ---- are_visibly_adjacent: any ground-truth segment of pano1 against any of pano2
    bool adjacent = false;
    const int64_t n_combos = (int64_t)n_gobj[0] * n_gobj[1];
    for (int64_t q = lane; q < n_combos; q += HYP_THREADS) {
        const double* a = gt_xy + 4 * (glo[0] + q / n_gobj[1]);
        const double* b = gt_xy + 4 * (glo[1] + q % n_gobj[1]);
        if (segment_hausdorff(a, b) < 0.1) adjacent = true;
    }
    const bool any_adjacent = __ballot(adjacent) != 0;

    // ---- the candidates, 64 at a time
    int n_kept = 0, n_valid = 0, n_rejected = 0;
    for (int base = 0; base < pr.capacity; base += HYP_THREADS) {
        const int c = base + lane;
        const bool active = c < pr.capacity;
        int type = 1, i = 0, j = 0, conf = 0;
        Fit f = {1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
        bool valid = false;
        if (active) {
            int q = c;
            if (q < n_door) { type = 1; conf = q & 1; q >>= 1; i = q / d2; j = q % d2; }
            else if ((q -= n_door) < n_window) { type = 0; i = q / w2; j = q % w2; }
            else { q -= n_window; type = 2; conf = q & 1; q >>= 1; i = q / o2; j = q % o2; }
            const double* b = wdo_xy + 4 * (lo[0] + idx[(0 * 3 + type) * HYP_PER_TYPE + i]);   // pano1's object
            const double* a = wdo_xy + 4 * (lo[1] + idx[(1 * 3 + type) * HYP_PER_TYPE + j]);   // pano2's
            const double b1x = b[0], b1y = b[1], b2x = b[2], b2y = b[3];
            double a1x = a[0], a1y = a[1], a2x = a[2], a2y = a[3];
            if (conf) { a1x = a[2]; a1y = a[3]; a2x = a[0]; a2y = a[1]; }   // WDO.get_rotated_version: pt1 and pt2 swapped
            f = fit_se2(a1x, a1y, a2x, a2y, b1x, b1y, b2x, b2y);
            const double wa = seg_width(a1x, a1y, a2x, a2y), wb = seg_width(b1x, b1y, b2x, b2y);
            const double ratio = (wb < wa ? wb : wa) / (wb > wa ? wb : wa);   // Python's min(w1, w2) / max(w1, w2)
            valid = ratio >= min_ratio;                                       // false for the NaN of two zero widths
        }
        n_valid += __popcll(__ballot(active && valid));
        n_rejected += __popcll(__ballot(active && !valid));
        bool alive = active && valid;
        // against the rows kept by earlier chunks
        for (int k = 0; k < n_kept; k++) {
            const float* kf = kept + 6 * k;
            const Fit kk = {kf[0], kf[1], kf[2], kf[3], kf[4], kf[5]};
            if (alive && fit_equal(f, kk)) alive = false;
        }
        // the chain inside the chunk: the lowest lane alive is kept; the higher lanes that equal it die
        int my_rank = -1;
        unsigned long long todo = __ballot(alive);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            Fit kk;
            kk.R00 = __shfl(f.R00, l, HYP_THREADS); kk.R01 = __shfl(f.R01, l, HYP_THREADS); kk.R10 = __shfl(f.R10, l, HYP_THREADS);
            kk.R11 = __shfl(f.R11, l, HYP_THREADS); kk.tx = __shfl(f.tx, l, HYP_THREADS); kk.ty = __shfl(f.ty, l, HYP_THREADS);
            if (lane == l) {
                my_rank = n_kept;
                float* kf = kept + 6 * n_kept;
                kf[0] = f.R00; kf[1] = f.R01; kf[2] = f.R10; kf[3] = f.R11; kf[4] = f.tx; kf[5] = f.ty;
            } else if (alive && lane > l && fit_equal(f, kk)) {
                alive = false;
            }
            n_kept++;
            const unsigned long long above = l == 63 ? 0ull : ~((2ull << l) - 1ull);
            todo = __ballot(alive) & above;
        }
        __syncthreads();   // the chunk's kept rows are in LDS before the next chunk reads them
        if (my_rank >= 0) {
            salve_hyp_row_t row;
            row.R[0] = f.R00; row.R[1] = f.R01; row.R[2] = f.R10; row.R[3] = f.R11;
            row.t[0] = f.tx; row.t[1] = f.ty;
            row.type = type; row.i = i; row.j = j; row.configuration = conf;
            row.label = label_of(f, G, type);
            row.reserved = 0;
            out_rows[pr.row_offset + my_rank] = row;
        }
    }
    if (lane == 0) {
        salve_hyp_pair_out_t o;
        o.n_kept = n_kept; o.n_valid = n_valid; o.n_rejected = n_rejected; o.visibly_adjacent = any_adjacent ? 1 : 0;
        o.R[0] = G.R00; o.R[1] = G.R01; o.R[2] = G.R10; o.R[3] = G.R11;
        o.t[0] = G.tx; o.t[1] = G.ty;
        o.s = G.s;
        out_pairs[p] = o;
    }
}

std::mutex g_hyp_lds_mu;
size_t g_hyp_lds_attr[64];

}  // namespace

extern "C" {

int salve_hypotheses_generate(const double* wdo_xy, const uint8_t* wdo_type, const int64_t* wdo_off, int64_t n_wdo, const double* gt_xy,
                              const int64_t* gt_off, int64_t n_gt, const salve_graph_node_out_t* poses, int32_t n_panos,
                              const salve_hyp_pair_t* pairs, int64_t n_pairs, int32_t max_capacity, double min_width_ratio,
                              salve_hyp_row_t* out_rows, int64_t n_rows, salve_hyp_pair_out_t* out_pairs, void* stream) {
    if (n_wdo < 0 || n_gt < 0 || n_panos < 0 || n_pairs < 0 || n_rows < 0) { salve_fail("salve_hypotheses_generate: negative count"); return SALVE_ERR_BAD_ARG; }
    if (max_capacity < 0 || max_capacity > SALVE_HYP_MAX_CAPACITY) {
        salve_fail("salve_hypotheses_generate: max_capacity must lie in 0 .. 5120 (32 W/D/Os per type and panorama)");
        return SALVE_ERR_BAD_ARG;
    }
    if (min_width_ratio != min_width_ratio) { salve_fail("salve_hypotheses_generate: min_width_ratio is NaN"); return SALVE_ERR_BAD_ARG; }
    if (n_pairs > 0x7FFFFFFFll) { salve_fail("salve_hypotheses_generate: more than 2^31 - 1 pairs in one call"); return SALVE_ERR_BAD_ARG; }
    if (n_pairs == 0) return SALVE_OK;
    if (!wdo_off || !gt_off || !poses || !pairs || !out_pairs || (n_wdo > 0 && (!wdo_xy || !wdo_type)) || (n_gt > 0 && !gt_xy) || (n_rows > 0 && !out_rows)) {
        salve_fail("salve_hypotheses_generate: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(wdo_xy) % 8 != 0 || reinterpret_cast<uintptr_t>(wdo_off) % 8 != 0 || reinterpret_cast<uintptr_t>(gt_xy) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(gt_off) % 8 != 0 || reinterpret_cast<uintptr_t>(poses) % 8 != 0 || reinterpret_cast<uintptr_t>(pairs) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(out_rows) % 4 != 0 || reinterpret_cast<uintptr_t>(out_pairs) % 8 != 0) {
        salve_fail("salve_hypotheses_generate: the float64 / int64 tables, poses, pairs and out_pairs must be 8-byte aligned, out_rows 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    const size_t lds = hyp_lds_bytes(max_capacity);
    if (lds > 64 * 1024) {   // opt in to more than 64 KB of dynamic LDS, per device
        std::lock_guard<std::mutex> lock(g_hyp_lds_mu);
        int dev = 0;
        SALVE_HIP_CHECK(hipGetDevice(&dev));
        const int slot = (dev >= 0 && dev < 64) ? dev : 0;
        if (dev != slot || lds > g_hyp_lds_attr[slot]) {
            SALVE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(hypotheses_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            g_hyp_lds_attr[slot] = lds;
        }
    }
    hipLaunchKernelGGL(hypotheses_kernel, dim3((unsigned)n_pairs), dim3(HYP_THREADS), lds, (hipStream_t)stream, wdo_xy, wdo_type, wdo_off, n_wdo, gt_xy,
                       gt_off, n_gt, poses, (int)n_panos, pairs, (int)max_capacity, min_width_ratio, out_rows, n_rows, out_pairs);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
