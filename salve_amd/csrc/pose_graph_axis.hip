// pose_graph_axis.hip -- axis alignment by vanishing angle for gfx950 (MI355X): every scored alignment hypothesis i2Si1 is turned about the
// W/D/O it was aligned on until the two panoramas' vanishing angles agree, and re-estimated from panorama i1's room.  Any number of floors
// in ONE launch, in front of salve_pose_graph_solve / salve_pose_graph_optimise, which read the table this file writes.  Compile with
// -ffp-contract=off -fno-slp-vectorize: the arithmetic below is the reference's float64 arithmetic operation by operation, and no product may
// be fused into a sum.
//
// The reference does this per measurement on the host (scripts/run_sfm.py:421-426 and salve/algorithms/pose2_slam.py:217-231):
//   salve/utils/axis_alignment_utils.py:175-263   align_pair_measurement_by_vanishing_angle
//   salve/utils/axis_alignment_utils.py:266-284   compute_vp_correction
//   salve/utils/axis_alignment_utils.py:295-323   compute_i2Ti1 (gtsam's Similarity3.Align over point pairs, then the degree round trip)
//   salve/utils/rotation_utils.py:14-42, 87-103   rotmat2d, rotmat2theta_deg, rotate_polygon_about_pt
//   salve/common/sim2.py:135-160                  Sim2.transform_from
//   salve/common/wdo.py:35-37                     WDO.centroid
// include/salve_hip.h (salve_pose_graph_axis_align) states the rules; this file states how they run.
//
//   axis_align_kernel   one workgroup of 256 threads per floor, ONE THREAD PER ROW (stride 256 over the floor's rows)
//
// Why a thread per row and not a wavefront per row: a room has 4 to 30 vertices, so a wavefront per row would idle 34 to 60 of its 64 lanes
// in each of the three passes over the polygon and would need a cross-lane float64 reduction whose order the rules would then have to name.
// A thread walks its room in ascending vertex order from 0.0, which IS the rule.  The rows of a floor are sorted by (i1, i2), so the lanes of
// a wavefront mostly share panorama i1: their room and W/D/O reads hit the same cache lines at the same loop step (a broadcast, not a
// gather).  What diverges is the trip count between neighbouring pairs (different rooms) and the early outs; both are short.
//
// The polygon is walked three times (centroids; H; the scale's two sums) and the moved, turned vertex is recomputed each time from the same
// operands in the same order -- equal bits -- instead of being kept: 65 vertices x 2 doubles per lane do not fit registers, and scratch would
// cost more than 14 float64 operations per vertex.
//
// One workgroup per floor, as salve_pose_graph_solve: the floor's extents are verified once, workgroup-uniformly, and the floor's status
// counts are an integer tree sum in LDS -- no atomic but the status word's OR, the same bytes on every run.
//
// Bound: latency.  A row reads 48 + 8 bytes and writes 48 + 40; the room (16 bytes a vertex) comes from L2 after the pair's first lane.  Per
// row: one atan2f, four float64 sin / cos, two float64 atan2, ~45 float64 operations per vertex.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "salve_common.h"

namespace {

constexpr int AXIS_THREADS = 256;
constexpr float RAD2DEG_F32 = 57.29577951308232f;    // (float)(180 / pi): np.rad2deg on a float32
constexpr double RAD2DEG_F64 = 57.29577951308232;    // 180 / pi
constexpr double DEG2RAD_F64 = 0.017453292519943295; // pi / 180
constexpr double MAX_ALLOWED_CORRECTION_DEG = 15.0;  // axis_alignment_utils.py:27

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7FF8000000000000LL); }

struct Move {   // Sim2.transform_from: ((p @ R.T) + t) * s, per entry
    double R00, R01, R10, R11, tx, ty, s;
    __device__ __forceinline__ void operator()(double x, double y, double* ox, double* oy) const {
        *ox = ((x * R00 + y * R01) + tx) * s;
        *oy = ((x * R10 + y * R11) + ty) * s;
    }
};

struct Turn {   // rotate_polygon_about_pt of a moved vertex: (q - c) . rotmat^T + c, rotmat = [[cs, -sn], [sn, cs]]
    Move mv;
    double cx, cy, cs, sn;
    __device__ __forceinline__ void operator()(double x, double y, double* ox, double* oy) const {
        double qx, qy;
        mv(x, y, &qx, &qy);
        const double dx = qx - cx, dy = qy - cy;
        *ox = (dx * cs + dy * (-sn)) + cx;
        *oy = (dx * sn + dy * cs) + cy;
    }
};

__global__ __launch_bounds__(AXIS_THREADS) void axis_align_kernel(
    const salve_graph_row_t* __restrict__ rows, int n_rows, const int32_t* __restrict__ floor_start, const int32_t* __restrict__ n_nodes,
    const salve_axis_wdo_t* __restrict__ row_wdo, const int32_t* __restrict__ pano_base, const int64_t* __restrict__ room_off,
    const double* __restrict__ room_xy, long long n_room_xy, const int64_t* __restrict__ wdo_off, const double* __restrict__ wdo_xy,
    const uint8_t* __restrict__ wdo_type, long long n_wdo, const double* __restrict__ vanishing_deg, int n_panos,
    salve_graph_row_t* __restrict__ out_rows, salve_axis_row_out_t* __restrict__ out_axis, salve_axis_floor_out_t* __restrict__ out_floors,
    int32_t* __restrict__ status) {
    __shared__ int s_count[SALVE_AXIS_N_STATUS][AXIS_THREADS];
    const int floor = blockIdx.x, tid = threadIdx.x;
    // the tables are device memory: verified before any address is formed from them (workgroup-uniform)
    int lo = floor_start[floor], hi = floor_start[floor + 1];
    const int n = n_nodes[floor], base = pano_base[floor];
    const bool bad_extent = lo < 0 || hi < lo || hi > n_rows;
    if (bad_extent) lo = hi = 0;   // no row of such a floor can be named: none is read or written
    const bool bad_panos = n < 0 || base < 0 || (long long)base + (long long)n > (long long)n_panos;   // every row of the floor is malformed

    int count[SALVE_AXIS_N_STATUS];
    for (int k = 0; k < SALVE_AXIS_N_STATUS; k++) count[k] = 0;

    for (int r = lo + tid; r < hi; r += AXIS_THREADS) {
        const salve_graph_row_t row = rows[r];
        const salve_axis_wdo_t w = row_wdo[r];
        salve_axis_row_out_t a;
        a.status = SALVE_AXIS_MALFORMED; a.reserved = 0;
        a.correction_deg = nan64(); a.theta_deg = nan64(); a.t[0] = nan64(); a.t[1] = nan64();
        salve_graph_row_t o = row;   // copied bit for bit unless the correction applies

        do {
            if (bad_panos || row.i1 < 0 || row.i1 >= n || row.i2 < 0 || row.i2 >= n) break;
            if (w.type < 0 || w.type > 2 || w.index < 0) break;
            const int p1 = base + row.i1, p2 = base + row.i2;
            const long long wlo = wdo_off[p1], whi = wdo_off[p1 + 1], rlo = room_off[p1], rhi = room_off[p1 + 1];
            if (wlo < 0 || whi < wlo || whi > n_wdo || rlo < 0 || rhi < rlo || rhi > n_room_xy) break;
            // the index counts WITHIN the type (getattr(pano, alignment_object + "s")[i1_wdo_idx])
            long long k = wlo;
            for (int seen = 0; k < whi; k++) {
                if (wdo_type[k] == (uint8_t)w.type && seen++ == w.index) break;
            }
            if (k >= whi) break;   // the panorama holds no such W/D/O

            const double vp1 = vanishing_deg[p1], vp2 = vanishing_deg[p2];
            if (!isfinite(vp1) || !isfinite(vp2)) { a.status = SALVE_AXIS_NO_ANGLE; break; }
            const long long nv = rhi - rlo - 1;   // the OPEN polygon: the stored room repeats its first vertex
            if (nv < 3) { a.status = SALVE_AXIS_NO_ROOM; break; }

            // compute_vp_correction: the row's own angle in float32 (numpy on Sim2's float32 entries), everything else float64
            const float theta32 = atan2f(row.R[2], row.R[0]) * RAD2DEG_F32;
            double corr = -((vp2 - vp1) + (double)theta32);
            corr = fmod(corr, 90.0);                 // Python's %: the sign of the divisor
            if (corr != 0.0) { if (corr < 0.0) corr += 90.0; } else corr = 0.0;
            if (corr > 45.0) corr = corr - 90.0;
            a.correction_deg = corr;
            if (fabs(corr) > MAX_ALLOWED_CORRECTION_DEG) { a.status = SALVE_AXIS_TOO_LARGE; break; }

            Turn turn;
            turn.mv.R00 = (double)row.R[0]; turn.mv.R01 = (double)row.R[1]; turn.mv.R10 = (double)row.R[2]; turn.mv.R11 = (double)row.R[3];
            turn.mv.tx = (double)row.t[0]; turn.mv.ty = (double)row.t[1]; turn.mv.s = row.s;
            const double rad = corr * DEG2RAD_F64;
            turn.cs = cos(rad); turn.sn = sin(rad);
            const double* wp = wdo_xy + 4 * k;   // WDO.centroid: the mean of the two endpoints
            turn.mv((wp[0] + wp[2]) / 2.0, (wp[1] + wp[3]) / 2.0, &turn.cx, &turn.cy);

            const double* v = room_xy + 2 * rlo;
            const double dn = (double)nv;
            // Similarity3.Align over the pairs (a, b) = (turned vertex in i2's frame, vertex in i1's frame)
            double sax = 0.0, say = 0.0, sbx = 0.0, sby = 0.0;
            for (long long i = 0; i < nv; i++) {
                double ax, ay;
                turn(v[2 * i], v[2 * i + 1], &ax, &ay);
                sax += ax; say += ay; sbx += v[2 * i]; sby += v[2 * i + 1];
            }
            const double cax = sax / dn, cay = say / dn, cbx = sbx / dn, cby = sby / dn;
            double H00 = 0.0, H01 = 0.0, H10 = 0.0, H11 = 0.0;
            for (long long i = 0; i < nv; i++) {
                double ax, ay;
                turn(v[2 * i], v[2 * i + 1], &ax, &ay);
                const double dax = ax - cax, day = ay - cay, dbx = v[2 * i] - cbx, dby = v[2 * i + 1] - cby;
                H00 += dax * dbx; H01 += dax * dby; H10 += day * dbx; H11 += day * dby;
            }
            const double phi = atan2(H10 - H01, H00 + H11);   // the planar closest rotation
            const double c1 = cos(phi), s1 = sin(phi);
            double x = 0.0, y = 0.0;
            for (long long i = 0; i < nv; i++) {
                double ax, ay;
                turn(v[2 * i], v[2 * i + 1], &ax, &ay);
                const double dax = ax - cax, day = ay - cay, dbx = v[2 * i] - cbx, dby = v[2 * i + 1] - cby;
                const double px = c1 * dbx + (-s1) * dby, py = s1 * dbx + c1 * dby;
                x += dax * px + day * py;
                y += px * px + py * py;
            }
            const double sc = x / y;
            const double Tx = (cax - sc * (c1 * cbx + (-s1) * cby)) / sc, Ty = (cay - sc * (s1 * cbx + c1 * cby)) / sc;
            // the degree round trip of compute_i2Ti1: rotmat2theta_deg, then Rot2.fromDegrees
            const double theta_deg = atan2(s1, c1) * RAD2DEG_F64;
            const double th = theta_deg * DEG2RAD_F64;
            const double c2 = cos(th), s2 = sin(th);
            a.status = SALVE_AXIS_APPLIED;
            a.theta_deg = theta_deg; a.t[0] = Tx; a.t[1] = Ty;
            o.R[0] = (float)c2; o.R[1] = (float)(-s2); o.R[2] = (float)s2; o.R[3] = (float)c2;
            o.t[0] = (float)Tx; o.t[1] = (float)Ty;
            o.s = 1.0;
        } while (false);

        out_rows[r] = o;
        out_axis[r] = a;
        count[a.status]++;
    }

    // the floor's counts: an integer tree sum in LDS, no atomic
    for (int k = 0; k < SALVE_AXIS_N_STATUS; k++) s_count[k][tid] = count[k];
    __syncthreads();
    for (int step = AXIS_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
            for (int k = 0; k < SALVE_AXIS_N_STATUS; k++) s_count[k][tid] += s_count[k][tid + step];
        }
        __syncthreads();
    }
    if (tid == 0) {
        salve_axis_floor_out_t fo;
        fo.n_applied = s_count[SALVE_AXIS_APPLIED][0]; fo.n_too_large = s_count[SALVE_AXIS_TOO_LARGE][0];
        fo.n_no_angle = s_count[SALVE_AXIS_NO_ANGLE][0]; fo.n_no_room = s_count[SALVE_AXIS_NO_ROOM][0];
        fo.n_malformed = s_count[SALVE_AXIS_MALFORMED][0];
        fo.bad_extent = bad_extent ? 1 : 0;
        out_floors[floor] = fo;
        if (status && (bad_extent || fo.n_malformed > 0)) atomicOr(status, SALVE_STATUS_BAD_AXIS_ROW);
    }
}

}  // namespace

extern "C" {

int salve_pose_graph_axis_align(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                                const salve_axis_wdo_t* row_wdo, const int32_t* pano_base, const int64_t* room_off, const double* room_xy,
                                int64_t n_room_xy, const int64_t* wdo_off, const double* wdo_xy, const uint8_t* wdo_type, int64_t n_wdo,
                                const double* vanishing_deg, int32_t n_panos, salve_graph_row_t* out_rows, salve_axis_row_out_t* out_axis,
                                salve_axis_floor_out_t* out_floors, int32_t* status, void* stream) {
    if (n_rows < 0 || n_floors < 0 || n_room_xy < 0 || n_wdo < 0 || n_panos < 0) {
        salve_fail("salve_pose_graph_axis_align: negative count");
        return SALVE_ERR_BAD_ARG;
    }
    if (n_floors == 0) return SALVE_OK;
    if (!floor_start || !n_nodes || !pano_base || !out_floors || (n_rows > 0 && (!rows || !row_wdo || !out_rows || !out_axis)) ||
        (n_panos > 0 && (!room_off || !wdo_off || !vanishing_deg)) || (n_room_xy > 0 && !room_xy) || (n_wdo > 0 && (!wdo_xy || !wdo_type))) {
        salve_fail("salve_pose_graph_axis_align: null pointer");
        return SALVE_ERR_BAD_ARG;
    }
    const auto mis = [](const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; };
    if (mis(rows, 8) || mis(out_rows, 8) || mis(out_axis, 8) || mis(room_off, 8) || mis(room_xy, 8) || mis(wdo_off, 8) || mis(wdo_xy, 8) ||
        mis(vanishing_deg, 8) || mis(row_wdo, 4) || mis(floor_start, 4) || mis(n_nodes, 4) || mis(pano_base, 4) || mis(out_floors, 4) || mis(status, 4)) {
        salve_fail("salve_pose_graph_axis_align: rows, out_rows, out_axis and the float64 / int64 tables must be 8-byte aligned, the int32 tables "
                   "4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(axis_align_kernel, dim3((unsigned)n_floors), dim3(AXIS_THREADS), 0, (hipStream_t)stream, rows, n_rows, floor_start, n_nodes,
                       row_wdo, pano_base, room_off, room_xy, (long long)n_room_xy, wdo_off, wdo_xy, wdo_type, (long long)n_wdo, vanishing_deg,
                       n_panos, out_rows, out_axis, out_floors, status);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
