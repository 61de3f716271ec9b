// jpeg_forward.h -- the forward half of libjpeg's baseline 4:2:0 chain as device functions, shared by jpeg_roundtrip.hip (which decodes
// the quantised coefficients again) and jpeg_encode.hip (which entropy-codes them): colour conversion, edge replication, h2v2
// downsampling, the slow-integer forward DCT and quantisation, in libjpeg's order and with its constants (jccolor.c, jcprepct.c,
// jcsample.c, jfdctint.c, jcdctmgr.c).  32-bit integer arithmetic only; every offset is 64-bit.
//
// The tile both files work on (jpeg_forward_rows, jpeg_forward_column): a workgroup of 256 threads owns four MCUs (16 x 16 pixels each)
// side by side.  Every thread converts one 2 x 2 pixel quad into LDS (four luma samples, one Cb, one Cr: jpeg_stage_quad); then each of
// the 24 blocks (16 luma, 4 Cb, 4 Cr) gets eight threads, one per row / column (JpegBlockMap), for the 1-D passes through LDS (JpegTile).
// The two end with the unquantised coefficients of a block's column in registers; what happens to them is the calling kernel's.
//
// At the end, the host side the three entries share: the geometry in whole MCUs and the refusals, each naming the entry that refused.
#ifndef SALVE_JPEG_FORWARD_H
#define SALVE_JPEG_FORWARD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "salve_common.h"

namespace {

constexpr int JPEG_THREADS = 256;
constexpr int MCUS = 4;            // MCUs of a workgroup, side by side
constexpr int TW = 16 * MCUS;      // its luma tile: 16 rows of TW samples
constexpr int SY = TW + 1;         // LDS row strides (odd: the column passes of a block's eight threads fall on different banks)
constexpr int SC = TW / 2 + 1;
constexpr int MAX_DIM = 4096, MAX_IMAGES = 65535;

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270;
constexpr int F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137;
constexpr int F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

struct QTables {
    uint16_t q[2][64];   // luma, chroma; natural order
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jccolor.c: rgb_ycc_convert (every sum is positive: the shifts are plain)
__device__ __forceinline__ void rgb_to_ycc(uint32_t p, int& y, int& cb, int& cr) {
    const int r = p & 255, g = (p >> 8) & 255, b = (p >> 16) & 255;
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint.c: one 1-D pass of jpeg_fdct_islow, in place
template <bool SECOND>
__device__ __forceinline__ void fdct_1d(int* d) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = SECOND ? CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS;
    d[0] = SECOND ? descale(t10 + t11, PASS1_BITS) : (t10 + t11) * (1 << PASS1_BITS);
    d[4] = SECOND ? descale(t10 - t11, PASS1_BITS) : (t10 - t11) * (1 << PASS1_BITS);
    int z1 = (t12 + t13) * F_0_541196100;
    d[2] = descale(z1 + t13 * F_0_765366865, n);
    d[6] = descale(z1 + t12 * (-F_1_847759065), n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int u4 = t4 * F_0_298631336, u5 = t5 * F_2_053119869, u6 = t6 * F_3_072711026, u7 = t7 * F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * (-F_1_961570560) + z5;
    z4 = z4 * (-F_0_390180644) + z5;
    d[7] = descale(u4 + z1 + z3, n);
    d[5] = descale(u5 + z2 + z4, n);
    d[3] = descale(u6 + z2 + z3, n);
    d[1] = descale(u7 + z1 + z4, n);
}

// jcdctmgr.c: the divisor is q << 3 (the forward DCT's scaling), the magnitude rounded half up, the sign restored; an exact 32-bit
// integer division.  Returns the quantised level.
__device__ __forceinline__ int jpeg_quantise(int d, int qk) {
    const uint32_t qv = (uint32_t)qk << 3;
    const uint32_t mag = ((uint32_t)(d < 0 ? -d : d) + (qv >> 1)) / qv;
    return d < 0 ? -(int)mag : (int)mag;
}

struct JpegTile {   // a workgroup's LDS, 6784 bytes: declare one __shared__ per kernel
    int y[16 * SY];      // luma, level-shifted; the passes work in place
    int c[2][8 * SC];    // Cb, Cr after downsampling
    int q[2][64];        // the quantisation tables: luma, chroma; natural order
};

// Colour conversion, edge replication and chroma downsampling of the tile whose first luma sample is (gx0, gy0): one 2 x 2 quad per
// thread, level-shifted samples into s_y [16 * SY] and s_c [2][8 * SC].
__device__ __forceinline__ void jpeg_stage_quad(const uint32_t* __restrict__ img, int h, int w, int gx0, int gy0, int tid, int* s_y,
                                                int (*s_c)[8 * SC]) {
    const int qx = tid & 31, qy = tid >> 5;
    const int x0 = gx0 + 2 * qx, y0 = gy0 + 2 * qy;
    const int X0 = min(x0, w - 1), X1 = min(x0 + 1, w - 1);
    const int Y0 = min(y0, h - 1), Y1 = min(y0 + 1, h - 1);
    uint32_t p00 = img[(int64_t)Y0 * w + X0], p01 = img[(int64_t)Y0 * w + X1];
    uint32_t p10 = img[(int64_t)Y1 * w + X0], p11 = img[(int64_t)Y1 * w + X1];
    int ya, yb, yc, yd, cb[4], cr[4];
    rgb_to_ycc(p00, ya, cb[0], cr[0]);
    rgb_to_ycc(p01, yb, cb[1], cr[1]);
    rgb_to_ycc(p10, yc, cb[2], cr[2]);
    rgb_to_ycc(p11, yd, cb[3], cr[3]);
    s_y[(2 * qy) * SY + 2 * qx] = ya - 128;
    s_y[(2 * qy) * SY + 2 * qx + 1] = yb - 128;
    s_y[(2 * qy + 1) * SY + 2 * qx] = yc - 128;
    s_y[(2 * qy + 1) * SY + 2 * qx + 1] = yd - 128;
    // chroma rows below the image repeat the last DOWNSAMPLED row: the box over rows 2 (ch - 1) and min(2 ch - 1, h - 1)
    const int ch = (h + 1) >> 1;
    const int cye = min(y0 >> 1, ch - 1);
    const int C0 = 2 * cye, C1 = min(2 * cye + 1, h - 1);
    if (C0 != Y0 || C1 != Y1) {
        int unused;
        rgb_to_ycc(img[(int64_t)C0 * w + X0], unused, cb[0], cr[0]);
        rgb_to_ycc(img[(int64_t)C0 * w + X1], unused, cb[1], cr[1]);
        rgb_to_ycc(img[(int64_t)C1 * w + X0], unused, cb[2], cr[2]);
        rgb_to_ycc(img[(int64_t)C1 * w + X1], unused, cb[3], cr[3]);
    }
    const int bias = 1 + ((x0 >> 1) & 1);   // 1, 2, 1, 2 ... from the row's first chroma sample
    s_c[0][qy * SC + qx] = ((cb[0] + cb[1] + cb[2] + cb[3] + bias) >> 2) - 128;
    s_c[1][qy * SC + qx] = ((cr[0] + cr[1] + cr[2] + cr[3] + bias) >> 2) - 128;
}

// Eight threads per block: blocks 0 .. 15 luma (MCU m: 4 m .. 4 m + 3, row-major inside the MCU), 16 .. 19 Cb, 20 .. 23 Cr
struct JpegBlockMap {
    int blk, r;      // block of the workgroup, row / column of this thread
    bool working, luma;
    int m, comp;     // MCU of the workgroup; 0 Y, 1 Cb, 2 Cr
    int by, bx;      // luma: block row / column inside the MCU
    int k;           // block inside the MCU, in the scan's order: 0 .. 3 luma (row-major), 4 Cb, 5 Cr
    int stride;      // LDS row stride of the block's plane
    int* base;       // the block's first sample in the tile
    __device__ __forceinline__ JpegBlockMap(int tid, JpegTile& t) {
        blk = tid >> 3;
        r = tid & 7;
        working = blk < 6 * MCUS;
        luma = blk < 4 * MCUS;
        m = luma ? blk >> 2 : (blk - 4 * MCUS) & (MCUS - 1);
        comp = luma ? 0 : 1 + ((blk - 4 * MCUS) >> 2);
        by = luma ? (blk >> 1) & 1 : 0;
        bx = luma ? blk & 1 : 0;
        k = luma ? by * 2 + bx : 3 + comp;
        stride = luma ? SY : SC;
        base = luma ? t.y + (by * 8) * SY + m * 16 + bx * 8 : t.c[working ? comp - 1 : 0] + m * 8;
    }
};

// The forward half of the workgroup's tile -- MCUs MCUS * blockIdx.x .. + MCUS - 1 of MCU row blockIdx.y of image blockIdx.z -- in two steps.
// jpeg_forward_rows: the tables into LDS (t.q), the samples (jpeg_stage_quad), the row pass in place; returns the thread's place in the
// tile.  EVERY thread of the workgroup calls it: it has two barriers, the second behind the row pass.
__device__ __forceinline__ JpegBlockMap jpeg_forward_rows(const uint32_t* __restrict__ in, int h, int w, const QTables& qt, JpegTile& t) {
    const int tid = threadIdx.x;
    const int gx0 = blockIdx.x * TW, gy0 = blockIdx.y * 16;   // the tile's first luma sample
    const uint32_t* img = in + (int64_t)blockIdx.z * h * w;
    if (tid < 128) t.q[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];
    jpeg_stage_quad(img, h, w, gx0, gy0, tid, t.y, t.c);   // colour conversion, edge replication and chroma downsampling
    __syncthreads();
    const JpegBlockMap map(tid, t);
    if (map.working) {
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = map.base[map.r * map.stride + k];
        fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; k++) map.base[map.r * map.stride + k] = d[k];
    }
    __syncthreads();
    return map;
}

// jpeg_forward_column, for a WORKING thread behind jpeg_forward_rows: d[0 .. 7] = column map.r of its block through the second pass,
// the coefficients scaled by 8 and not yet quantised.  (A step of its own so that the calling kernel goes on under the same
// `if (map.working)`: two such regions in a row compile to more instructions than one.)
__device__ __forceinline__ void jpeg_forward_column(const JpegBlockMap& map, int* d) {
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = map.base[k * map.stride + map.r];
    fdct_1d<true>(d);
}

// ---------------------------------------------------------------- host side of the entries

struct JpegGeometry {   // an image in whole MCUs: 16 x 16 (4:2:0, the default), or the MCU of another sampling of jpeg_entropy.h's JE_SAMPLING_*
    int mcu_w, mcu_h;             // the MCU in luma samples: 16 x 16 (4:2:0), 16 wide x 8 high (4:2:2), 8 x 8 (4:4:4, greyscale)
    int mcus_w, mcus_h, Wm, Hm;   // MCUs across and down; the padded size (the planes' of jpeg_inverse.h)
    JpegGeometry(int32_t h, int32_t w, int sampling = 0)
        : mcu_w(sampling <= 1 ? 16 : 8), mcu_h(sampling == 0 ? 16 : 8), mcus_w((w + mcu_w - 1) / mcu_w), mcus_h((h + mcu_h - 1) / mcu_h),
          Wm(mcus_w * mcu_w), Hm(mcus_h * mcu_h) {}
    size_t mcus() const { return (size_t)mcus_w * mcus_h; }
};

// The refusals.  `entry` is the exported function that refuses; every helper returns false after recording "<entry>: <why>".
inline bool jpeg_refuse(const char* entry, const std::string& why) { return salve_fail((std::string(entry) + ": " + why).c_str()); }

inline bool jpeg_shape_ok(const char* entry, int32_t n, int32_t h, int32_t w) {
    if (n > 0 && n <= MAX_IMAGES && h >= 1 && h <= MAX_DIM && w >= 1 && w <= MAX_DIM) return true;
    return jpeg_refuse(entry, "n outside 1..65535 or h / w outside 1..4096");
}

// qtab: uint16 [2][64] on the host, natural order
inline bool jpeg_load_qtables(const char* entry, const uint16_t* qtab, QTables* qt) {
    for (int i = 0; i < 128; i++) {
        if (qtab[i] < 1 || qtab[i] > 255) return jpeg_refuse(entry, "a quantisation table entry outside 1..255 (baseline)");
        qt->q[i >> 6][i & 63] = qtab[i];
    }
    return true;
}

// need: what <entry>_workspace_bytes returns for the call's n, h, w
inline bool jpeg_workspace_ok(const char* entry, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes >= need && !((uintptr_t)ws & 15)) return true;
    return jpeg_refuse(entry, std::string("the workspace is smaller than ") + entry + "_workspace_bytes says or not 16-byte aligned");
}

}  // namespace

#endif  // SALVE_JPEG_FORWARD_H
