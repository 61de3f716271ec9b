// jpeg_roundtrip.hip -- decode(encode(img)) of baseline 4:2:0 JPEG on gfx950 (MI355X), bit for bit what libjpeg's defaults give,
// without an entropy coder or a file (opt-in: BevRasteriser.jpeg_roundtrip, RenderVerifyPipeline(jpeg_quality=),
// RenderedTrainSource(jpeg_quality=)).
//
// The reference writes every BEV render as a JPEG (imageio -> Pillow -> libjpeg, quality 75; bev_rendering_utils.py:629-630) and
// trains and evaluates on the decoded files (zind_data.py:306-315).  Baseline JPEG with the slow-integer DCT is pure integer
// arithmetic, and quantised coefficients of 8-bit data always fit the Huffman code range, so the decoded pixels depend on the
// quantised coefficients alone.  The stages, in libjpeg's order and with its constants:
//   rgb -> YCbCr       16-bit fixed point (jccolor.c)
//   edges              luma: right and bottom edge replicated to whole blocks.  chroma: rows replicated to a whole row group (2)
//                      and columns to whole blocks BEFORE downsampling, the DOWNSAMPLED rows replicated to whole blocks AFTER it
//                      (jcprepct.c) -- for an even height that is no multiple of 16 the two differ
//   downsampling       h2v2 box, bias alternating 1, 2 along a row (jcsample.c)
//   forward DCT        jpeg_fdct_islow on samples - 128 (jfdctint.c), outputs scaled by 8
//   quantisation       divisor q << 3, magnitude rounded half up, sign restored (jcdctmgr.c); an exact 32-bit integer division
//   dequantisation, inverse DCT   jpeg_idct_islow with its masked range-limit table (jidctint.c)
//   upsampling         h2v2 "fancy" triangle filter, biases 8 and 7, nearer sample taken twice at the first / last column and the
//                      top / bottom row; plain replication where the chroma plane is at most two samples wide (jdsample.c)
//   YCbCr -> rgb       16-bit fixed point and the range limit (jdcolor.c)
//
// Two launches.  jpeg_blocks_kernel: a workgroup of 256 threads owns four MCUs (16 x 16 pixels each) side by side.  Every thread
// converts one 2 x 2 pixel quad into LDS (four luma samples, one Cb, one Cr); then each of the 24 blocks (16 luma, 4 Cb, 4 Cr) gets
// eight threads, one per row / column, for the four 1-D passes through LDS; a thread leaves the decoded row of its block as ONE
// 8-byte store into the workspace's planes (luma [Hm][Wm], Cb and Cr [Hm/2][Wm/2] bytes, Hm and Wm the image rounded up to whole
// MCUs).  jpeg_pixels_kernel: a thread per pair of output pixels upsamples the chroma (it needs a one-sample halo across block
// borders, which is why this is a launch of its own), converts and stores 4 bytes per pixel with the top byte 0.  The input is
// read by the first launch only and the output written by the second only: in place is allowed.
// Integer arithmetic only (32-bit: libjpeg's DCTs are built to fit it for 8-bit samples), no atomics, every output has one writer:
// the same inputs give the same bits.  Every offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
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

// jidctint.c: one 1-D pass of jpeg_idct_islow, in place, descaled by n bits (its zero-AC short cuts give what these formulas give)
__device__ __forceinline__ void idct_1d(int* d, int n) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * F_0_541196100;
    int t2 = z1 + z3 * (-F_1_847759065), t3 = z1 + z2 * F_0_765366865;
    int t0 = (d[0] + d[4]) * (1 << CONST_BITS), t1 = (d[0] - d[4]) * (1 << CONST_BITS);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7];
    t1 = d[5];
    t2 = d[3];
    t3 = d[1];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * F_1_175875602;
    t0 *= F_0_298631336;
    t1 *= F_2_053119869;
    t2 *= F_3_072711026;
    t3 *= F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * (-F_1_961570560) + z5;
    z4 = z4 * (-F_0_390180644) + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    d[0] = descale(t10 + t3, n);
    d[7] = descale(t10 - t3, n);
    d[1] = descale(t11 + t2, n);
    d[6] = descale(t11 - t2, n);
    d[2] = descale(t12 + t1, n);
    d[5] = descale(t12 - t1, n);
    d[3] = descale(t13 + t0, n);
    d[4] = descale(t13 - t0, n);
}

// jidctint.c: range_limit[v & RANGE_MASK], the table that stands behind the level shift
__device__ __forceinline__ uint32_t idct_range_limit(int v) {
    const int i = v & 1023;
    return (uint32_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// grid (MCU groups across, MCU rows, images)
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_blocks_kernel(const uint32_t* __restrict__ in, uint8_t* __restrict__ ws, int h, int w, int Hm,
                                                                   int Wm, QTables qt) {
    __shared__ int s_y[16 * SY];
    __shared__ int s_c[2][8 * SC];
    __shared__ int s_q[2][64];
    const int tid = threadIdx.x;
    const int gx0 = blockIdx.x * TW, gy0 = blockIdx.y * 16;   // the tile's first luma sample
    const uint32_t* img = in + (int64_t)blockIdx.z * h * w;
    if (tid < 128) s_q[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];

    {   // colour conversion, edge replication and chroma downsampling: one 2 x 2 quad per thread
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
    __syncthreads();

    // eight threads per block: blocks 0 .. 15 luma (MCU m: 4 m .. 4 m + 3, row-major inside the MCU), 16 .. 19 Cb, 20 .. 23 Cr
    const int blk = tid >> 3, r = tid & 7;
    const bool working = blk < 6 * MCUS;
    const bool luma = blk < 4 * MCUS;
    const int m = luma ? blk >> 2 : (blk - 4 * MCUS) & (MCUS - 1);
    const int comp = luma ? 0 : 1 + ((blk - 4 * MCUS) >> 2);          // 0 Y, 1 Cb, 2 Cr
    const int by = luma ? (blk >> 1) & 1 : 0, bx = luma ? blk & 1 : 0;
    const int stride = luma ? SY : SC;
    int* base = luma ? s_y + (by * 8) * SY + m * 16 + bx * 8 : s_c[working ? comp - 1 : 0] + m * 8;
    const int* q = s_q[luma ? 0 : 1];
    int d[8];
    if (working) {   // forward pass 1: rows
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = base[r * stride + k];
        fdct_1d<false>(d);
#pragma unroll
        for (int k = 0; k < 8; k++) base[r * stride + k] = d[k];
    }
    __syncthreads();
    if (working) {   // forward pass 2 on column r, quantise, dequantise, inverse pass 1 on the same column
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = base[k * stride + r];
        fdct_1d<true>(d);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int qk = q[k * 8 + r];
            const uint32_t qv = (uint32_t)qk << 3;
            const uint32_t mag = ((uint32_t)(d[k] < 0 ? -d[k] : d[k]) + (qv >> 1)) / qv;   // exact 32-bit division
            d[k] = (d[k] < 0 ? -(int)mag : (int)mag) * qk;
        }
        idct_1d(d, CONST_BITS - PASS1_BITS);
#pragma unroll
        for (int k = 0; k < 8; k++) base[k * stride + r] = d[k];
    }
    __syncthreads();
    const int mcu = blockIdx.x * MCUS + m;
    if (working && mcu * 16 < Wm) {   // inverse pass 2 on row r; the decoded row leaves as one 8-byte store
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = base[r * stride + k];
        idct_1d(d, CONST_BITS + PASS1_BITS + 3);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            lo |= idct_range_limit(d[k]) << (8 * k);
            hi |= idct_range_limit(d[k + 4]) << (8 * k);
        }
        const int64_t ysize = (int64_t)Hm * Wm;
        uint8_t* planes = ws + (int64_t)blockIdx.z * (ysize + ysize / 2);
        uint8_t* dst;
        if (luma) dst = planes + (int64_t)(gy0 + by * 8 + r) * Wm + mcu * 16 + bx * 8;
        else dst = planes + ysize + (comp - 1) * (ysize / 4) + (int64_t)(gy0 / 2 + r) * (Wm / 2) + mcu * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

// 3 * nearer row + further row of one chroma column (jdsample.c: thiscolsum)
__device__ __forceinline__ int colsum(const uint8_t* __restrict__ near_row, const uint8_t* __restrict__ far_row, int c) {
    return 3 * (int)near_row[c] + (int)far_row[c];
}

// block (64, 4): a thread per pair of pixels (2 cx, 2 cx + 1) of one row; grid (pairs across / 64, rows / 4, images)
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pixels_kernel(const uint8_t* __restrict__ ws, uint32_t* __restrict__ out, int h, int w, int Hm,
                                                                   int Wm) {
    const int cx = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    if (cx >= cw || y >= h) return;
    const int64_t ysize = (int64_t)Hm * Wm;
    const uint8_t* planes = ws + (int64_t)blockIdx.z * (ysize + ysize / 2);
    const uint8_t* yrow = planes + (int64_t)y * Wm;
    const int cy = y >> 1;
    int c_even[2], c_odd[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint8_t* plane = planes + ysize + k * (ysize / 4);
        const uint8_t* near_row = plane + (int64_t)cy * (Wm / 2);
        if (cw <= 2) {   // libjpeg upsamples a component of at most two samples a row by replication
            c_even[k] = c_odd[k] = near_row[cx];
            continue;
        }
        const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
        const uint8_t* far_row = plane + (int64_t)fy * (Wm / 2);
        const int here = colsum(near_row, far_row, cx);
        c_even[k] = cx == 0 ? (here * 4 + 8) >> 4 : (here * 3 + colsum(near_row, far_row, cx - 1) + 8) >> 4;
        c_odd[k] = cx == cw - 1 ? (here * 4 + 7) >> 4 : (here * 3 + colsum(near_row, far_row, cx + 1) + 7) >> 4;
    }
    uint32_t* orow = out + ((int64_t)blockIdx.z * h + y) * w;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int x = 2 * cx + e;
        if (x >= w) break;
        const int Y = yrow[x], cbx = (e ? c_odd[0] : c_even[0]) - 128, crx = (e ? c_odd[1] : c_even[1]) - 128;
        // jdcolor.c: the four tables of ycc_rgb_convert (arithmetic shifts of negative sums, as RIGHT_SHIFT)
        const int R = clamp255(Y + ((91881 * crx + 32768) >> 16));
        const int B = clamp255(Y + ((116130 * cbx + 32768) >> 16));
        const int G = clamp255(Y + ((-22554 * cbx + 32768 - 46802 * crx) >> 16));
        orow[x] = (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
    }
}

bool good_shape(int32_t n, int32_t h, int32_t w) { return n > 0 && n <= MAX_IMAGES && h >= 1 && h <= MAX_DIM && w >= 1 && w <= MAX_DIM; }

}  // namespace

extern "C" {

size_t salve_bev_jpeg_roundtrip_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!good_shape(n, h, w)) {
        salve_fail("salve_bev_jpeg_roundtrip_workspace_bytes: n outside 1..65535 or h / w outside 1..4096");
        return 0;
    }
    const size_t Hm = ((size_t)h + 15) / 16 * 16, Wm = ((size_t)w + 15) / 16 * 16;
    return (size_t)n * (Hm * Wm + Hm * Wm / 2);
}

int salve_bev_jpeg_roundtrip(const uint32_t* bev_in, uint32_t* bev_out, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!bev_in || !bev_out || !qtab || !ws) { salve_fail("salve_bev_jpeg_roundtrip: null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!good_shape(n, h, w)) { salve_fail("salve_bev_jpeg_roundtrip: n outside 1..65535 or h / w outside 1..4096"); return SALVE_ERR_BAD_ARG; }
    if (((uintptr_t)bev_in | (uintptr_t)bev_out) & 3) { salve_fail("salve_bev_jpeg_roundtrip: the images must be 4-byte aligned"); return SALVE_ERR_BAD_ARG; }
    QTables qt;
    for (int i = 0; i < 128; i++) {
        if (qtab[i] < 1 || qtab[i] > 255) { salve_fail("salve_bev_jpeg_roundtrip: a quantisation table entry outside 1..255 (baseline)"); return SALVE_ERR_BAD_ARG; }
        qt.q[i >> 6][i & 63] = qtab[i];
    }
    if (ws_bytes < salve_bev_jpeg_roundtrip_workspace_bytes(n, h, w) || ((uintptr_t)ws & 15)) {
        salve_fail("salve_bev_jpeg_roundtrip: the workspace is smaller than salve_bev_jpeg_roundtrip_workspace_bytes says or not 16-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    const int Hm = (h + 15) / 16 * 16, Wm = (w + 15) / 16 * 16;
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)((Wm + TW - 1) / TW), (unsigned)(Hm / 16), (unsigned)n), dim3(JPEG_THREADS), 0,
                       (hipStream_t)stream, bev_in, (uint8_t*)ws, (int)h, (int)w, Hm, Wm, qt);
    SALVE_HIP_CHECK(hipGetLastError());
    const int cw = (w + 1) / 2;
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)((cw + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)n), dim3(64, 4), 0, (hipStream_t)stream,
                       (const uint8_t*)ws, bev_out, (int)h, (int)w, Hm, Wm);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // extern "C"
