// jpeg_inverse.h -- the inverse half of libjpeg's baseline 4:2:0 chain as device code, shared by jpeg_roundtrip.hip (which takes the
// quantised coefficients from the forward chain) and jpeg_decode.hip (which takes them from a file's entropy-coded scan): the 1-D pass of
// the slow-integer inverse DCT with its range limit (jidctint.c), the store of a block's decoded row into the planes
// (jpeg_store_decoded_row: the planes' layout is written there, once), and the launch that upsamples the chroma planes, converts to RGB
// and stores the pixels (jpeg_pixels_kernel behind jpeg_launch_pixels; jdsample.c, jdcolor.c).  32-bit integer arithmetic only; every
// offset is 64-bit.
#ifndef SALVE_JPEG_INVERSE_H
#define SALVE_JPEG_INVERSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_forward.h"   // the DCT's constants, descale, JPEG_THREADS, JpegGeometry

namespace {

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

// The planes, the layout contract between the kernels that decode blocks and jpeg_pixels_kernel: per image, luma [Hm][Wm] bytes, then Cb
// [Hm / 2][Wm / 2], then Cr likewise, Hm and Wm the image rounded up to whole 16 x 16 MCUs; the images follow each other without a gap.
__host__ __device__ __forceinline__ int64_t jpeg_image_planes_bytes(int Hm, int Wm) {
    const int64_t ysize = (int64_t)Hm * Wm;
    return ysize + ysize / 2;   // a multiple of 384
}

inline size_t jpeg_planes_bytes(int32_t n, const JpegGeometry& g) { return (size_t)n * (size_t)jpeg_image_planes_bytes(g.Hm, g.Wm); }

// Inverse pass 2 on row r of block k (JpegBlockMap::k: 0 .. 3 luma, 4 Cb, 5 Cr) of MCU (my, mx): d[0 .. 7] is that row after pass 1.
// Range limit, and the row leaves as ONE 8-byte store into the planes of image blockIdx.z of `ws`.
__device__ __forceinline__ void jpeg_store_decoded_row(int* d, uint8_t* __restrict__ ws, int Hm, int Wm, int my, int mx, int k, int r) {
    idct_1d(d, CONST_BITS + PASS1_BITS + 3);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        lo |= idct_range_limit(d[j]) << (8 * j);
        hi |= idct_range_limit(d[j + 4]) << (8 * j);
    }
    const int64_t ysize = (int64_t)Hm * Wm;
    uint8_t* planes = ws + blockIdx.z * jpeg_image_planes_bytes(Hm, Wm);
    uint8_t* dst;
    if (k < 4) dst = planes + (int64_t)(my * 16 + (k >> 1) * 8 + r) * Wm + mx * 16 + (k & 1) * 8;
    else dst = planes + ysize + (k - 4) * (ysize / 4) + (int64_t)(my * 8 + r) * (Wm / 2) + mx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

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
    const uint8_t* planes = ws + blockIdx.z * jpeg_image_planes_bytes(Hm, Wm);
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

// The planes of n images -> their pixels (out: uint32 [n][h][w], 0x00BBGGRR)
inline hipError_t jpeg_launch_pixels(const uint8_t* planes, uint32_t* out, int32_t n, int32_t h, int32_t w, const JpegGeometry& g, hipStream_t stream) {
    const int cw = (w + 1) / 2;
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)((cw + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)n), dim3(64, 4), 0, stream, planes, out,
                       (int)h, (int)w, g.Hm, g.Wm);
    return hipGetLastError();
}

}  // namespace

#endif  // SALVE_JPEG_INVERSE_H
