// jpeg_inverse.h -- the inverse half of libjpeg's baseline 4:2:0 chain as device code, shared by jpeg_roundtrip.hip (which takes the
// quantised coefficients from the forward chain) and jpeg_decode.hip (which takes them from a file's entropy-coded scan): the 1-D pass of
// the slow-integer inverse DCT with its range limit (jidctint.c), and the launch that upsamples the chroma planes, converts to RGB and
// stores the pixels (jdsample.c, jdcolor.c).  Both files leave the decoded samples in the same planes: luma [Hm][Wm], Cb and Cr
// [Hm / 2][Wm / 2] bytes per image, Hm and Wm the image rounded up to whole 16 x 16 MCUs.  32-bit integer arithmetic only; every offset
// is 64-bit.
#ifndef SALVE_JPEG_INVERSE_H
#define SALVE_JPEG_INVERSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_forward.h"   // the DCT's constants, descale, JPEG_THREADS

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

}  // namespace

#endif  // SALVE_JPEG_INVERSE_H
