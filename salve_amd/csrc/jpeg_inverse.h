// jpeg_inverse.h -- the inverse half of libjpeg's baseline chain (4:2:0, and for jpeg_decode.hip 4:2:2, 4:4:4 and greyscale) as device code, shared by jpeg_roundtrip.hip (which takes the
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

// The planes, the layout contract between the kernels that decode blocks and the pixels kernels: per image, the component planes back to
// back -- luma [Hm][Wm] bytes, then Cb, then Cr -- Hm and Wm the image rounded up to whole MCUs of its sampling (JpegGeometry); the images
// follow each other without a gap.  A chroma plane is [Hm / 2][Wm / 2] for 4:2:0 (16 x 16 MCUs: the default, and all jpeg_roundtrip.hip
// knows), [Hm][Wm / 2] for 4:2:2 (16 x 8), [Hm][Wm] for 4:4:4 (8 x 8); greyscale has the luma plane alone.  JpegPlanes is that contract
// for sampling S (jpeg_entropy.h: JE_SAMPLING_*), a compile-time argument of every kernel that touches the planes.
template <int S>
struct JpegPlanes {
    static constexpr int cshift_x = S <= 1 ? 1 : 0, cshift_y = S == 0 ? 1 : 0;   // luma samples per chroma sample, as shifts
    static constexpr int chroma_planes = S == 3 ? 0 : 2;
    static constexpr int luma_across = S <= 1 ? 2 : 1, luma_down = S == 0 ? 2 : 1;   // luma blocks of an MCU
    static constexpr int luma_blocks = luma_across * luma_down;
    __host__ __device__ static __forceinline__ int64_t chroma_bytes(int Hm, int Wm) { return ((int64_t)Hm * Wm) >> (cshift_x + cshift_y); }
    __host__ __device__ static __forceinline__ int64_t image_bytes(int Hm, int Wm) { return (int64_t)Hm * Wm + chroma_planes * chroma_bytes(Hm, Wm); }   // a multiple of 64
};

__host__ __device__ __forceinline__ int64_t jpeg_image_planes_bytes(int Hm, int Wm) { return JpegPlanes<0>::image_bytes(Hm, Wm); }   // 4:2:0: a multiple of 384

inline size_t jpeg_planes_bytes(int32_t n, const JpegGeometry& g) { return (size_t)n * (size_t)jpeg_image_planes_bytes(g.Hm, g.Wm); }

// Inverse pass 2 on row r of block k of MCU (my, mx), k in the scan's order (for 4:2:0 JpegBlockMap::k: 0 .. 3 luma, 4 Cb, 5 Cr): d[0 .. 7]
// is that row after pass 1.  Range limit, and the row leaves as ONE 8-byte store into the planes of image blockIdx.z of `ws`.
template <int S = 0>
__device__ __forceinline__ void jpeg_store_decoded_row(int* d, uint8_t* __restrict__ ws, int Hm, int Wm, int my, int mx, int k, int r) {
    using P = JpegPlanes<S>;
    idct_1d(d, CONST_BITS + PASS1_BITS + 3);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        lo |= idct_range_limit(d[j]) << (8 * j);
        hi |= idct_range_limit(d[j + 4]) << (8 * j);
    }
    const int64_t ysize = (int64_t)Hm * Wm;
    uint8_t* planes = ws + blockIdx.z * P::image_bytes(Hm, Wm);
    uint8_t* dst;
    if (k < P::luma_blocks) {
        const int by = P::luma_across == 2 ? k >> 1 : 0, bx = P::luma_across == 2 ? k & 1 : 0;
        dst = planes + (int64_t)((my * P::luma_down + by) * 8 + r) * Wm + (mx * P::luma_across + bx) * 8;
    } else {
        dst = planes + ysize + (k - P::luma_blocks) * P::chroma_bytes(Hm, Wm) + (int64_t)(my * 8 + r) * (Wm >> P::cshift_x) + mx * 8;
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jdcolor.c: the four tables of ycc_rgb_convert (arithmetic shifts of negative sums, as RIGHT_SHIFT) on one sample -> 0x00BBGGRR
__device__ __forceinline__ uint32_t jpeg_ycc_pixel(int Y, int cb, int cr) {
    const int cbx = cb - 128, crx = cr - 128;
    const int R = clamp255(Y + ((91881 * crx + 32768) >> 16));
    const int B = clamp255(Y + ((116130 * cbx + 32768) >> 16));
    const int G = clamp255(Y + ((-22554 * cbx + 32768 - 46802 * crx) >> 16));
    return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
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
        orow[x] = jpeg_ycc_pixel(yrow[x], e ? c_odd[0] : c_even[0], e ? c_odd[1] : c_even[1]);
    }
}

// The pixels of the samplings beyond 4:2:0 (S: JE_SAMPLING_422, _444 or _GREY), the same thread map and grid.  4:2:2 is jdsample.c's
// h2v1_fancy_upsample, horizontally only: 3/4 of the nearer chroma sample and 1/4 of the further, rounded with + 1 to the left and + 2 to
// the right, the row's two end pixels copied; 4:4:4 takes its chroma as it stands; greyscale is Y in all three bytes (Pillow's mode L
// repeated into three channels).
template <int S>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pixels_sampled_kernel(const uint8_t* __restrict__ ws, uint32_t* __restrict__ out, int h, int w,
                                                                           int Hm, int Wm) {
    static_assert(S >= 1 && S <= 3, "4:2:0 is jpeg_pixels_kernel");
    using P = JpegPlanes<S>;
    const int cx = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int cw = (w + 1) >> 1;
    if (cx >= cw || y >= h) return;
    const int64_t ysize = (int64_t)Hm * Wm;
    const uint8_t* planes = ws + blockIdx.z * P::image_bytes(Hm, Wm);
    const uint8_t* yrow = planes + (int64_t)y * Wm;
    uint32_t* orow = out + ((int64_t)blockIdx.z * h + y) * w;
    int c_even[2] = {0, 0}, c_odd[2] = {0, 0};
    if (S == 1) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint8_t* row = planes + ysize + k * P::chroma_bytes(Hm, Wm) + (int64_t)y * (Wm >> 1);
            const int here = row[cx];
            if (cw <= 2) {   // libjpeg upsamples a component of at most two samples a row by replication
                c_even[k] = c_odd[k] = here;
                continue;
            }
            c_even[k] = cx == 0 ? here : (3 * here + (int)row[cx - 1] + 1) >> 2;
            c_odd[k] = cx == cw - 1 ? here : (3 * here + (int)row[cx + 1] + 2) >> 2;
        }
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int x = 2 * cx + e;
        if (x >= w) break;
        const int Y = yrow[x];
        if (S == 3) {
            orow[x] = (uint32_t)Y | ((uint32_t)Y << 8) | ((uint32_t)Y << 16);
        } else if (S == 2) {
            orow[x] = jpeg_ycc_pixel(Y, planes[ysize + (int64_t)y * Wm + x], planes[2 * ysize + (int64_t)y * Wm + x]);
        } else {
            orow[x] = jpeg_ycc_pixel(Y, e ? c_odd[0] : c_even[0], e ? c_odd[1] : c_even[1]);
        }
    }
}

// The planes of n images -> their pixels (out: uint32 [n][h][w], 0x00BBGGRR)
inline hipError_t jpeg_launch_pixels(const uint8_t* planes, uint32_t* out, int32_t n, int32_t h, int32_t w, const JpegGeometry& g, hipStream_t stream) {
    const int cw = (w + 1) / 2;
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)((cw + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)n), dim3(64, 4), 0, stream, planes, out,
                       (int)h, (int)w, g.Hm, g.Wm);
    return hipGetLastError();
}

template <int S>
inline hipError_t jpeg_launch_pixels_sampled(const uint8_t* planes, uint32_t* out, int32_t n, int32_t h, int32_t w, const JpegGeometry& g, hipStream_t stream) {
    const int cw = (w + 1) / 2;
    hipLaunchKernelGGL(jpeg_pixels_sampled_kernel<S>, dim3((unsigned)((cw + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)n), dim3(64, 4), 0, stream, planes,
                       out, (int)h, (int)w, g.Hm, g.Wm);
    return hipGetLastError();
}

}  // namespace

#endif  // SALVE_JPEG_INVERSE_H
