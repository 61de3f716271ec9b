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
#include "jpeg_forward.h"   // the forward chain, shared with jpeg_encode.hip
#include "jpeg_inverse.h"   // the inverse DCT pass and jpeg_pixels_kernel, shared with jpeg_decode.hip
#include "salve_common.h"

namespace {

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

    jpeg_stage_quad(img, h, w, gx0, gy0, tid, s_y, s_c);   // colour conversion, edge replication and chroma downsampling
    __syncthreads();

    // eight threads per block: blocks 0 .. 15 luma (MCU m: 4 m .. 4 m + 3, row-major inside the MCU), 16 .. 19 Cb, 20 .. 23 Cr
    const JpegBlockMap map(tid);
    const int r = map.r, m = map.m, comp = map.comp, by = map.by, bx = map.bx, stride = map.stride;
    const bool working = map.working, luma = map.luma;
    int* base = map.base(s_y, s_c);
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
            d[k] = jpeg_quantise(d[k], qk) * qk;
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

}  // namespace

extern "C" {

size_t salve_bev_jpeg_roundtrip_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!jpeg_good_shape(n, h, w)) {
        salve_fail("salve_bev_jpeg_roundtrip_workspace_bytes: n outside 1..65535 or h / w outside 1..4096");
        return 0;
    }
    const size_t Hm = ((size_t)h + 15) / 16 * 16, Wm = ((size_t)w + 15) / 16 * 16;
    return (size_t)n * (Hm * Wm + Hm * Wm / 2);
}

int salve_bev_jpeg_roundtrip(const uint32_t* bev_in, uint32_t* bev_out, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!bev_in || !bev_out || !qtab || !ws) { salve_fail("salve_bev_jpeg_roundtrip: null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!jpeg_good_shape(n, h, w)) { salve_fail("salve_bev_jpeg_roundtrip: n outside 1..65535 or h / w outside 1..4096"); return SALVE_ERR_BAD_ARG; }
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
