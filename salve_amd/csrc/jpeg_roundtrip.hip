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
// Two launches.  jpeg_blocks_kernel: the forward tile of jpeg_forward.h (a workgroup of 256 threads owns four MCUs side by side, eight
// threads per block; jpeg_forward_rows, jpeg_forward_column), then, on the same registers and LDS: quantise, dequantise, the two inverse
// passes; a thread leaves the decoded row of its block as ONE 8-byte store into the workspace's planes (jpeg_inverse.h:
// jpeg_store_decoded_row, where their layout is written down).  jpeg_pixels_kernel (jpeg_inverse.h): a thread per pair of output pixels
// upsamples the chroma (it needs a one-sample halo across block borders, which is why this is a launch of its own), converts and stores
// 4 bytes per pixel with the top byte 0.  The input is read by the first launch only and the output written by the second only: in
// place is allowed.
// Integer arithmetic only (32-bit: libjpeg's DCTs are built to fit it for 8-bit samples), no atomics, every output has one writer:
// the same inputs give the same bits.  Every offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "jpeg_forward.h"   // the forward tile, shared with jpeg_encode.hip; the entries' shared refusals
#include "jpeg_inverse.h"   // the inverse DCT pass, the planes and jpeg_pixels_kernel, shared with jpeg_decode.hip
#include "salve_common.h"

namespace {

// grid (MCU groups across, MCU rows, images)
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_blocks_kernel(const uint32_t* __restrict__ in, uint8_t* __restrict__ ws, int h, int w, int Hm,
                                                                   int Wm, QTables qt) {
    __shared__ JpegTile t;
    const JpegBlockMap map = jpeg_forward_rows(in, h, w, qt, t);
    const int r = map.r, stride = map.stride;
    int* base = map.base;
    int d[8];
    if (map.working) {   // forward pass 2 on column r, quantise, dequantise, inverse pass 1 on the same column
        const int* q = t.q[map.luma ? 0 : 1];
        jpeg_forward_column(map, d);
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
    const int mcu = blockIdx.x * MCUS + map.m;
    if (map.working && mcu * 16 < Wm) {   // inverse pass 2 on row r
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = base[r * stride + k];
        jpeg_store_decoded_row(d, ws, Hm, Wm, blockIdx.y, mcu, map.k, r);
    }
}

}  // namespace

extern "C" {

size_t salve_bev_jpeg_roundtrip_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!jpeg_shape_ok("salve_bev_jpeg_roundtrip_workspace_bytes", n, h, w)) return 0;
    return jpeg_planes_bytes(n, JpegGeometry(h, w));
}

int salve_bev_jpeg_roundtrip(const uint32_t* bev_in, uint32_t* bev_out, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, void* ws,
                             size_t ws_bytes, void* stream) {
    const char* me = "salve_bev_jpeg_roundtrip";
    if (!bev_in || !bev_out || !qtab || !ws) { jpeg_refuse(me, "null pointer"); return SALVE_ERR_BAD_ARG; }
    if (!jpeg_shape_ok(me, n, h, w)) return SALVE_ERR_BAD_ARG;
    if (((uintptr_t)bev_in | (uintptr_t)bev_out) & 3) { jpeg_refuse(me, "the images must be 4-byte aligned"); return SALVE_ERR_BAD_ARG; }
    QTables qt;
    const JpegGeometry g(h, w);
    if (!jpeg_load_qtables(me, qtab, &qt) || !jpeg_workspace_ok(me, ws, ws_bytes, jpeg_planes_bytes(n, g))) return SALVE_ERR_BAD_ARG;
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)((g.mcus_w + MCUS - 1) / MCUS), (unsigned)g.mcus_h, (unsigned)n), dim3(JPEG_THREADS), 0,
                       (hipStream_t)stream, bev_in, (uint8_t*)ws, (int)h, (int)w, g.Hm, g.Wm, qt);
    SALVE_HIP_CHECK(hipGetLastError());
    SALVE_HIP_CHECK(jpeg_launch_pixels((const uint8_t*)ws, bev_out, n, h, w, g, (hipStream_t)stream));
    return SALVE_OK;
}

}  // extern "C"
