// jpeg_decode.hip -- the tile data set's JPEG files decoded on gfx950 (MI355X), in whole batches, bit for bit what Pillow's decoder
// (libjpeg: slow-integer inverse DCT, fancy upsampling) gives (opt-in: BevRasteriser.jpeg_decode, train_files.TileFileSource).
//
// The reference trains and evaluates from rendered tiles on disk and decodes every file with Pillow (zind_data.py:306-315).  One call
// here decodes n images of one size that share their tables: baseline, 8-bit, three components, 4:2:0, one interleaved scan, no
// restart interval.  The host has parsed the headers (salve_amd/jpeg.py: parse_file); the device gets the entropy-coded scans as they
// stand in the files.  Three launches, asynchronous on the caller's stream:
//   jpeg_entropy_kernel   ONE WAVEFRONT PER IMAGE (Huffman decoding is serial in the bit position): jpeg_entropy.h -- the lanes stage
//                         the scan into LDS in coalesced runs and expand the look-ahead tables there; the symbol loop runs on
//                         wave-uniform values; every block leaves as one 128-byte store of int16 coefficients, natural order,
//                         MCU-interleaved, into the workspace.  A batch's images are resident together: the grid is n workgroups of 64.
//   jpeg_idct_kernel      eight threads per block, 32 blocks per workgroup: dequantise, the column pass (jpeg_inverse.h: idct_1d), then
//                         jpeg_store_decoded_row, the function salve_bev_jpeg_roundtrip ends with: the row pass, the range limit, one
//                         8-byte store per block row into the planes.  The luma blocks of an edge MCU that lie outside the image land
//                         in the planes' margin, which nothing reads.
//   jpeg_pixels_kernel    jpeg_inverse.h (jpeg_launch_pixels): upsampling, colour conversion, the pixels.
// The `_sampled` entries take the MCU's block pattern as an argument (SALVE_JPEG_SAMPLING_*: 4:2:0, 4:2:2, 4:4:4, greyscale).  It is a
// template argument of every kernel here (JeSampling for the entropy stages, JpegPlanes for the planes): each sampling has its own
// instantiations, and no lane branches on it.  The entries without it are the `_sampled` ones at 4:2:0.
// `stages` selects the first launch alone, the other two alone (on the coefficients in the workspace) or, as every product path does,
// all three: a measurement can put events between the entropy stage and the inverse stage.
// A malformed scan sets bits in its image's status word (include/salve_hip.h: SALVE_JPEG_*), keeps what it had decoded, has zeros
// for the rest and still goes through the inverse stages; the other images do not notice.  Integer arithmetic only, plain stores only,
// one writer per output: the same input gives the same bits.  Every offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/salve_hip.h"
#include "jpeg_entropy.h"
#include "jpeg_entropy_lanes.h"
#include "jpeg_inverse.h"
#include "salve_common.h"

static_assert(JE_BAD_CODE == SALVE_JPEG_BAD_CODE && JE_COEF_OVERRUN == SALVE_JPEG_COEF_OVERRUN && JE_TRUNCATED == SALVE_JPEG_TRUNCATED &&
                  JE_DC_RANGE == SALVE_JPEG_DC_RANGE && JE_LEFTOVER == SALVE_JPEG_LEFTOVER && JE_MARKER == SALVE_JPEG_MARKER &&
                  JE_BAD_SLOT == SALVE_JPEG_BAD_SLOT,
              "jpeg_entropy.h and salve_hip.h name the same status bits");
static_assert(JE_SAMPLING_420 == SALVE_JPEG_SAMPLING_420 && JE_SAMPLING_422 == SALVE_JPEG_SAMPLING_422 && JE_SAMPLING_444 == SALVE_JPEG_SAMPLING_444 &&
                  JE_SAMPLING_GREY == SALVE_JPEG_SAMPLING_GREY,
              "jpeg_entropy.h and salve_hip.h name the same samplings");
static_assert(sizeof(JlSegment) == sizeof(salve_jpeg_segment_t) && sizeof(JlSegment) == 24 && JE_SUBSEQ % 4 == 0 && JE_SUBSEQ >= 4,
              "jpeg_entropy_lanes.h and salve_hip.h name the same segment");

namespace {

constexpr int IDCT_BLOCKS = JPEG_THREADS / 8;   // blocks of a workgroup of jpeg_idct_kernel
constexpr int IDCT_STRIDE = 65;                 // ints per block in LDS (odd: the blocks' column passes fall on different banks)

// grid (images), 64 threads
template <int S>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ scans, const int64_t* __restrict__ scan_offset,
                                                          const int32_t* __restrict__ scan_bytes, uint64_t scans_size, int mcus, JeTables tab,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ image_status) {
    __shared__ JeShared sh;
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    je_prepare(sh, tab, lane, 64);
    int64_t off = scan_offset[i];
    int32_t nbytes = scan_bytes[i];
    uint32_t status = 0;
    if (off < 0 || nbytes < 0 || (uint64_t)off + (uint64_t)nbytes + SALVE_JPEG_SCAN_PADDING > scans_size) {   // not inside the buffer: decode nothing
        status = JE_BAD_SLOT;
        off = 0;
        nbytes = 0;
    }
    const uint32_t decoded = je_decode_image<S>(sh, scans + off, nbytes, mcus, coef + i * mcus * JeSampling<S>::coefs, lane, 64);   // (a bad slot: all coefficients zero)
    if (lane == 0) image_status[i] = (int32_t)(status ? status : decoded);
}

// The lane-parallel entropy stage (jpeg_entropy_lanes.h): grid (segments), JL_LANES threads; one lane per JE_SUBSEQ bytes of the segment's
// stuffed stream.  coef and image_status are ZERO on entry (salve_bev_jpeg_decode_lanes clears them on the stream).  A segment's status
// bits are OR-ed into its image's word: bit-wise OR into a zeroed word does not depend on the order of the segments.
template <int S>
__global__ __launch_bounds__(JL_LANES) void jpeg_entropy_lanes_kernel(const uint8_t* __restrict__ scans, const JlSegment* __restrict__ segments, uint64_t scans_size,
                                                                      int n, int mcus, JeTables tab, int16_t* __restrict__ coef, int32_t* __restrict__ image_status) {
    __shared__ JlShared sh;
    const JlSegment seg = segments[blockIdx.x];
    if (seg.image < 0 || seg.image >= n) return;   // (whole workgroup) no image to report to: the wrapper refuses such a table
    if (!jl_segment_inside(seg, scans_size, mcus)) {   // not inside the buffer or the image: decode nothing
        if (threadIdx.x == 0) atomicOr(&image_status[seg.image], (int)JE_BAD_SLOT);
        return;
    }
    je_prepare_tables(sh, tab, (int)threadIdx.x, JL_LANES);
    const uint32_t status = jl_decode_segment<S>(sh, scans + seg.offset, seg.bytes, seg.mcu_count, coef + ((int64_t)seg.image * mcus + seg.first_mcu) * JeSampling<S>::coefs, nullptr);
    if (threadIdx.x == 0 && status) atomicOr(&image_status[seg.image], (int)status);
}

// grid (blocks of an image / 32, 1, images)
template <int S>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ ws, int mcus_w, int nblocks, int Hm,
                                                                 int Wm, QTables qt) {
    __shared__ int s_d[IDCT_BLOCKS * IDCT_STRIDE];
    __shared__ int s_q[2][64];
    const int tid = threadIdx.x;
    if (tid < 128) s_q[tid >> 6][tid & 63] = qt.q[tid >> 6][tid & 63];
    __syncthreads();
    const int b = tid >> 3, r = tid & 7;
    const int g = blockIdx.x * IDCT_BLOCKS + b;   // block of the image, in the scan's order
    const bool working = g < nblocks;
    const int mcu = g / JeSampling<S>::blocks, k = g - JeSampling<S>::blocks * mcu;
    const int* q = s_q[je_comp<S>(k) ? 1 : 0];
    int* base = s_d + b * IDCT_STRIDE;
    int d[8];
    if (working) {   // dequantise, inverse pass 1 on column r
        const int16_t* src = coef + ((int64_t)blockIdx.z * nblocks + g) * 64;
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = (int)src[j * 8 + r] * q[j * 8 + r];
        idct_1d(d, CONST_BITS - PASS1_BITS);
#pragma unroll
        for (int j = 0; j < 8; j++) base[j * 8 + r] = d[j];
    }
    __syncthreads();
    if (working) {   // inverse pass 2 on row r
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = base[r * 8 + j];
        const int my = mcu / mcus_w, mx = mcu - my * mcus_w;
        jpeg_store_decoded_row<S>(d, ws, Hm, Wm, my, mx, k, r);
    }
}

}  // namespace

// The launches of one call at sampling S: the planes, then the coefficients, in the workspace.
template <int S>
static int jpeg_decode_launch(const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes, const salve_jpeg_segment_t* segments,
                              int32_t n_segments, int32_t n, int32_t h, int32_t w, const QTables& qt, const JeTables& tab, uint32_t* bev_out, int32_t* image_status,
                              void* ws, uint32_t stages, hipStream_t stream) {
    const JpegGeometry g(h, w, S);
    const int mcus = (int)g.mcus(), nblocks = JeSampling<S>::blocks * mcus;
    uint8_t* planes = (uint8_t*)ws;
    int16_t* coef = (int16_t*)(planes + (size_t)n * (size_t)JpegPlanes<S>::image_bytes(g.Hm, g.Wm));
    if ((stages & SALVE_JPEG_STAGE_ENTROPY) && segments) {   // the lanes write the non-zero coefficients and OR the status bits: both zero first
        SALVE_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)n * mcus * JeSampling<S>::coefs * sizeof(int16_t), stream));
        SALVE_HIP_CHECK(hipMemsetAsync(image_status, 0, (size_t)n * sizeof(int32_t), stream));
        hipLaunchKernelGGL(jpeg_entropy_lanes_kernel<S>, dim3((unsigned)n_segments), dim3(JL_LANES), 0, stream, scans, (const JlSegment*)segments,
                           (uint64_t)scans_size, n, mcus, tab, coef, image_status);
        SALVE_HIP_CHECK(hipGetLastError());
    } else if (stages & SALVE_JPEG_STAGE_ENTROPY) {
        hipLaunchKernelGGL(jpeg_entropy_kernel<S>, dim3((unsigned)n), dim3(64), 0, stream, scans, scan_offset, scan_bytes, (uint64_t)scans_size, mcus, tab, coef,
                           image_status);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    if (stages & SALVE_JPEG_STAGE_INVERSE) {   // from the coefficients the entropy stage left in this workspace
        hipLaunchKernelGGL(jpeg_idct_kernel<S>, dim3((unsigned)((nblocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), 1, (unsigned)n), dim3(JPEG_THREADS), 0, stream,
                           (const int16_t*)coef, planes, g.mcus_w, nblocks, g.Hm, g.Wm, qt);
        SALVE_HIP_CHECK(hipGetLastError());
        if constexpr (S == JE_SAMPLING_420) {
            SALVE_HIP_CHECK(jpeg_launch_pixels(planes, bev_out, n, h, w, g, stream));
        } else {
            SALVE_HIP_CHECK(jpeg_launch_pixels_sampled<S>(planes, bev_out, n, h, w, g, stream));
        }
    }
    return SALVE_OK;
}

static bool jpeg_sampling_ok(const char* me, int32_t sampling) {
    if (sampling >= SALVE_JPEG_SAMPLING_420 && sampling <= SALVE_JPEG_SAMPLING_GREY) return true;
    return jpeg_refuse(me, "sampling must be one of SALVE_JPEG_SAMPLING_420, _422, _444, _GREY");
}

// The planes and the coefficients of n images: 1.5 / 2 / 3 / 1 bytes per MCU-rounded pixel and 128 bytes per block.
static size_t jpeg_decode_need(int32_t n, int32_t h, int32_t w, int32_t sampling) {
    const JpegGeometry g(h, w, sampling);
    const size_t pixels = (size_t)g.Hm * g.Wm;
    const size_t planes = sampling == SALVE_JPEG_SAMPLING_420 ? pixels + pixels / 2 : sampling == SALVE_JPEG_SAMPLING_422 ? 2 * pixels
                          : sampling == SALVE_JPEG_SAMPLING_444 ? 3 * pixels : pixels;
    const size_t blocks = sampling == SALVE_JPEG_SAMPLING_420 ? 6 : sampling == SALVE_JPEG_SAMPLING_422 ? 4 : sampling == SALVE_JPEG_SAMPLING_444 ? 3 : 1;
    return (size_t)n * (planes + g.mcus() * blocks * 64 * sizeof(int16_t));
}

// The entries differ in their entropy stage alone: segments == nullptr is salve_bev_jpeg_decode(_sampled).
static int jpeg_decode_any(const char* me, const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes,
                           const salve_jpeg_segment_t* segments, int32_t n_segments, int32_t n, int32_t h, int32_t w, int32_t sampling, const uint16_t* qtab,
                           const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status, void* ws, size_t ws_bytes, uint32_t stages, void* stream) {
    const bool null = !scans || !qtab || !huffman || !bev_out || !image_status || !ws;
    if (null) { jpeg_refuse(me, "null pointer"); return SALVE_ERR_BAD_ARG; }
    if (stages < SALVE_JPEG_STAGE_ENTROPY || stages > SALVE_JPEG_STAGES_ALL) { jpeg_refuse(me, "stages must be SALVE_JPEG_STAGE_ENTROPY, SALVE_JPEG_STAGE_INVERSE or both"); return SALVE_ERR_BAD_ARG; }
    if (!jpeg_shape_ok(me, n, h, w) || !jpeg_sampling_ok(me, sampling)) return SALVE_ERR_BAD_ARG;
    if (scans_size < SALVE_JPEG_SCAN_PADDING) { jpeg_refuse(me, "the scan buffer is smaller than its padding"); return SALVE_ERR_BAD_ARG; }
    if (((uintptr_t)scan_offset & 7) || (((uintptr_t)scan_bytes | (uintptr_t)bev_out | (uintptr_t)image_status) & 3)) {
        jpeg_refuse(me, "scan_offset must be 8-byte, scan_bytes, bev_out and image_status 4-byte aligned");
        return SALVE_ERR_BAD_ARG;
    }
    QTables qt;
    if (!jpeg_load_qtables(me, qtab, &qt)) return SALVE_ERR_BAD_ARG;
    JeTables tab;
    if (!je_make_tables(huffman, &tab)) { jpeg_refuse(me, "a Huffman table's BITS over-subscribe the code space or sum past 256"); return SALVE_ERR_BAD_ARG; }
    if (!jpeg_workspace_ok(me, ws, ws_bytes, jpeg_decode_need(n, h, w, sampling))) return SALVE_ERR_BAD_ARG;
#define JPEG_DECODE_AT(S) \
    jpeg_decode_launch<S>(scans, scans_size, scan_offset, scan_bytes, segments, n_segments, n, h, w, qt, tab, bev_out, image_status, ws, stages, (hipStream_t)stream)
    switch (sampling) {
        case SALVE_JPEG_SAMPLING_422: return JPEG_DECODE_AT(JE_SAMPLING_422);
        case SALVE_JPEG_SAMPLING_444: return JPEG_DECODE_AT(JE_SAMPLING_444);
        case SALVE_JPEG_SAMPLING_GREY: return JPEG_DECODE_AT(JE_SAMPLING_GREY);
        default: return JPEG_DECODE_AT(JE_SAMPLING_420);
    }
#undef JPEG_DECODE_AT
}

static bool jpeg_segments_ok(const char* me, const salve_jpeg_segment_t* segments, int32_t n_segments, int32_t n) {
    if (!segments) return jpeg_refuse(me, "null pointer");
    if (((uintptr_t)segments & 7)) return jpeg_refuse(me, "segments must be 8-byte aligned");
    if (n_segments < n || n_segments > SALVE_JPEG_MAX_SEGMENTS) return jpeg_refuse(me, "n_segments must lie in [n, 2^24]");
    return true;
}

extern "C" {

size_t salve_bev_jpeg_decode_sampled_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t sampling) {
    const char* me = "salve_bev_jpeg_decode_sampled_workspace_bytes";
    if (!jpeg_shape_ok(me, n, h, w) || !jpeg_sampling_ok(me, sampling)) return 0;
    return jpeg_decode_need(n, h, w, sampling);
}

size_t salve_bev_jpeg_decode_lanes_sampled_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_segments, int32_t sampling) {
    const char* me = "salve_bev_jpeg_decode_lanes_sampled_workspace_bytes";
    if (!jpeg_shape_ok(me, n, h, w) || !jpeg_sampling_ok(me, sampling)) return 0;
    if (n_segments < n || n_segments > SALVE_JPEG_MAX_SEGMENTS) { jpeg_refuse(me, "n_segments must lie in [n, 2^24]"); return 0; }
    return jpeg_decode_need(n, h, w, sampling);   // the planes and the coefficients; the lanes keep their state in LDS
}

size_t salve_bev_jpeg_decode_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!jpeg_shape_ok("salve_bev_jpeg_decode_workspace_bytes", n, h, w)) return 0;
    return jpeg_decode_need(n, h, w, SALVE_JPEG_SAMPLING_420);
}

size_t salve_bev_jpeg_decode_lanes_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_segments) {
    const char* me = "salve_bev_jpeg_decode_lanes_workspace_bytes";
    if (!jpeg_shape_ok(me, n, h, w)) return 0;
    if (n_segments < n || n_segments > SALVE_JPEG_MAX_SEGMENTS) { jpeg_refuse(me, "n_segments must lie in [n, 2^24]"); return 0; }
    return jpeg_decode_need(n, h, w, SALVE_JPEG_SAMPLING_420);
}

int32_t salve_bev_jpeg_subseq_bytes(void) { return JE_SUBSEQ; }

int salve_bev_jpeg_decode_lanes_sampled(const uint8_t* scans, size_t scans_size, const salve_jpeg_segment_t* segments, int32_t n_segments, int32_t n, int32_t h,
                                        int32_t w, int32_t sampling, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status,
                                        void* ws, size_t ws_bytes, uint32_t stages, void* stream) {
    const char* me = "salve_bev_jpeg_decode_lanes_sampled";
    if (!jpeg_segments_ok(me, segments, n_segments, n)) return SALVE_ERR_BAD_ARG;
    return jpeg_decode_any(me, scans, scans_size, nullptr, nullptr, segments, n_segments, n, h, w, sampling, qtab, huffman, bev_out, image_status, ws, ws_bytes,
                           stages, stream);
}

int salve_bev_jpeg_decode_sampled(const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes, int32_t n, int32_t h, int32_t w,
                                  int32_t sampling, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status, void* ws,
                                  size_t ws_bytes, uint32_t stages, void* stream) {
    const char* me = "salve_bev_jpeg_decode_sampled";
    if (!scan_offset || !scan_bytes) { jpeg_refuse(me, "null pointer"); return SALVE_ERR_BAD_ARG; }
    return jpeg_decode_any(me, scans, scans_size, scan_offset, scan_bytes, nullptr, 0, n, h, w, sampling, qtab, huffman, bev_out, image_status, ws, ws_bytes, stages,
                           stream);
}

int salve_bev_jpeg_decode_lanes(const uint8_t* scans, size_t scans_size, const salve_jpeg_segment_t* segments, int32_t n_segments, int32_t n, int32_t h,
                                int32_t w, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status, void* ws,
                                size_t ws_bytes, uint32_t stages, void* stream) {
    const char* me = "salve_bev_jpeg_decode_lanes";
    if (!jpeg_segments_ok(me, segments, n_segments, n)) return SALVE_ERR_BAD_ARG;
    return jpeg_decode_any(me, scans, scans_size, nullptr, nullptr, segments, n_segments, n, h, w, SALVE_JPEG_SAMPLING_420, qtab, huffman, bev_out, image_status, ws,
                           ws_bytes, stages, stream);
}

int salve_bev_jpeg_decode(const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes, int32_t n, int32_t h, int32_t w,
                          const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status, void* ws, size_t ws_bytes,
                          uint32_t stages, void* stream) {
    const char* me = "salve_bev_jpeg_decode";
    if (!scan_offset || !scan_bytes) { jpeg_refuse(me, "null pointer"); return SALVE_ERR_BAD_ARG; }
    return jpeg_decode_any(me, scans, scans_size, scan_offset, scan_bytes, nullptr, 0, n, h, w, SALVE_JPEG_SAMPLING_420, qtab, huffman, bev_out, image_status, ws,
                           ws_bytes, stages, stream);
}

}  // extern "C"
