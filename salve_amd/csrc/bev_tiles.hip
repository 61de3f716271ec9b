// bev_tiles.hip -- image -> tensor for gfx950 (MI355X): everything that turns a rendered BEV image (uint32 0x00BBGGRR) or a panorama
// into what the next stage reads.  Compile with -ffp-contract=off.
//
// The reference does this on the CPU, per image, with OpenCV and torchvision-style transforms: Resize (cv2 INTER_LINEAR on uint8:
// 11-bit fixed-point taps) -> Crop -> flips -> ToTensor -> Normalize (train_utils.py:63-159, transform.py:105-123, 177-202, 256-272,
// 386-420), the channel concatenation of models/early_fusion.py:52-60, and cv2.resize of every panorama before back-projection
// (bev_rendering_utils.py:370-375).  Here the taps {src0, src1, w0, w1} per resized row and column and the table (v - mean) / std
// come from the host (salve_amd/rasteriser.py), and the arithmetic is bev_tile_math.h's: the integers are cv2's, bit for bit.
// Kernels, one thread per output pixel, 256 threads per workgroup:
//
//   bev_tile_kernel         salve_bev_tiles: the test transform of one image per job -- fp32 NCHW, fp16 NHWC, or the resized and cropped
//                           bytes themselves (SALVE_TILE_U8X4)
//   bev_tile_aug_kernel     salve_bev_tiles_aug: the train transform (crop at the job's offset, then the flips), fp32 NCHW
//   bev_tile_pair_kernel    salve_bev_tile_pairs: both tiles of an early-fusion pair, six fp16 channels in whole-pixel stores
//   bev_train_tile_kernel   salve_bev_train_tiles: the train transform of a whole batch as NHWC [batch, crop, crop, CP], fp32 or bf16
//   bev_jitter_grey_sum_kernel   salve_bev_train_tiles_jitter: ColorJitter's contrast needs the mean grey level of the whole resized image;
//                           this launch sums it, bev_train_tile_kernel<.., JITTER> then runs the colour chain in front of the table lookup
//   bev_export_kernel       salve_bev_export_u8: uint32 -> uint8 [.., 3], the array render_bev_image returns
//   resize_rgb_kernel       salve_resize_rgb_u8: the panorama ingest's cv2.resize on uint8 RGB
//
// (The densify kernel's phase H in bev_render.hip is bev_tile_pair_kernel fused behind a render; it shares the header, not this file.)
// Bounds: all are bandwidth kernels -- a gather of four source pixels per output pixel out of images that stay in the L2, and the
// output written once; the workgroups of one pair or sample are placed on one XCD so that its images go through one L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/salve_hip.h"
#include "bev_tile_math.h"
#include "salve_common.h"

namespace {

__global__ __launch_bounds__(256) void bev_tile_kernel(const uint32_t* __restrict__ bev, int W,
                                                       const salve_tile_job_t* __restrict__ jobs,
                                                       const int32_t* __restrict__ coef_y,
                                                       const int32_t* __restrict__ coef_x, int resize, int crop,
                                                       const float* __restrict__ lut, void* __restrict__ out, int fmt,
                                                       int out_c) {
    const salve_tile_job_t job = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= crop * crop) return;
    const int i = idx / crop, j = idx % crop;
    const int off = (resize - crop) / 2;
    const int4 cy = reinterpret_cast<const int4*>(coef_y)[i + off];
    const int4 cx = reinterpret_cast<const int4*>(coef_x)[j + off];
    const uint32_t* img = bev + job.bev_offset;
    const uint32_t p00 = img[(size_t)cy.x * W + cx.x], p01 = img[(size_t)cy.x * W + cx.y];
    const uint32_t p10 = img[(size_t)cy.y * W + cx.x], p11 = img[(size_t)cy.y * W + cx.y];
    float v[3];
    int rq[3];   // tile_pixel, keeping the resized bytes for SALVE_TILE_U8X4
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        rq[ch] = bilinear_u8((p00 >> (8 * ch)) & 255, (p01 >> (8 * ch)) & 255, (p10 >> (8 * ch)) & 255, (p11 >> (8 * ch)) & 255, cy, cx);
        v[ch] = lut[ch * 256 + rq[ch]];
    }
    if (fmt == SALVE_TILE_U8X4) {   // the resized + cropped image itself (before ToTensor / Normalize): 0x00BBGGRR, one image per slot
        reinterpret_cast<uint32_t*>(out)[(size_t)job.slot * crop * crop + idx] = (uint32_t)rq[0] | ((uint32_t)rq[1] << 8) | ((uint32_t)rq[2] << 16);
    } else if (fmt == SALVE_TILE_F32_NCHW) {
        float* o = reinterpret_cast<float*>(out) + ((size_t)job.slot * out_c + job.chan) * crop * crop + idx;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[(size_t)ch * crop * crop] = v[ch];
    } else {
        uint16_t* o = reinterpret_cast<uint16_t*>(out) + ((size_t)job.slot * crop * crop + idx) * out_c + job.chan;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[ch] = f32_to_f16(v[ch]);
    }
}

// salve_bev_tiles_aug: the train transform's tile -- bev_tile_kernel's F32_NCHW arithmetic (tile_pixel: the same taps, the same LUT) at
// the job's crop offset, with the output pixel (i, j) taken from the crop's (crop-1-i if VFLIP, crop-1-j if HFLIP): the flips come after
// the crop, as in the reference's Compose.  Offsets are clamped into [0, resize - crop] so that no tap outside the tables is read.
__global__ __launch_bounds__(256) void bev_tile_aug_kernel(const uint32_t* __restrict__ bev, int W, const salve_tile_job_t* __restrict__ jobs,
                                                           const salve_tile_aug_t* __restrict__ aug, const int32_t* __restrict__ coef_y,
                                                           const int32_t* __restrict__ coef_x, int resize, int crop, const float* __restrict__ lut,
                                                           float* __restrict__ out, int out_c) {
    const salve_tile_job_t job = jobs[blockIdx.y];
    const salve_tile_aug_t a = aug[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= crop * crop) return;
    const int i = idx / crop, j = idx % crop;
    const int oy = min(max(a.crop_y, 0), resize - crop), ox = min(max(a.crop_x, 0), resize - crop);
    const int si = (a.flags & SALVE_TILE_VFLIP) ? crop - 1 - i : i, sj = (a.flags & SALVE_TILE_HFLIP) ? crop - 1 - j : j;
    const int4 cy = reinterpret_cast<const int4*>(coef_y)[si + oy];
    const int4 cx = reinterpret_cast<const int4*>(coef_x)[sj + ox];
    float v[3];
    tile_pixel(bev + job.bev_offset, W, cy, cx, lut, v);
    float* o = out + ((size_t)job.slot * out_c + job.chan) * crop * crop + idx;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[(size_t)ch * crop * crop] = v[ch];
}

// Both tiles of an early-fusion pair per thread, six channels (plus the sample's zero padding behind its last group) in
// whole-pixel stores: see salve_bev_tile_pairs in salve_hip.h.
__global__ __launch_bounds__(256) void bev_tile_pair_kernel(const uint32_t* __restrict__ bev_a, const uint32_t* __restrict__ bev_b, int W,
                                                            const salve_tile_job_t* __restrict__ jobs_a, const salve_tile_job_t* __restrict__ jobs_b,
                                                            const int32_t* __restrict__ coef_y, const int32_t* __restrict__ coef_x, int resize,
                                                            int crop, const float* __restrict__ lut, uint16_t* __restrict__ out, int out_c,
                                                            int n_pairs, int n_blocks, int xcd_group, int b_pretiled) {
    // (the workgroups of one pair read the same two BEV images: same id % 8 = same XCD = one L2 -- as in bev_splat_kernel)
    int job, blk;
    if (xcd_group) {
        const int id = blockIdx.x, s_ = id >> 3;
        job = (s_ / n_blocks) * 8 + (id & 7);
        blk = s_ % n_blocks;
        if (job >= n_pairs) return;
    } else {
        job = blockIdx.x / n_blocks;
        blk = blockIdx.x % n_blocks;
    }
    const salve_tile_job_t ja = jobs_a[job], jb = jobs_b[job];
    const int idx = blk * 256 + threadIdx.x;
    if (idx >= crop * crop) return;
    const int i = idx / crop, j = idx % crop;
    const int off = (resize - crop) / 2;
    const int4 cy = reinterpret_cast<const int4*>(coef_y)[i + off];
    const int4 cx = reinterpret_cast<const int4*>(coef_x)[j + off];
    float va[3], vb[3];
    tile_pixel(bev_a + ja.bev_offset, W, cy, cx, lut, va);
    if (b_pretiled) {   // image b was resized and cropped before (SALVE_TILE_U8X4, once per panorama): ToTensor + Normalize only
        const uint32_t q = bev_b[jb.bev_offset + idx];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) vb[ch] = lut[ch * 256 + ((q >> (8 * ch)) & 255u)];
    } else {
        tile_pixel(bev_b + jb.bev_offset, W, cy, cx, lut, vb);
    }
    const bool a_first = ja.chan < jb.chan;
    const int c0 = a_first ? ja.chan : jb.chan;   // first of the group's six channels (a multiple of 6)
    const float* lo = a_first ? va : vb;
    const float* hi = a_first ? vb : va;
    const uint32_t w0 = (uint32_t)f32_to_f16(lo[0]) | ((uint32_t)f32_to_f16(lo[1]) << 16);   // the six halves, two per word
    const uint32_t w1 = (uint32_t)f32_to_f16(lo[2]) | ((uint32_t)f32_to_f16(hi[0]) << 16);
    const uint32_t w2 = (uint32_t)f32_to_f16(hi[1]) | ((uint32_t)f32_to_f16(hi[2]) << 16);
    store_pair_pixel(out + ((size_t)ja.slot * crop * crop + idx) * out_c, w0, w1, w2, c0, out_c);
}

// salve_bev_train_tiles: the TRAIN transform of a whole batch in the training model's input layout -- NHWC [batch, crop, crop, CP],
// fp32 or bf16, the channels behind the last image written as zero.  The workgroups of sample `smp` read its 2 * per_sample images (posed
// renders from bev_a, identity renders from bev_b) with tile_pixel -- bev_tile_aug_kernel's arithmetic at the sample's ONE draw -- and a
// thread stores all CP channels of its pixel with 16-byte stores.  The job tables live in device memory, so their ranges are checked HERE,
// before any address is formed: a job outside its sample, its channels or its image array raises SALVE_STATUS_BAD_TILE_JOB and the
// sample is left unwritten.
struct TrainTiles {
    const uint32_t* bev_a;
    const uint32_t* bev_b;
    const salve_tile_job_t* jobs_a;   // [batch][per_sample]
    const salve_tile_job_t* jobs_b;   // [batch][per_sample]
    const salve_tile_aug_t* aug;      // [batch]
    const int32_t* coef_y;
    const int32_t* coef_x;
    const float* lut;
    void* out;
    int32_t* status;
    long long px_a, px_b;             // uint32 elements of bev_a / bev_b
    int W, HW, resize, crop, batch, per_sample, n_blocks;
    const salve_tile_jitter_t* jitter;   // [batch][2 * per_sample], and the grey sums beside it: salve_bev_train_tiles_jitter only
    uint32_t* grey_sum;
};

// The jobs of sample smp into ja / jb (k >= per_sample: naming no channel group); true if one of them is outside its sample, the channels
// [0, chan_end) or its image array.
template <int MAX_S>
__device__ __forceinline__ bool train_jobs_bad(const TrainTiles& t, int smp, int chan_end, salve_tile_job_t ja[MAX_S], salve_tile_job_t jb[MAX_S]) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < MAX_S; k++) {
        if (k < t.per_sample) {
            ja[k] = t.jobs_a[(size_t)smp * t.per_sample + k];
            jb[k] = t.jobs_b[(size_t)smp * t.per_sample + k];
            bad |= ja[k].slot != smp || ja[k].chan < 0 || ja[k].chan % 3 != 0 || ja[k].chan + 3 > chan_end || ja[k].bev_offset < 0 || ja[k].bev_offset + t.HW > t.px_a;
            bad |= jb[k].slot != smp || jb[k].chan < 0 || jb[k].chan % 3 != 0 || jb[k].chan + 3 > chan_end || jb[k].bev_offset < 0 || jb[k].bev_offset + t.HW > t.px_b;
        } else {
            ja[k].chan = jb[k].chan = -1;   // names no channel group
            ja[k].bev_offset = jb[k].bev_offset = 0;
        }
    }
    return bad;
}

// The image whose job names channel group g of the sample, or null.
template <int MAX_S>
__device__ __forceinline__ const uint32_t* train_group_image(const TrainTiles& t, const salve_tile_job_t ja[MAX_S], const salve_tile_job_t jb[MAX_S], int g) {
    const uint32_t* img = nullptr;
#pragma unroll
    for (int k = 0; k < MAX_S; k++) {
        if (ja[k].chan == 3 * g) img = t.bev_a + ja[k].bev_offset;
        if (jb[k].chan == 3 * g) img = t.bev_b + jb[k].bev_offset;
    }
    return img;
}

// ---- salve_bev_train_tiles_jitter: ColorJitter on the resized bytes (bev_tile_math.h), per image by its record.
__device__ __forceinline__ bool jitter_record_bad(const salve_tile_jitter_t& r) {
    int seen = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) seen |= r.order[k] < 4 ? 1 << r.order[k] : 16;
    const float f[7] = {r.brightness, r.contrast, r.saturation, r.hue, r.brightness_c, r.contrast_c, r.saturation_c};
    bool bad = seen != 15 || (r.mask & ~15) != 0;
#pragma unroll
    for (int k = 0; k < 7; k++) bad |= !(fabsf(f[k]) <= 3.402823466e38f);   // NaN and the infinities
    return bad;
}

// The record's enabled operations on one pixel, in its order.  UNTIL_CONTRAST: only the ones in front of contrast (what the grey sum is
// taken over; `mean` is unused).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_pixel(const salve_tile_jitter_t& r, int q[3], float mean) {
    for (int k = 0; k < 4; k++) {
        const int op = r.order[k];
        if (UNTIL_CONTRAST && op == SALVE_JITTER_CONTRAST) return;
        if (!((r.mask >> op) & 1)) continue;
        if (op == SALVE_JITTER_BRIGHTNESS) jitter_blend(q, 0.0f, r.brightness, r.brightness_c);
        else if (op == SALVE_JITTER_CONTRAST) jitter_blend(q, mean, r.contrast, r.contrast_c);
        else if (op == SALVE_JITTER_SATURATION) jitter_blend(q, (float)jitter_grey(q), r.saturation, r.saturation_c);
        else jitter_hue(q, r.hue);
    }
}

// First launch: grey_sum[smp][g] += grey of every pixel of the WHOLE resized image of channel group g of sample smp, as the operations in
// front of contrast leave it -- GREY_PIXELS resized pixels per thread, summed over the workgroup, one integer atomic add per workgroup
// (integer adds commute: the sum does not depend on their order).  The workgroups of one image on one XCD, as the second launch's: image
// (id >> 3) / n_blocks * 8 + (id & 7).  A sample with a bad job or record is skipped here and reported by the second launch; so is an
// image whose contrast is disabled.
constexpr int GREY_PIXELS = 8;

__global__ __launch_bounds__(256) void bev_jitter_grey_sum_kernel(const TrainTiles t, int n_blocks) {
    const int G = 2 * t.per_sample, id = blockIdx.x, s_ = id >> 3;
    const int image = (s_ / n_blocks) * 8 + (id & 7), blk = s_ % n_blocks;
    if (image >= t.batch * G) return;
    const int smp = image / G, g = image % G;
    salve_tile_job_t ja[3], jb[3];
    bool bad = train_jobs_bad<3>(t, smp, 3 * G, ja, jb);
    for (int k = 0; k < G; k++) bad |= jitter_record_bad(t.jitter[(size_t)smp * G + k]);
    const uint32_t* img = train_group_image<3>(t, ja, jb, g);
    const salve_tile_jitter_t r = t.jitter[(size_t)image];
    if (bad || !img || !((r.mask >> SALVE_JITTER_CONTRAST) & 1)) return;   // (workgroup-uniform)
    uint32_t grey = 0;
    for (int p = 0; p < GREY_PIXELS; p++) {
        const int idx = (blk * GREY_PIXELS + p) * 256 + threadIdx.x;
        if (idx >= t.resize * t.resize) break;
        const int4 cy = reinterpret_cast<const int4*>(t.coef_y)[idx / t.resize];
        const int4 cx = reinterpret_cast<const int4*>(t.coef_x)[idx % t.resize];
        int q[3];
        tile_bytes(img, t.W, cy, cx, q);
        jitter_pixel<true>(r, q, 0.0f);
        grey += (uint32_t)jitter_grey(q);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) grey += __shfl_down(grey, o, 64);
    __shared__ uint32_t part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = grey;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&t.grey_sum[(size_t)image], part[0] + part[1] + part[2] + part[3]);
}

template <int CP, bool BF16, bool JITTER>
__global__ __launch_bounds__(256) void bev_train_tile_kernel(const TrainTiles t) {
    typedef __attribute__((__ext_vector_type__(8))) float f32x8;
    typedef __attribute__((__ext_vector_type__(8))) __bf16 bf16x8;
    constexpr int MAX_S = CP / 6, GROUPS = CP / 3;
    // (the workgroups of one sample read the same images: same id % 8 = same XCD = one L2 -- as in bev_tile_pair_kernel)
    const int id = blockIdx.x, s_ = id >> 3;
    const int smp = (s_ / t.n_blocks) * 8 + (id & 7), blk = s_ % t.n_blocks;
    if (smp >= t.batch) return;
    const salve_tile_aug_t a = t.aug[smp];
    salve_tile_job_t ja[MAX_S], jb[MAX_S];
    bool bad = (a.flags & ~(SALVE_TILE_HFLIP | SALVE_TILE_VFLIP)) != 0;
    bad |= train_jobs_bad<MAX_S>(t, smp, JITTER ? 6 * t.per_sample : CP, ja, jb);
    if (JITTER)
        for (int k = 0; k < 2 * t.per_sample; k++) bad |= jitter_record_bad(t.jitter[(size_t)smp * 2 * t.per_sample + k]);
    if (bad) {
        if (t.status && blk == 0 && threadIdx.x == 0) atomicOr(t.status, SALVE_STATUS_BAD_TILE_JOB);
        return;
    }
    const int idx = blk * 256 + threadIdx.x;
    if (idx >= t.crop * t.crop) return;
    const int i = idx / t.crop, j = idx % t.crop;
    const int oy = min(max(a.crop_y, 0), t.resize - t.crop), ox = min(max(a.crop_x, 0), t.resize - t.crop);
    const int si = (a.flags & SALVE_TILE_VFLIP) ? t.crop - 1 - i : i, sj = (a.flags & SALVE_TILE_HFLIP) ? t.crop - 1 - j : j;
    const int4 cy = reinterpret_cast<const int4*>(t.coef_y)[si + oy];
    const int4 cx = reinterpret_cast<const int4*>(t.coef_x)[sj + ox];
    float v[CP];
#pragma unroll
    for (int c = 0; c < CP; c++) v[c] = 0.0f;
#pragma unroll
    for (int g = 0; g < GROUPS; g++) {   // channel group g = channels 3 g .. 3 g + 2: the image whose job names it (workgroup-uniform)
        const uint32_t* img = train_group_image<MAX_S>(t, ja, jb, g);
        if (!img) continue;
        if (JITTER) {   // (a group with an image lies below 2 * per_sample: its jobs were checked against 6 * per_sample channels)
            const salve_tile_jitter_t r = t.jitter[(size_t)smp * 2 * t.per_sample + g];
            const float mean = (float)t.grey_sum[(size_t)smp * 2 * t.per_sample + g] / (float)(t.resize * t.resize);   // torch.mean: ONE division
            int q[3];
            tile_bytes(img, t.W, cy, cx, q);
            jitter_pixel<false>(r, q, mean);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) v[3 * g + ch] = t.lut[ch * 256 + q[ch]];
        } else {
            tile_pixel(img, t.W, cy, cx, t.lut, &v[3 * g]);
        }
    }
    const size_t px = ((size_t)smp * t.crop * t.crop + idx) * CP;
    if (BF16) {
        uint4* o = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(t.out) + px);
#pragma unroll
        for (int c = 0; c < CP / 8; c++) {   // one rounding to nearest even (v_cvt_pk_bf16_f32), as conv_train_bf16.hip's epilogue
            const f32x8 f = {v[8 * c], v[8 * c + 1], v[8 * c + 2], v[8 * c + 3], v[8 * c + 4], v[8 * c + 5], v[8 * c + 6], v[8 * c + 7]};
            o[c] = __builtin_bit_cast(uint4, __builtin_convertvector(f, bf16x8));
        }
    } else {
        float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(t.out) + px);
#pragma unroll
        for (int c = 0; c < CP / 4; c++) o[c] = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
    }
}

template <int CP, bool JITTER>
void launch_train_tiles(bool bf16, dim3 grid, hipStream_t s, const TrainTiles& t) {
    if (bf16) hipLaunchKernelGGL((bev_train_tile_kernel<CP, true, JITTER>), grid, dim3(256), 0, s, t);
    else hipLaunchKernelGGL((bev_train_tile_kernel<CP, false, JITTER>), grid, dim3(256), 0, s, t);
}

template <bool JITTER>
void launch_train_tiles(int out_c, bool bf16, dim3 grid, hipStream_t s, const TrainTiles& t) {
    switch (out_c) {
        case 8: launch_train_tiles<8, JITTER>(bf16, grid, s, t); break;
        case 16: launch_train_tiles<16, JITTER>(bf16, grid, s, t); break;
        default: launch_train_tiles<24, JITTER>(bf16, grid, s, t);
    }
}

__global__ __launch_bounds__(256) void bev_export_kernel(const uint32_t* __restrict__ bev, size_t npx,
                                                         uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const uint32_t v = bev[i];
    out[3 * i] = (uint8_t)v;
    out[3 * i + 1] = (uint8_t)(v >> 8);
    out[3 * i + 2] = (uint8_t)(v >> 16);
}

// Panorama ingest: cv2.resize(rgb, (w, h), INTER_LINEAR) on uint8 RGB (bev_rendering_utils.py:370-375).  OpenCV turns an
// exact 2x down-scale into its INTER_AREA fast path ((a + b + c + d + 2) >> 2); everything else is the 11-bit fixed-point
// bilinear of the tile kernels above.  One thread per destination pixel.
__global__ __launch_bounds__(256) void resize_rgb_kernel(const uint8_t* __restrict__ src, int n, int Hs, int Ws,
                                                         uint8_t* __restrict__ dst, int Hd, int Wd,
                                                         const int32_t* __restrict__ coef_y, const int32_t* __restrict__ coef_x,
                                                         int area2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * Hd * Wd) return;
    const int x = (int)(i % Wd), y = (int)((i / Wd) % Hd);
    const uint8_t* img = src + (i / ((size_t)Hd * Wd)) * (size_t)Hs * Ws * 3;
    uint8_t* o = dst + i * 3;
    if (area2) {
        const uint8_t* r0 = img + ((size_t)(2 * y) * Ws + 2 * x) * 3;
        const uint8_t* r1 = r0 + (size_t)Ws * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[ch] = (uint8_t)((r0[ch] + r0[3 + ch] + r1[ch] + r1[3 + ch] + 2) >> 2);
        return;
    }
    const int4 cy = reinterpret_cast<const int4*>(coef_y)[y];
    const int4 cx = reinterpret_cast<const int4*>(coef_x)[x];
    const uint8_t* p00 = img + ((size_t)cy.x * Ws + cx.x) * 3;
    const uint8_t* p01 = img + ((size_t)cy.x * Ws + cx.y) * 3;
    const uint8_t* p10 = img + ((size_t)cy.y * Ws + cx.x) * 3;
    const uint8_t* p11 = img + ((size_t)cy.y * Ws + cx.y) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch] = (uint8_t)bilinear_u8(p00[ch], p01[ch], p10[ch], p11[ch], cy, cx);
}

// The refusals the tile entries share, in the one order all of them keep: pointers and sizes, the crop and the entry's rule for out_c,
// the format (salve_bev_tiles answers an unknown one with SALVE_ERR_UNSUPPORTED), the count.  A count of zero never gets here.
int refuse_tiles(const char* entry, bool args_ok, int32_t resize, int32_t crop, bool out_c_ok, const char* out_c_rule, int32_t n,
                 bool format_ok = true, int format_code = SALVE_ERR_BAD_ARG) {
    char msg[200];
    int code = SALVE_ERR_BAD_ARG;
    if (!args_ok) snprintf(msg, sizeof(msg), "%s: null pointer or bad size", entry);
    else if (crop <= 0 || resize < crop || !out_c_ok) snprintf(msg, sizeof(msg), "%s: need 0 < crop <= resize, %s", entry, out_c_rule);
    else if (!format_ok) { snprintf(msg, sizeof(msg), "%s: unknown tile format", entry); code = format_code; }
    else if (n > 65535) snprintf(msg, sizeof(msg), "%s: at most 65535 tiles, pairs or samples per call", entry);
    else return SALVE_OK;
    salve_fail(msg);
    return code;
}

// salve_bev_train_tiles and salve_bev_train_tiles_jitter: one set of refusals, one launch geometry; with_jitter adds the entry's own
// refusals, the zeroed grey sums and the launch that fills them.
int train_tiles(const char* entry, const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b, int32_t per_sample, const salve_tile_aug_t* aug, int32_t batch,
                const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut, void* out, int32_t out_format,
                int32_t out_c, bool with_jitter, const salve_tile_jitter_t* jitter, void* workspace, size_t workspace_bytes, int32_t* status,
                void* stream) {
    char msg[200];
    if (batch == 0) return SALVE_OK;
    if (per_sample < 1 || per_sample > 3) { snprintf(msg, sizeof(msg), "%s: 1 to 3 images per sample and table", entry); salve_fail(msg); return SALVE_ERR_BAD_ARG; }
    const int st = refuse_tiles(entry,
                                bev_a && bev_b && jobs_a && jobs_b && aug && coef_y && coef_x && lut && out && batch > 0 && n_bev_a > 0 && n_bev_b > 0 && bev_h > 0 && bev_w > 0,
                                resize, crop, out_c % 8 == 0 && out_c >= 6 * per_sample && out_c <= 24,
                                "out_c a multiple of 8 that holds the sample's 6 * per_sample channels (8, 16 or 24)", batch,
                                out_format == SALVE_TILE_F32_NHWC || out_format == SALVE_TILE_BF16_NHWC);
    if (st != SALVE_OK) return st;
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0) { snprintf(msg, sizeof(msg), "%s: out must be 16-byte aligned", entry); salve_fail(msg); return SALVE_ERR_BAD_ARG; }
    const int n_blocks = (crop * crop + 255) / 256;
    const TrainTiles t = {bev_a, bev_b, jobs_a, jobs_b, aug, coef_y, coef_x, lut, out, status, (long long)n_bev_a * bev_h * bev_w,
                          (long long)n_bev_b * bev_h * bev_w, bev_w, bev_h * bev_w, resize, crop, batch, per_sample, n_blocks,
                          jitter, reinterpret_cast<uint32_t*>(workspace)};
    const dim3 g((unsigned)((batch + 7) / 8 * 8 * n_blocks));
    const bool bf16 = out_format == SALVE_TILE_BF16_NHWC;
    if (!with_jitter) {
        launch_train_tiles<false>(out_c, bf16, g, (hipStream_t)stream, t);
        SALVE_HIP_CHECK(hipGetLastError());
        return SALVE_OK;
    }
    if ((long long)resize * resize * 255 >= (1LL << 24)) {
        snprintf(msg, sizeof(msg), "%s: resize * resize * 255 must stay below 2^24 (resize <= 256): the grey sum is an exact float32", entry);
        salve_fail(msg);
        return SALVE_ERR_UNSUPPORTED;
    }
    if (!jitter || !workspace || reinterpret_cast<uintptr_t>(workspace) % 4 != 0) {
        snprintf(msg, sizeof(msg), "%s: null jitter table or workspace, or a misaligned workspace", entry);
        salve_fail(msg);
        return SALVE_ERR_BAD_ARG;
    }
    const size_t need = salve_bev_train_tiles_jitter_workspace_bytes(batch, per_sample);
    if (workspace_bytes < need) { snprintf(msg, sizeof(msg), "%s: workspace too small", entry); salve_fail(msg); return SALVE_ERR_WORKSPACE; }
    SALVE_HIP_CHECK(hipMemsetAsync(workspace, 0, need, (hipStream_t)stream));
    const int sum_blocks = (resize * resize + 256 * GREY_PIXELS - 1) / (256 * GREY_PIXELS), images = batch * 2 * per_sample;
    hipLaunchKernelGGL(bev_jitter_grey_sum_kernel, dim3((unsigned)((images + 7) / 8 * 8 * sum_blocks)), dim3(256), 0, (hipStream_t)stream, t, sum_blocks);
    SALVE_HIP_CHECK(hipGetLastError());
    launch_train_tiles<true>(out_c, bf16, g, (hipStream_t)stream, t);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

}  // namespace

extern "C" {

int salve_bev_export_u8(const uint32_t* bev, int32_t n, int32_t bev_h, int32_t bev_w, uint8_t* out, void* stream) {
    if (n == 0) return SALVE_OK;
    if (!bev || !out || n < 0 || bev_h <= 0 || bev_w <= 0) { salve_fail("salve_bev_export_u8: bad argument"); return SALVE_ERR_BAD_ARG; }
    const size_t npx = (size_t)n * bev_h * bev_w;
    hipLaunchKernelGGL(bev_export_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bev, npx, out);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_resize_rgb_u8(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, uint8_t* dst, int32_t dst_h, int32_t dst_w,
                        const int32_t* coef_y, const int32_t* coef_x, void* stream) {
    if (n == 0) return SALVE_OK;
    if (!src || !dst || n < 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) {
        salve_fail("salve_resize_rgb_u8: null pointer or bad size");
        return SALVE_ERR_BAD_ARG;
    }
    const int area2 = (src_h == 2 * dst_h && src_w == 2 * dst_w) ? 1 : 0;
    if (!area2 && (!coef_y || !coef_x)) { salve_fail("salve_resize_rgb_u8: tap tables are required unless the scale is exactly 2"); return SALVE_ERR_BAD_ARG; }
    const size_t total = (size_t)n * dst_h * dst_w;
    hipLaunchKernelGGL(resize_rgb_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n, src_h, src_w, dst,
                       dst_h, dst_w, coef_y, coef_x, area2);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_bev_tiles(const uint32_t* bev, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs, int32_t n_jobs,
                    const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                    void* out, int32_t out_format, int32_t out_c, void* stream) {
    if (n_jobs == 0) return SALVE_OK;
    const int st = refuse_tiles("salve_bev_tiles", bev && jobs && coef_y && coef_x && lut && out && n_jobs > 0 && bev_h > 0 && bev_w > 0, resize, crop,
                                out_c >= 3, "out_c >= 3", n_jobs,
                                out_format == SALVE_TILE_F32_NCHW || out_format == SALVE_TILE_F16_NHWC || out_format == SALVE_TILE_U8X4, SALVE_ERR_UNSUPPORTED);
    if (st != SALVE_OK) return st;
    dim3 g((crop * crop + 255) / 256, n_jobs);
    hipLaunchKernelGGL(bev_tile_kernel, g, dim3(256), 0, (hipStream_t)stream, bev, bev_w, jobs, coef_y, coef_x, resize, crop,
                       lut, out, out_format, out_c);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_bev_tiles_aug(const uint32_t* bev, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs, const salve_tile_aug_t* aug,
                        int32_t n_jobs, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                        float* out, int32_t out_c, void* stream) {
    if (n_jobs == 0) return SALVE_OK;
    const int st = refuse_tiles("salve_bev_tiles_aug", bev && jobs && aug && coef_y && coef_x && lut && out && n_jobs > 0 && bev_h > 0 && bev_w > 0,
                                resize, crop, out_c >= 3, "out_c >= 3", n_jobs);
    if (st != SALVE_OK) return st;
    dim3 g((crop * crop + 255) / 256, n_jobs);
    hipLaunchKernelGGL(bev_tile_aug_kernel, g, dim3(256), 0, (hipStream_t)stream, bev, bev_w, jobs, aug, coef_y, coef_x, resize, crop, lut, out,
                       out_c);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_bev_tile_pairs(const uint32_t* bev_a, const uint32_t* bev_b, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs_a,
                         const salve_tile_job_t* jobs_b, int32_t n_pairs, const int32_t* coef_y, const int32_t* coef_x, int32_t resize,
                         int32_t crop, const float* lut, void* out, int32_t out_c, int32_t b_pretiled, void* stream) {
    if (n_pairs == 0) return SALVE_OK;
    const int st = refuse_tiles("salve_bev_tile_pairs", bev_a && bev_b && jobs_a && jobs_b && coef_y && coef_x && lut && out && n_pairs > 0 && bev_h > 0 && bev_w > 0,
                                resize, crop, out_c >= 6 && out_c % 2 == 0, "even out_c >= 6", n_pairs);
    if (st != SALVE_OK) return st;
    const int n_blocks = (crop * crop + 255) / 256;
    const int xcd_group = 1;   // the workgroups of a pair on one XCD: its two BEV images are read through one L2 (round 3: -0.3 ms per 4096)
    dim3 g((unsigned)((xcd_group ? (n_pairs + 7) / 8 * 8 : n_pairs) * n_blocks));
    hipLaunchKernelGGL(bev_tile_pair_kernel, g, dim3(256), 0, (hipStream_t)stream, bev_a, bev_b, bev_w, jobs_a, jobs_b, coef_y, coef_x,
                       resize, crop, lut, reinterpret_cast<uint16_t*>(out), out_c, n_pairs, n_blocks, xcd_group, b_pretiled ? 1 : 0);
    SALVE_HIP_CHECK(hipGetLastError());
    return SALVE_OK;
}

int salve_bev_train_tiles(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                          const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b, int32_t per_sample, const salve_tile_aug_t* aug,
                          int32_t batch, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                          void* out, int32_t out_format, int32_t out_c, int32_t* status, void* stream) {
    return train_tiles("salve_bev_train_tiles", bev_a, n_bev_a, bev_b, n_bev_b, bev_h, bev_w, jobs_a, jobs_b, per_sample, aug, batch, coef_y, coef_x, resize, crop,
                       lut, out, out_format, out_c, false, nullptr, nullptr, 0, status, stream);
}

size_t salve_bev_train_tiles_jitter_workspace_bytes(int32_t batch, int32_t per_sample) {
    if (batch <= 0 || batch > 65535 || per_sample < 1 || per_sample > 3) return 0;
    return (size_t)batch * 2 * per_sample * sizeof(uint32_t);   // the grey sums
}

int salve_bev_train_tiles_jitter(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                                 const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b, int32_t per_sample, const salve_tile_aug_t* aug,
                                 int32_t batch, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                                 void* out, int32_t out_format, int32_t out_c, const salve_tile_jitter_t* jitter, void* workspace,
                                 size_t workspace_bytes, int32_t* status, void* stream) {
    return train_tiles("salve_bev_train_tiles_jitter", bev_a, n_bev_a, bev_b, n_bev_b, bev_h, bev_w, jobs_a, jobs_b, per_sample, aug, batch, coef_y, coef_x, resize,
                       crop, lut, out, out_format, out_c, true, jitter, workspace, workspace_bytes, status, stream);
}

}  // extern "C"
