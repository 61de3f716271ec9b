// resnet_f32.hip -- the early-fusion ResNet verifier in fp32 for gfx950 (MI355X): the reference's own precision.
//
// Stands behind salve/models/early_fusion.py:41-83 evaluated as salve/train_utils.py:18-41 evaluates it -- in float32, no
// AMP.  It runs the SAME op program as resnet.hip (salve_resnet_op_t rows, ktab, in2 projection shortcuts), with an fp32
// weight blob, fp32 NHWC activations and v_mfma_f32_32x32x2_f32: f32 operands, f32 accumulation, one rounding per fma and
// no reduced-precision shortcut (gfx950 has no xf32).  Nothing is stored in fp16, so nothing saturates and no status bit
// exists for magnitudes; NaN propagates through every op as it does in torch (the fp16 engine's ReLUs swallow it).
//
// The engine runs the program op by op: no fusion, no persistent kernels.
//   input_nchw_to_nhwc_kernel  the caller's fp32 NCHW [B, C, H, W] -> NHWC [B, H, W, Cpad] in the workspace (pad channels 0)
//   conv_f32_kernel            every SALVE_OP_CONV row: implicit GEMM, M = B * Ho * Wo pixels, N = Cout, K walked through ktab
//                              (conv_f32.h: shared with the per-convolution training entries of conv_train_f32.hip)
//   conv_bf16x3_kernel         the same rows in a handle of salve_resnet_bf16x3_create: every fp32 operand as two bf16 pieces, three
//                              v_mfma_f32_32x32x16_bf16 per k-step (conv_bf16x3.h); everything else in this list is shared
//   maxpool_f32_kernel         3 x 3 / 2 / pad 1
//   avgpool_fc_f32_kernel      fp32 mean over the pixels, then the linear layer in fp32
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <vector>

#include "../../include/salve_hip.h"
#include "salve_common.h"
#include "conv_f32.h"
#include "conv_bf16x3.h"

namespace {

// NCHW [B, C, H, W] -> NHWC [B, H, W, Cp] (channels C..Cp-1 zero), one thread per pixel: the reads of a channel are coalesced
// across the wave, the pixel's Cp floats are written as 16-byte stores.
__global__ __launch_bounds__(256) void input_nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C,
                                                                 int HW, int Cp) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * HW) return;
    const long long b = idx / HW, px = idx % HW;
    const float* src = in + b * C * HW + px;
    float4* dst = reinterpret_cast<float4*>(out + idx * Cp);
    for (int c4 = 0; c4 < Cp; c4 += 4) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = c4 + e < C ? src[(long long)(c4 + e) * HW] : 0.f;
        dst[c4 / 4] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// 3 x 3 / stride 2 / pad 1 max-pool on NHWC fp32, 4 channels per thread.  Padding is -inf (torch); a NaN in the window wins.
__global__ __launch_bounds__(256) void maxpool_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int Hi, int Wi,
                                                          int C, int Ho, int Wo) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C / 4;
    if (idx >= (long long)B * Ho * Wo * c4) return;
    const int ch = (int)(idx % c4);
    long long t = idx / c4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = 0; dy < 3; dy++) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= Hi) continue;
        for (int dx = 0; dx < 3; dx++) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= Wi) continue;
            const float4 v = *reinterpret_cast<const float4*>(in + (((long long)b * Hi + iy) * Wi + ix) * C + ch * 4);
            const float w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) best[e] = (w[e] > best[e] || w[e] != w[e]) ? w[e] : best[e];
        }
    }
    *reinterpret_cast<float4*>(out + (((long long)b * Ho + oy) * Wo + ox) * C + ch * 4) = make_float4(best[0], best[1], best[2], best[3]);
}

// Global average pool + linear layer, one workgroup per sample: a thread sums 4 channels over the HW pixels in fp32, divides by
// HW (torch's mean), multiplies with the fc row; the per-class partial dot products are reduced across the workgroup.
__global__ __launch_bounds__(256) void avgpool_fc_f32_kernel(const float* __restrict__ in, int HW, int C, const float* __restrict__ fcw,
                                                             const float* __restrict__ fcb, int ncls, float* __restrict__ logits) {
    __shared__ float red[8][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = in + (long long)b * HW * C;
    float part[8];  // ncls <= 8
#pragma unroll
    for (int k = 0; k < 8; k++) part[k] = 0.f;
    for (int c0 = tid * 4; c0 < C; c0 += 256 * 4) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < HW; i++) {
            const float4 v = *reinterpret_cast<const float4*>(x + (long long)i * C + c0);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        }
        for (int k = 0; k < ncls; k++) {
            const float* wk = fcw + (long long)k * C + c0;
#pragma unroll
            for (int e = 0; e < 4; e++) part[k] += (s[e] / (float)HW) * wk[e];
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float v = part[k];
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (tid < ncls) logits[(long long)b * ncls + tid] = ((red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3])) + fcb[tid];
}

struct ResnetF32Handle {
    std::vector<salve_resnet_op_t> ops;
    float* d_weights = nullptr;
    float* d_params = nullptr;
    int32_t* d_ktab = nullptr;
    size_t max_act_elems = 0;   // per sample, floats of the largest activation buffer
    size_t in_elems = 0;        // per sample, floats of the padded NHWC input
    int n_bufs = 0;
    int num_layers = 0, in_channels = 0, in_pad = 0, ncls = 0;
    bool bf16x3 = false;        // salve_resnet_bf16x3_create: d_weights holds the split bf16 planes (conv_bf16x3.h), same offsets
};

bool check_op_f32(const salve_resnet_op_t& o, size_t w_elems, size_t p_elems, size_t ktab_entries) {
    if (o.op == SALVE_OP_CONV) {
        const size_t K = (size_t)o.KH * o.KW * o.Cin + (o.in2_buf != SALVE_NO_BUF ? (size_t)o.Cin2 : 0);
        if (o.Cout % 64 != 0) return salve_fail("conv: Cout must be a multiple of 64");
        if (o.Cin % 8 != 0) return salve_fail("conv: Cin must be a multiple of 8");
        if ((o.KH * o.KW * o.Cin) % F_BK != 0) return salve_fail("conv: KH*KW*Cin must be a multiple of 32");
        if (o.in_buf == o.out_buf || (o.res_buf != SALVE_NO_BUF && o.res_buf == o.out_buf) || o.out_buf < 0)
            return salve_fail("conv: the output buffer must be a workspace buffer other than its inputs");
        if (o.in2_buf != SALVE_NO_BUF) {
            if (o.KH != 1 || o.KW != 1 || o.stride != 1 || o.pad != 0 || o.res_buf != SALVE_NO_BUF || o.in2_buf == o.out_buf)
                return salve_fail("conv: a second source needs a 1x1 / stride 1 / pad 0 convolution without residual");
            if (o.Cin2 <= 0 || o.Cin2 % F_BK != 0 || o.stride2 < 1 || (o.Hi2 - 1) / o.stride2 + 1 != o.Ho || (o.Wi2 - 1) / o.stride2 + 1 != o.Wo)
                return salve_fail("conv: bad second-source geometry");
        } else if ((size_t)o.ktab_off + K / 8 > ktab_entries) {
            return salve_fail("conv: k table out of range");
        }
        if ((size_t)o.w_off + (size_t)o.Cout * K > w_elems || (size_t)o.b_off + (size_t)o.Cout > p_elems)
            return salve_fail("conv: weight or bias offset out of range");
        if (o.Ho != (o.Hi + 2 * o.pad - o.KH) / o.stride + 1) return salve_fail("conv: bad output height");
    } else if (o.op == SALVE_OP_MAXPOOL) {
        if (o.Cin % 4 != 0 || o.Cout != o.Cin || o.out_buf < 0 || o.out_buf == o.in_buf) return salve_fail("maxpool: bad channels or buffers");
    } else if (o.op == SALVE_OP_AVGPOOL_FC) {
        if (o.Cout < 1 || o.Cout > 8) return salve_fail("fc: 1..8 classes supported");
        if (o.Cin % 4 != 0) return salve_fail("fc: C must be a multiple of 4");
        if ((size_t)o.w_off + (size_t)o.Cout * o.Cin > p_elems || (size_t)o.b_off + (size_t)o.Cout > p_elems)
            return salve_fail("fc: parameter offset out of range");
    } else {
        return salve_fail("unknown op");
    }
    return true;
}


}  // namespace

extern "C" {

void* salve_resnet_f32_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                              const float* weights_f32, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                              const int32_t* ktab, size_t ktab_entries, int32_t flags) {
    if (!ops || n_ops <= 0 || !weights_f32 || !params_f32 || !ktab) {
        salve_fail("salve_resnet_f32_create: null argument");
        return nullptr;
    }
    if (flags != 0) {
        salve_fail("salve_resnet_f32_create: flags must be 0 (the fp32 engine has one kernel selection)");
        return nullptr;
    }
    if (in_channels <= 0) {
        salve_fail("salve_resnet_f32_create: in_channels must be positive");
        return nullptr;
    }
    const size_t w_elems = weights_bytes / sizeof(float), p_elems = params_bytes / sizeof(float);
    ResnetF32Handle* h = new ResnetF32Handle();
    h->num_layers = num_layers;
    h->in_channels = in_channels;
    h->in_pad = (in_channels + 7) / 8 * 8;
    bool have_input = false;
    for (int i = 0; i < n_ops; i++) {
        const salve_resnet_op_t& o = ops[i];
        if (!check_op_f32(o, w_elems, p_elems, ktab_entries)) { delete h; return nullptr; }
        if (o.in_buf == SALVE_NET_INPUT) {
            if (o.op != SALVE_OP_CONV || o.Cin != h->in_pad) {
                salve_fail("salve_resnet_f32_create: in_channels padded to a multiple of 8 must equal the Cin of the convolution that reads the input");
                delete h;
                return nullptr;
            }
            const size_t e = (size_t)o.Hi * o.Wi * o.Cin;
            if (have_input && e != h->in_elems) { salve_fail("salve_resnet_f32_create: two input shapes"); delete h; return nullptr; }
            h->in_elems = e;
            have_input = true;
        }
        if (o.res_buf == SALVE_NET_INPUT || o.in2_buf == SALVE_NET_INPUT) {
            salve_fail("salve_resnet_f32_create: only a convolution's first source may be the network input");
            delete h;
            return nullptr;
        }
        h->ops.push_back(o);
        if (o.op != SALVE_OP_AVGPOOL_FC) {
            const size_t e = (size_t)o.Ho * o.Wo * o.Cout;
            if (e > h->max_act_elems) h->max_act_elems = e;
            if (o.out_buf + 1 > h->n_bufs) h->n_bufs = o.out_buf + 1;
        } else {
            h->ncls = o.Cout;
        }
    }
    if (!have_input || h->ncls == 0 || h->ops.back().op != SALVE_OP_AVGPOOL_FC) {
        salve_fail("salve_resnet_f32_create: the program must read the input and end in AVGPOOL_FC");
        delete h;
        return nullptr;
    }
    for (const salve_resnet_op_t& o : h->ops) {   // every read stays inside a buffer of the workspace (or the input)
        const bool conv = o.op == SALVE_OP_CONV;
        const int reads[3] = {o.in_buf, conv ? o.res_buf : SALVE_NO_BUF, conv ? o.in2_buf : SALVE_NO_BUF};
        const size_t extent[3] = {(size_t)o.Hi * o.Wi * o.Cin, (size_t)o.Ho * o.Wo * o.Cout, (size_t)o.Hi2 * o.Wi2 * o.Cin2};
        for (int r = 0; r < 3; r++) {
            const int b = reads[r];
            if (b == SALVE_NO_BUF) continue;
            const bool ok = b == SALVE_NET_INPUT ? extent[r] <= h->in_elems : (b >= 0 && b < h->n_bufs && extent[r] <= h->max_act_elems);
            if (!ok || o.Hi <= 0 || o.Wi <= 0 || o.Ho <= 0 || o.Wo <= 0) {
                salve_fail("salve_resnet_f32_create: an op reads outside the buffers of the workspace");
                delete h;
                return nullptr;
            }
        }
    }
    if (hipMalloc(&h->d_weights, weights_bytes) != hipSuccess || hipMalloc(&h->d_params, params_bytes) != hipSuccess ||
        hipMalloc(&h->d_ktab, (ktab_entries ? ktab_entries : 1) * sizeof(int32_t)) != hipSuccess) {
        salve_fail("salve_resnet_f32_create: hipMalloc failed");
        salve_resnet_f32_destroy(h);
        return nullptr;
    }
    if (hipMemcpy(h->d_weights, weights_f32, weights_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_params, params_f32, params_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        (ktab_entries && hipMemcpy(h->d_ktab, ktab, ktab_entries * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)) {
        salve_fail("salve_resnet_f32_create: hipMemcpy failed");
        salve_resnet_f32_destroy(h);
        return nullptr;
    }
    return h;
}

void* salve_resnet_bf16x3_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                                 const float* weights_f32, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                                 const int32_t* ktab, size_t ktab_entries, int32_t flags) {
    if (flags != 0) {
        salve_fail("salve_resnet_bf16x3_create: flags must be 0 (the bf16x3 engine has one kernel selection)");
        return nullptr;
    }
    // the fp32 engine's checks, program and uploads (its refusals carry its name); then the weights are split in place of the fp32 blob
    ResnetF32Handle* h = reinterpret_cast<ResnetF32Handle*>(salve_resnet_f32_create(num_layers, in_channels, ops, n_ops, weights_f32, weights_bytes,
                                                                                    params_f32, params_bytes, ktab, ktab_entries, 0));
    if (!h) return nullptr;
    uint16_t* split = nullptr;
    if (hipMalloc(&split, weights_bytes) != hipSuccess) {
        salve_fail("salve_resnet_bf16x3_create: hipMalloc failed");
        salve_resnet_f32_destroy(h);
        return nullptr;
    }
    bool ok = hipMemset(split, 0, weights_bytes) == hipSuccess;
    for (const salve_resnet_op_t& o : h->ops) {
        if (!ok || o.op != SALVE_OP_CONV) continue;
        const long long n = (long long)o.Cout * ((long long)o.KH * o.KW * o.Cin + (o.in2_buf != SALVE_NO_BUF ? o.Cin2 : 0));
        hipLaunchKernelGGL(split_weights_bf16x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, h->d_weights + o.w_off,
                           split + 2 * (size_t)o.w_off, n);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    (void)hipFree(h->d_weights);
    h->d_weights = reinterpret_cast<float*>(split);
    h->bf16x3 = true;
    if (!ok) {
        salve_fail("salve_resnet_bf16x3_create: splitting the weights failed");
        salve_resnet_f32_destroy(h);
        return nullptr;
    }
    return h;
}

void salve_resnet_f32_destroy(void* handle) {
    ResnetF32Handle* h = reinterpret_cast<ResnetF32Handle*>(handle);
    if (!h) return;
    if (h->d_weights) (void)hipFree(h->d_weights);
    if (h->d_params) (void)hipFree(h->d_params);
    if (h->d_ktab) (void)hipFree(h->d_ktab);
    delete h;
}

size_t salve_resnet_f32_workspace_bytes(void* handle, int32_t batch) {
    ResnetF32Handle* h = reinterpret_cast<ResnetF32Handle*>(handle);
    if (!h || batch <= 0) return 0;
    return ((size_t)h->n_bufs * h->max_act_elems + h->in_elems) * (size_t)batch * sizeof(float) + 256;
}

int salve_resnet_f32_forward(void* handle, const float* input, int32_t batch, float* logits, void* workspace, size_t workspace_bytes,
                             int32_t* status, void* stream) {
    (void)status;   // fp32 has the reference's range: no bit to raise (the argument keeps the call shape of salve_resnet_forward)
    ResnetF32Handle* h = reinterpret_cast<ResnetF32Handle*>(handle);
    if (!h || !input || !logits || !workspace || batch <= 0) {
        salve_fail("salve_resnet_f32_forward: null argument or bad batch");
        return SALVE_ERR_BAD_ARG;
    }
    if (workspace_bytes < salve_resnet_f32_workspace_bytes(handle, batch)) {
        salve_fail("salve_resnet_f32_forward: workspace too small");
        return SALVE_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float* base = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const size_t buf_elems = (size_t)batch * h->max_act_elems;
    float* x_nhwc = base + (size_t)h->n_bufs * buf_elems;
    auto buf = [&](int i) -> float* { return i == SALVE_NET_INPUT ? x_nhwc : (i < 0 ? nullptr : base + (size_t)i * buf_elems); };
    {
        const int HW = (int)(h->in_elems / h->in_pad);
        const long long n = (long long)batch * HW;
        hipLaunchKernelGGL(input_nchw_to_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, input, x_nhwc, batch, h->in_channels,
                           HW, h->in_pad);
        SALVE_HIP_CHECK(hipGetLastError());
    }
    for (const salve_resnet_op_t& o : h->ops) {
        if (o.op == SALVE_OP_CONV) {
            ConvF32Args a;
            a.in = buf(o.in_buf);
            a.w = h->d_weights + o.w_off;
            a.bias = h->d_params + o.b_off;
            a.res = o.res_buf == SALVE_NO_BUF ? nullptr : buf(o.res_buf);
            a.out = buf(o.out_buf);
            a.ktab = h->d_ktab + o.ktab_off;
            a.in2 = o.in2_buf == SALVE_NO_BUF ? nullptr : buf(o.in2_buf);
            a.Hi = o.Hi; a.Wi = o.Wi; a.Cin = o.Cin; a.Ho = o.Ho; a.Wo = o.Wo; a.Cout = o.Cout;
            a.stride = o.stride; a.pad = o.pad; a.relu = o.relu;
            a.Hi2 = o.Hi2; a.Wi2 = o.Wi2; a.Cin2 = o.Cin2; a.stride2 = o.stride2;
            a.nkt1 = o.KH * o.KW * o.Cin / F_BK;
            a.K = o.KH * o.KW * o.Cin + (a.in2 ? o.Cin2 : 0);
            const long long M = (long long)batch * o.Ho * o.Wo;
            if (M > 0x7FFFFFFFll - F_BM) { salve_fail("batch too large"); return SALVE_ERR_BAD_ARG; }
            a.M = (int)M;
            a.m_tiles = (int)((M + F_BM - 1) / F_BM);
            int st;
            if (o.Cout % 128 == 0) {
                a.n_tiles = o.Cout / 128;
                st = h->bf16x3 ? launch_conv_bf16x3<128>(a, s) : launch_conv<128>(a, s);
            } else {
                a.n_tiles = o.Cout / 64;
                st = h->bf16x3 ? launch_conv_bf16x3<64>(a, s) : launch_conv<64>(a, s);
            }
            if (st != SALVE_OK) return st;
        } else if (o.op == SALVE_OP_MAXPOOL) {
            const long long total = (long long)batch * o.Ho * o.Wo * (o.Cin / 4);
            hipLaunchKernelGGL(maxpool_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, buf(o.in_buf), buf(o.out_buf), batch,
                               o.Hi, o.Wi, o.Cin, o.Ho, o.Wo);
            SALVE_HIP_CHECK(hipGetLastError());
        } else {
            hipLaunchKernelGGL(avgpool_fc_f32_kernel, dim3(batch), dim3(256), 0, s, buf(o.in_buf), o.Hi * o.Wi, o.Cin, h->d_params + o.w_off,
                               h->d_params + o.b_off, o.Cout, logits);
            SALVE_HIP_CHECK(hipGetLastError());
        }
    }
    return SALVE_OK;
}

}  // extern "C"
