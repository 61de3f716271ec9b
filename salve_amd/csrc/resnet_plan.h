// resnet_plan.h -- which kernel runs which ops of a verifier program: the launch plan of resnet.hip, decided once per handle.
//
// Host only: include/salve_hip.h and the standard library, no HIP (tests/host/resnet_plan_host.cpp compiles it with g++ and pins
// the plans on the CPU: the logits are bit-identical whichever kernels run, so a GPU test cannot see a wrong plan that still computes).
// salve_resnet_create calls plan_resnet once; salve_resnet_forward walks the steps and launches one kernel per step.  A step names
// the ops it consumes -- nothing else does arithmetic on an op index.  A new fusion is one more StepKind (or form), one rule in
// plan_resnet at its place in the precedence, and one launch function in resnet.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/salve_hip.h"

bool salve_fail(const char* msg);   // abi.hip: records the message for salve_last_error(), returns false (salve_common.h declares it next to the HIP plumbing)

namespace salve_plan {

// what the planner has to know of the kernels (resnet.hip asserts that they are the kernels' own constants)
constexpr int PLAN_BK = 64;        // conv_igemm_kernel's k-tile
constexpr int PLAN_STEM_W = 224;   // stem_pool_kernel: the input width it is written for
constexpr int PLAN_STEM_R = 4;     //                   pooled rows per strip

enum StepKind { STEM_POOL, BOTTLENECK, EXPAND_CHAIN, CONV, MAXPOOL, AVGPOOL_FC };

// bottleneck_kernel<64, 8, PROJ, NEXT> (bottleneck.h)
enum BlockForm {
    BLOCK_PLAIN,   // three ops: reduce, 3x3, expand + residual
    BLOCK_PROJ,    // three ops: the first block of layer 1, its projection shortcut in the last convolution's k
    BLOCK_NEXT     // four ops: the plain block and the following block's first 1x1 convolution
};

// expand_chain_kernel<MID, MIDN, R, CHAIN, AHEAD, NW, NSPLIT> (expand_chain.h): X = expand only (one op), C = chained with the next
// block's first convolution (two ops).  _SPLIT: 16 waves, the channels split over wave pairs (the 256-channel shapes, unless
// SALVE_RESNET_CHAIN_NO_SPLIT); _W16: 16 waves on tiles of 256 pixels (SALVE_RESNET_CHAIN_16_WAVES, the all-128-channel shapes).
enum ChainForm { CHAIN_X128, CHAIN_X256, CHAIN_C128_128, CHAIN_C128_256, CHAIN_C256_256, CHAIN_X256_SPLIT, CHAIN_C128_256_SPLIT, CHAIN_C256_256_SPLIT,
                 CHAIN_X128_W16, CHAIN_C128_128_W16 };

// SALVE_CONV_WIDE (ablation build, read when a handle is created): unset = the 8-phase 256 x 256 kernel (conv8.h) on the compute-bound shapes
// that fit it, 0 = conv_igemm_kernel everywhere, 8 = the 8-phase kernel wherever it fits.  d | e | f select the wide-tile /
// split-role kernels of conv_wide.h, which were measured per shape on MI355X and rejected: they exist
// only in the ablation build (-DSALVE_BUILD_ABLATIONS, tools/probe/build_ablations.sh) -- the product library treats them as 0.
// All of them are bit-identical to conv_igemm_kernel (same k order, same fp32 accumulation).
enum { WIDE_OFF = 0, WIDE_256_K64_S2 = 4, WIDE_128_K64_S1 = 5, WIDE_PC_128 = 6, WIDE_8PHASE = 7, WIDE_AUTO = 8 };

struct Step {            // one launch
    StepKind kind;
    int first, count;    // it consumes ops[first .. first + count), 1 <= count <= 4
    int form;            // BOTTLENECK: BlockForm.  EXPAND_CHAIN: ChainForm.  CONV: WIDE_* (never WIDE_AUTO)
    bool chained;        // EXPAND_CHAIN: a C form (count == 2)
    bool y_even;         // BLOCK_NEXT / chained EXPAND_CHAIN: Y is stored at its even pixels only
    bool wide_auto;      // CONV with WIDE_8PHASE: only in launches large enough for it (conv_runs_wide)
};

typedef salve_resnet_op_t Op;

// ------------------------------------------------------------------------------------------------ what is accepted
static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static inline bool pointwise(const Op& o) { return o.KH == 1 && o.KW == 1 && o.stride == 1 && o.pad == 0; }

static inline bool check_op(const Op& o) {
    if (o.op == SALVE_OP_CONV) {
        if (o.Cout % 64 != 0) return salve_fail("conv: Cout must be a multiple of 64");
        if (o.Cin % 8 != 0) return salve_fail("conv: Cin must be a multiple of 8");
        if ((o.KH * o.KW * o.Cin) % PLAN_BK != 0) return salve_fail("conv: KH*KW*Cin must be a multiple of 64");
        if (o.in2_buf != SALVE_NO_BUF) {
            if (!pointwise(o) || o.res_buf != SALVE_NO_BUF)
                return salve_fail("conv: a second source needs a 1x1 / stride 1 / pad 0 convolution without residual");
            if (o.Cin2 <= 0 || o.Cin2 % PLAN_BK != 0 || o.stride2 < 1 || (o.Hi2 - 1) / o.stride2 + 1 != o.Ho || (o.Wi2 - 1) / o.stride2 + 1 != o.Wo)
                return salve_fail("conv: bad second-source geometry");
        }
    } else if (o.op == SALVE_OP_MAXPOOL) {
        if (o.Cin % 8 != 0) return salve_fail("maxpool: C must be a multiple of 8");
    } else if (o.op == SALVE_OP_AVGPOOL_FC) {
        if (o.Cout < 1 || o.Cout > 8) return salve_fail("fc: 1..8 classes supported");
        if (o.Cin % 8 != 0) return salve_fail("fc: C must be a multiple of 8");
    } else {
        return salve_fail("unknown op");
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ predicates on one op
// the plain point-wise ReLU convolution: 1x1 / stride 1 / pad 0 with ReLU, no residual, no second source
static inline bool plain_pointwise_relu(const Op& o) {
    return o.op == SALVE_OP_CONV && pointwise(o) && o.relu && o.res_buf == SALVE_NO_BUF && o.in2_buf == SALVE_NO_BUF;
}
// the 3x3 / stride 1 / pad 1 ReLU convolution in the middle of a bottleneck block, mid -> mid channels
static inline bool plain_3x3_relu(const Op& o, int mid) {
    return o.op == SALVE_OP_CONV && o.KH == 3 && o.KW == 3 && o.stride == 1 && o.pad == 1 && o.relu && o.res_buf == SALVE_NO_BUF &&
           o.in2_buf == SALVE_NO_BUF && o.Cin == mid && o.Cout == mid;
}
static inline bool writes(const Op& o, int b) { return o.op != SALVE_OP_AVGPOOL_FC && o.out_buf == b; }

// ------------------------------------------------------------------------------------------------ predicates on a buffer's life
// Both look at ops[k ..] up to and including the buffer's next writer (which may read it before it overwrites it).

// "buffer b is dead from op k on": nobody reads it before its next writer
static inline bool dead_from(const Op* ops, int n, int k, int b) {
    for (; k < n; k++) {
        const Op& o = ops[k];
        if (o.in_buf == b || (o.op == SALVE_OP_CONV && (o.res_buf == b || o.in2_buf == b))) return false;
        if (writes(o, b)) break;
    }
    return true;
}

// "buffer b is read only by stride-2 shortcuts of geometry H x W from op k on": its readers are second sources (projection shortcuts)
// that sample an H x W image at stride 2, and there is at least one -- only b's even pixels are ever read
static inline bool only_stride2_shortcuts_from(const Op* ops, int n, int k, int b, int H, int W) {
    bool any = false;
    for (; k < n; k++) {
        const Op& o = ops[k];
        if (o.in_buf == b || (o.op == SALVE_OP_CONV && o.res_buf == b)) return false;
        if (o.op == SALVE_OP_CONV && o.in2_buf == b) {
            if (o.stride2 != 2 || o.Hi2 != H || o.Wi2 != W) return false;
            any = true;
        }
        if (writes(o, b)) break;
    }
    return any;
}

// ------------------------------------------------------------------------------------------------ the kernels' shapes
// expand_chain_kernel shapes: (MID, MIDN) of the chained form, MID of the expand-only form
static inline bool chain_shape(int mid, int midn) { return (mid == 128 && (midn == 128 || midn == 256)) || (mid == 256 && midn == 256); }
static inline bool expand_shape(int mid) { return mid == 128 || mid == 256; }   // (512: measured 0.80 ms against 0.71 ms for conv8_kernel at batch 4096: compute-bound there)

static inline int choose_wide(const Op& o, int force) {
    if (o.op != SALVE_OP_CONV || force == WIDE_OFF) return WIDE_OFF;
    const int K = o.KH * o.KW * o.Cin + (o.in2_buf != SALVE_NO_BUF ? o.Cin2 : 0);
    if (!pointwise(o) && (!is_pow2(o.Cin) || o.Cin < 64)) return WIDE_OFF;   // the stem keeps its table-driven gather
    if (K < 128 || K % 64 != 0) return WIDE_OFF;
    if (force == WIDE_8PHASE || force == WIDE_AUTO) {
        const bool fits = o.Cout % 256 == 0 && is_pow2(o.Cin) && o.Cin >= 64 && (o.in2_buf == SALVE_NO_BUF || o.Cin2 % 64 == 0);
        // by default only where the convolution is compute-bound (measured per shape): k >= 512
        // K = 384 (layer 2's projection pair) measured the same on either kernel (r3)
        return (fits && (force == WIDE_8PHASE || K >= 512)) ? WIDE_8PHASE : WIDE_OFF;
    }
    if (force == WIDE_256_K64_S2) return o.Cout % 256 == 0 ? force : WIDE_OFF;
    return o.Cout % 128 == 0 ? force : WIDE_OFF;
}

// 16 / 24 input channels: the fused stem kernel needs K ordered (group of 8 channels, kh, kw, channel): read it off the k table
static inline bool stem_k_order(const Op& a, const int32_t* ktab, size_t ktab_entries) {
    if (a.Cin == 8) return true;
    if (!((a.Cin == 16 || a.Cin == 24) && a.KH == 7 && a.KW == 8 && (size_t)a.ktab_off + (size_t)(a.Cin / 8) * 7 * 8 <= ktab_entries)) return false;
    for (int q = 0; q < (a.Cin / 8) * 7 * 8; q++) {
        const int g = q / 56, kh = (q % 56) / 8, kw = q % 8;
        if (ktab[a.ktab_off + q] != ((kh & 0xFF) | ((kw & 0xFF) << 8) | ((8 * g) << 16))) return false;
    }
    return true;
}

// ops[i], ops[i + 1]: the 7x7 / 2 convolution and the max-pool behind it as stem_pool_kernel
static inline bool stem_pool_fits(const Op* ops, int n, int i, const int32_t* ktab, size_t ktab_entries) {
    if (i + 1 >= n) return false;
    const Op &a = ops[i], &b = ops[i + 1];
    if (a.op != SALVE_OP_CONV || b.op != SALVE_OP_MAXPOOL) return false;
    return a.KH == 7 && a.KW == 8 && a.stride == 2 && a.pad == 3 && (a.Cin == 8 || a.Cin == 16 || a.Cin == 24) && stem_k_order(a, ktab, ktab_entries) &&
           a.Cout == 64 && a.relu && a.res_buf == SALVE_NO_BUF && a.in2_buf == SALVE_NO_BUF && b.in_buf == a.out_buf && b.Cin == 64 &&
           a.Hi % 4 == 0 && a.Wi % 4 == 0 && a.Wi == PLAN_STEM_W && (a.Hi / 4) % PLAN_STEM_R == 0 &&
           a.Ho == a.Hi / 2 && a.Wo == a.Wi / 2 && b.Ho == a.Hi / 4 && b.Wo == a.Wi / 4 &&
           dead_from(ops, n, i + 2, a.out_buf);   // nobody else may read the un-pooled convolution output
}

// ops[i .. i + 2] as bottleneck_kernel: BLOCK_PLAIN, BLOCK_PROJ or -1.
// Measured at batch 512: the 64-channel blocks (56 x 56) gain 15 % fused; the 128-channel blocks (28 x 28, 4 x 16 tiles) come out
// even, so they stay on the three-kernel path.
static inline int block_form(const Op* ops, int n, int i, int flags) {
    if ((flags & SALVE_RESNET_NO_BLOCK_FUSE) || i + 2 >= n) return -1;
    const Op &a = ops[i], &b = ops[i + 1], &c = ops[i + 2];
    const int mid = a.Cout;
    if (mid != 64 || a.Hi % 8 != 0) return -1;
    if (!plain_pointwise_relu(a) || !plain_3x3_relu(b, mid) || b.in_buf != a.out_buf || c.op != SALVE_OP_CONV || !pointwise(c) || !c.relu ||
        c.Cin != mid || c.Cout != 4 * mid || c.in_buf != b.out_buf || c.out_buf == a.in_buf || a.in_buf < 0 || a.Hi != c.Ho || a.Wi != c.Wo ||
        b.Hi != a.Hi || b.Ho != a.Hi)
        return -1;
    const bool plain = a.Cin == 4 * mid && c.in2_buf == SALVE_NO_BUF && c.res_buf == a.in_buf;
    // ... or the first block of layer 1: input of `mid` channels, the projection shortcut in the last convolution's k
    const bool proj = a.Cin == mid && c.res_buf == SALVE_NO_BUF && c.in2_buf == a.in_buf && c.Cin2 == mid && c.stride2 == 1 && c.Hi2 == a.Hi &&
                      c.Wi2 == a.Wi && !(flags & SALVE_RESNET_NO_PROJ_FUSE);
    if (!plain && !proj) return -1;
    // the two intermediate tensors are not produced by the fused kernel: nobody may read them afterwards
    if (!dead_from(ops, n, i + 3, a.out_buf) || !dead_from(ops, n, i + 3, b.out_buf)) return -1;
    return plain ? BLOCK_PLAIN : BLOCK_PROJ;
}

// (r6) The last fused block of layer 1 takes the following block's first convolution along (bottleneck_kernel's NEXT form): a plain
// point-wise ReLU convolution, 4 MID -> 2 MID channels, that reads the block's output Y and nothing else, and that heads no fused block itself.
static inline bool block_takes_next(const Op* ops, int n, int i, int flags) {
    if ((flags & SALVE_RESNET_NO_NEXT_FUSE) || i + 3 >= n) return false;
    const Op &a = ops[i], &c = ops[i + 2], &x = ops[i + 3];
    const int mid = a.Cout;
    return plain_pointwise_relu(x) && x.in_buf == c.out_buf && x.Cin == 4 * mid && x.Cout == 2 * mid && x.Hi == c.Ho && x.Wi == c.Wo &&
           x.out_buf >= 0 && x.out_buf != c.out_buf && x.out_buf != a.in_buf && block_form(ops, n, i + 3, flags) < 0;
}

// ops[i] as expand_chain_kernel: a block's last 1x1 convolution with its residual, MID -> 4 MID channels
static inline bool expand_fits(const Op& c) {
    return c.op == SALVE_OP_CONV && pointwise(c) && c.relu && c.res_buf != SALVE_NO_BUF && c.in2_buf == SALVE_NO_BUF && c.Cout == 4 * c.Cin &&
           expand_shape(c.Cin) && c.res_buf != c.out_buf && c.in_buf != c.out_buf && c.in_buf >= 0 && c.res_buf >= 0;
}

// ... chained with ops[i + 1], the next block's first convolution, where that one follows directly and heads no fused block
static inline bool expand_takes_next(const Op* ops, int n, int i, int flags) {
    if (i + 1 >= n) return false;
    const Op &c = ops[i], &a = ops[i + 1];
    return plain_pointwise_relu(a) && a.in_buf == c.out_buf && a.Cin == c.Cout && a.Hi == c.Ho && a.Wi == c.Wo && chain_shape(c.Cin, a.Cout) &&
           a.out_buf != c.out_buf && a.out_buf != c.in_buf && a.out_buf != c.res_buf && block_form(ops, n, i + 1, flags) < 0;
}

static inline ChainForm chain_form(int mid, int midn, bool chained, int flags) {
    // SALVE_RESNET_CHAIN_16_WAVES: 16 waves, tiles of 256 pixels, where the registers allow it (<= 128 per lane).  Four waves per SIMD
    // issue more densely than two -- with every memory operation switched off the layer-2 launch takes 1.22 instead of
    // 1.55 ms -- but with them it takes the same 1.95 ms: at 4.1 TB/s of mixed reads and writes in 64-byte row pieces the
    // memory system is what is left.  Bit-identical; not the default.
    const bool w16 = (flags & SALVE_RESNET_CHAIN_16_WAVES) && mid == 128 && (!chained || midn == 128);
    // 16 waves with the channels split over wave pairs (128-pixel tiles) for the 256-channel shapes: they are bound by
    // their instruction issue at two waves per SIMD (236-246 VGPRs), not by memory
    const bool split = !w16 && !(flags & SALVE_RESNET_CHAIN_NO_SPLIT) && (mid == 256 || (chained && midn == 256));
    if (!chained) return mid == 128 ? (w16 ? CHAIN_X128_W16 : CHAIN_X128) : (split ? CHAIN_X256_SPLIT : CHAIN_X256);
    if (mid == 256) return split ? CHAIN_C256_256_SPLIT : CHAIN_C256_256;
    if (midn == 256) return split ? CHAIN_C128_256_SPLIT : CHAIN_C128_256;
    return w16 ? CHAIN_C128_128_W16 : CHAIN_C128_128;
}

// ------------------------------------------------------------------------------------------------ the planner
// The steps of a program, in order, every op in exactly one of them; empty (and salve_fail's message) if an op is refused.
// Precedence at an op: stem + max-pool, fused block, expand (+ chain), plain convolution.  The ops inside a fused block are
// consumed by its step, so they are never chain candidates; a step takes a following op along only if that op heads no fused block.
// conv_wide_override: a WIDE_* mode for every convolution (the ablation build's SALVE_CONV_WIDE), -1 = what the flags say.
static inline std::vector<Step> plan_resnet(const Op* ops, int n_ops, const int32_t* ktab, size_t ktab_entries, int flags, int conv_wide_override = -1) {
    std::vector<Step> plan;
    for (int i = 0; i < n_ops; i++)
        if (!check_op(ops[i])) return plan;
    // default: the 8-phase kernel on the compute-bound shapes that fit it, in launches large enough for it
    const int wide_mode = conv_wide_override >= 0 ? conv_wide_override
                          : ((flags & SALVE_RESNET_CONV_IGEMM_ONLY) ? WIDE_OFF : ((flags & SALVE_RESNET_CONV8_WHEREVER) ? WIDE_8PHASE : WIDE_AUTO));
    const bool store_all = (flags & SALVE_RESNET_CHAIN_STORE_ALL) != 0;
    for (int i = 0; i < n_ops;) {
        const Op& o = ops[i];
        Step st = {CONV, i, 1, 0, false, false, false};
        int form;
        if (o.op == SALVE_OP_MAXPOOL) {
            st.kind = MAXPOOL;
        } else if (o.op == SALVE_OP_AVGPOOL_FC) {
            st.kind = AVGPOOL_FC;
        } else if (!(flags & SALVE_RESNET_NO_STEM_FUSE) && stem_pool_fits(ops, n_ops, i, ktab, ktab_entries)) {   // else: the implicit-GEMM stem and the separate max-pool
            st.kind = STEM_POOL;
            st.count = 2;
        } else if ((form = block_form(ops, n_ops, i, flags)) >= 0) {
            st.kind = BOTTLENECK;
            st.form = form;
            st.count = 3;
            if (form == BLOCK_PLAIN && block_takes_next(ops, n_ops, i, flags)) {
                // If Y's only other readers, up to the buffer's next writer, are stride-2 projection shortcuts, only its even pixels are stored.
                const Op& c = ops[i + 2];
                st.form = BLOCK_NEXT;
                st.count = 4;
                st.y_even = !store_all && c.Ho == c.Wo && !(c.Ho & 1) && only_stride2_shortcuts_from(ops, n_ops, i + 4, c.out_buf, c.Ho, c.Wo);
            }
        } else if (!(flags & SALVE_RESNET_NO_CHAIN) && expand_fits(o)) {
            st.kind = EXPAND_CHAIN;
            st.chained = !(flags & SALVE_RESNET_CHAIN_EXPAND_ONLY) && expand_takes_next(ops, n_ops, i, flags);
            st.count = st.chained ? 2 : 1;
            const int midn = st.chained ? ops[i + 1].Cout : 0;
            st.form = chain_form(o.Cin, midn, st.chained, flags);
            // (r5) A chained block whose output Y is otherwise read only by a stride-2 projection shortcut (the last block of a stage: the
            // next block's first convolution is computed in the kernel, its shortcut samples Y at even rows and columns) stores only those
            // pixels: 3/4 of Y's bytes never cross HBM.  Every reader of the buffer up to its next writer is checked.
            st.y_even = st.chained && !store_all && o.Ho == o.Wo && !(o.Ho & 1) && midn != o.Cin &&   // expand_chain_kernel: YEVEN = MIDN != MID
                        only_stride2_shortcuts_from(ops, n_ops, i + 2, o.out_buf, o.Ho, o.Wo);
        } else {
            st.form = choose_wide(o, wide_mode);
            st.wide_auto = st.form == WIDE_8PHASE && wide_mode == WIDE_AUTO;
        }
        plan.push_back(st);
        i += st.count;
    }
    return plan;
}

// The one choice that depends on the batch: does this CONV step run its WIDE_* kernel, or conv_igemm_kernel?
// (The 256 x 256 tiles of the 8-phase kernel are a quarter as many workgroups, one per CU: small launches stay on
//  conv_igemm_kernel -- the results are bit-identical either way.)
// Measured on ResNet-50 (tools/measure/bench_resnet.py): +1 % for the whole forward at batch 4096, -1 % at 2048 and below
// (one workgroup per CU: a launch of fewer than six rounds loses more in its last round than the kernel gains).
static inline bool conv_runs_wide(const Step& st, const Op& o, int batch) {
    if (st.form == WIDE_OFF) return false;
    if (!st.wide_auto) return true;
    const long long M = (long long)batch * o.Ho * o.Wo;
    return ((M + 255) / 256) * (long long)(o.Cout / 256) >= 1536;
}

}  // namespace salve_plan
