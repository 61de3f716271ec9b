// bottleneck.h -- a whole 56 x 56 bottleneck block as ONE kernel, in its plain, projection (PROJ) and with-the-next-convolution (NEXT) forms
// (included by resnet.hip inside its namespace, behind the device helpers it shares with conv_igemm_kernel).
//
// One ResNet bottleneck block without down-sampling,  Y = relu(Wc . relu(Wb (*) relu(Wa . X + ba) + bb) + bc + X),
// in ONE kernel: the two intermediate tensors never leave LDS and X is read once (plus a 1-pixel halo) instead of twice.
// For the 56x56 and 28x28 stages the three convolutions are bound by activation traffic (3.3 GB per block and 512
// samples at 56x56); fused, the block moves 1.8 GB.
//
// A workgroup (4 waves) owns a tile of TH x 16 output pixels of one image:
//   GEMM 1  t1[halo pixel][MID]   = relu(X[halo pixel][4 MID] . Wa^T + ba), zero outside the image (that IS the 3x3
//           convolution's zero padding); halo = (TH+2) x 18 pixels, padded to M1 rows; K = 4 MID in k-tiles of 64;
//           operands staged by global_load_lds exactly as in conv_igemm_kernel; result to LDS (fp16, swizzled rows).
//   GEMM 2  t2[pixel][MID] = relu(sum over the 9 taps  t1[pixel + tap][MID] . Wb[tap]^T + bb): the A fragments are read
//           straight out of t1 -- the 16 pixels of a tile row are 16 consecutive halo rows --, Wb streams through LDS.
//   GEMM 3  Y[pixel][4 MID] = relu(t2 . Wc^T + bc + X[pixel]), 128 output channels at a time, epilogue through LDS with
//           16-byte coalesced residual loads and stores as in conv_igemm_kernel.
// MFMA operands are swapped (acc = W-fragment x A-fragment) so that a lane owns 4 consecutive channels of one pixel.
//
// TRANSPOSED TILES (r6).  A 56-pixel image row is 3.5 tiles of 16 columns: with four tile columns the fourth is half empty -- 28 tiles
// per image for 24.5 tiles' worth of pixels, an eighth of the block's three GEMMs multiplying rows that do not exist.  The strip of TH
// columns right of the last whole tile column is therefore covered by tiles of 16 rows x TH columns -- the SAME tile with the roles of
// row and column exchanged (tile pixel (r, c) is image pixel (oy0 + c, ox0 + r)); its halo is the same (TH + 2) x 18 pixels, every LDS
// offset, fragment read and counted wait stays where it is, and only the image addresses (GEMM 1's rows, the output stores) and the
// tap -> halo offset of GEMM 2 exchange their coordinates.  GEMM 2 still walks the taps in the IMAGE's (dy, dx) order, so the sums are
// the same sums in the same order: bit-identical to the three-kernel path.  56 x 56: 21 + 4 = 25 tiles per image instead of 28.
struct BottleneckArgs {
    const uint16_t* x;
    uint16_t* y;
    const uint16_t *wa, *wb, *wc;  // [MID][4 MID], [MID][3][3][MID], [4 MID][MID]  (BatchNorm folded, fp16)
    const float *ba, *bb, *bc;
    const uint16_t* zeros;
    int B, H, W, tiles_x, tiles_y;
    int tiles_t;      // transposed tiles per image (below): 0, or ceil(H / 16) tiles of 16 rows x TH columns for the strip right of tiles_x * 16
    // NEXT form (the last block of layer 1): the FOLLOWING block's first 1x1 convolution rides along as a fourth GEMM on the Y tile
    const uint16_t* wd;   // [MIDN][4 MID] fp16, BatchNorm folded
    const float* bd;
    uint16_t* t1n;        // [B, H, W, MIDN]
    int y_even;           // 1: only the pixels of Y with even row and column are stored (its one other reader samples it at stride 2)
    int32_t* status;
    int xcd_contig;   // 1: every XCD owns a contiguous range of tiles (xcd_linear), so the tiles of one image share an L2
};

constexpr int BN_THREADS = 512;  // 8 waves: two workgroups per CU give 4 waves per SIMD to hide the many short phases

// 16-byte store of an output that nobody reads before the next launch.  (Cache-policy bits on it -- sc1, nt, sc0 sc1, sc1 nt -- were
// timed in round 4 and change nothing; the timing-only builds of this file are tools/probe/ablations/timing_switches.patch.)
__device__ __forceinline__ void store16_stream(uint16_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

// PROJ: the first block of layer 1 -- its input has MID channels (not 4 MID) and its shortcut is a 1x1 projection, which rides
//       in GEMM 3 as MID more k: Y = relu([t2 | X] . [Wc | Ws]^T + (bc + bs)), the weight rows K-concatenated as the
//       three-kernel path stores them (conv1x1_with_shortcut), 64 output channels at a time.
// NEXT: the last block of a stage whose successor keeps the resolution in its first convolution (layer 1 -> layer 2: torchvision's v1.5
//       puts the stride on the 3x3) -- that convolution,  t1' = relu(Wd . Y + bd)  with MIDN = 2 MID output channels, is a FOURTH GEMM on
//       the Y tile while each 128-channel chunk of it sits in the staging tile (fp16, exactly the values the separate launch would read
//       back): K = 4 MID in the same ascending k-tiles of 64, so t1' is bit-identical to conv_igemm_kernel's; its accumulators live
//       across the two chunks, Wd streams through the Wc chunk's buffer (and, in the last chunk, through the dead t2).  Y itself is then
//       read from memory only by the next stage's stride-2 projection shortcut: with y_even only a quarter of it is stored.  Per 4096
//       samples that removes the launch that re-read Y (6.6 GB) to write t1' (3.3 GB), and 4.9 GB of Y's stores.
template <int MID, int TH, bool PROJ = false, bool NEXT = false>
__global__ __launch_bounds__(BN_THREADS, 4) void bottleneck_kernel(BottleneckArgs p) {
    static_assert(!NEXT || (!PROJ && MID == 64 && TH == 8), "the NEXT form is written for the plain 64-channel block");
    constexpr int C4 = 4 * MID;
    constexpr int CIN = PROJ ? MID : C4;   // channels of the block's input
    constexpr int HC = 18, HALO = (TH + 2) * HC;
    constexpr int M1 = (HALO + 63) / 64 * 64;   // GEMM-1 rows (halo pixels, zero padded): 192 (TH 8) / 128 (TH 4)
    constexpr int MT1 = M1 / 64;                // GEMM 1: 16-row tiles per wave (4 wave rows x 2 wave columns)
    constexpr int NT1 = MID / 32;               // GEMM 1: 16-channel tiles per wave
    constexpr int MO = TH * 16;                 // output pixels of the tile
    constexpr int RT = TH / 4;                  // GEMM 2/3: 16-pixel row tiles per wave (4 wave rows x 2 wave columns)
    constexpr int NT2 = MID / 32;               // GEMM 2: 16-channel tiles per wave (2 wave columns)
    constexpr int KT_MID = MID / 64;            // k-tiles of 64 in MID
    constexpr int LDC = 128 + 8;
    constexpr int STAGE_TILES = MID == 64 ? 3 : 1;  // GEMM 2: 64-deep Wb tiles per stage (MID 64: a whole kernel row)
    // LDS map (uint16 elements); every phase double-buffers its streamed operand inside the same 72 KB:
    //   GEMM 1   stage s at [s * ST1_E, ...): X tile (M1 x 64) + Wa tile (MID x 64)
    //   t1       [0, T1_E)                           written after GEMM 1's last barrier
    //   GEMM 2   Wb stage s at [T1_E + s * BSB_E, ...)
    //   t2       [0, T2_E)                           written after GEMM 2's last barrier (t1 is dead)
    //   GEMM 3   Wc chunk at [T2_E, ...), output staging behind it
    constexpr int ST1_E = (M1 + MID) * 64;
    constexpr int T1_E = M1 * MID, T2_E = MO * MID;
    constexpr int BSB_E = STAGE_TILES * MID * 64;
    constexpr int BSC_E = 128 * MID, CS_E = MO * LDC;
    constexpr int LDC_P = 64 + 8;                                           // PROJ: 64 output channels per chunk
    constexpr int EC_P = T2_E + MO * 64 + 64 * (MID + CIN) + MO * LDC_P;    // PROJ: t2 | X centre tile | weight chunk | staging
    constexpr int EA = 2 * ST1_E, EB = T1_E + 2 * BSB_E, EC = PROJ ? EC_P : T2_E + BSC_E + CS_E;
    constexpr int SMEM_E = EA > EB ? (EA > EC ? EA : EC) : (EB > EC ? EB : EC);
    __shared__ __attribute__((aligned(1024))) uint16_t smem[SMEM_E];
    uint16_t* T1 = smem;
    uint16_t* T2 = smem;
    uint16_t* BsB = smem + T1_E;
    uint16_t* BsC = smem + T2_E;
    uint16_t* Cs = BsC + BSC_E;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: LDS-DMA bases need no per-load readfirstlane
    const int wr = wave >> 1, wc = wave & 1;   // GEMM 2 / 3
    const int wm = wave & 3, wn = wave >> 2;   // GEMM 1
    const int t = xcd_linear(blockIdx.x, gridDim.x, p.xcd_contig);
    const int n_upright = p.tiles_x * p.tiles_y, per_image = n_upright + p.tiles_t;
    const int b = t / per_image, kt_img = t % per_image;
    const bool TR = kt_img >= n_upright;   // a transposed tile: 16 image rows x TH image columns (workgroup-uniform)
    const int oy0 = TR ? (kt_img - n_upright) * 16 : (kt_img / p.tiles_x) * TH;
    const int ox0 = TR ? p.tiles_x * 16 : (kt_img % p.tiles_x) * 16;
    // tile pixel (r, c) -> image pixel
    auto img_y = [&](int r, int c) { return oy0 + (TR ? c : r); };
    auto img_x = [&](int r, int c) { return ox0 + (TR ? r : c); };
    const uint16_t* ximg = p.x + (long long)b * p.H * p.W * CIN;
    const int frag_row = lane & 15, frag_q = lane >> 4;
    const int row_base = tid >> 3;
    const int chunk = (tid & 7) ^ ((row_base >> 1) & 7);   // source-side swizzle, as in conv_igemm_kernel
    float amax = 0.f;

    // Wb stage `st` -> buffer st & 1 (6 or 8 loads per thread)
#define ISSUE_WB(ST)                                                                                                   \
    {                                                                                                                  \
        _Pragma("unroll") for (int q = 0; q < STAGE_TILES; q++) {                                                      \
            const int ktile_ = (ST) * STAGE_TILES + q;                                                                 \
            _Pragma("unroll") for (int j = 0; j < MID / 64; j++)                                                       \
                __builtin_amdgcn_global_load_lds(                                                                      \
                    (global_cptr)(p.wb + (long long)(row_base + 64 * j) * (9 * MID) + ktile_ * 64 + chunk * 8),        \
                    (lds_ptr)(BsB + ((ST) & 1) * BSB_E + q * MID * 64 + (wave * 8 + 64 * j) * 64), 16, 0, 0);          \
        }                                                                                                              \
    }
    constexpr int WB_LOADS = STAGE_TILES * (MID / 64);

    // The residual of GEMM 3 is the block's own input at the output pixels -- a subset of the halo tile GEMM 1 streams through
    // LDS.  Each thread copies the 8-byte pieces its GEMM-3 accumulators will need (pixel rows wr * RT + i, the 16 channels per
    // accumulator tile of wave column wc: k-tile kt serves the waves with wc == (kt & 1), chunk nc = kt >> 1) out of the
    // stage buffers into registers while the tile is there: 32 VGPRs instead of a second trip to memory for 64 KB per tile
    // (round 3, PMC: the re-read came from beyond the L2 and was 30 % of the kernel's HBM traffic).
    uint2 resid[PROJ ? 1 : C4 / 128][RT][4];
    int res_off[RT];   // element offset of the pixel's row in a stage buffer, and its swizzle
    int res_swz[RT];
#pragma unroll
    for (int i = 0; i < RT; i++) {
        const int m = (wr * RT + i) * 16 + frag_row;
        const int h = ((m >> 4) + 1) * HC + (m & 15) + 1;
        res_off[i] = h * 64 + 4 * (frag_q & 1);
        res_swz[i] = (h >> 1) & 7;
    }

    // ------------------------------------------------------------------ GEMM 1: t1 = relu(Xhalo . Wa^T + ba)
    {
        const uint16_t* rowp[M1 / 64];
#pragma unroll
        for (int i = 0; i < M1 / 64; i++) {
            const int h = row_base + 64 * i;
            const int hy = img_y(h / HC - 1, h % HC - 1), hx = img_x(h / HC - 1, h % HC - 1);
            const bool ok = h < HALO && hy >= 0 && hy < p.H && hx >= 0 && hx < p.W;
            rowp[i] = ok ? ximg + ((long long)hy * p.W + hx) * CIN + chunk * 8 : nullptr;
        }
        const uint16_t* wrow = p.wa + (long long)row_base * CIN + chunk * 8;
        constexpr int A_LOADS = M1 / 64 + MID / 64;
#define ISSUE_A(KT)                                                                                                    \
    {                                                                                                                  \
        uint16_t* As_ = smem + ((KT) & 1) * ST1_E;                                                                     \
        _Pragma("unroll") for (int i = 0; i < M1 / 64; i++) {                                                          \
            const uint16_t* src = rowp[i] ? rowp[i] + (KT) * 64 : p.zeros;                                             \
            __builtin_amdgcn_global_load_lds((global_cptr)src, (lds_ptr)(As_ + (wave * 8 + 64 * i) * 64), 16, 0, 0);   \
        }                                                                                                              \
        _Pragma("unroll") for (int j = 0; j < MID / 64; j++)                                                           \
            __builtin_amdgcn_global_load_lds((global_cptr)(wrow + (long long)j * 64 * CIN + (KT) * 64),                \
                                             (lds_ptr)(As_ + M1 * 64 + (wave * 8 + 64 * j) * 64), 16, 0, 0);           \
    }
        f32x4 acc[MT1][NT1];
#pragma unroll
        for (int i = 0; i < MT1; i++)
#pragma unroll
            for (int j = 0; j < NT1; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        constexpr int NK1 = CIN / 64;
        ISSUE_A(0);
        // (Round 3: touching the later k-tiles' lines up front -- one 4-byte LDS-DMA lane per 128-byte line into scratch LDS, so
        // that the stages after the first hit the L2 -- measured +1 % on the forward: the phases are not waiting for those lines.)
#pragma unroll
        for (int kt = 0; kt < NK1; kt++) {
            // the next tile goes into the other buffer (last read one iteration ago, behind a barrier) and stays in
            // flight under this tile's MFMAs: counted wait, raw barriers (a __syncthreads() would drain it)
            if (kt + 1 < NK1) {
                ISSUE_A(kt + 1);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LOADS) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_barrier" ::: "memory");
            const uint16_t* As = smem + (kt & 1) * ST1_E;
            const uint16_t* BsA = As + M1 * 64;
            if constexpr (!PROJ) {
                if (wc == (kt & 1)) {
#pragma unroll
                    for (int i = 0; i < RT; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            resid[kt >> 1][i][j] = lds_read8(As + res_off[i] + (((2 * j + (frag_q >> 1)) ^ res_swz[i]) << 3));   // (typed so that no vmcnt(0) lands in front of it: the next k-tile is in flight)
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const int slot = ((ks * 4 + frag_q) ^ ((frag_row >> 1) & 7)) * 8;
                act8 af[MT1], bfr[NT1];
#pragma unroll
                for (int i = 0; i < MT1; i++)
                    af[i] = *reinterpret_cast<const act8*>(As + ((wm * MT1 + i) * 16 + frag_row) * 64 + slot);
#pragma unroll
                for (int j = 0; j < NT1; j++)
                    bfr[j] = *reinterpret_cast<const act8*>(BsA + ((wn * NT1 + j) * 16 + frag_row) * 64 + slot);
#pragma unroll
                for (int i = 0; i < MT1; i++)
#pragma unroll
                    for (int j = 0; j < NT1; j++)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc[i][j], 0, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");  // everyone is done reading this buffer
        }
#undef ISSUE_A
        ISSUE_WB(0);  // first Wb stage: lands while t1 is written (its buffer is behind t1)
        // t1 rows: MID halves = MID / 8 chunks of 16 bytes, chunk q of row h stored at slot q ^ swz(h)
#pragma unroll
        for (int i = 0; i < MT1; i++) {
            const int h = (wm * MT1 + i) * 16 + frag_row;
            const int hy = img_y(h / HC - 1, h % HC - 1), hx = img_x(h / HC - 1, h % HC - 1);
            const bool inside = h < HALO && hy >= 0 && hy < p.H && hx >= 0 && hx < p.W;
            const uint32_t keep = inside ? 0xFFFFFFFFu : 0u;   // (a mask, not a select around the conversions: hipcc made branches of those)
            const int swz = MID == 64 ? ((h >> 1) & 7) : (h & 15);
#pragma unroll
            for (int j = 0; j < NT1; j++) {
                const int c0 = (wn * NT1 + j) * 16 + 4 * frag_q;
                const float4 bias = *reinterpret_cast<const float4*>(p.ba + c0);
                uint2 o = pack4<true>(amax, acc[i][j] + vec4(bias));
                o.x &= keep; o.y &= keep;
                *reinterpret_cast<uint2*>(T1 + h * MID + (((c0 >> 3) ^ swz) << 3) + (c0 & 7)) = o;
            }
        }
    }

    // ------------------------------------------------------------------ GEMM 2: t2 = relu(3x3(t1) . Wb + bb)
    {
        f32x4 acc[RT][NT2];
#pragma unroll
        for (int i = 0; i < RT; i++)
#pragma unroll
            for (int j = 0; j < NT2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        constexpr int N_STAGES = 9 * KT_MID / STAGE_TILES;
        for (int st = 0; st < N_STAGES; st++) {
            if (st + 1 < N_STAGES) {
                ISSUE_WB(st + 1);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WB_LOADS) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (first stage: this wave's t1 stores)
            asm volatile("s_barrier" ::: "memory");
            const uint16_t* Bst = BsB + (st & 1) * BSB_E;
#pragma unroll
            for (int q = 0; q < STAGE_TILES; q++) {
                const int ktile = st * STAGE_TILES + q;
                const int tap = ktile / KT_MID, kh = ktile % KT_MID;  // kh: which 64 channels of t1
                const int dy = tap / 3, dx = tap % 3;
                const int ro = TR ? dx : dy, co = TR ? dy : dx;   // the tap's offset in TILE rows / columns (transposed tiles: exchanged)
#pragma unroll
                for (int ks = 0; ks < 2; ks++) {
                    act8 af[RT], bfr[NT2];
#pragma unroll
                    for (int i = 0; i < RT; i++) {
                        const int h = (wr * RT + i + ro) * HC + co + frag_row;
                        const int swz = MID == 64 ? ((h >> 1) & 7) : (h & 15);
                        af[i] = *reinterpret_cast<const act8*>(T1 + h * MID + (((kh * 8 + ks * 4 + frag_q) ^ swz) << 3));
                    }
                    const int slot = ((ks * 4 + frag_q) ^ ((frag_row >> 1) & 7)) * 8;
#pragma unroll
                    for (int j = 0; j < NT2; j++)
                        bfr[j] = *reinterpret_cast<const act8*>(Bst + q * MID * 64 + ((wc * NT2 + j) * 16 + frag_row) * 64 + slot);
#pragma unroll
                    for (int i = 0; i < RT; i++)
#pragma unroll
                        for (int j = 0; j < NT2; j++)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < RT; i++) {
            const int m = (wr * RT + i) * 16 + frag_row;  // output pixel of the tile, row-major
            const int swz = MID == 64 ? ((m >> 1) & 7) : (m & 15);
#pragma unroll
            for (int j = 0; j < NT2; j++) {
                const int c0 = (wc * NT2 + j) * 16 + 4 * frag_q;
                const float4 bias = *reinterpret_cast<const float4*>(p.bb + c0);
                *reinterpret_cast<uint2*>(T2 + m * MID + (((c0 >> 3) ^ swz) << 3) + (c0 & 7)) =
                    pack4<true>(amax, acc[i][j] + vec4(bias));
            }
        }
    }
#undef ISSUE_WB

    // ------------------------------------------------------------------ GEMM 3 (PROJ): Y = relu([t2 | X] . [Wc | Ws]^T + b)
    if constexpr (PROJ) {
        static_assert(!PROJ || MID == 64, "the projection variant is written for 64 mid channels");
        constexpr int KP = MID + CIN;               // 128: k-tile 0 = t2, k-tile 1 = the block's input at the output pixels
        uint16_t* Xc = smem + T2_E;                 // [MO][64], staged like a GEMM-1 tile (chunk q of row r at q ^ ((r >> 1) & 7))
        uint16_t* Wp = Xc + MO * 64;                // weight chunk: two tiles of 64 rows x 64 k
        uint16_t* Cp = Wp + 64 * KP;                // output staging [MO][LDC_P]
        constexpr int CH_PER_ROW = 64 / 8;
        constexpr int C_ITERS = (MO * CH_PER_ROW) / BN_THREADS;
#pragma unroll
        for (int i = 0; i < MO / 64; i++) {         // X centre tile (L2: GEMM 1 has just read it), lands with the first weights
            const int r = row_base + 64 * i;
            const int oy = img_y(r >> 4, r & 15), ox = img_x(r >> 4, r & 15);
            const uint16_t* src = (ox < p.W && oy < p.H) ? ximg + ((long long)oy * p.W + ox) * CIN + chunk * 8 : p.zeros;
            __builtin_amdgcn_global_load_lds((global_cptr)src, (lds_ptr)(Xc + (wave * 8 + 64 * i) * 64), 16, 0, 0);
        }
        for (int nc = 0; nc < C4 / 64; nc++) {
#pragma unroll
            for (int q = 0; q < KP / 64; q++)
                __builtin_amdgcn_global_load_lds((global_cptr)(p.wc + (long long)(nc * 64 + row_base) * KP + q * 64 + chunk * 8),
                                                 (lds_ptr)(Wp + q * 64 * 64 + (wave * 8) * 64), 16, 0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // (first chunk: also orders the t2 stores)
            f32x4 acc[RT][2];
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < KP / 64; q++)
#pragma unroll
                for (int ks = 0; ks < 2; ks++) {
                    act8 af[RT], bfr[2];
                    const uint16_t* A = q == 0 ? T2 : Xc;
#pragma unroll
                    for (int i = 0; i < RT; i++) {
                        const int m = (wr * RT + i) * 16 + frag_row;
                        af[i] = *reinterpret_cast<const act8*>(A + m * 64 + (((ks * 4 + frag_q) ^ ((m >> 1) & 7)) << 3));
                    }
                    const int slot = ((ks * 4 + frag_q) ^ ((frag_row >> 1) & 7)) * 8;
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        bfr[j] = *reinterpret_cast<const act8*>(Wp + q * 64 * 64 + ((wc * 2 + j) * 16 + frag_row) * 64 + slot);
#pragma unroll
                    for (int i = 0; i < RT; i++)
#pragma unroll
                        for (int j = 0; j < 2; j++)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int ncol = (wc * 2 + j) * 16 + 4 * frag_q;
                const float4 bias = *reinterpret_cast<const float4*>(p.bc + nc * 64 + ncol);
#pragma unroll
                for (int i = 0; i < RT; i++) {
                    const int m = (wr * RT + i) * 16 + frag_row;
                    *reinterpret_cast<uint2*>(Cp + m * LDC_P + ncol) =
                        pack4<true>(amax, acc[i][j] + vec4(bias));
                }
            }
            __syncthreads();
            uint16_t* yimg = p.y + (long long)b * p.H * p.W * C4;
#pragma unroll
            for (int it = 0; it < C_ITERS; it++) {
                const int id = tid + it * BN_THREADS;
                const int m = id / CH_PER_ROW, ch = id % CH_PER_ROW;
                const int oy = img_y(m >> 4, m & 15), ox = img_x(m >> 4, m & 15);
                if (ox < p.W && oy < p.H)
                    store16_stream(yimg + ((long long)oy * p.W + ox) * C4 + nc * 64 + ch * 8, *reinterpret_cast<const uint4*>(Cp + m * LDC_P + ch * 8));
            }
            __syncthreads();  // staging and weight chunk are reused by the next chunk
        }
    } else
    // ------------------------------------------------------------------ GEMM 3: Y = relu(t2 . Wc^T + bc + X)   (+ NEXT: GEMM 4 on Y)
    {
        constexpr int CH_PER_ROW = 128 / 8;
        constexpr int C_ITERS = (MO * CH_PER_ROW) / BN_THREADS;
        constexpr int MIDN = 2 * MID;                        // NEXT: output channels of the following block's first convolution (128)
        f32x4 acc4[NEXT ? RT : 1][NEXT ? MIDN / 32 : 1];     // NEXT: t1' accumulators, 16 pixels x 16 channels each, alive across both chunks
        // NEXT: Wd k-tile KT (MIDN rows x 64 k of the [MIDN][4 MID] matrix) -> DST, laid out like a Wc tile (128 rows x 128 bytes, source-side swizzle)
#define ISSUE_WD(KT, DST)                                                                                              \
    {                                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < MIDN / 64; j++)                                                          \
            __builtin_amdgcn_global_load_lds((global_cptr)(p.wd + (long long)(row_base + 64 * j) * C4 + (KT) * 64 + chunk * 8), \
                                             (lds_ptr)((DST) + (wave * 8 + 64 * j) * 64), 16, 0, 0);                   \
    }
        // NEXT: one k-tile of GEMM 4: A = 64 channels of the Y chunk in the staging tile (rows of LDC halves), B = a Wd tile
#define GEMM4_KTILE(ACOL, BT)                                                                                          \
    {                                                                                                                  \
        _Pragma("unroll") for (int ks = 0; ks < 2; ks++) {                                                             \
            act8 af[RT], bfr[MIDN / 32];                                                                               \
            _Pragma("unroll") for (int i = 0; i < RT; i++)                                                             \
                af[i] = *reinterpret_cast<const act8*>(Cs + ((wr * RT + i) * 16 + frag_row) * LDC + (ACOL) + ks * 32 + frag_q * 8); \
            const int slot = ((ks * 4 + frag_q) ^ ((frag_row >> 1) & 7)) * 8;                                          \
            _Pragma("unroll") for (int j = 0; j < MIDN / 32; j++)                                                      \
                bfr[j] = *reinterpret_cast<const act8*>((BT) + ((wc * (MIDN / 32) + j) * 16 + frag_row) * 64 + slot);  \
            _Pragma("unroll") for (int i = 0; i < RT; i++)                                                             \
                _Pragma("unroll") for (int j = 0; j < MIDN / 32; j++)                                                  \
                    acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc4[i][j], 0, 0, 0);          \
        }                                                                                                              \
    }
#pragma unroll
        for (int nc = 0; nc < C4 / 128; nc++) {
            // Wc chunk: 128 output channels x MID, as KT_MID tiles of 128 rows x 64
#pragma unroll
            for (int q = 0; q < KT_MID; q++)
#pragma unroll
                for (int j = 0; j < 2; j++)
                    __builtin_amdgcn_global_load_lds((global_cptr)(p.wc + (long long)(nc * 128 + row_base + 64 * j) * MID + q * 64 + chunk * 8),
                                                     (lds_ptr)(BsC + q * 128 * 64 + (wave * 8 + 64 * j) * 64), 16, 0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // (first chunk: also orders the t2 stores)
            // (NEXT: the chunk in two passes of 64 channels -- 16 accumulator registers next to the 32 of GEMM 4 and the residual's; in one
            //  pass the kernel needs 50 registers more than the 128 that four waves per SIMD leave, and a scratch reload is a vmcnt load
            //  queued behind the LDS-DMA stages)
            constexpr int NH = NEXT ? 2 : 1, JN = 4 / NH;
#pragma unroll
            for (int hf = 0; hf < NH; hf++) {
                f32x4 acc[RT][JN];
#pragma unroll
                for (int i = 0; i < RT; i++)
#pragma unroll
                    for (int j = 0; j < JN; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < KT_MID; q++)
#pragma unroll
                    for (int ks = 0; ks < 2; ks++) {
                        act8 af[RT], bfr[JN];
#pragma unroll
                        for (int i = 0; i < RT; i++) {
                            const int m = (wr * RT + i) * 16 + frag_row;
                            const int swz = MID == 64 ? ((m >> 1) & 7) : (m & 15);
                            af[i] = *reinterpret_cast<const act8*>(T2 + m * MID + (((q * 8 + ks * 4 + frag_q) ^ swz) << 3));
                        }
                        const int slot = ((ks * 4 + frag_q) ^ ((frag_row >> 1) & 7)) * 8;
#pragma unroll
                        for (int j = 0; j < JN; j++)
                            bfr[j] = *reinterpret_cast<const act8*>(BsC + q * 128 * 64 + ((wc * 4 + hf * JN + j) * 16 + frag_row) * 64 + slot);
#pragma unroll
                        for (int i = 0; i < RT; i++)
#pragma unroll
                            for (int j = 0; j < JN; j++)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                    }
                if constexpr (NEXT) {
                    if (hf == NH - 1) {
                        // everyone is done with the Wc chunk (and, in the last chunk, with t2): the first Wd k-tile of this chunk lands in the Wc
                        // buffer while the epilogue below runs; the last chunk brings both of its k-tiles, the second into the dead t2
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        asm volatile("s_barrier" ::: "memory");
                        ISSUE_WD(2 * nc, BsC);
                        if (nc == C4 / 128 - 1) ISSUE_WD(2 * nc + 1, T2);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < JN; jj++) {
                    const int j = hf * JN + jj;
                    const int ncol = (wc * 4 + j) * 16 + 4 * frag_q;
                    const float4 bias = *reinterpret_cast<const float4*>(p.bc + nc * 128 + ncol);
#pragma unroll
                    for (int i = 0; i < RT; i++) {
                        const int m = (wr * RT + i) * 16 + frag_row;
                        const uint2 r = resid[nc][i][j];   // (a pixel beyond the image's right edge holds zeros: its halo row was the zero page)
                        const uint2 o = pack4<true>(amax, acc[i][jj] + vec4(bias) + vec4(r));
                        if constexpr (NEXT) lds_write8(Cs + m * LDC + ncol, o);   // (typed: no compiler vmcnt(0) in front of it -- the Wd tile is in flight)
                        else *reinterpret_cast<uint2*>(Cs + m * LDC + ncol) = o;
                    }
                }
            }
            if constexpr (NEXT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of the Wd tile(s)
            __syncthreads();
            uint16_t* yimg = p.y + (long long)b * p.H * p.W * C4;
            int tl = tid;
            if constexpr (NEXT) asm volatile("" : "+v"(tl));   // (opaque: the store addresses are computed HERE, not hoisted above GEMM 1 and kept in registers -- or scratch -- across the kernel)
#pragma unroll
            for (int it = 0; it < C_ITERS; it++) {
                const int id = tl + it * BN_THREADS;
                const int m = id / CH_PER_ROW, ch = id % CH_PER_ROW;
                const int oy = img_y(m >> 4, m & 15), ox = img_x(m >> 4, m & 15);
                bool keep = ox < p.W && oy < p.H;
                if constexpr (NEXT) keep = keep && (!p.y_even || (((oy | ox) & 1) == 0));
                if (keep)
                    store16_stream(yimg + ((long long)oy * p.W + ox) * C4 + nc * 128 + ch * 8, *reinterpret_cast<const uint4*>(Cs + m * LDC + ch * 8));
            }
            if constexpr (NEXT) {
                if (nc == 0) {   // (zeroed here, not in front of the chunk loop: 32 registers that are not live through the first chunk's GEMM 3)
#pragma unroll
                    for (int i = 0; i < RT; i++)
#pragma unroll
                        for (int j = 0; j < MIDN / 32; j++) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                GEMM4_KTILE(0, BsC);
                if (nc == C4 / 128 - 1) {
                    GEMM4_KTILE(64, T2);
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    asm volatile("s_barrier" ::: "memory");   // everyone is done with the first Wd k-tile
                    ISSUE_WD(2 * nc + 1, BsC);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    asm volatile("s_barrier" ::: "memory");
                    GEMM4_KTILE(64, BsC);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __syncthreads();  // staging and Wc tile are reused by the next chunk
        }
        if constexpr (NEXT) {
            // t1' = relu(acc4 + bd): through the staging tile (free now), then 16-byte coalesced stores of whole 256-byte pixel rows
#pragma unroll
            for (int j = 0; j < MIDN / 32; j++) {
                const int ncol = (wc * (MIDN / 32) + j) * 16 + 4 * frag_q;
                const float4 bias = *reinterpret_cast<const float4*>(p.bd + ncol);
#pragma unroll
                for (int i = 0; i < RT; i++) {
                    const int m = (wr * RT + i) * 16 + frag_row;
                    *reinterpret_cast<uint2*>(Cs + m * LDC + ncol) = pack4<true>(amax, acc4[i][j] + vec4(bias));
                }
            }
            __syncthreads();
            uint16_t* timg = p.t1n + (long long)b * p.H * p.W * MIDN;
            constexpr int CPR = MIDN / 8;
            int tl = tid;
            asm volatile("" : "+v"(tl));
#pragma unroll
            for (int it = 0; it < (MO * CPR) / BN_THREADS; it++) {
                const int id = tl + it * BN_THREADS;
                const int m = id / CPR, ch = id % CPR;
                const int oy = img_y(m >> 4, m & 15), ox = img_x(m >> 4, m & 15);
                if (ox < p.W && oy < p.H)
                    store16_stream(timg + ((long long)oy * p.W + ox) * MIDN + ch * 8, *reinterpret_cast<const uint4*>(Cs + m * LDC + ch * 8));
            }
        }
#undef ISSUE_WD
#undef GEMM4_KTILE
    }
    report_range(p.status, amax);
}
