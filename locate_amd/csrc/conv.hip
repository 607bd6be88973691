// Dense contractions of the LocAtE hot path as LDS-tiled implicit GEMMs on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32, 157 TFLOP/s dense peak on MI355X).  No im2col buffer is ever
// materialised: the activation operand is gathered straight from NCHW into LDS.
//
// Everything is expressed through ONE regular convolution R
//     out[b, m, oh, ow] = sum_{c, kh, kw} w[m, c, kh, kw] * in[b, c, oh*s - ph + kh, ow*s - pw + kw]
// and its two adjoints:
//     locate_conv_fwd    R            Conv2d / Conv1d(k=1) / Linear forward  (reference libs/conv.py:14-20,
//                                     attention.py:18-46, scale.py:25-34, linear.py:10); ConvTranspose2d dgrad
//     locate_conv_dgrad  R^T (data)   Conv2d dgrad; ConvTranspose2d FORWARD (conv.py:49-52: both convs of a
//                                     transposed stage are ConvTranspose2d, weights [C_in, C_out, k, k])
//     locate_conv_wgrad  R^T (weight) weight gradient of either (roles of the two activations swapped by the
//                                     caller for the transposed case): convwgrad.hip
// A stride-s adjoint is decomposed into s*s sub-pixel phases, each a stride-1 gather with its own tap subset
// (4x4 s2 p1 ConvTranspose = four 2x2 convolutions; 5x5 s2 p2 dgrad = 3x3 + 3x2 + 2x3 + 2x2 taps).
//
// The weight operand is re-laid out once per weight update into a K-major [Kpad][Mpad] panel (zero padded;
// the packing kernels are in convpack.hip, this file plans the panels: conv_plan);
// the spectral-norm factor 1/sigma multiplies the accumulator in the epilogue (reference
// libs/spectral_norm.py:31-32 materialises W_bar/sigma as a separate full-size tensor on every forward).
//
// Tiling: 256 threads = 4 waves, block tile BM x 128 (BM in {128, 96, 64, 32}), K step 16, double-buffered
// LDS with register prefetch of the next K step, one barrier per step.
#include "igemm.h"

template <int WGM, int WGN, int TM, int TN>
__global__ void __launch_bounds__(256) conv_igemm_kernel(const IgParams p) {
    constexpr int BK = IG_BK;
    constexpr int BM = WGM * TM * 32;
    constexpr int BN = WGN * TN * 32;
    constexpr int KPT = BK * BN / 256;                // gathered elements per thread per K step
    constexpr int A_F4 = BK * BM / 4;                 // float4 per A tile
    constexpr int A_PT = (A_F4 + 255) / 256;
    static_assert(WGM * WGN == 4, "four waves");
    static_assert(BN % 64 == 0 && KPT == 8, "one 8-row group of the offset table per thread and step");
    static_assert(BK <= IG_TAIL, "panel tail shorter than the prefetch distance (one stage beyond the last)");

    __shared__ __attribute__((aligned(16))) float As[2][BK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];

    int bx, by, bz;
    xcd_tile(bx, by, bz, p.tile_nphase);
    const int zphase = bz / p.ksplit, zsplit = bz - zphase * p.ksplit;
    const IgPhase& ph = p.ph[zphase];
    const int N = p.B * ph.QH * ph.QW;
    const int n0 = bx * BN;
    const int m0 = by * BM;
    if (n0 >= N) return;   // phases can have different extents; uniform per block

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;

    // ---- per-thread gather column (fixed for the whole K loop): base pointer and the set of taps inside the input
    const int ncol = tid % BN;
    const int kgrp = __builtin_amdgcn_readfirstlane(tid / BN);   // wave-uniform
    const GatherCol gc = gather_setup(p, ph, n0 + ncol, N);
    float col_scale[TN];
    igemm_col_scales<WGM, WGN, TM, TN>(p, ph, col_scale, N, n0, wn, lane);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // ---- K range of this block (split-K) and the running addresses of its prefetch
    const int total_steps = ph.Kpad / BK;
    const int per_split = (total_steps + p.ksplit - 1) / p.ksplit;
    const int step0 = zsplit * per_split;
    int nsteps = total_steps - step0;
    if (nsteps > per_split) nsteps = per_split;
    if (nsteps < 0) nsteps = 0;

    const float4* aptr[A_PT];      // weight-panel rows: advance BK rows per step; the panel has IG_TAIL spare rows
    bool a_ok[A_PT];
    int a_row[A_PT], a_c4[A_PT];
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
        const int idx = tid + i * 256;
        const int idc = ((i + 1) * 256 <= A_F4 || idx < A_F4) ? idx : 0;
        a_row[i] = idc / (BM / 4);
        a_c4[i] = idc - a_row[i] * (BM / 4);
        const int col = m0 + a_c4[i] * 4;
        a_ok[i] = col < ph.ld;
        aptr[i] = reinterpret_cast<const float4*>(ph.wp + (long long)(step0 * BK + a_row[i]) * ph.ld + (a_ok[i] ? col : 0));
    }
    const long long a_step = (long long)BK * ph.ld / 4;            // float4 units
    int kidx = step0 * BK + kgrp * KPT;                           // wave-uniform first table row of the next load

    float breg[KPT];
    float4 areg[A_PT];
    auto issue_loads = [&]() {
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            areg[i] = *aptr[i];
            aptr[i] += a_step;
        }
        const int ks = __builtin_amdgcn_readfirstlane(kidx);
        const i32x8 offs = *reinterpret_cast<const i32x8*>(ph.koff + ks);                      // s_load_dwordx8
        const unsigned long long taps = *reinterpret_cast<const unsigned long long*>(ph.ktap + ks);   // s_load_dwordx2
#pragma unroll
        for (int j = 0; j < KPT; ++j) breg[j] = gather_load(gc, offs[j], (unsigned)(taps >> (8 * j)) & 31u);
        kidx += BK;
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PT; ++i) {
            const int idx = tid + i * 256;
            if ((i + 1) * 256 <= A_F4 || idx < A_F4) {
                float4 v = areg[i];
                v.x = a_ok[i] ? v.x : 0.f; v.y = a_ok[i] ? v.y : 0.f; v.z = a_ok[i] ? v.z : 0.f; v.w = a_ok[i] ? v.w : 0.f;
                *reinterpret_cast<float4*>(&As[buf][a_row[i]][a_c4[i] * 4]) = v;
            }
        }
#pragma unroll
        for (int j = 0; j < KPT; ++j) Bs[buf][kgrp * KPT + j][ncol] = breg[j];
    };

    if (nsteps > 0) {
        issue_loads();
        store_tiles(0);
    }
    __syncthreads();
    const int lrow = lane >> 5, lcol = lane & 31;
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        // One basic block per iteration: the loads of step s+1 first (pinned by the fence), the MFMAs of step s, the
        // LDS writes of step s+1, one barrier.  The last iteration's prefetch is redundant but branch-free (zero tail
        // rows of the panel and of the offset table).
        issue_loads();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k2 = 0; k2 < BK / 2; ++k2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf][k2 * 2 + lrow][(wm * TM + i) * 32 + lcol];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[buf][k2 * 2 + lrow][(wn * TN + j) * 32 + lcol];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        store_tiles(buf ^ 1);
        __syncthreads();
    }

    igemm_epilogue<WGM, WGN, TM, TN>(p, ph, acc, col_scale, N, n0, m0, zsplit, wm, wn, lane, nullptr, p.ksplit > 1);
}

// ---------------------------------------------------------------------------------------------
// "bf16 x 6": the same GEMM with BOTH operands split into three bf16 pieces x = h + m + l (exact: 3 x 8 significant
// bits cover fp32's 24) and the six products of combined order <= 2^-16 kept: h*h, h*m, m*h, m*m, h*l, l*h.  The
// dropped m*l, l*m, l*l terms are O(2^-24) of the product - fp32-level accuracy (the results agree with the fp32
// MFMA path to summation order) at 192 instead of 512 matrix-core cycles per 32x32x16 slice.  The weights are split once
// per optimizer step (panel planes w3), the gathered activations while their tile is written to LDS.
// LDS images are [piece][k / 8][column][8 bf16]: one ds_read_b128 per lane delivers an MFMA fragment (lane (r, h)
// holds k = 8h .. 8h + 7 of row / column r), one ds_write_b128 per gathered fragment, conflict-free both ways.
// ---------------------------------------------------------------------------------------------
#define B6_BK 16

// NP = 3: the exact three-piece form above.  NP = 1: "bf16 operands" - both operands rounded (to nearest even) to ONE bf16
// piece, one MFMA per slice, fp32 accumulation: the precision of a bf16 mixed-precision training step (BASELINE configs[1]),
// a third of the LDS traffic and a sixth of the matrix work.  Storage stays fp32 on both sides of the kernel.
// NW = 8: eight waves on the same 128-column tile with K steps of 32 - every thread still gathers ONE fragment per stage, so a
// stage covers twice the reduction depth at the same per-thread work, each wave owns half the rows of a four-wave tile, and two
// waves per SIMD cover each other's waits: for launches that cannot put more than one block on a CU anyway (mid-sized layers:
// a hundred-odd tiles), where a lone four-wave block walks its K loop at ~1.2 us per 16-deep stage.
// Resident blocks per CU: one eight-wave block; two of the tall tiles; FOUR of the 96 x 128 and 64 x 128 two-piece tiles (117 - 128 VGPRs, at most 8 bytes of
// scratch: the 96-channel stage is 2048 blocks of 24 short K steps - more waves in flight are worth more there than registers:
// 0.108 - 0.112 -> 0.104 - 0.105 ms forward, same call, alternating); three otherwise (the other small tiles spill at 128)
#define IG_FOUR_BLOCKS_TILES 3
#define IG_FOUR_BLOCKS_MIN 2
template <int WGM, int WGN, int TM, int TN, int NP, int NW = 4>
__global__ void __launch_bounds__(64 * NW, (NW == 8 ? 1 : (WGM * TM > 4 ? 2 : ((WGM * TM * TN <= IG_FOUR_BLOCKS_TILES && WGM * TM * TN >= IG_FOUR_BLOCKS_MIN && NP <= 2) ? 4 : 3)))) conv_igemm_bx6_kernel(const IgParams p) {
    constexpr int BK = 4 * NW, KB = BK / 8, KS = BK / 16, NT = 64 * NW;
    constexpr int BM = WGM * TM * 32;
    constexpr int BN = WGN * TN * 32;
    static_assert(NW == 4 || NW == 8, "four or eight waves");
    static_assert(WGM * WGN == NW, "wave grid");
    static_assert(BN == 128 && KB * BN == NT, "one gathered fragment (k-block) per thread and stage");
    static_assert(KB * BM <= 2 * NT, "at most two weight fragments per thread and stage");
    static_assert(B6_BK == 16, "the host's split-K accounting counts 16-deep steps");
    constexpr bool A2 = KB * BM > NT;       // tall tiles (BM = 192: 64 x 96 per wave, twice the MFMAs per gathered element)
    // the pipeline issues the loads of two stages beyond the last one (tiles nsteps and nsteps + 1): their weight chunks and
    // offset-table rows must lie inside the panel's zero tail
    static_assert(2 * BK <= IG_TAIL && (IG_TAIL % 8) == 0, "panel tail shorter than the prefetch distance");

    // ONE LDS array (a second __shared__ object beside it can cost a vmcnt(0) per stage, cdna_hip_programming.md section 5):
    // operand images of the K loop, then - they are dead after its last barrier - four 32 x 33 float patches of the staged
    // epilogue and the split-K "I am last" word
    constexpr int A_U4 = 2 * NP * KB * BM, B_U4 = 2 * NP * KB * BN;
    constexpr int EPI_U4 = (NW * 32 * 33 + 8 + 3) / 4;
    constexpr int SMEM_U4 = A_U4 + B_U4 > EPI_U4 ? A_U4 + B_U4 : EPI_U4;
    __shared__ uint4 smem[SMEM_U4];
    uint4 (*As)[NP][KB][BM] = reinterpret_cast<uint4 (*)[NP][KB][BM]>(smem);
    uint4 (*Bs)[NP][KB][BN] = reinterpret_cast<uint4 (*)[NP][KB][BN]>(smem + A_U4);

    int bx, by, bz;
    xcd_tile(bx, by, bz, p.tile_nphase);
    const int zphase = bz / p.ksplit, zsplit = bz - zphase * p.ksplit;
    const IgPhase& ph = p.ph[zphase];
    const int N = p.B * ph.QH * ph.QW;
    const int n0 = bx * BN;
    const int m0 = by * BM;
    if (n0 >= N) return;   // phases can have different extents; uniform per block

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;

    // ---- per-thread gather column (fixed for the whole K loop): base pointer and the set of taps inside the input
    const int ncol = tid % BN;
    const int kgrp = __builtin_amdgcn_readfirstlane(tid / BN);   // wave-uniform k-block of this thread's fragment
    const GatherCol gc = gather_setup(p, ph, n0 + ncol, N);
    float col_scale[TN];
    igemm_col_scales<WGM, WGN, TM, TN>(p, ph, col_scale, N, n0, wn, lane);
    // fp16 pieces: both operands are scaled by powers of two into fp16's range (the weights when their planes were packed,
    // the gathered tensor below); the exact inverse factors go back in after the K loop
    float b_scale = 1.0f, a_unscale = 1.0f, b_unscale = 1.0f;
    if constexpr (NP == 2) {
        const int kb_ = f16_scale_exp(absmax_read(p.b_absmax));
        const int ka_ = f16_scale_exp(__builtin_amdgcn_readfirstlane(*ph.a_absmax));
        b_scale = pow2f(kb_);
        unscale_pair(ka_, kb_, a_unscale, b_unscale);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // ---- K range of this block (split-K)
    const int total_steps = ph.Kpad / BK;
    const int per_split = (total_steps + p.ksplit - 1) / p.ksplit;
    const int step0 = zsplit * per_split;
    int nsteps = total_steps - step0;
    if (nsteps > per_split) nsteps = per_split;
    if (nsteps < 0) nsteps = 0;

    // weight fragment of this thread: chunk (k-block a_kb, column m0 + a_m) of the three pre-split planes
    const bool a_thread = KB * BM == NT || tid < KB * BM;
    const int a_kb = a_thread ? tid / BM : 0, a_m = a_thread ? tid % BM : 0;
    // every tile column lies inside the panel: ld = round_up(M, 32) = round_up(M, BM) for the BM pick_bm() chooses (checked by
    // launch_igemm), and the columns M .. ld - 1 are zero - no masking in the loop
    const uint4* ap = ph.w3 + (long long)(step0 * KB + a_kb) * ph.ld + (m0 + a_m);
    const long long a_step = (long long)KB * ph.ld, a_plane = ph.w3_plane;
    // second weight fragment of tall tiles: chunk index tid + NT
    const bool b_thread = A2 && tid + NT < KB * BM;
    const int b_kb = b_thread ? (tid + NT) / BM : 0, b_m = b_thread ? (tid + NT) % BM : 0;
    const uint4* bp = ph.w3 + (long long)(step0 * KB + b_kb) * ph.ld + (m0 + b_m);
    int kidx = step0 * BK + kgrp * 8;                             // wave-uniform first table row of the next load

    uint4 areg0, areg1, areg2;     // three named registers: as an array this spills to scratch (clang keeps it in memory)
    uint4 areg3, areg4, areg5;
    float breg[8];
    // the offset-table rows are fetched one stage ahead of the gather that uses them: the scalar load's round trip is
    // then off the per-stage critical path (it used to sit in front of every stage's buffer loads)
    i32x8 offs = *reinterpret_cast<const i32x8*>(ph.koff + __builtin_amdgcn_readfirstlane(kidx));                       // s_load_dwordx8
    unsigned long long taps = *reinterpret_cast<const unsigned long long*>(ph.ktap + __builtin_amdgcn_readfirstlane(kidx));   // s_load_dwordx2
    auto issue_loads = [&]() {
        areg0 = ap[0];
        if constexpr (NP >= 2) areg1 = ap[a_plane];
        if constexpr (NP == 3) areg2 = ap[2 * a_plane];
        ap += a_step;
        if constexpr (A2) {
            areg3 = bp[0];
            if constexpr (NP >= 2) areg4 = bp[a_plane];
            if constexpr (NP == 3) areg5 = bp[2 * a_plane];
            bp += a_step;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) breg[j] = gather_load(gc, offs[j], (unsigned)(taps >> (8 * j)) & 31u);
        kidx += BK;
        const int ks = __builtin_amdgcn_readfirstlane(kidx);
        offs = *reinterpret_cast<const i32x8*>(ph.koff + ks);
        taps = *reinterpret_cast<const unsigned long long*>(ph.ktap + ks);
    };
    auto store_tiles = [&](int buf) {
        if (a_thread) {
            As[buf][0][a_kb][a_m] = areg0;
            if constexpr (NP >= 2) As[buf][NP >= 2 ? 1 : 0][a_kb][a_m] = areg1;
            if constexpr (NP == 3) As[buf][NP - 1][a_kb][a_m] = areg2;
        }
        if constexpr (A2) {
            if (b_thread) {
                As[buf][0][b_kb][b_m] = areg3;
                if constexpr (NP >= 2) As[buf][NP >= 2 ? 1 : 0][b_kb][b_m] = areg4;
                if constexpr (NP == 3) As[buf][NP - 1][b_kb][b_m] = areg5;
            }
        }
        if constexpr (NP == 2) {
            uint4 h, l;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = breg[j];
            split2_f16x8(v, b_scale, h, l);
            Bs[buf][0][kgrp][ncol] = h;
            Bs[buf][NP - 1][kgrp][ncol] = l;
        } else if constexpr (NP == 3) {
            uint4 h, m, l;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = breg[j];
            split3_trunc_x8(v, h, m, l);
            Bs[buf][0][kgrp][ncol] = h;
            Bs[buf][NP - 2][kgrp][ncol] = m;
            Bs[buf][NP - 1][kgrp][ncol] = l;
        } else {
            bf16x8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (__bf16)breg[j];          // round to nearest even (v_cvt_pk_bf16_f32)
            Bs[buf][0][kgrp][ncol] = *reinterpret_cast<uint4*>(&h);
        }
    };

    // Software pipeline: while the matrix pipe works through the first half of a stage's MFMAs, the wave converts and
    // writes the NEXT tile (its global loads were issued half a stage earlier) and immediately re-issues the loads for the
    // tile after that into the registers it just freed; the second half of the MFMAs follows.  Global-load latency and
    // the fp32 -> 3 x bf16 split are then in the shadow of the wave's own MFMAs, with no additional registers.
    if (nsteps > 0) {
        issue_loads();                       // tile 0
        store_tiles(0);
        issue_loads();                       // tile 1 (past the end: inside the panel's zero tail, IG_TAIL rows)
    }
    __syncthreads();
    const int lrow = lane >> 5, lcol = lane & 31;
    constexpr int PROD = NP == 3 ? 6 : (NP == 2 ? 3 : 1);
    constexpr int NMF = TM * TN * PROD, HALF = KS == 1 ? NMF / 2 : NMF;
    using frag_t = typename std::conditional<NP == 2, f16x8, bf16x8>::type;
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        frag_t a[TM][NP], b[TN][NP];
        auto fragments = [&](int ksub) {          // the 16-deep slice `ksub` of the stage
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < NP; ++q) a[i][q] = *reinterpret_cast<const frag_t*>(&As[buf][q][2 * ksub + lrow][(wm * TM + i) * 32 + lcol]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < NP; ++q) b[j][q] = *reinterpret_cast<const frag_t*>(&Bs[buf][q][2 * ksub + lrow][(wn * TN + j) * 32 + lcol]);
        };
        fragments(0);
        auto mfmas = [&](int lo, int hi) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int base = (i * TN + j) * PROD;
                    if constexpr (NP == 2) {          // smallest terms first: l h, h l, h h (l l, 2^-22 of the product, is dropped)
                        if (base + 0 >= lo && base + 0 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);
                        if (base + 1 >= lo && base + 1 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);
                        if (base + 2 >= lo && base + 2 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                    } else if constexpr (NP == 3) {
                        if (base + 0 >= lo && base + 0 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 1], b[j][0], acc[i][j], 0, 0, 0);   // l h
                        if (base + 1 >= lo && base + 1 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 1], acc[i][j], 0, 0, 0);   // h l
                        if (base + 2 >= lo && base + 2 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][NP - 2], acc[i][j], 0, 0, 0);   // m m
                        if (base + 3 >= lo && base + 3 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][0], acc[i][j], 0, 0, 0);   // m h
                        if (base + 4 >= lo && base + 4 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 2], acc[i][j], 0, 0, 0);   // h m
                        if (base + 5 >= lo && base + 5 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);   // h h
                    } else {
                        if (base >= lo && base < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                    }
                }
        };
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0, HALF);
        __builtin_amdgcn_sched_barrier(0);
        store_tiles(buf ^ 1);                // tile s + 1
        __builtin_amdgcn_sched_barrier(0);
        issue_loads();                       // tile s + 2
        if constexpr (KS == 1) {
            mfmas(HALF, NMF);
        } else {
            fragments(1);                    // the stage's second 16-deep slice
            mfmas(0, NMF);
        }
        // one vector-memory instruction (and its address arithmetic) in the shadow of every MFMA: the memory pipe takes
        // ~100 cycles per wave instruction when twelve waves queue on it, the matrix pipe 32 per MFMA
        if constexpr (NP >= 2) {
#pragma unroll
            for (int k = 0; k < (KS == 1 ? NMF - HALF : NMF); ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
            }
        }
        __syncthreads();
    }
    if constexpr (NP == 2) {       // undo the two power-of-two scales in two exact steps of half the total exponent each (unscale_pair:
                                   // neither their product nor acc * one of them need be a normal fp32 number): whatever leaves this block - output or split-K partial - is unscaled
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] * a_unscale) * b_unscale;
    }
    // the operand tiles are dead after the loop's last barrier: each wave takes a 32 x 33 float patch of them
    float* const stage = reinterpret_cast<float*>(smem) + wid * (32 * 33);
    bool combined = false;
    if (p.ksplit > 1 && p.combine) {
        // ---- split-K combined inside the launch (no reduction kernel, no slab in the output's layout) ----
        // Every block of a tile stores its partial accumulators as they sit in its registers - thread t, fragment f at
        // [z][tile][f][t][4]: one contiguous KiB per store instruction - write-through (sc1), drains them, and one lane
        // takes a ticket from the tile's counter.  The block that draws the last ticket sums all ksplit partials IN z
        // ORDER (its own included, re-read: the result does not depend on which block came last - bit-reproducible),
        // and runs the ordinary epilogue.  Protocol (cdna_hip_programming.md, Guideline 16, counter form): sc1 payload
        // stores -> every storing wave s_waitcnt vmcnt(0) -> workgroup barrier -> one relaxed agent-scope fetch_add;
        // last arriver: agent-scope acquire -> s_waitcnt vmcnt(0) -> barrier -> sc1 loads.  The counter is reset by the last
        // arriver, so the counter block stays zero between launches (it must be zero before its first use).
        constexpr int FR = TM * TN * 4;                                   // 16-byte fragments per thread
        const int tile = (zphase * (int)gridDim.y + by) * (int)gridDim.x + bx;
        const int ntiles = p.nphase * (int)gridDim.y * (int)gridDim.x;
        const unsigned tile_bytes = FR * NT * 16;
        __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(p.slab, 0, (int)((unsigned)p.ksplit * ntiles * tile_bytes), 0x00020000);
        const unsigned my = ((unsigned)(zsplit * ntiles + tile)) * tile_bytes + (unsigned)tid * 16u;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    u32x4 v;
                    v[0] = __float_as_uint(acc[i][j][4 * q + 0]); v[1] = __float_as_uint(acc[i][j][4 * q + 1]);
                    v[2] = __float_as_uint(acc[i][j][4 * q + 2]); v[3] = __float_as_uint(acc[i][j][4 * q + 3]);
                    __builtin_amdgcn_raw_buffer_store_b128(v, srs, (int)(my + (unsigned)(((i * TN + j) * 4 + q) * NT * 16)), 0, 16);   // aux 16 = sc1
                }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned* const flag = reinterpret_cast<unsigned*>(smem) + NW * 32 * 33 + 4;    // beyond the waves' 32 x 33 patches
        if (tid == 0) {
            const unsigned ticket = __hip_atomic_fetch_add(p.counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = ticket == (unsigned)(p.ksplit - 1);
            if (last) {
                __hip_atomic_store(p.counters + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *flag = last ? 1u : 0u;
        }
        __syncthreads();
        if (*flag == 0u) return;
        const unsigned t0 = (unsigned)tile * tile_bytes + (unsigned)tid * 16u;
        const unsigned zstride = (unsigned)ntiles * tile_bytes;
        // the accumulators (stored above) become the sum; one z at a time, its fragments in two batches of loads in flight
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        // four fragments of four consecutive z in flight (16 loads: this block is the launch's tail, every round trip it
        // waits for is exposed); a z beyond ksplit lies beyond the descriptor's extent and reads as 0
        constexpr int HB = 4, ZB = 4;
#pragma unroll
        for (int h0 = 0; h0 < FR; h0 += HB) {
            for (int z0 = 0; z0 < p.ksplit; z0 += ZB) {
                u32x4 v[ZB][HB];
#pragma unroll
                for (int zz = 0; zz < ZB; ++zz)
#pragma unroll
                    for (int f = 0; f < HB; ++f)
                        v[zz][f] = __builtin_amdgcn_raw_buffer_load_b128(srs, (int)(t0 + (unsigned)(z0 + zz) * zstride + (unsigned)((h0 + f) * NT * 16)), 0, 16);
#pragma unroll
                for (int zz = 0; zz < ZB; ++zz)
#pragma unroll
                    for (int f = 0; f < HB; ++f) {
                        const int g = h0 + f, i = g / (TN * 4), j = (g / 4) % TN, q = g % 4;
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] += __uint_as_float(v[zz][f][e]);
                    }
            }
        }
        __syncthreads();      // the flag word's patch neighbours are about to be reused by the staged epilogue
        combined = true;
    }
    igemm_epilogue<WGM, WGN, TM, TN>(p, ph, acc, col_scale, N, n0, m0, combined ? 0 : zsplit, wm, wn, lane, stage, p.ksplit > 1 && !combined);
}

// out[b, m, :] = bias[m] + scale * sum_z slab[z][b, m, :]
__global__ void __launch_bounds__(256) igemm_slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                                const float* __restrict__ bias, const float* __restrict__ scale,
                                                                int scale_bg, int scale_stride, int B, int M, int plane,
                                                                long long out_bs, long long slab_stride, int ksplit,
                                                                float* __restrict__ act_out, long long act_bs,
                                                                const float* __restrict__ mul_pre, long long mul_bs,
                                                                unsigned* __restrict__ out_absmax) {
    // flat indices stay below 2^31 (host entry): power-of-two shifts or one 32-bit division instead of 64-bit ones
    const unsigned per_b = (unsigned)M * (unsigned)plane;
    const unsigned total = (unsigned)B * per_b;
    const unsigned stride = gridDim.x * blockDim.x;
    const DivU32 dpb(per_b), dpl((unsigned)plane);
    float am = 0.0f;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        unsigned b, r;
        dpb.divmod(i, b, r);
        // eight slabs' loads in flight, added in z order (one load - wait - add per slab is ksplit exposed round trips)
        float acc = 0.0f;
        const float* __restrict__ sp = slab + i;
        int z = 0;
        for (; z + 8 <= ksplit; z += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = sp[(long long)(z + q) * slab_stride];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += v[q];
        }
        {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = z + q < ksplit ? sp[(long long)(z + q) * slab_stride] : 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += v[q];          // + 0.0f beyond ksplit: exact
        }
        if (scale) acc *= scale[(scale_bg ? (int)b / scale_bg : 0) * scale_stride];
        if (bias) acc += bias[dpl.div(r)];
        // the fused forms of igemm_epilogue (IgParams::act_out / mul_pre)
        if (mul_pre) { acc = roottanh_grad_f(mul_pre[(long long)b * mul_bs + r], acc); am = fmaxf(am, fabsf(acc)); }
        out[(long long)b * out_bs + r] = acc;
        if (act_out) { const float a = roottanh_f(acc); act_out[(long long)b * act_bs + r] = a; am = fmaxf(am, fabsf(a)); }
    }
    if (out_absmax) absmax_publish_wave(am, out_absmax);
}

// ---------------------------------------------------------------------------------------------
// Pointwise (1x1, stride 1, no padding) contraction with few channels on both sides (K, M <= 64) over many pixels:
// an HBM-bound stream (the self-attention gates at 64x64 read and write 50 MB each for ~1 GFLOP), where the
// tile machinery of the MFMA kernel costs more than the arithmetic.  One thread = 2 adjacent pixels x all output
// channels; the weight row of each k is wave-uniform and comes through scalar loads; 8-byte coalesced loads / stores.
//   out[b, m, q] = scale_g(b) * sum_k wp[k][m] * in[b, k, q] (+ bias[m])
// ---------------------------------------------------------------------------------------------
template <int MT, int PX>
__global__ void __launch_bounds__(256) conv_pointwise_kernel(const IgParams p) {
    const IgPhase& ph = p.ph[0];
    const int HW = p.H * p.W;
    const long long npx = (long long)p.B * HW / PX;
    const long long i_ = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i_ < npx;          // (no early return: the fused epilogue's largest-magnitude word is a wave reduction)
    const long long i = live ? i_ : 0;
    const long long n = PX * i;
    const int b = (int)(n / HW), q = (int)(n - (long long)b * HW);
    const float* ip = p.in + (long long)b * p.in_bs + q;
    const float* __restrict__ wp = ph.wp;
    const int ld = ph.ld, K = ph.K;
    float acc[MT][PX];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int e = 0; e < PX; ++e) acc[m][e] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 4) {
        float xv[4][PX];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = min(k0 + kk, K - 1);          // rows >= K of the panel are zero
            const float* xp = ip + (long long)k * HW;
            if (PX == 2) {
                const float2 t = *reinterpret_cast<const float2*>(xp);
                xv[kk][0] = t.x; xv[kk][PX - 1] = t.y;
            } else {
                xv[kk][0] = *xp;
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float* wr = wp + (long long)(k0 + kk) * ld;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float wv = wr[m];
#pragma unroll
                for (int e = 0; e < PX; ++e) acc[m][e] = fmaf(wv, xv[kk][e], acc[m][e]);
            }
        }
    }
    const float sc = p.scale ? p.scale[(p.scale_bg ? b / p.scale_bg : 0) * p.scale_stride] : 1.0f;
    float* op = p.out + (long long)b * p.out_bs + q;
    if (p.act_out == nullptr && p.mul_pre == nullptr) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < p.M && live) {
                const float bv = p.bias ? p.bias[m] : 0.0f;
                const float v0 = fmaf(acc[m][0], sc, bv), v1 = fmaf(acc[m][PX - 1], sc, bv);
                if (PX == 2) *reinterpret_cast<float2*>(op + (long long)m * HW) = make_float2(v0, v1);
                else op[(long long)m * HW] = v0;
            }
        }
        return;
    }
    // the fused forms of igemm_epilogue (IgParams::act_out / mul_pre); pointwise_ok has checked their alignment
    float am = 0.0f;
    const float* zp = p.mul_pre ? p.mul_pre + (long long)b * p.mul_bs + q : nullptr;
    float* ap = p.act_out ? p.act_out + (long long)b * p.act_bs + q : nullptr;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m < p.M && live) {
            const float bv = p.bias ? p.bias[m] : 0.0f;
            float v0 = fmaf(acc[m][0], sc, bv), v1 = fmaf(acc[m][PX - 1], sc, bv);
            if (zp) {
                float z0, z1;
                if (PX == 2) { const float2 t = *reinterpret_cast<const float2*>(zp + (long long)m * HW); z0 = t.x; z1 = t.y; }
                else { z0 = zp[(long long)m * HW]; z1 = z0; }
                v0 = roottanh_grad_f(z0, v0); v1 = roottanh_grad_f(z1, v1);
                am = fmaxf(am, fmaxf(fabsf(v0), fabsf(v1)));
            }
            if (PX == 2) *reinterpret_cast<float2*>(op + (long long)m * HW) = make_float2(v0, v1);
            else op[(long long)m * HW] = v0;
            if (ap) {
                const float a0 = roottanh_f(v0), a1 = roottanh_f(v1);
                if (PX == 2) *reinterpret_cast<float2*>(ap + (long long)m * HW) = make_float2(a0, a1);
                else ap[(long long)m * HW] = a0;
                am = fmaxf(am, fmaxf(fabsf(a0), fabsf(a1)));
            }
        }
    }
    if (p.out_absmax) absmax_publish_wave(am, p.out_absmax);
}


// ---------------------------------------------------------------------------------------------
// Contractions on 1x1 maps (the style linears, the squeeze convs of the channel gates, the discriminator's head: a batch of
// 64 ... 192 rows times a [C, M] matrix, <= 0.1 GFLOP) - 45 launches per step that the tile machinery above runs in
// 8 ... 25 us each: one or two 128-wide tiles, a dozen dependent memory round trips of prologue, K loop, split-K combine and
// staged store, for microseconds' worth of arithmetic.  They get a direct form in plain fp32 FMAs (exact fp32 products):
//   out[n][j] = scale(n) * sum_r in[n][r] * P[r][j] + bias[j]
// lane = output column j (the K-major fp32 panel row P[r][.] is one coalesced load), the activations in[n][r] are
// wave-uniform and come through the scalar cache, the eight waves of a block take interleaved 32-row chunks of the reduction
// and their partial sums are added in wave order through LDS (deterministic).  Forward (adjoint-0 panel: r = c, j = m) and
// input gradient (adjoint-1 panel: r = m, j = c) are the same kernel.
// ---------------------------------------------------------------------------------------------
#define SK_NT 4           // batch rows per block
#define SK_RC 32          // reduction rows per wave and chunk
#define SK_WAVES 8        // waves per block: they take interleaved chunks of the reduction

__global__ void __launch_bounds__(64 * SK_WAVES) skinny_rows_kernel(const IgParams p) {
    const IgPhase& ph = p.ph[0];
    const int R = ph.K, J = p.M, N = p.B, ld = ph.ld;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int j = blockIdx.x * 64 + lane;
    const int n0 = blockIdx.y * SK_NT;
    const bool jok = j < ld;                                   // panel columns J .. ld - 1 are zero
    const float* __restrict__ P = ph.wp + (jok ? j : 0);
    const float* __restrict__ in = p.in;
    float acc[SK_NT];
#pragma unroll
    for (int t = 0; t < SK_NT; ++t) acc[t] = 0.0f;
    const int nchunk = (R + SK_RC - 1) / SK_RC;               // rows up to round_up(R, 32) - 1 exist in the panel (zero beyond R)
    float cur[SK_RC], nxt[SK_RC];
    if (wid < nchunk) {
#pragma unroll
        for (int i = 0; i < SK_RC; ++i) cur[i] = P[(long long)(wid * SK_RC + i) * ld];
    }
    for (int c = wid; c < nchunk; c += SK_WAVES) {
        const int r0 = c * SK_RC;
        if (c + SK_WAVES < nchunk) {
#pragma unroll
            for (int i = 0; i < SK_RC; ++i) nxt[i] = P[(long long)(r0 + SK_WAVES * SK_RC + i) * ld];
        }
        if (r0 + SK_RC <= R) {
#pragma unroll
            for (int t = 0; t < SK_NT; ++t) {
                if (n0 + t < N) {
                    const float* __restrict__ xr = in + (long long)(n0 + t) * p.in_bs + r0;       // wave-uniform: scalar loads
#pragma unroll
                    for (int i = 0; i < SK_RC; ++i) acc[t] = fmaf(xr[i], cur[i], acc[t]);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < SK_NT; ++t) {
                if (n0 + t < N) {
                    const float* __restrict__ xr = in + (long long)(n0 + t) * p.in_bs + r0;
#pragma unroll
                    for (int i = 0; i < SK_RC; ++i) {
                        const float xv = r0 + i < R ? xr[i] : 0.0f;      // never read past the row (the last row ends the tensor)
                        acc[t] = fmaf(xv, cur[i], acc[t]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < SK_RC; ++i) cur[i] = nxt[i];
    }
    __shared__ float red[SK_WAVES][SK_NT][64];
#pragma unroll
    for (int t = 0; t < SK_NT; ++t) red[wid][t][lane] = acc[t];
    __syncthreads();
    // wave t finishes row t of the tile: the partial sums in wave order, then scale and bias
    if (wid < SK_NT) {
        const int n = n0 + wid;
        float am = 0.0f;
        if (n < N && j < J) {
            float s = red[0][wid][lane];
#pragma unroll
            for (int w = 1; w < SK_WAVES; ++w) s += red[w][wid][lane];
            const float sc = p.scale ? p.scale[(p.scale_bg ? n / p.scale_bg : 0) * p.scale_stride] : 1.0f;
            float v = fmaf(s, sc, p.bias ? p.bias[j] : 0.0f);
            if (p.mul_pre) { v = roottanh_grad_f(p.mul_pre[(long long)n * p.mul_bs + j], v); am = fabsf(v); }
            p.out[(long long)n * p.out_bs + j] = v;
            if (p.act_out) { const float a = roottanh_f(v); p.act_out[(long long)n * p.act_bs + j] = a; am = fabsf(a); }
        }
        if (p.out_absmax) absmax_publish_wave(am, p.out_absmax);
        if (p.lat && blockIdx.x == 0 && n < N)          // the latent columns of the next link's input row n
            for (int c = lane; c < p.lat_z; c += 64) p.act_out[(long long)n * p.act_bs - p.lat_z + c] = p.lat[(long long)n * p.lat_bs + c];
    }
}

static bool skinny_ok(const IgParams& p) {
    if (p.nphase != 1 || path_disabled("skinny")) return false;
    const IgPhase& ph = p.ph[0];
    return ph.T == 1 && p.H == 1 && p.W == 1 && p.OH == 1 && p.OW == 1 && ph.dy0 == 0 && ph.dx0 == 0 && ph.K >= 1;
}

static void launch_skinny(const IgParams& p, hipStream_t st) {
    skinny_rows_kernel<<<dim3((p.M + 63) / 64, (p.B + SK_NT - 1) / SK_NT), 64 * SK_WAVES, 0, st>>>(p);
}

static bool pointwise_ok(const IgParams& p) {
    if (p.nphase != 1 || path_disabled("pointwise")) return false;
    const IgPhase& ph = p.ph[0];
    const int HW = p.H * p.W;
    return ph.T == 1 && p.istride == 1 && p.ostep == 1 && ph.dy0 == 0 && ph.dx0 == 0 && p.H == p.OH && p.W == p.OW &&
           ph.K >= 1 && ph.K <= 64 && p.M <= 64 && ph.ld >= ((p.M + 15) / 16) * 16 && (HW & 1) == 0 && (p.in_bs & 1) == 0 &&
           (p.out_bs & 1) == 0 && (reinterpret_cast<uintptr_t>(p.in) & 7) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 7) == 0 &&
           (long long)p.B * HW >= 131072 &&
           (!p.act_out || ((p.act_bs & 1) == 0 && (reinterpret_cast<uintptr_t>(p.act_out) & 7) == 0)) &&
           (!p.mul_pre || ((p.mul_bs & 1) == 0 && (reinterpret_cast<uintptr_t>(p.mul_pre) & 7) == 0));
}

template <int PX>
static void launch_pointwise_px(const IgParams& p, hipStream_t st) {
    const long long npx = (long long)p.B * p.H * p.W / PX;
    const int blocks = (int)((npx + 255) / 256);
    const int mt = (p.M + 15) / 16;
    if (mt == 1) conv_pointwise_kernel<16, PX><<<blocks, 256, 0, st>>>(p);
    else if (mt == 2) conv_pointwise_kernel<32, PX><<<blocks, 256, 0, st>>>(p);
    else if (mt == 3) conv_pointwise_kernel<48, PX><<<blocks, 256, 0, st>>>(p);
    else conv_pointwise_kernel<64, PX><<<blocks, 256, 0, st>>>(p);
}

static void launch_pointwise(const IgParams& p, hipStream_t st) {
    // two pixels per thread only when that still leaves >= 4 blocks per CU
    if ((long long)p.B * p.H * p.W >= (long long)knob_int("LOCATE_PX2_MIN", 2 * 256 * 1024)) launch_pointwise_px<2>(p, st);
    else launch_pointwise_px<1>(p, st);
}

// Tile height of the implicit-GEMM launch.  Tall 192 x 128 tiles (each wave 96 x 64: twice the MFMAs per gathered, split and
// LDS-written activation element, two blocks per CU) for the wide layers when the launch still fills the chip with them.
// (pick_bm and the tile table with_tile: igemm.h)
static int igemm_bm(int M, int nmax, int nphase) {
    if (M % 192 == 0 && M >= 192 && !path_disabled("tall") && !path_disabled("bx6")) {
        // only where the tall tiling alone fills its two blocks per CU (512 slots): with split-K on top, or on launches of a
        // hundred-odd blocks, the 128-row tiles at three blocks per CU measured faster (profiles/r02_igemm_tiles.txt)
        const long long tiles = (long long)((nmax + 127) / 128) * (M / 192) * nphase;
        if (tiles >= 512) return 192;
    }
    return pick_bm(M);
}

// Split K over extra blocks when the (M, N) tiling alone cannot fill 256 CUs (deep discriminator layers and the
// first generator stages: N = B*OH*OW is only 64 ... 1024 there while K = C*KH*KW is up to 12 800).
static int igemm_ksplit(int M, int nmax, int nphase, int min_kpad) {
    const int bm = igemm_bm(M, nmax, nphase);
    const long long tiles = (long long)((nmax + 127) / 128) * ((M + bm - 1) / bm) * nphase;
    const int slots = bm == 192 ? 512 : 768;        // resident blocks: 256 CUs x 2 (tall tiles) or x 3
    // launches of >= one full round of resident blocks, or an exact multiple of 256 from 512 up, are balanced
    if (tiles >= slots || (tiles >= 512 && tiles % 256 == 0)) return 1;
    const int steps = min_kpad / IG_BK;
    long long want = (slots + tiles - 1) / tiles;
    // at least 8 K steps (128 reduction elements) per block - 2 when the output is tiny (the style linears, the deep
    // discriminator layers at batch-sized N): those launches are a latency chain of K steps on a handful of blocks and
    // their partial tiles cost next to nothing
    const int min_steps = (long long)M * nmax <= (1 << 16) ? 2 : 8;
    if (steps < 8) return 1;                                   // a K step of a lone block is ~1.2 us, the reduction launch ~3
    const int max_split = steps / min_steps > 0 ? steps / min_steps : 1;
    if (want > max_split) want = max_split;
    if (want > 64) want = 64;
    if (want > knob_int("LOCATE_KS_MAX", 64)) want = knob_int("LOCATE_KS_MAX", 64);
    return want < 1 ? 1 : (int)want;
}

// How one launch splits K: the split count, whether the partial tiles are combined inside the launch (see the kernel) or by
// igemm_slab_reduce_kernel, and the slab space either way.  In-launch combining reads ksplit x tile bytes serially in the
// tile's last block, so it is taken only while that stays small (<= 512 KiB: ~5 us) and the tile count fits the counter
// block; deep splits of tiny outputs (the style linears, the discriminator's 1x1 ... 4x4 tail) keep the reduction kernel,
// which spreads the same bytes over the whole chip.
#define IG_MAX_COUNTERS 1024
struct SplitPlan {
    int ksplit, combine, gx, gy;
    size_t slab_floats;
};

static SplitPlan igemm_split_plan(const IgParams& p, int nmax, bool have_counters) {
    SplitPlan sp;
    const int bm = igemm_bm(p.M, nmax, p.nphase);
    int min_kpad = 1 << 30;
    for (int i = 0; i < p.nphase; ++i) min_kpad = p.ph[i].Kpad < min_kpad ? p.ph[i].Kpad : min_kpad;
    int ks = igemm_ksplit(p.M, nmax, p.nphase, min_kpad);
    if (ks > min_kpad / IG_BK) ks = min_kpad / IG_BK;
    if (ks < 1) ks = 1;
    sp.ksplit = ks;
    sp.gx = (nmax + 127) / 128;
    sp.gy = (p.M + bm - 1) / bm;
    const long long ntiles = (long long)sp.gx * sp.gy * p.nphase;
    const long long tile_floats = (long long)bm * 128;
    const long long legacy = ks > 1 ? (long long)ks * p.B * p.M * p.OH * p.OW : 0;
    const long long fused = ks > 1 ? (long long)ks * ntiles * tile_floats : 0;
    sp.combine = have_counters && ks > 1 && (long long)ks * tile_floats * 4 <= (512 << 10) && ntiles <= IG_MAX_COUNTERS &&
                 fused * 4 < (1ll << 31) && (p.precision == 1 || !path_disabled("bx6")) && !path_disabled("combine");
    sp.slab_floats = (size_t)(sp.combine ? fused : legacy);
    return sp;
}

void launch_slab_reduce(const IgParams& p, hipStream_t st) {
    igemm_slab_reduce_kernel<<<stream_grid(p.slab_stride, 256), 256, 0, st>>>(p.slab, p.out, p.bias, p.scale, p.scale_bg, p.scale_stride, p.B, p.M, p.OH * p.OW,
                                                                              p.out_bs, p.slab_stride, p.ksplit, p.act_out, p.act_bs, p.mul_pre, p.mul_bs, p.out_absmax);
}

// NP pieces per operand (see conv_igemm_bx6_kernel).  The eight-wave tiles are a table of their own: 128 or 64 rows of 2 x 4 waves.
template <int NP>
static void launch_bx6(const IgParams& p, dim3 grid, int bm, bool w8, hipStream_t st) {
    if (w8) {
        if (bm == 128) conv_igemm_bx6_kernel<2, 4, 2, 1, NP, 8><<<grid, 512, 0, st>>>(p);
        else conv_igemm_bx6_kernel<2, 4, 1, 1, NP, 8><<<grid, 512, 0, st>>>(p);
        return;
    }
    with_tile<true>(bm, [&](auto t) { using T = decltype(t); conv_igemm_bx6_kernel<T::wgm, T::wgn, T::tm, T::tn, NP><<<grid, 256, 0, st>>>(p); });
}

static int launch_igemm(IgParams& p, int nmax, void* slab_ws, unsigned* counters, hipStream_t st, const char* who) {
    // phase-fastest tile order (xcd_tile) where the output map is large enough for its lines to matter (same-box A/B, gather kernels:
    // 64x64 maps -5 ... -9 %, 32x32 -3 ... -11 %, 16x16 and 8x8 even; on 4x4 maps the four phases' weight panels thrash the
    // XCD's L2 instead: +25 %)
    p.tile_nphase = (path_disabled("phasefast") || (long long)p.OH * p.OW < 1024) ? 1 : p.nphase;
    if (p.win) return launch_win_igemm(p, nmax, slab_ws, counters, st, who);
    if (skinny_ok(p)) {
        p.ksplit = 1;
        launch_skinny(p, st);
        LOCATE_LAUNCH_CHECK(who);
        return LOCATE_OK;
    }
    if (pointwise_ok(p)) {
        p.ksplit = 1;
        launch_pointwise(p, st);
        LOCATE_LAUNCH_CHECK(who);
        return LOCATE_OK;
    }
    const int bm = igemm_bm(p.M, nmax, p.nphase);
    const SplitPlan sp = igemm_split_plan(p, nmax, counters != nullptr);
    p.ksplit = sp.ksplit;
    p.combine = sp.combine;
    p.counters = counters;
    p.slab = static_cast<float*>(slab_ws);
    p.slab_stride = (long long)p.B * p.M * p.OH * p.OW;
    dim3 grid(sp.gx, sp.gy, p.nphase * p.ksplit);
    for (int i = 0; i < p.nphase; ++i)
        LOCATE_REQUIRE(round_up(p.M, bm) <= p.ph[i].ld, "%s: tile height %d does not divide the panel width %d", who, bm, p.ph[i].ld);
    if (p.precision == 3) {          // fp8 operands (convfp8.hip): the same tiling and split plan, 32-deep stages
        launch_fp8_igemm(p, grid, bm, st);
        LOCATE_LAUNCH_CHECK(who);
        if (p.ksplit > 1 && !p.combine) {
            LOCATE_REQUIRE(p.slab_stride < (1ll << 31), "%s: split-K output of %lld elements exceeds the 32-bit index range", who, p.slab_stride);
            launch_slab_reduce(p, st);
            LOCATE_LAUNCH_CHECK(who);
        }
        return LOCATE_OK;
    }
    // launches of at most ~one block per CU: the eight-wave form (see the kernel)
    const bool w8 = !path_disabled("w8") && !path_disabled("bx6") && (bm == 128 || bm == 64) &&
                    (long long)grid.x * grid.y * grid.z <= knob_int("LOCATE_W8_MAX", 320);
    if (p.precision == 2) LOCATE_REQUIRE(!path_disabled("bx6"), "%s: fp16 pieces need the bf16/fp16 MFMA kernels", who);
    if (p.precision == 1) launch_bx6<1>(p, grid, bm, w8, st);
    else if (p.precision == 2) launch_bx6<2>(p, grid, bm, w8, st);
    else if (!path_disabled("bx6")) launch_bx6<3>(p, grid, bm, w8, st);
    else with_tile<false>(bm, [&](auto t) { using T = decltype(t); conv_igemm_kernel<T::wgm, T::wgn, T::tm, T::tn><<<grid, 256, 0, st>>>(p); });
    LOCATE_LAUNCH_CHECK(who);
    if (p.ksplit > 1 && !p.combine) {
        const long long total = p.slab_stride;
        LOCATE_REQUIRE(total < (1ll << 31), "%s: split-K output of %lld elements exceeds the 32-bit index range", who, total);
        launch_slab_reduce(p, st);
        LOCATE_LAUNCH_CHECK(who);
    }
    return LOCATE_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// geom = {B, C, H, W, M, KH, KW, stride, pad_h, pad_w, OH, OW} of the regular convolution R
static size_t slab_floats(const IgParams& p, int nmax) {
    if (p.win) return win_slab_floats(p, nmax);
    if (skinny_ok(p)) return 0;
    // the caller may or may not pass counters: room for whichever form the launch then takes
    const size_t a = igemm_split_plan(p, nmax, false).slab_floats, b = igemm_split_plan(p, nmax, true).slab_floats;
    return a > b ? a : b;
}

// Taps that can ever meet the input.  On the deepest maps most of a kernel only ever sees padding (a 5x5 s2 p2 conv that
// maps 2x2 -> 1x1 reads 4 of its 25 taps, a 3x3 p1 conv on a 1x1 map one of 9): the contraction then runs over the bounding
// range of useful taps only - fewer K rows to stream, pack and multiply - with identical results (the dropped taps
// contribute exact zeros).
//   regular direction: tap k reads input i = o*s - pad + k for outputs o in [0, out): useful iff some i lands in [0, in)
static void useful_taps(int in, int out, int k, int s, int pad, int* lo, int* n) {
    if (path_disabled("taps")) { *lo = 0; *n = k; return; }
    int first = -1, last = -1;
    for (int t = 0; t < k; ++t) {
        bool any = false;
        for (int o = 0; o < out && !any; ++o) {
            const int i = o * s - pad + t;
            any = i >= 0 && i < in;
        }
        if (any) { if (first < 0) first = t; last = t; }
    }
    if (first < 0) { first = 0; last = 0; }          // nothing useful: keep one tap (it reads zeros)
    *lo = first; *n = last - first + 1;
}
//   adjoint phase: tap th reads the gathered map at q + d0 - th for phase rows q in [0, Q): useful iff that lands in [0, out)
static void useful_phase_taps(int Q, int out, int d0, int T, int* lo, int* n) {
    if (path_disabled("taps")) { *lo = 0; *n = T > 0 ? T : 1; return; }
    int first = T > 0 ? d0 - out + 1 : 0, last = d0 + Q - 1;
    if (first < 0) first = 0;
    if (last > T - 1) last = T - 1;
    if (first > last) { first = 0; last = 0; }
    *lo = first; *n = last - first + 1;
}

static void phase_taps(int parity, int pad, int K, int s, int* k0, int* d0, int* T) {
    *k0 = (parity + pad) % s;
    *d0 = (parity + pad - *k0) / s;
    *T = *k0 < K ? (K - *k0 + s - 1) / s : 0;
}

// most negative displacement dy*W + dx over the taps of a phase (0 if none is negative)
static int tap_dmin(const PackArgs& a) {
    int best = 0;
    for (int th = 0; th < a.TH; ++th)
        for (int tw = 0; tw < a.TW; ++tw) {
            const int d = (a.dy0 + a.dys * th) * a.gW + a.dx0 + a.dxs * tw;
            if (d < best) best = d;
        }
    return best;
}

static void phase_finish(IgPhase& ph, const PackArgs& pa, float* panel_base) {
    ph.wp = panel_base;
    ph.koff = reinterpret_cast<const int*>(panel_base + (size_t)pa.rows * pa.ld);
    ph.ktap = reinterpret_cast<const unsigned char*>(ph.koff + pa.rows);
    ph.w3 = reinterpret_cast<const uint4*>(panel_base + panel_split_offset(pa.rows, pa.ld) + (pa.fmt ? PANEL_HDR : 0));
    ph.a_absmax = pa.fmt ? reinterpret_cast<const unsigned*>(panel_base + panel_split_offset(pa.rows, pa.ld)) : nullptr;
    ph.w3_plane = (long long)(pa.rows / 8) * pa.ld;
    ph.dmin = pa.dmin;
    ph.K = pa.K; ph.Kpad = pa.rows - IG_TAIL; ph.ld = pa.ld;
    ph.TW = pa.TW > 0 ? pa.TW : 1; ph.tw_magic = (65536 + ph.TW - 1) / ph.TW;
    ph.dy0 = pa.dy0; ph.dys = pa.dys; ph.dx0 = pa.dx0; ph.dxs = pa.dxs;
}

// Window form of a planned contraction (convwin.hip): turns the phase table conv_plan built into the window kernels' - panel
// layout in unit order, tile structure, LDS window geometry, per-tap slot displacements - or returns false when this geometry
// has none (the caller then keeps the gather kernels).  What the window kernels need:
//   * >= 16 reduction channels, a multiple of 8; an even map width and even plane size (8-byte loads of pixel pairs; a power of
//     two for stride-2 gathers);
//   * column tiles (128 or 256 wide) that are whole rows of one image (BN % QW == 0) or whole images (BN % (QH QW) == 0), in every phase;
//   * every phase with more than one tap, or a single phase with one tap (then the map is treated as flat pixel runs);
//   * operand images that fit the LDS budget below.
// The caller's alignment conditions on the tensor itself (base address, batch stride) are checked at launch.
#define WIN_LDS_BUDGET (128 * 1024)
static bool win_finish(IgParams& p, PackBatch& batch, int fmt, float* panel, size_t* off_out) {
    if (path_disabled("win") || p.nphase < 1 || p.C < 16 || (p.C & 7)) return false;
    bool any1 = false;
    for (int i = 0; i < p.nphase; ++i) {
        if (p.ph[i].T < 1) return false;
        any1 = any1 || p.ph[i].T == 1;
    }
    if (any1 && (p.nphase > 1 || p.istride != 1 || p.ostep != 1 || p.ph[0].dy0 != 0 || p.ph[0].dx0 != 0 || p.H != p.OH || p.W != p.OW)) return false;
    if (any1) {
        // single tap: the map is a flat run of pixels; re-shape it into rows of min(HW, tile width) pixels
        const long long HW = (long long)p.H * p.W;
        if (HW < 2 || (HW & (HW - 1)) != 0) return false;          // powers of two only (every map of the model is)
        int bn1 = 128;
        if (knob_int("LOCATE_WIN_BM", 0) > 0 && p.M % knob_int("LOCATE_WIN_BM", 0) == 0) bn1 = win_pick_bn(knob_int("LOCATE_WIN_BM", 0));
        if (knob_int("LOCATE_WIN_BN", 0) > 0) bn1 = knob_int("LOCATE_WIN_BN", 0);
        const int Wc = HW >= bn1 ? bn1 : (int)HW;
        p.W = p.OW = Wc; p.H = p.OH = (int)(HW / Wc);
        p.ph[0].QW = Wc; p.ph[0].QH = p.H;
        p.ph[0].TW = 1; p.ph[0].tw_magic = 65536;
    }
    if ((p.W & 1) || (((long long)p.H * p.W) & 1)) return false;
    int bm = win_pick_bm(p.M), bn = win_pick_bn(bm);
    if (any1) {
        // single-tap layers (plain GEMMs of a few GFLOP): 64 x 128 tiles while that gives every CU a block, else 32 x 128
        // (measured: profiles/notes_r04_experiments.md)
        const long long N1 = (long long)p.B * p.H * p.W;
        bn = 128;
        bm = ((N1 + 127) / 128) * ((p.M + 63) / 64) >= 256 ? 64 : 32;
        if (round_up(p.M, 64) != round_up(p.M, 32)) bm = 32;          // (the panel is round_up(M, 32) columns wide: M = 96 has no 64-row tiling)
    }
    {   // (debug library: force a tile - LOCATE_WIN_BM rows, LOCATE_WIN_BN columns)
        const int fbm = knob_int("LOCATE_WIN_BM", 0), fbn = knob_int("LOCATE_WIN_BN", 0);
        if (fbm > 0 && p.M % fbm == 0) { bm = fbm; bn = win_pick_bn(bm); }
        if (fbn > 0) bn = fbn;
    }
    const int C8G = (p.C + 7) / 8;
    int X[4], nx = 0;
    for (int i = 0; i < p.nphase; ++i) X[nx++] = any1 ? C8G : p.ph[i].T;
    const int SL = win_pick_sl(X, nx), U = 2 * SL;
    const int NP = fmt ? 2 : 3;
    int slotsp = 0, bpt = 1;
    size_t off = 0;
    for (int i = 0; i < p.nphase; ++i) {
        IgPhase& ph = p.ph[i];
        PackArgs& pa = batch.ph[i];
        const int QHW = ph.QH * ph.QW;
        if (QHW >= bn) {
            if (QHW % bn != 0 || bn % ph.QW != 0) return false;
            ph.win_NI = 1; ph.win_TR = bn / ph.QW;
        } else {
            if (bn % QHW != 0) return false;
            ph.win_NI = bn / QHW; ph.win_TR = ph.QH;
        }
        const int T = ph.T, TH = T / ph.TW;
        if (TH * ph.TW != T || T > 25) return false;
        const int dyA = ph.dy0, dyB = ph.dy0 + ph.dys * (TH - 1);
        const int dymin = dyA < dyB ? dyA : dyB, dymax = dyA < dyB ? dyB : dyA;
        int WR = (ph.win_TR - 1) * p.istride + (dymax - dymin) + 1;
        if (WR > p.H) WR = p.H;
        ph.win_WR = WR;
        fastdiv_make((unsigned)(WR * p.W), &ph.win_wrw_mul, &ph.win_wrw_s1, &ph.win_wrw_s2);
        ph.win_Tp = T == 1 ? 1 : round_up(T, U);
        ph.win_NG = T == 1 ? 1 : ph.win_Tp / U;
        const int slots = ph.win_NI * WR * p.W;
        if (slots + 2 > slotsp) slotsp = slots + 2;          // + the trash slot (masked items' chunks) and the zero slot (taps outside the input)
        // the loader's capacity: at most two items (pixel pairs x 8 channels) per thread and stage
        const long long items = (long long)(T == 1 ? U : 1) * (slots / 2);
        if (items > 2ll * 256 * ph.win_NG) return false;
        if (items > 256ll * ph.win_NG) bpt = 2;
        for (int t = 0; t < 32; ++t) {
            int c = 0;
            if (t < T) {
                const int th = t / ph.TW, tw = t - th * ph.TW;
                const int dy = ph.dy0 + ph.dys * th, dx = ph.dx0 + ph.dxs * tw;
                c = dy * p.W + (p.istride == 2 ? (dx & 1) * (p.W / 2) + (dx >> 1) : dx);
            }
            ph.tapc[t] = c;
        }
        const int C8Gp = T == 1 ? round_up(C8G, U) : C8G;
        pa.win = 1; pa.Tp = ph.win_Tp; pa.urows = C8Gp * ph.win_Tp + WIN_TAIL_UNITS;
        pa.out = panel ? panel + off : nullptr;
        // the panel is header + planes: the K-major fp32 rows, offset tables and their pointers do not exist
        ph.wp = nullptr; ph.koff = nullptr; ph.ktap = nullptr;
        ph.a_absmax = (fmt && pa.out) ? reinterpret_cast<const unsigned*>(pa.out) : nullptr;
        ph.w3 = pa.out ? reinterpret_cast<const uint4*>(pa.out + PANEL_HDR) : nullptr;
        ph.w3_plane = (long long)pa.urows * pa.ld;
        ph.Kpad = C8Gp * ph.win_Tp * 8;
        // non-direct packing reads its scale from the panel's own header (win_absmax_jobs_kernel)
        pa.wmax = (fmt && pa.out) ? reinterpret_cast<const unsigned*>(pa.out) : nullptr;
        pa.wmax_single = 1;
        off += win_panel_floats(pa.urows, pa.ld, fmt);
    }
    if (p.istride == 2 && (p.W & (p.W - 1))) return false;          // (the parity de-interleave masks with W - 1)
    int ngm = 1;
    for (int i = 0; i < p.nphase; ++i) ngm = p.ph[i].win_NG > ngm ? p.ph[i].win_NG : ngm;
    const size_t lds = ((size_t)2 * NP * U * bm + (size_t)2 * NP * (any1 ? U : 1) * slotsp) * 16 + (size_t)ngm * bpt * 256 * 8;
    if (lds > WIN_LDS_BUDGET) return false;
    if (any1)
        for (int t = 0; t < 32; ++t) p.ph[0].tapc[t] = t < U ? t * slotsp : 0;
    p.win = 1; p.win_U = U; p.win_slotsp = slotsp; p.win_bm = bm; p.win_bn = bn;
    *off_out = off;
    return true;
}

// Fills the phase table of R (adjoint = 0) or of its data adjoint (adjoint = 1: one phase per sub-pixel).
// `panel` is the packed-weight buffer (may be null when only sizes are wanted); with `pack` the packing kernels
// are launched.  Returns the panel size in floats and the largest per-phase N.
static int conv_plan(const ConvGeom& g, int adjoint_fmt, const float* w, float* panel, IgParams& p, int* nmax_out,
                     size_t* panel_floats_out, bool pack, hipStream_t st, PackBatch* batch_out = nullptr) {
    // adjoint_fmt: bit 0 = direction (0: R, 1: its data adjoint), bit 1 = panel format (0: bf16 planes, 1: fp16-piece planes),
    // bit 2 = window panel (chunk rows in unit order for the LDS-window kernels of convwin.hip; win_finish below)
    // bit 3 = fp8 panel (one e4m3 plane, convfp8.hip)
    const int adjoint = adjoint_fmt & 1, fmt = (adjoint_fmt & 8) ? 2 : ((adjoint_fmt >> 1) & 1);
    size_t off = 0;
    int nmax = 0;
    p.nphase = 0;
    PackBatch batch;
    if (!adjoint) {
        p.B = g.B; p.C = g.C; p.H = g.H; p.W = g.W; p.M = g.M; p.OH = g.OH; p.OW = g.OW;
        p.istride = g.stride; p.ostep = 1; p.nphase = 1;
        PackArgs pa;
        pa.w = w; pa.out = panel;
        pa.M = g.M; pa.C = g.C; pa.KH = g.KH; pa.KW = g.KW; pa.mode = 0;
        pa.s = 1;
        useful_taps(g.H, g.OH, g.KH, g.stride, g.pad_h, &pa.kh0, &pa.TH);
        useful_taps(g.W, g.OW, g.KW, g.stride, g.pad_w, &pa.kw0, &pa.TW);
        pa.K = g.C * pa.TH * pa.TW; pa.rows = round_up(pa.K, IG_KPAD) + IG_TAIL; pa.ld = round_up(g.M, 32);
        pa.gHW = g.H * g.W; pa.gW = g.W; pa.dy0 = pa.kh0 - g.pad_h; pa.dys = 1; pa.dx0 = pa.kw0 - g.pad_w; pa.dxs = 1;
        pa.dmin = tap_dmin(pa);
        pa.fmt = fmt; pa.wmax = nullptr; pa.direct = 0; pa.keep_f32 = 1;
        pa.win = 0; pa.Tp = 0; pa.urows = 0; pa.wmax_single = 0;
        batch.ph[0] = pa;
        IgPhase& ph = p.ph[0];
        phase_finish(ph, pa, panel);
        ph.T = pa.TH * pa.TW;
        ph.oy0 = ph.ox0 = 0; ph.QH = g.OH; ph.QW = g.OW;
        off = panel_floats(pa.rows, pa.ld, fmt);
        nmax = g.B * g.OH * g.OW;
    } else {
        p.B = g.B; p.C = g.M; p.H = g.OH; p.W = g.OW; p.M = g.C; p.OH = g.H; p.OW = g.W;
        p.istride = 1; p.ostep = g.stride;
        for (int py = 0; py < g.stride; ++py)
            for (int px = 0; px < g.stride; ++px) {
                int kh0, dy0, TH, kw0, dx0, TW;
                phase_taps(py, g.pad_h, g.KH, g.stride, &kh0, &dy0, &TH);
                phase_taps(px, g.pad_w, g.KW, g.stride, &kw0, &dx0, &TW);
                const int QH = py < g.H ? (g.H - py + g.stride - 1) / g.stride : 0;
                const int QW = px < g.W ? (g.W - px + g.stride - 1) / g.stride : 0;
                if (QH == 0 || QW == 0) continue;
                {
                    int lo, n;
                    useful_phase_taps(QH, g.OH, dy0, TH, &lo, &n);
                    kh0 += g.stride * lo; dy0 -= lo; TH = TH > 0 ? n : 0;
                    useful_phase_taps(QW, g.OW, dx0, TW, &lo, &n);
                    kw0 += g.stride * lo; dx0 -= lo; TW = TW > 0 ? n : 0;
                }
                IgPhase& ph = p.ph[p.nphase++];
                PackArgs pa;
                pa.w = w; pa.out = panel ? panel + off : nullptr;
                pa.M = g.M; pa.C = g.C; pa.KH = g.KH; pa.KW = g.KW; pa.mode = 1;
                pa.kh0 = kh0; pa.kw0 = kw0; pa.s = g.stride; pa.TH = TH; pa.TW = TW;
                pa.K = g.M * TH * TW; pa.rows = round_up(pa.K > 0 ? pa.K : 1, IG_KPAD) + IG_TAIL; pa.ld = round_up(g.C, 32);
                pa.gHW = g.OH * g.OW; pa.gW = g.OW; pa.dy0 = dy0; pa.dys = -1; pa.dx0 = dx0; pa.dxs = -1;
                pa.dmin = tap_dmin(pa);
                pa.fmt = fmt; pa.wmax = nullptr; pa.direct = 0; pa.keep_f32 = 1;
                pa.win = 0; pa.Tp = 0; pa.urows = 0; pa.wmax_single = 0;
                batch.ph[p.nphase - 1] = pa;
                phase_finish(ph, pa, pa.out);
                ph.T = TH * TW;
                ph.oy0 = py; ph.ox0 = px; ph.QH = QH; ph.QW = QW;
                off += panel_floats(pa.rows, pa.ld, fmt);
                const int nph = g.B * QH * QW;
                if (nph > nmax) nmax = nph;
            }
    }
    p.win = 0;
    if (adjoint_fmt & 4) {
        LOCATE_REQUIRE(win_finish(p, batch, fmt, panel, &off), "conv: this geometry has no window form (ask locate_conv_win_ok first)");
    }
    if (nmax_out) *nmax_out = nmax;
    if (panel_floats_out) *panel_floats_out = off;
    if (batch_out) *batch_out = batch;
    if (pack && p.nphase > 0)
        if (int e = launch_pack(batch, p.nphase, st, "locate_conv_pack_panel")) return e;
    return LOCATE_OK;
}

// adjoint = 0: panel for locate_conv_fwd; adjoint = 1: panels (one per sub-pixel phase) for locate_conv_dgrad
LOCATE_API size_t locate_conv_panel_bytes(const int* geom, int adjoint) {
    IgParams p;
    size_t n = 0;
    conv_plan(make_geom(geom), adjoint, nullptr, nullptr, p, nullptr, &n, false, nullptr);
    return n * sizeof(float);
}

// Re-lays W [M, C, KH, KW] out as the K-major, zero-padded panel(s) the implicit GEMM streams, followed by the
// gather offset table of this geometry.  Only needs to be redone when W changes (once per optimizer step), not per
// forward: the spectral-norm 1/sigma is applied in the GEMM epilogue instead of being baked into the weights.
LOCATE_API int locate_conv_pack_panel(const int* geom, int adjoint, const float* w, float* panel, void* stream) {
    const ConvGeom g = make_geom(geom);
    if (int e = geom_check(g, "locate_conv_pack_panel")) return e;
    LOCATE_REQUIRE(w && panel, "locate_conv_pack_panel: null pointer");
    IgParams p;
    return conv_plan(g, adjoint, w, panel, p, nullptr, nullptr, true, as_stream(stream));
}

// Batched form (all panels of a network in ONE launch after an optimizer step): the caller fills one host record per
// panel with locate_conv_pack_job (block_start = running sum of the returned block counts), uploads the array and
// calls locate_conv_pack_panels.  Records hold raw pointers: rebuild them when a weight or panel buffer moves.

// direct != 0: the job RE-packs a panel that has been packed in full before (its offset tables and zero tails are kept) in its
// direct form - the piece planes in one pass, straight from the weights, the K-major fp32 rows only where a kernel reads them.
// A fp16-piece panel needs weight_absmax for that: locate_absmax_words() device words holding the largest magnitude of w as it
// is NOW (the optimizer kernel leaves them, locate_nadam_step); without them - and for geometries the direct bodies do not
// cover - the job silently takes the two-pass form.
LOCATE_API int locate_conv_pack_job(const int* geom, int adjoint, const float* w, float* panel, int block_start, void* job_out,
                                    int* blocks_out, int direct, const void* weight_absmax) {
    const ConvGeom g = make_geom(geom);
    if (int e = geom_check(g, "locate_conv_pack_job")) return e;
    LOCATE_REQUIRE(w && panel && job_out && blocks_out && block_start >= 0, "locate_conv_pack_job: bad arguments");
    IgParams p;
    PackBatch batch;
    if (int e = conv_plan(g, adjoint, w, panel, p, nullptr, nullptr, false, nullptr, &batch)) return e;
    LOCATE_REQUIRE(p.nphase > 0, "locate_conv_pack_job: empty panel");
    if (batch.ph[0].win) {
        // window panels are always packed in one pass; "direct" = their scale is at hand (bf16 pieces need none, fp16 pieces take
        // the optimizer's absmax words) - otherwise the launch runs the absmax pre-pass into the panel headers first
        for (int i = 0; i < p.nphase; ++i) {
            if (weight_absmax && (adjoint & 2)) { batch.ph[i].wmax = static_cast<const unsigned*>(weight_absmax); batch.ph[i].wmax_single = 0; }
            batch.ph[i].direct = (weight_absmax || !(adjoint & 2)) ? 1 : 0;
        }
    } else if (direct && (weight_absmax || !(adjoint & 10))) {          // (fp16-piece and fp8 panels need the weights' absmax words)
        const PackArgs& a0 = batch.ph[0];
        const bool transpose = a0.mode == 0 && p.nphase == 1;
        const bool adj = a0.mode == 1 && a0.KH * a0.KW <= PACK_MAX_TAPS;
        if (transpose || adj) {
            // single-tap panels feed the pointwise / 1x1-map kernels, which read the fp32 rows; the debug library's fp32-MFMA
            // fallback reads them for every panel
            bool keep = path_disabled("bx6") || path_disabled("direct_planes_only");
            for (int i = 0; i < p.nphase; ++i) keep = keep || (p.nphase == 1 && batch.ph[i].TH * batch.ph[i].TW == 1);
            for (int i = 0; i < p.nphase; ++i) {
                batch.ph[i].wmax = static_cast<const unsigned*>(weight_absmax);
                batch.ph[i].direct = 1;
                batch.ph[i].keep_f32 = keep ? 1 : 0;
            }
        }
    }
    PackJob j = make_pack_job(batch, p.nphase);
    j.block_start = block_start;
    memcpy(job_out, &j, sizeof(PackJob));
    *blocks_out = j.gx * j.gy;
    return LOCATE_OK;
}


// optional activated second output of locate_conv_fwd (HOST struct, see IgParams::act_out)
struct LocateActEpilogue {
    void* act_out;
    long long act_bs;
    const void* lat;
    long long lat_bs;
    int lat_z, pad;
    const void* mul_pre;
    long long mul_bs;
    void* out_absmax;
};

static int run_igemm(const ConvGeom& g, int adjoint, const float* in, int64_t in_bs, const float* panel, const float* scale,
                     int scale_bg, int scale_stride, const float* bias, float* out, int64_t out_bs, float* ws, unsigned* counters,
                     int precision, const unsigned* in_absmax, hipStream_t st, const char* who, const LocateActEpilogue* epi = nullptr) {
    const int win = (precision >> 4) & 1;          // bit 4: the panel is a window panel (locate_conv_win_ok)
    precision &= 15;
    LOCATE_REQUIRE(precision >= 0 && precision <= 3, "%s: precision must be 0 (fp32-faithful, bf16 pieces), 1 (bf16 operands), 2 (fp32-faithful, fp16 pieces) or 3 (fp8 operands)", who);
    LOCATE_REQUIRE(precision < 2 || in_absmax, "%s: precisions 2 and 3 need the gathered tensor's absmax words", who);
    LOCATE_REQUIRE(!(win && precision == 3), "%s: no window form of the fp8 contractions", who);
    IgParams p;
    p.precision = precision;
    p.b_absmax = in_absmax;
    p.act_out = nullptr; p.act_bs = 0; p.lat = nullptr; p.lat_bs = 0; p.lat_z = 0;
    p.mul_pre = nullptr; p.mul_bs = 0; p.out_absmax = nullptr;
    int nmax = 0;
    if (int e = conv_plan(g, (adjoint & 1) | (win ? 4 : 0) | (precision == 2 ? 2 : 0) | (precision == 3 ? 8 : 0), nullptr, const_cast<float*>(panel), p, &nmax, nullptr, false, st)) return e;
    LOCATE_REQUIRE(p.nphase > 0, "%s: empty output", who);
    LOCATE_REQUIRE(!win || ((in_bs & 1) == 0 && (reinterpret_cast<uintptr_t>(in) & 7) == 0), "%s: the window form loads pixel pairs: 8-byte aligned tensor, even batch stride", who);
    p.in = in; p.out = out; p.bias = bias; p.scale = scale; p.in_bs = in_bs; p.out_bs = out_bs;
    p.scale_bg = scale_bg; p.scale_stride = scale_stride;
    {
        const long long extent = 4ll * ((long long)(p.B - 1) * in_bs + (long long)p.C * p.H * p.W);
        LOCATE_REQUIRE(in_bs >= 0 && extent > 0 && extent < (1ll << 31) - (1 << 20), "%s: gathered tensor of %lld bytes exceeds the 2 GiB a buffer descriptor addresses", who, extent);
        p.in_bytes = (unsigned)extent;
    }
    LOCATE_REQUIRE(scale_bg >= 0 && (scale_bg == 0 || g.B % scale_bg == 0), "%s: batch %d is not a multiple of the scale group %d", who, g.B, scale_bg);
    LOCATE_REQUIRE(ws || slab_floats(p, nmax) == 0, "%s: split-K needs a workspace", who);
    if (epi && epi->act_out) {
        LOCATE_REQUIRE(!epi->lat || skinny_ok(p), "%s: the latent prefix of the activated second output exists for 1x1-map layers only", who);
        LOCATE_REQUIRE(!epi->lat || (epi->lat_z > 0 && epi->act_bs >= epi->lat_z + g.M), "%s: bad latent prefix", who);
        LOCATE_REQUIRE(!epi->mul_pre, "%s: an epilogue either activates or multiplies by the activation's derivative", who);
        LOCATE_REQUIRE(epi->act_bs >= (long long)p.M * p.OH * p.OW, "%s: activated output's batch stride is smaller than one element of the batch", who);
        p.act_out = static_cast<float*>(epi->act_out); p.act_bs = epi->act_bs;
        p.lat = static_cast<const float*>(epi->lat); p.lat_bs = epi->lat_bs; p.lat_z = epi->lat ? epi->lat_z : 0;
    }
    if (epi && epi->mul_pre) {
        LOCATE_REQUIRE(epi->mul_bs >= (long long)p.M * p.OH * p.OW, "%s: pre-activation's batch stride is smaller than one element of the batch", who);
        p.mul_pre = static_cast<const float*>(epi->mul_pre); p.mul_bs = epi->mul_bs;
    }
    if (epi && (epi->act_out || epi->mul_pre)) p.out_absmax = static_cast<unsigned*>(epi->out_absmax);
    return launch_igemm(p, nmax, ws, counters, st, who);
}

static size_t igemm_ws_bytes(const int* geom, int adjoint) {
    IgParams p;
    p.precision = 0;
    int nmax = 0;
    if (conv_plan(make_geom(geom), adjoint, nullptr, nullptr, p, &nmax, nullptr, false, nullptr)) return 0;
    return (p.nphase > 0 ? slab_floats(p, nmax) : 0) * sizeof(float);
}

// Whether this geometry and direction (bit 0 of adjoint_fmt; bit 1 = fp16-piece planes) has a WINDOW form (convwin.hip): the
// caller then packs the panel with format bit 2 set (adjoint_fmt | 4, here and in locate_conv_panel_bytes / _pack_panel / _pack_job)
// and passes adjoint-direction entry points the same panel as before; locate_conv_fwd / locate_conv_dgrad take the flag through
// their `precision` argument's bit 4 (precision | 16).  x_bs / x: the gathered tensor's batch stride and address (pixel pairs are
// loaded 8 bytes wide).  1x1 maps and the narrow streaming layers keep their own kernels: 0 for them.  Returns 1 where the window
// form is also the faster one on MI355X (what the Python layer takes by default), 2 where it merely exists.
LOCATE_API int locate_conv_win_ok(const int* geom, int adjoint_fmt, int64_t x_bs, const void* x) {
    const ConvGeom g = make_geom(geom);
    if (geom_check(g, "locate_conv_win_ok")) return 0;
    if ((x_bs & 1) || (reinterpret_cast<uintptr_t>(x) & 7)) return 0;
    IgParams p;
    p.precision = 0;
    int nmax = 0;
    if (conv_plan(g, adjoint_fmt & 1, nullptr, nullptr, p, &nmax, nullptr, false, nullptr) || p.nphase < 1) return 0;
    p.in = static_cast<const float*>(x); p.out = nullptr; p.in_bs = x_bs; p.out_bs = 2;
    if (skinny_ok(p)) return 0;
    {   // the narrow pointwise stream (geometry part of pointwise_ok)
        const IgPhase& ph = p.ph[0];
        if (p.nphase == 1 && ph.T == 1 && p.istride == 1 && p.ostep == 1 && p.H == p.OH && p.W == p.OW && ph.K <= 64 && p.M <= 64 &&
            (long long)p.B * p.H * p.W >= 131072 && !path_disabled("pointwise")) return 0;
    }
    if (conv_plan(g, (adjoint_fmt & 3) | 4, nullptr, nullptr, p, &nmax, nullptr, false, nullptr) || !p.win) return 0;
    // 1: the window form is the measured choice (profiles/notes_r04_experiments.md: the weight-streaming layers - a single tap over
    // >= 384 reduction channels, the four 2x2-tap phases of a transposed 4x4 stride-2 conv over >= 512); 2: it exists and is
    // correct, the gather kernels measured as fast or faster
    bool taps4 = p.nphase == 4;
    for (int i = 0; i < p.nphase; ++i) taps4 = taps4 && p.ph[i].T == 4;
    const bool best = p.M >= 128 && ((p.nphase == 1 && p.ph[0].T == 1 && p.C >= 384) || (taps4 && p.C >= 512));
    return best ? 1 : 2;
}
// split-K workspace of the window form (0 when the launch already fills the chip)
LOCATE_API size_t locate_conv_win_workspace_bytes(const int* geom, int adjoint_fmt) {
    IgParams p;
    p.precision = (adjoint_fmt & 2) ? 2 : 0;
    int nmax = 0;
    if (conv_plan(make_geom(geom), (adjoint_fmt & 3) | 4, nullptr, nullptr, p, &nmax, nullptr, false, nullptr) || !p.win) return 0;
    return win_slab_floats(p, nmax) * sizeof(float);
}

// split-K slab space (0 when the launch already fills the chip)
LOCATE_API size_t locate_conv_fwd_workspace_bytes(const int* geom) { return igemm_ws_bytes(geom, 0); }
LOCATE_API size_t locate_conv_dgrad_workspace_bytes(const int* geom) { return igemm_ws_bytes(geom, 1); }

// y[b, m, oh, ow] = bias[m] + scale_g(b) * sum w[m, c, kh, kw] x[b, c, oh*s-ph+kh, ow*s-pw+kw]     (panel: adjoint = 0)
// x_bs / y_bs: batch strides in elements (channel-sliced views of a contiguous NCHW tensor are allowed).
// scale (nullable): scale_group_batch = 0 -> one device scalar; > 0 -> batch element b uses
// scale[(b / scale_group_batch) * scale_stride] (several forwards stacked along the batch, each with its own sigma).
LOCATE_API size_t locate_conv_counter_bytes(void) { return IG_MAX_COUNTERS * sizeof(unsigned); }

// counters (nullable): locate_conv_counter_bytes() bytes of device memory, ZERO before the first call that uses them and
// left zero by every completed call, not shared by launches that may run concurrently.  With counters the split-K partial
// tiles of mid-sized launches are combined inside the launch instead of by a second kernel.
LOCATE_API int locate_conv_fwd(const int* geom, const float* x, int64_t x_bs, const float* panel, const float* scale,
                               int scale_group_batch, int scale_stride, const float* bias, float* y, int64_t y_bs,
                               void* workspace, void* counters, int precision, const void* x_absmax, const void* act_epilogue,
                               void* stream) {
    const ConvGeom g = make_geom(geom);
    if (int e = geom_check(g, "locate_conv_fwd")) return e;
    LOCATE_REQUIRE(x && panel && y, "locate_conv_fwd: null pointer");
    return run_igemm(g, 0, x, x_bs, panel, scale, scale_group_batch, scale_stride, bias, y, y_bs, static_cast<float*>(workspace),
                     static_cast<unsigned*>(counters), precision, static_cast<const unsigned*>(x_absmax), as_stream(stream), "locate_conv_fwd",
                     static_cast<const LocateActEpilogue*>(act_epilogue));
}

// gx[b, c, i, j] = bias[c] + scale * sum_{m, kh, kw} gy[b, m, oh, ow] w[m, c, kh, kw],  i = oh*s - ph + kh, j = ow*s - pw + kw
// (data adjoint of R; also the FORWARD of ConvTranspose2d with weight [C_in = M, C_out = C, KH, KW]; panel: adjoint = 1).
// Every element of gx [B, C, H, W] is written.
LOCATE_API int locate_conv_dgrad(const int* geom, const float* gy, int64_t gy_bs, const float* panel, const float* scale,
                                 int scale_group_batch, int scale_stride, const float* bias, float* gx, int64_t gx_bs,
                                 void* workspace, void* counters, int precision, const void* gy_absmax, const void* act_epilogue,
                                 void* stream) {
    const ConvGeom g = make_geom(geom);
    if (int e = geom_check(g, "locate_conv_dgrad")) return e;
    LOCATE_REQUIRE(gy && panel && gx, "locate_conv_dgrad: null pointer");
    return run_igemm(g, 1, gy, gy_bs, panel, scale, scale_group_batch, scale_stride, bias, gx, gx_bs,
                     static_cast<float*>(workspace), static_cast<unsigned*>(counters), precision, static_cast<const unsigned*>(gy_absmax),
                     as_stream(stream), "locate_conv_dgrad", static_cast<const LocateActEpilogue*>(act_epilogue));
}
