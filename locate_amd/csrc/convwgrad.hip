// Weight gradients of the dense contractions (the weight adjoint of the regular convolution R of conv.hip): the general tiled
// kernels (fp32 MFMA and bf16 / fp16 / fp8 pieces), the narrow pointwise stream, the 1x1-map and one-output-pixel kernels, the
// slab reductions, and the ONE plan (wgrad_route) that every size query and every launch of them asks.
#include "igemm.h"

// ---------------------------------------------------------------------------------------------
// weight gradient:  gw[m, c, kh, kw] = sum_{b, oh, ow} gy[b, m, oh, ow] * x[b, c, oh*s-ph+kh, ow*s-pw+kw]
// GEMM rows = m, columns r = (c, kh, kw), reduction over n = (b, oh, ow) split over blockIdx.z into slabs
// (deterministic: slabs are summed in a fixed order by a second kernel).
// ---------------------------------------------------------------------------------------------
#define WG_BK 32

struct WgParams {
    const float* x;     // gathered activation [B, C, H, W]
    const float* gy;    // dense activation    [B, M, OH, OW]
    float* slab;        // [nsplit][M * R]
    long long x_bs, gy_bs;
    unsigned x_bytes;   // extent of the x view in bytes (buffer descriptor bound of the bf16 path)
    int B, C, H, W, M, OH, OW, KH, KW, stride, pad_h, pad_w;
    int R;              // C * KH * KW
    int N;              // B * OH * OW
    int chunk;          // reduction elements per split (multiple of WG_BK)
    int zper, Ng;       // splits per stacked call and reduction elements per call: split z covers elements
                        // [(z / zper) Ng + (z % zper) chunk, ...) and never crosses a call boundary (one call: zper = nsplit, Ng = N)
    unsigned q_mul, ow_mul;   // division by Q = OH*OW and by OW as multiply-high + shifts (see fastdiv)
    int q_s1, q_s2, ow_s1, ow_s2;
    // single-split launches finish in the epilogue (no slab, no reduce kernel):
    int gscale_bg, gscale_stride;   // > 0: gy of batch element b is multiplied by inv_scale[(b / gscale_bg) * gscale_stride]
                              // while it is loaded (stacked forwards with different sigma); inv_scale then is NOT
                              // applied in the epilogue
    float* direct_out;        // gw, or null when slabs are used
    const float* w_ref;       // W_bar for the fused <G, W_bar> partial sums (nullable)
    const float* inv_scale;   // device scalar 1/sigma (nullable)
    double* partial;          // one double per block (nullable)
    const unsigned* x_absmax; // fp16 pieces (NP = 2): largest magnitudes of x and of gy, AMAX_WORDS words of bit patterns each
    const unsigned* g_absmax;
};


// Shared epilogue of the weight-gradient kernels.
template <int WGM, int WGN, int TM, int TN>
__device__ __forceinline__ void wgrad_epilogue(const WgParams& p, f32x16 (&acc)[TM][TN], int r0, int m0, int wm, int wn, int lane,
                                               int wid, int tid) {
    const int lrow = lane >> 5, lcol = lane & 31;
    // epilogue.  With a single split the result is final: scale by 1/sigma, write the gradient in the weight's own
    // layout and reduce this block's share of <G, W_bar> (spectral-norm backward needs it) - no slab round trip.
    __shared__ double red[4];
    const bool direct = p.direct_out != nullptr;
    float* dst = direct ? p.direct_out : p.slab + (long long)blockIdx.z * p.M * p.R;
    const float sc = (direct && p.inv_scale && p.gscale_bg == 0) ? p.inv_scale[0] : 1.0f;
    double dot = 0.0;
    const bool want_dot = direct && p.w_ref != nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int r = r0 + (wn * TN + j) * 32 + lcol;
        const bool r_ok = r < p.R;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            // this lane's 16 rows of the 32x32 tile: W_bar values first (branch-free, all loads in flight), then the
            // products in fp32 per tile and the running sum in fp64
            float wref[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lrow;
                const bool ok = want_dot && r_ok && m < p.M;
                const float* wp_ = ok ? p.w_ref + (long long)m * p.R + r : p.gy;      // always a mapped address
                wref[e] = ok ? *wp_ : 0.0f;
            }
            float part = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lrow;
                const float v = acc[i][j][e];
                part = fmaf(v, wref[e], part);
                if (r_ok && m < p.M) dst[(long long)m * p.R + r] = v * sc;
            }
            dot += (double)part;
        }
    }
    if (direct && p.partial) {
        dot = wave_sum_d(dot);
        if (lane == 0) red[wid] = dot;
        __syncthreads();
        if (tid == 0) p.partial[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

template <int WGM, int WGN, int TM, int TN>
__global__ void __launch_bounds__(256) conv_wgrad_kernel(const WgParams p) {
    constexpr int BM = WGM * TM * 32;
    constexpr int BR = WGN * TN * 32;
    constexpr int G_PT = WG_BK * BM / 256;
    constexpr int X_PT = WG_BK * BR / 256;
    static_assert(WGM * WGN == 4, "four waves");

    __shared__ float Gs[2][WG_BK][BM + 1];
    __shared__ float Xs[2][WG_BK][BR + 1];
    __shared__ int rt_off[BR];       // c*H*W + dy*W + dx, or INT_MIN for r >= R
    __shared__ signed char rt_dy[BR], rt_dx[BR];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int r0 = blockIdx.x * BR, m0 = blockIdx.y * BM;
    const int taps = p.KH * p.KW;
    for (int i = tid; i < BR; i += 256) {
        const int r = r0 + i;
        if (r < p.R) {
            const int c = r / taps, t = r - c * taps;
            const int kh = t / p.KW, kw = t - kh * p.KW;
            rt_dy[i] = (signed char)(kh - p.pad_h);
            rt_dx[i] = (signed char)(kw - p.pad_w);
            rt_off[i] = c * p.H * p.W + (kh - p.pad_h) * p.W + (kw - p.pad_w);
        } else {
            rt_dy[i] = rt_dx[i] = 0;
            rt_off[i] = -2147483647 - 1;
        }
    }
    __syncthreads();

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int zgrp = (int)blockIdx.z / p.zper;
    const int n_begin = zgrp * p.Ng + ((int)blockIdx.z - zgrp * p.zper) * p.chunk;
    int n_end = n_begin + p.chunk;
    if (n_end > (zgrp + 1) * p.Ng) n_end = (zgrp + 1) * p.Ng;
    const int nl = tid & 31, sub = tid >> 5;   // reduction lane, row/column subgroup (0..7)
    const int Q = p.OH * p.OW;

    float greg[G_PT], xreg[X_PT];
    unsigned gmask = 0, xmask = 0;   // validity bits, applied when the tiles are written to LDS (loads are unconditional
                                     // from clamped addresses so that they all issue back to back, see conv_igemm_kernel)
    // per-thread invariants of the gathered operand: this thread always loads the same X_PT im2col columns
    int xoff[X_PT], xdyx[X_PT];
#pragma unroll
    for (int i = 0; i < X_PT; ++i) {
        const int rl = sub + 8 * i;
        xoff[i] = rt_off[rl];
        xdyx[i] = ((int)rt_dy[rl] & 0xffff) | ((int)rt_dx[rl] << 16);
    }
    // group scales (at most 4 groups) live in registers; gsc = the scale of the tile currently held in greg[]
    float gs0 = 1.0f, gs1 = 1.0f, gs2 = 1.0f, gs3 = 1.0f, gsc = 1.0f;
    if (p.gscale_bg > 0) {
        const int ng = p.B / p.gscale_bg;
        gs0 = p.inv_scale[0];
        gs1 = ng > 1 ? p.inv_scale[p.gscale_stride] : 1.0f;
        gs2 = ng > 2 ? p.inv_scale[2 * p.gscale_stride] : 1.0f;
        gs3 = ng > 3 ? p.inv_scale[3 * p.gscale_stride] : 1.0f;
    }
    auto load_tiles = [&](int nb) {
        const int n = nb + nl;
        const bool ok = n < n_end;
        const int nn = ok ? n : 0;
        const int b = fastdiv(nn, p.q_mul, p.q_s1, p.q_s2), q = nn - b * Q;
        const int oh = fastdiv(q, p.ow_mul, p.ow_s1, p.ow_s2), ow = q - oh * p.OW;
        const float* gp = p.gy + (long long)b * p.gy_bs + q;
        if (p.gscale_bg > 0) {       // group of batch element b (at most 4 groups): compares, no division in the hot loop
            const int bg = p.gscale_bg;
            gsc = gs0;
            gsc = b >= bg ? gs1 : gsc;
            gsc = b >= 2 * bg ? gs2 : gsc;
            gsc = b >= 3 * bg ? gs3 : gsc;
        }
        gmask = 0;
#pragma unroll
        for (int i = 0; i < G_PT; ++i) {
            const int m = m0 + sub + 8 * i;
            const bool v = ok && m < p.M;
            greg[i] = gp[v ? (long long)m * Q : 0];
            gmask |= (v ? 1u : 0u) << i;
        }
        const int iy0 = oh * p.stride, ix0 = ow * p.stride;
        const int base = iy0 * p.W + ix0;
        const float* xp = p.x + (long long)b * p.x_bs;       // start of batch image b
        xmask = 0;
#pragma unroll
        for (int i = 0; i < X_PT; ++i) {
            const int dy = (short)(xdyx[i] & 0xffff), dx = xdyx[i] >> 16;
            const bool v = ok && xoff[i] != (-2147483647 - 1) && (unsigned)(iy0 + dy) < (unsigned)p.H &&
                           (unsigned)(ix0 + dx) < (unsigned)p.W;
            xreg[i] = xp[v ? base + xoff[i] : 0];            // masked lanes read element 0 of the image (always valid)
            xmask |= (v ? 1u : 0u) << i;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < G_PT; ++i) Gs[buf][nl][sub + 8 * i] = ((gmask >> i) & 1u) ? greg[i] * gsc : 0.0f;
#pragma unroll
        for (int i = 0; i < X_PT; ++i) Xs[buf][nl][sub + 8 * i] = ((xmask >> i) & 1u) ? xreg[i] : 0.0f;
    };

    const int nsteps = (n_end - n_begin + WG_BK - 1) / WG_BK;
    const int lrow = lane >> 5, lcol = lane & 31;
    if (nsteps > 0) {
        load_tiles(n_begin);
        store_tiles(0);
    }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load_tiles(n_begin + (s + 1) * WG_BK);
#pragma unroll
        for (int k2 = 0; k2 < WG_BK / 2; ++k2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Gs[buf][k2 * 2 + lrow][(wm * TM + i) * 32 + lcol];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Xs[buf][k2 * 2 + lrow][(wn * TN + j) * 32 + lcol];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < nsteps) store_tiles(buf ^ 1);
        __syncthreads();
    }

    wgrad_epilogue<WGM, WGN, TM, TN>(p, acc, r0, m0, wm, wn, lane, wid, tid);
}

// ---------------------------------------------------------------------------------------------
// The weight gradient on the bf16 matrix cores with exact three-way splits (see conv_igemm_bx6_kernel).  The reduction
// index n = (b, oh, ow) is the MFMA's k: every thread loads PAIRS of adjacent n (coalesced along n), splits them and
// writes the packed bf16 pairs to LDS images [piece][row][n] (n contiguous, 32-byte rows with an XOR swizzle of the two
// halves: conflict-free ds_read_b128 fragments of 8 consecutive n; 48 KiB per block, three blocks per CU).  Needs even OH*OW and OW (a pair never straddles an image or a row).
// ---------------------------------------------------------------------------------------------
#define WB_BK 16                      // reduction elements per stage = one MFMA k
#define WB_PITCH 8                    // dwords per LDS row (16 bf16, no padding): the two 16-byte halves of a row are
                                      // swapped on rows with bit 3 set, which makes both the ds_read_b128 fragment reads
                                      // (16-lane groups = 16 consecutive rows) and the dword writes conflict-free

// NP = 4: fp8 operands (BASELINE configs[4], the arithmetic of convfp8.hip): both operands scaled into e4m3's range, rounded to e4m3
// (v_cvt_pk_fp8_f32, a pair per instruction) and multiplied on v_mfma_f32_32x32x16_fp8_fp8.  LDS rows are 16 bytes (16 consecutive
// n of one row / column); lane (r, h) reads the 8 bytes k = 8h .. 8h + 7, the two halves swapped on rows with bit 4 set (conflict-free
// ds_read_b64 over 32 rows); a thread's pair goes in as one 16-bit store.
template <int WGM, int WGN, int TM, int TN, int NP>       // NP = 3: exact splits; NP = 1: bf16 operands; NP = 2: two scaled fp16 pieces (see conv_igemm_bx6_kernel)
__global__ void __launch_bounds__(256, (WGM * TM > 4 ? 2 : 3)) conv_wgrad_bx6_kernel(const WgParams p) {
    constexpr int BM = WGM * TM * 32;
    constexpr int BR = WGN * TN * 32;
    constexpr int G_PT = BM / 32;          // row groups per thread: rows sub + 32 i
    constexpr int X_PT = BR / 32;
    static_assert(WGM * WGN == 4, "four waves");

    constexpr int NPL = NP == 4 ? 1 : NP;          // piece planes in LDS
    __shared__ unsigned Gs[2][NPL][NP == 4 ? 1 : BM][WB_PITCH];
    __shared__ unsigned Xs[2][NPL][NP == 4 ? 1 : BR][WB_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned short G8[2][NP == 4 ? BM : 1][8];          // fp8: 16 bytes per row, addressed in pairs
    __shared__ __attribute__((aligned(16))) unsigned short X8[2][NP == 4 ? BR : 1][8];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int r0 = blockIdx.x * BR, m0 = blockIdx.y * BM;
    const int taps = p.KH * p.KW;
    const int np = tid & 7, sub = tid >> 3;      // pair index inside the stage (n = nb + 2 np), row/column subgroup 0..31
    const int Q = p.OH * p.OW;

    // per-thread invariants of the gathered operand: this thread always loads the same X_PT im2col columns
    int xoff[X_PT], xdy[X_PT], xdx[X_PT];
#pragma unroll
    for (int i = 0; i < X_PT; ++i) {
        const int r = r0 + sub + 32 * i;
        if (r < p.R) {
            const int c = r / taps, t = r - c * taps;
            const int kh = t / p.KW, kw = t - kh * p.KW;
            xdy[i] = kh - p.pad_h;
            xdx[i] = kw - p.pad_w;
            xoff[i] = 4 * (c * p.H * p.W + xdy[i] * p.W + xdx[i]);
        } else {
            xdy[i] = -(1 << 20);               // never inside the input
            xdx[i] = 0;
            xoff[i] = 0;
        }
    }
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)p.x_bytes, 0x00020000);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int zgrp = (int)blockIdx.z / p.zper;
    const int n_begin = zgrp * p.Ng + ((int)blockIdx.z - zgrp * p.zper) * p.chunk;
    int n_end = n_begin + p.chunk;
    if (n_end > (zgrp + 1) * p.Ng) n_end = (zgrp + 1) * p.Ng;

    // group scales (at most 4 groups) live in registers; gsc = the scale of the pairs currently held in greg[]
    float gs0 = 1.0f, gs1 = 1.0f, gs2 = 1.0f, gs3 = 1.0f, gsc = 1.0f;
    if (p.gscale_bg > 0) {
        const int ng = p.B / p.gscale_bg;
        gs0 = p.inv_scale[0];
        gs1 = ng > 1 ? p.inv_scale[p.gscale_stride] : 1.0f;
        gs2 = ng > 2 ? p.inv_scale[2 * p.gscale_stride] : 1.0f;
        gs3 = ng > 3 ? p.inv_scale[3 * p.gscale_stride] : 1.0f;
    }

    // fp16 pieces: both operands go through powers of two into fp16's range (gy after its per-call 1/sigma, whose largest
    // value bounds the product), the exact inverses are applied to the accumulators after the loop
    float g_scale = 1.0f, x_scale = 1.0f, g_unscale = 1.0f, x_unscale = 1.0f;
    if constexpr (NP == 2) {
        const float gmax = __uint_as_float(absmax_read(p.g_absmax)) * fmaxf(fmaxf(gs0, gs1), fmaxf(gs2, gs3));
        const int kg_ = f16_scale_exp(__float_as_uint(gmax), p.gscale_bg > 0 ? 1u : 0u);    // (product rounded: one binade of slack)
        const int kx_ = f16_scale_exp(absmax_read(p.x_absmax));
        g_scale = pow2f(kg_); x_scale = pow2f(kx_);
        unscale_pair(kg_, kx_, g_unscale, x_unscale);
    }
    if constexpr (NP == 4) {
        const float gmax = __uint_as_float(absmax_read(p.g_absmax)) * fmaxf(fmaxf(gs0, gs1), fmaxf(gs2, gs3));
        const int kg_ = f8_scale_exp(__float_as_uint(gmax), p.gscale_bg > 0 ? 1u : 0u);
        const int kx_ = f8_scale_exp(absmax_read(p.x_absmax));
        g_scale = pow2f(kg_); x_scale = pow2f(kx_);
        unscale_pair(kg_, kx_, g_unscale, x_unscale);
    }
    // a pair of values rounded to e4m3: two bytes
    auto q8_pair = [](float v0, float v1) { return (unsigned short)(__builtin_amdgcn_cvt_pk_fp8_f32(v0, v1, 0, false) & 0xffff); };
    // pair np of a row: halfword (np & 3) of the row's 8-byte half np >> 2, the halves swapped on rows with bit 4 set
    auto h8 = [](int row, int pair) { return ((((pair >> 2) ^ (row >> 4)) & 1) << 2) | (pair & 3); };

    float2 greg[G_PT], xreg[X_PT];
    auto load_tiles = [&](int nb) {
        const int n = nb + 2 * np;                 // even; n + 1 is in the same image and output row
        const bool ok = n < n_end;                 // n_end is even as well
        const int nn = ok ? n : 0;
        const int b = fastdiv(nn, p.q_mul, p.q_s1, p.q_s2), q = nn - b * Q;
        const int oh = fastdiv(q, p.ow_mul, p.ow_s1, p.ow_s2), ow = q - oh * p.OW;
        const float* gp = p.gy + (long long)b * p.gy_bs + q;
        if (p.gscale_bg > 0) {       // group of batch element b (at most 4 groups): compares, no division in the hot loop
            const int bg = p.gscale_bg;
            gsc = gs0;
            gsc = b >= bg ? gs1 : gsc;
            gsc = b >= 2 * bg ? gs2 : gsc;
            gsc = b >= 3 * bg ? gs3 : gsc;
        }
#pragma unroll
        for (int i = 0; i < G_PT; ++i) {
            const int m = m0 + sub + 32 * i;
            const bool v = ok && m < p.M;
            const float2 t = *reinterpret_cast<const float2*>(gp + (v ? (long long)m * Q : 0));
            greg[i] = v ? t : make_float2(0.0f, 0.0f);
        }
        const int iy0 = oh * p.stride, ix0 = ow * p.stride;
        const unsigned base = (unsigned)(4 * ((long long)b * p.x_bs + (long long)iy0 * p.W + ix0));
#pragma unroll
        for (int i = 0; i < X_PT; ++i) {
            const bool vy = ok && (unsigned)(iy0 + xdy[i]) < (unsigned)p.H;
            const bool v0 = vy && (unsigned)(ix0 + xdx[i]) < (unsigned)p.W;
            const bool v1 = vy && (unsigned)(ix0 + p.stride + xdx[i]) < (unsigned)p.W;
            const unsigned o = base + (unsigned)xoff[i];
            // an out-of-range voffset makes the buffer load return 0 without touching memory (zero padding)
            xreg[i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, (int)(v0 ? o : 0x80000000u), 0, 0));
            xreg[i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, (int)(v1 ? o + 4u * (unsigned)p.stride : 0x80000000u), 0, 0));
        }
    };
    // dword column of this thread's pair inside its rows: rows sub + 32 i all have bit 3 of `sub`
    const int wcol = (((np >> 2) ^ ((sub >> 3) & 1)) << 2) | (np & 3);
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < G_PT; ++i) {
            if constexpr (NP == 2) {
                unsigned h, l;
                split2_f16_pair(greg[i].x * gsc * g_scale, greg[i].y * gsc * g_scale, h, l);
                Gs[buf][0][sub + 32 * i][wcol] = h;
                Gs[buf][NP - 1][sub + 32 * i][wcol] = l;
            } else if constexpr (NP == 3) {
                unsigned h, m, l;
                split3_trunc_pair(greg[i].x * gsc, greg[i].y * gsc, h, m, l);
                Gs[buf][0][sub + 32 * i][wcol] = h;
                Gs[buf][NP - 2][sub + 32 * i][wcol] = m;
                Gs[buf][NP - 1][sub + 32 * i][wcol] = l;
            } else if constexpr (NP == 4) {
                G8[buf][sub + 32 * i][h8(sub + 32 * i, np)] = q8_pair(greg[i].x * gsc * g_scale, greg[i].y * gsc * g_scale);
            } else {
                Gs[buf][0][sub + 32 * i][wcol] = round_bf16_pair(greg[i].x * gsc, greg[i].y * gsc);
            }
        }
#pragma unroll
        for (int i = 0; i < X_PT; ++i) {
            if constexpr (NP == 2) {
                unsigned h, l;
                split2_f16_pair(xreg[i].x * x_scale, xreg[i].y * x_scale, h, l);
                Xs[buf][0][sub + 32 * i][wcol] = h;
                Xs[buf][NP - 1][sub + 32 * i][wcol] = l;
            } else if constexpr (NP == 3) {
                unsigned h, m, l;
                split3_trunc_pair(xreg[i].x, xreg[i].y, h, m, l);
                Xs[buf][0][sub + 32 * i][wcol] = h;
                Xs[buf][NP - 2][sub + 32 * i][wcol] = m;
                Xs[buf][NP - 1][sub + 32 * i][wcol] = l;
            } else if constexpr (NP == 4) {
                X8[buf][sub + 32 * i][h8(sub + 32 * i, np)] = q8_pair(xreg[i].x * x_scale, xreg[i].y * x_scale);
            } else {
                Xs[buf][0][sub + 32 * i][wcol] = round_bf16_pair(xreg[i].x, xreg[i].y);
            }
        }
    };

    const int nsteps = (n_end - n_begin + WB_BK - 1) / WB_BK;
    const int lrow = lane >> 5, lcol = lane & 31;
    const int rhalf = lrow ^ ((lcol >> 3) & 1);          // fragment rows are tile_row0 + lcol with tile_row0 % 32 == 0
    // same software pipeline as conv_igemm_bx6_kernel: the next tile is split and written, and the loads of the one after
    // it re-issued, between the two halves of a stage's MFMAs
    if (nsteps > 0) {
        load_tiles(n_begin);
        store_tiles(0);
        load_tiles(n_begin + WB_BK);                 // beyond n_end: every lane masked, nothing is read
    }
    __syncthreads();
    constexpr int PROD = NP == 3 ? 6 : (NP == 2 ? 3 : 1);
    constexpr int NMF = TM * TN * PROD, HALF = NMF / 2;
    using frag_t = typename std::conditional<NP == 2, f16x8, bf16x8>::type;
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        frag_t a[TM][NPL], b[TN][NPL];
        long a8[TM], b8[TN];
        if constexpr (NP == 4) {
            const int half8 = (lrow ^ (lcol >> 4)) & 1;          // (tile rows start at multiples of 32: bit 4 of the row = bit 4 of lcol)
#pragma unroll
            for (int i = 0; i < TM; ++i) a8[i] = *reinterpret_cast<const long*>(&G8[buf][(wm * TM + i) * 32 + lcol][half8 * 4]);
#pragma unroll
            for (int j = 0; j < TN; ++j) b8[j] = *reinterpret_cast<const long*>(&X8[buf][(wn * TN + j) * 32 + lcol][half8 * 4]);
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < NPL; ++q) a[i][q] = *reinterpret_cast<const frag_t*>(&Gs[buf][q][(wm * TM + i) * 32 + lcol][rhalf * 4]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) b[j][q] = *reinterpret_cast<const frag_t*>(&Xs[buf][q][(wn * TN + j) * 32 + lcol][rhalf * 4]);
        }
        auto mfmas = [&](int lo, int hi) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int base = (i * TN + j) * PROD;
                    if constexpr (NP == 2) {
                        if (base + 0 >= lo && base + 0 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);   // l h
                        if (base + 1 >= lo && base + 1 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);   // h l
                        if (base + 2 >= lo && base + 2 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);   // h h
                    } else if constexpr (NP == 3) {
                        if (base + 0 >= lo && base + 0 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 1], b[j][0], acc[i][j], 0, 0, 0);   // l h
                        if (base + 1 >= lo && base + 1 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 1], acc[i][j], 0, 0, 0);   // h l
                        if (base + 2 >= lo && base + 2 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][NP - 2], acc[i][j], 0, 0, 0);   // m m
                        if (base + 3 >= lo && base + 3 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][0], acc[i][j], 0, 0, 0);   // m h
                        if (base + 4 >= lo && base + 4 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 2], acc[i][j], 0, 0, 0);   // h m
                        if (base + 5 >= lo && base + 5 < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);   // h h
                    } else if constexpr (NP == 4) {
                        if (base >= lo && base < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a8[i], b8[j], acc[i][j], 0, 0, 0);
                    } else {
                        if (base >= lo && base < hi) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                    }
                }
        };
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0, HALF);
        __builtin_amdgcn_sched_barrier(0);
        store_tiles(buf ^ 1);                               // tile s + 1
        load_tiles(n_begin + (s + 2) * WB_BK);              // tile s + 2
        __builtin_amdgcn_sched_barrier(0);
        mfmas(HALF, NMF);
        __syncthreads();
    }
    if constexpr (NP == 2 || NP == 4) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] * g_unscale) * x_unscale;
    }
    wgrad_epilogue<WGM, WGN, TM, TN>(p, acc, r0, m0, wm, wn, lane, wid, tid);
}

// out = (sum_z slab[z]) * inv_scale;  partial[block] = this block's share of <sum_z slab[z], w_ref>.
// ZP = 1: one thread per element walks all slabs.  ZP = 4: four z-groups per element (many slabs, few elements: the
// 1x1 / attention layers), combined through LDS in a fixed order - results stay bit-reproducible.
// Stacked calls (groups > 1; the slabs of call k are z = k zper ... (k + 1) zper - 1, each already weighted by 1 / sigma_k):
// the block emits one partial of <G_k / sigma_k, W_bar> PER CALL (partial[k * nblocks + bid]) - what the spectral-norm backward
// of stacked calls needs for d(sigma_k), from slab values this pass reads anyway (the activation-side dots <gy_k, y_k - b>
// it replaces read both activations of every layer once more).
// V = 4: four consecutive elements per thread (16-byte accesses, n % 4 == 0) - the same additions per element in the same order
// as V = 1 (whose 4-byte accesses in 64-byte runs reached 1.5 TB/s on the 150 MB of a generator pass's slabs).
template <int V>
__device__ __forceinline__ void slab_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}

template <int ZP, int V>
__device__ __forceinline__ void slab_reduce_groups(const float* __restrict__ slab, float* __restrict__ out, int64_t n, int nsplit,
                                                   const float* __restrict__ w_ref, double* __restrict__ partial, int bid, int nblocks,
                                                   int groups, int zper, float* zbuf, double* gscratch) {
    float (*gzsum)[ZP][256 / ZP][V] = reinterpret_cast<float (*)[ZP][256 / ZP][V]>(zbuf);          // [4][ZP][256 / ZP][V]
    constexpr int TPB = 256 / ZP, EPB = TPB * V;
    const int ex = threadIdx.x % TPB, ez = threadIdx.x / TPB;
    const int64_t stride = (int64_t)nblocks * EPB;
    double dot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i0 = (int64_t)bid * EPB; i0 < n; i0 += stride) {
        const int64_t i = i0 + V * ex;
        float acc[4][V];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[k][e] = 0.0f;
        if (i < n) {
            // z walks ALL slabs, call-major, eight loads in flight; slab z belongs to call z / zper and is added to that call's sum
            // (the other calls' sums take + 0.0f: exact), in z order within each call
            const float* __restrict__ sp = slab + i;
            for (int z = ez; z < nsplit; z += 8 * ZP) {
                float v[8][V];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (z + q * ZP < nsplit) slab_load<V>(sp + (int64_t)(z + q * ZP) * n, v[q]);
                    else
#pragma unroll
                        for (int e = 0; e < V; ++e) v[q][e] = 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int zz = z + q * ZP;
                    const int k = (zz >= zper) + (zz >= 2 * zper) + (zz >= 3 * zper);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        acc[0][e] += k == 0 ? v[q][e] : 0.0f;
                        acc[1][e] += k == 1 ? v[q][e] : 0.0f;
                        acc[2][e] += k == 2 ? v[q][e] : 0.0f;
                        acc[3][e] += k == 3 ? v[q][e] : 0.0f;
                    }
                }
            }
        }
        if (ZP > 1) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < V; ++e) gzsum[k][ez][ex][e] = acc[k][e];
            __syncthreads();
            if (ez == 0)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        float a = 0.0f;
#pragma unroll
                        for (int g = 0; g < ZP; ++g) a += gzsum[k][g][ex][e];
                        acc[k][e] = a;
                    }
        }
        if (ez == 0 && i < n) {
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double w = w_ref ? (double)w_ref[i + e] : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) dot[k] += (double)acc[k][e] * w;
                o[e] = ((acc[0][e] + acc[1][e]) + acc[2][e]) + acc[3][e];          // calls beyond `groups` contribute + 0.0f: exact
            }
            if constexpr (V == 4) *reinterpret_cast<float4*>(out + i) = make_float4(o[0], o[1], o[2], o[3]);
            else out[i] = o[0];
        }
    }
    if (partial) {
        for (int k = 0; k < groups; ++k) {
            const double t = block_sum<double>(dot[k], gscratch);
            if (threadIdx.x == 0) partial[(int64_t)k * nblocks + bid] = t;
        }
    }
}

template <int ZP, int V>
__device__ __forceinline__ void slab_reduce_body_v(const float* __restrict__ slab, float* __restrict__ out, int64_t n, int nsplit,
                                                   const float* __restrict__ w_ref, const float* __restrict__ inv_scale,
                                                   double* __restrict__ partial, int bid, int nblocks, int groups, int zper,
                                                   float* zbuf, double* scratch) {
    if (groups > 1) {
        slab_reduce_groups<ZP, V>(slab, out, n, nsplit, w_ref, partial, bid, nblocks, groups, zper, zbuf, scratch);
        return;
    }
    float (*zsum)[256 / ZP][V] = reinterpret_cast<float (*)[256 / ZP][V]>(zbuf);          // [ZP][256 / ZP][V]
    const float sc = inv_scale ? inv_scale[0] : 1.0f;
    constexpr int TPB = 256 / ZP, EPB = TPB * V;        // threads / elements per block pass
    const int ex = threadIdx.x % TPB, ez = threadIdx.x / TPB;
    const int64_t stride = (int64_t)nblocks * EPB;
    double dot = 0.0;
    for (int64_t i0 = (int64_t)bid * EPB; i0 < n; i0 += stride) {
        const int64_t i = i0 + V * ex;
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.0f;
        if (i < n) {
            // eight slabs' loads in flight, added in z order
            const float* __restrict__ sp = slab + i;
            for (int z = ez; z < nsplit; z += 8 * ZP) {
                float v[8][V];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (z + q * ZP < nsplit) slab_load<V>(sp + (int64_t)(z + q * ZP) * n, v[q]);
                    else
#pragma unroll
                        for (int e = 0; e < V; ++e) v[q][e] = 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += v[q][e];      // + 0.0f beyond nsplit: exact
            }
        }
        if (ZP > 1) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < V; ++e) zsum[ez][ex][e] = acc[e];
            __syncthreads();
            if (ez == 0)
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float a = 0.0f;
#pragma unroll
                    for (int g = 0; g < ZP; ++g) a += zsum[g][ex][e];
                    acc[e] = a;
                }
        }
        if (ez == 0 && i < n) {
            if (w_ref)
#pragma unroll
                for (int e = 0; e < V; ++e) dot += (double)acc[e] * (double)w_ref[i + e];
            if constexpr (V == 4) *reinterpret_cast<float4*>(out + i) = make_float4(acc[0] * sc, acc[1] * sc, acc[2] * sc, acc[3] * sc);
            else out[i] = acc[0] * sc;
        }
    }
    if (partial) {
        dot = block_sum<double>(dot, scratch);
        if (threadIdx.x == 0) partial[bid] = dot;
    }
}

template <int ZP>
__device__ __forceinline__ void slab_reduce_body(const float* __restrict__ slab, float* __restrict__ out, int64_t n, int nsplit,
                                                 const float* __restrict__ w_ref, const float* __restrict__ inv_scale,
                                                 double* __restrict__ partial, int bid, int nblocks, int groups = 0, int zper = 0) {
    // one LDS area for whichever form runs: [4 calls][256 threads][4 values]
    __shared__ __attribute__((aligned(16))) float zbuf[4 * 256 * 4];
    __shared__ double scratch[16];
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(slab) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    // (ZP = 16 - a handful of elements under hundreds of slabs - stays scalar: its sixteen-way LDS sums times four values spill)
    if constexpr (ZP <= 4) {
        if (vec) {
            slab_reduce_body_v<ZP, 4>(slab, out, n, nsplit, w_ref, inv_scale, partial, bid, nblocks, groups, zper, zbuf, scratch);
            return;
        }
    }
    slab_reduce_body_v<ZP, 1>(slab, out, n, nsplit, w_ref, inv_scale, partial, bid, nblocks, groups, zper, zbuf, scratch);
}

template <int ZP>
__global__ void __launch_bounds__(256, 4) slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int64_t n,
                                                          int nsplit, const float* __restrict__ w_ref,
                                                          const float* __restrict__ inv_scale, double* __restrict__ partial,
                                                          int groups, int zper) {
    slab_reduce_body<ZP>(slab, out, n, nsplit, w_ref, inv_scale, partial, blockIdx.x, gridDim.x, groups, zper);
}

// The split reductions of ALL weight gradients of one backward pass in one launch: a weight gradient only feeds a parameter
// gradient, so its slab sum can wait for the end of the pass like the other finalisers (finalise.hip) - each of the ~30 per
// iteration is a launch-floor-sized kernel behind its GEMM.  Records by value; per layer the same blocks, the same z order and
// the same <G, W_bar> partials as the single launch.
struct SlabRec {
    const float* slab; float* out; const float* w_ref; const float* inv_scale; double* partial;
    long long n;
    int nsplit, zp, grid, block0, groups, zper;
};
#define SLAB_MAX 32
struct SlabBatch {
    SlabRec r[SLAB_MAX];
};

__global__ void __launch_bounds__(256, 4) slab_reduce_batch_kernel(const SlabBatch b, int nrec) {
    int k = 0;
    for (int i = 1; i < nrec; ++i)
        if ((int)blockIdx.x >= b.r[i].block0) k = i;          // block0 ascending
    const SlabRec& r = b.r[k];
    const int bid = (int)blockIdx.x - r.block0;
    if (r.zp == 16) slab_reduce_body<16>(r.slab, r.out, r.n, r.nsplit, r.w_ref, r.inv_scale, r.partial, bid, r.grid, r.groups, r.zper);
    else if (r.zp == 4) slab_reduce_body<4>(r.slab, r.out, r.n, r.nsplit, r.w_ref, r.inv_scale, r.partial, bid, r.grid, r.groups, r.zper);
    else slab_reduce_body<1>(r.slab, r.out, r.n, r.nsplit, r.w_ref, r.inv_scale, r.partial, bid, r.grid, r.groups, r.zper);
}

// The general tiled kernels' plan: tile height, the split of the reduction over blockIdx.z, the (m, r) tile count.
// groups > 1 (stacked calls whose per-call <G_k, W_bar> the reduction is to emit): every call's share of the reduction is split on
// its own - nsplit = groups x zper slabs, none crossing a call boundary, at least one slab per call.  One call: zper = nsplit.
static void wgrad_plan(const ConvGeom& g, int groups, int* bm, int* nsplit, int* chunk, int* zper, int* tiles_out) {
    *bm = pick_bm(g.M);
    const int R = g.C * g.KH * g.KW;
    // tall 192 x 128 tiles (96 x 64 per wave: a third more MFMAs per gathered and split element, two blocks per CU) for the wide
    // layers, as in the forward kernels (same-box A/B of the step: 9.031 / 9.039 -> 9.010 / 8.997 ms); paired-load kernels only
    if (g.M % 192 == 0 && ((g.OH * g.OW) & 1) == 0 && (g.OW & 1) == 0 && knob_int("LOCATE_WG_TALL", 1) && !path_disabled("wbx6") && (int64_t)(g.M / 192) * ((R + 127) / 128) >= knob_int("LOCATE_WG_TALL_MIN_TILES", 24)) *bm = 192;
    const int64_t slots = *bm == 192 ? 512 : 768;
    const int64_t tiles = (int64_t)((g.M + *bm - 1) / *bm) * ((R + 127) / 128);
    const int64_t calls = groups > 1 ? groups : 1;
    const int64_t Ng = (int64_t)(g.B / calls) * g.OH * g.OW;          // reduction elements per call
    // Split each call's reduction over s blocks per tile so that the launch fills whole rounds of the 768 resident blocks
    // (256 CUs x 3): cost(s) = rounds(s) x reduction elements per block, plus the slab traffic of more than one slab expressed in
    // the same unit (one output tile written and re-read ~ 96 reduction elements of MFMA time).
    const int wg_min = knob_int("LOCATE_WG_MIN_CHUNK", 64);
    const int64_t max_split = Ng >= 2 * wg_min ? Ng / wg_min : 1;     // at least 64 reduction elements per block (the split
    // reductions of a pass run as ONE batched launch at its end, so a deeper split costs slab traffic only: the deep layers' 8 - 24
    // tiles x 3 splits of 256 were latency chains of 16 steps on a tenth of the chip; same-box A/B of the step: 256 -> 9.13 / 9.12,
    // 128 -> 9.06 / 9.05, 64 -> 9.05 / 9.03, 32 -> 9.06 / 9.06 ms)
    int64_t best_s = 1;
    double best_cost = 1e300;
    for (int64_t s_ = 1; s_ <= max_split && s_ * calls <= 512; ++s_) {
        int64_t ch = (Ng + s_ - 1) / s_;
        ch = (ch + WG_BK - 1) / WG_BK * WG_BK;
        const int64_t ns = calls * ((Ng + ch - 1) / ch);
        const int64_t rounds = (tiles * ns + slots - 1) / slots;
        const double cost = (double)rounds * (double)ch + (ns > 1 ? 96.0 * (double)ns * (double)tiles / (double)slots : 0.0);
        if (cost < best_cost * 0.999) { best_cost = cost; best_s = s_; }
    }
    int64_t ch = (Ng + best_s - 1) / best_s;
    ch = (ch + WG_BK - 1) / WG_BK * WG_BK;
    *chunk = (int)ch;
    *zper = (int)((Ng + ch - 1) / ch);
    *nsplit = (int)calls * *zper;
    *tiles_out = (int)tiles;
}

static int wgrad_reduce_zp(int nsplit, int64_t n) {
    // few outputs, many slabs: 16 threads share one output element - below 4096 elements only: from there on the four-way form with
    // its 16-byte accesses is faster (same-call A/B of the step, threshold 65536 / 16384 / 4096 / 1024: 8.97, 8.96 / 8.95, 8.96 / 8.92,
    // 8.94 / 8.94, 8.96 ms)
    if (nsplit >= 64 && n < knob_int("LOCATE_ZP16_MAX_N", 1 << 12)) return 16;
    return (nsplit >= 16 && n < (1 << 20)) ? 4 : 1;
}
static int wgrad_reduce_grid(int64_t n, int nsplit) {
    const int epb = 256 / wgrad_reduce_zp(nsplit, n);
    int g = stream_grid(n, epb);
    return g > 2048 ? 2048 : g;
}

// ---------------------------------------------------------------------------------------------
// Weight gradient of 1x1 stride-1 layers with few channels on both sides (<= 128: the attention gates' convs, the skip
// branches' 1x1 convs, the generator's head) over many pixels:  gw[m][c] = sum_{b, p} gy[b][m][p] x[b][c][p].
// Both operands are contiguous along the reduction index p, which is exactly the MFMA fragment layout (lane (r, h) holds
// k = 8h .. 8h + 7 of row r): every wave loads its fragments straight from global memory - two 16-byte loads per fragment
// row - splits them in registers and multiplies; no LDS image, no barrier, no gather tables in the loop.  These launches
// are HBM streams (a 64 x 64 output tile per wave against 8 KB of operands per 16 pixels); the general kernel above, built
// for wide layers, ran them at 15-25 % of that.  A wave owns one (row tile, column tile) and a contiguous run of 16-pixel
// steps; the four waves of a block add their tiles in wave order through LDS and write one slab, summed (with 1/sigma and
// the <G, W_bar> partials) by slab_reduce_kernel like every split weight gradient.
// ---------------------------------------------------------------------------------------------
struct PwParams {
    const float* x;
    const float* gy;
    float* slab;
    const float* inv_scale;
    long long x_bs, gy_bs;
    int B, C, M, P;            // P = H * W
    int N;                     // B * P
    int steps, chunk;          // 16-pixel steps in all, steps per wave
    int tiles_c;
    int gscale_bg, gscale_stride;
    const unsigned* x_absmax;  // NP = 2 (two scaled fp16 pieces, three MFMAs - conv_igemm_bx6_kernel's form): largest magnitudes of
    const unsigned* g_absmax;  // x and of gy, AMAX_WORDS words each
};

template <int TM, int TN, int NP>
__global__ void __launch_bounds__(256) pw_wgrad_kernel(const PwParams p) {
    __shared__ float red[3][TM * TN * 16][64];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lrow = lane >> 5, lcol = lane & 31;
    const int tm = blockIdx.y / p.tiles_c, tc = blockIdx.y - tm * p.tiles_c;
    const int m0 = tm * (TM * 32), c0 = tc * (TN * 32);
    const int z = blockIdx.x * 4 + wid;
    const int s_begin = z * p.chunk;
    int s_end = s_begin + p.chunk;
    if (s_end > p.steps) s_end = p.steps;

    float gs0 = 1.0f, gs1 = 1.0f, gs2 = 1.0f, gs3 = 1.0f;
    if (p.gscale_bg > 0) {
        const int ng = p.B / p.gscale_bg;
        gs0 = p.inv_scale[0];
        gs1 = ng > 1 ? p.inv_scale[p.gscale_stride] : 1.0f;
        gs2 = ng > 2 ? p.inv_scale[2 * p.gscale_stride] : 1.0f;
        gs3 = ng > 3 ? p.inv_scale[3 * p.gscale_stride] : 1.0f;
    }
    // rows of this lane's fragments (clamped to a valid row; masked when beyond the tensor)
    long long arow[TM], brow[TN];
    bool aok[TM], bok[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + i * 32 + lcol;
        aok[i] = m < p.M;
        arow[i] = (long long)(aok[i] ? m : 0) * p.P;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int c = c0 + j * 32 + lcol;
        bok[j] = c < p.C;
        brow[j] = (long long)(bok[j] ? c : 0) * p.P;
    }
    const DivU32 dp((unsigned)p.P);
    float x_scale = 1.0f, g_scale = 1.0f, x_unscale = 1.0f, g_unscale = 1.0f;
    if constexpr (NP == 2) {          // powers of two into fp16's range; the exact inverses go back in after the loop
        const int kx = f16_scale_exp(absmax_read(p.x_absmax)), kg = f16_scale_exp(absmax_read(p.g_absmax));
        x_scale = pow2f(kx); g_scale = pow2f(kg);
        unscale_pair(kg, kx, g_unscale, x_unscale);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    float4 ca[TM][2], cb[TN][2], na[TM][2], nb[TN][2];
    float csc = 1.0f, nsc = 1.0f;
    auto load = [&](int s, float4 (&fa)[TM][2], float4 (&fb)[TN][2], float& sc) {
        // this lane's eight pixels n .. n + 7 of step s (P % 8 == 0: they lie in one image)
        const unsigned n = (unsigned)s * 16u + 8u * (unsigned)lrow;
        const bool ok = s < s_end && n < (unsigned)p.N;
        unsigned b, q;
        dp.divmod(ok ? n : 0u, b, q);
        const float* gp = p.gy + (long long)b * p.gy_bs + q;
        const float* xp = p.x + (long long)b * p.x_bs + q;
        sc = 1.0f;
        if (p.gscale_bg > 0) {
            const int bg = p.gscale_bg;
            sc = gs0;
            sc = (int)b >= bg ? gs1 : sc;
            sc = (int)b >= 2 * bg ? gs2 : sc;
            sc = (int)b >= 3 * bg ? gs3 : sc;
        }
        if (!ok) sc = 0.0f;                                  // beyond this wave's run: the loads below are valid, the values dropped
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float4* g4 = reinterpret_cast<const float4*>(gp + arow[i]);
            fa[i][0] = g4[0];
            fa[i][1] = g4[1];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float4* x4 = reinterpret_cast<const float4*>(xp + brow[j]);
            fb[j][0] = x4[0];
            fb[j][1] = x4[1];
        }
    };
    if (s_begin < s_end) load(s_begin, ca, cb, csc);
    for (int s = s_begin; s < s_end; ++s) {
        load(s + 1, na, nb, nsc);
        using pfrag_t = typename std::conditional<NP == 2, f16x8, bf16x8>::type;
        pfrag_t a[TM][NP], b[TN][NP];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float w = aok[i] ? csc : 0.0f;
            float v[8] = {ca[i][0].x * w, ca[i][0].y * w, ca[i][0].z * w, ca[i][0].w * w,
                          ca[i][1].x * w, ca[i][1].y * w, ca[i][1].z * w, ca[i][1].w * w};
            if constexpr (NP == 2) {
                uint4 h, l;
                split2_f16x8(v, g_scale, h, l);
                a[i][0] = *reinterpret_cast<pfrag_t*>(&h);
                a[i][NP - 1] = *reinterpret_cast<pfrag_t*>(&l);
            } else if constexpr (NP == 3) {
                uint4 h, m, l;
                split3_trunc_x8(v, h, m, l);
                a[i][0] = *reinterpret_cast<pfrag_t*>(&h);
                a[i][NP - 2] = *reinterpret_cast<pfrag_t*>(&m);
                a[i][NP - 1] = *reinterpret_cast<pfrag_t*>(&l);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[i][0][e] = (__bf16)v[e];
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float w = (bok[j] && csc != 0.0f) ? 1.0f : 0.0f;
            float v[8] = {cb[j][0].x * w, cb[j][0].y * w, cb[j][0].z * w, cb[j][0].w * w,
                          cb[j][1].x * w, cb[j][1].y * w, cb[j][1].z * w, cb[j][1].w * w};
            if constexpr (NP == 2) {
                uint4 h, l;
                split2_f16x8(v, x_scale, h, l);
                b[j][0] = *reinterpret_cast<pfrag_t*>(&h);
                b[j][NP - 1] = *reinterpret_cast<pfrag_t*>(&l);
            } else if constexpr (NP == 3) {
                uint4 h, m, l;
                split3_trunc_x8(v, h, m, l);
                b[j][0] = *reinterpret_cast<pfrag_t*>(&h);
                b[j][NP - 2] = *reinterpret_cast<pfrag_t*>(&m);
                b[j][NP - 1] = *reinterpret_cast<pfrag_t*>(&l);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) b[j][0][e] = (__bf16)v[e];
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (NP == 2) {          // smallest terms first: l h, h l, h h
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][NP - 1], b[j][0], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][NP - 1], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                } else if constexpr (NP == 3) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 1], b[j][0], acc[i][j], 0, 0, 0);        // l h
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 1], acc[i][j], 0, 0, 0);        // h l
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][NP - 2], acc[i][j], 0, 0, 0);   // m m
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][NP - 2], b[j][0], acc[i][j], 0, 0, 0);        // m h
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][NP - 2], acc[i][j], 0, 0, 0);        // h m
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);             // h h
                } else {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
                }
            }
#pragma unroll
        for (int i = 0; i < TM; ++i) { ca[i][0] = na[i][0]; ca[i][1] = na[i][1]; }
#pragma unroll
        for (int j = 0; j < TN; ++j) { cb[j][0] = nb[j][0]; cb[j][1] = nb[j][1]; }
        csc = nsc;
    }
    if constexpr (NP == 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] * g_unscale) * x_unscale;
    }
    // the block's four tiles, added in wave order; wave 0 writes the slab
    if (wid > 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[wid - 1][(i * TN + j) * 16 + r][lane] = acc[i][j][r];
    }
    __syncthreads();
    if (wid != 0) return;
    float* out = p.slab + (long long)blockIdx.x * p.M * p.C;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int c = c0 + j * 32 + lcol;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
                const int e = (i * TN + j) * 16 + r;
                const float v = ((acc[i][j][r] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane];
                if (m < p.M && c < p.C) out[(long long)m * p.C + c] = v;
            }
        }
}

struct PwPlan {
    bool ok;
    int tm, tn, tiles_m, tiles_c, steps, chunk, nslab, zper;
};

// groups > 1: the slabs are to stay inside one stacked call each (see wgrad_plan); q.zper slabs per call, or q.zper = 0 when the
// call length does not divide into whole blocks of four wave runs (the caller then takes the dots on the activation side)
static PwPlan pw_plan(const ConvGeom& g, int groups = 0) {
    PwPlan q;
    q.zper = 0;
    const long long P = (long long)g.H * g.W;
    q.ok = !path_disabled("pwgrad") && g.KH == 1 && g.KW == 1 && g.stride == 1 && g.pad_h == 0 && g.pad_w == 0 && g.OH == g.H &&
           g.OW == g.W && (P % 8) == 0 && g.M <= 128 && g.C <= 128 && (long long)g.B * P >= 4096 && (long long)g.B * P < (1ll << 31);
    q.tm = g.M <= 32 ? 1 : 2;
    q.tn = g.C <= 32 ? 1 : 2;
    q.tiles_m = (g.M + q.tm * 32 - 1) / (q.tm * 32);
    q.tiles_c = (g.C + q.tn * 32 - 1) / (q.tn * 32);
    const long long N = (long long)g.B * P;
    q.steps = (int)((N + 15) / 16);
    // ~2048 waves (two per SIMD) over all tiles, at least 8 steps each
    const int tiles = q.tiles_m * q.tiles_c;
    int waves = 2048 / tiles;
    if (waves < 4) waves = 4;
    int chunk = (q.steps + waves - 1) / waves;
    if (chunk < 8) chunk = 8;
    if (groups > 1 && q.ok) {
        const long long per = ((long long)(g.B / groups) * P) / 16;          // 16-pixel steps per call
        if (((long long)(g.B / groups) * P) % 64 != 0) return q;             // zper stays 0
        while (chunk > 4 && per % (4ll * chunk) != 0) --chunk;
        if (per % (4ll * chunk) != 0) return q;
        q.chunk = chunk;
        q.zper = (int)(per / (4ll * chunk));
        q.nslab = groups * q.zper;
        return q;
    }
    q.chunk = chunk;
    const int nw = (q.steps + chunk - 1) / chunk;
    q.nslab = (nw + 3) / 4;
    q.zper = q.nslab;
    return q;
}

// Weight gradient of the same 1x1-map layers (skinny_rows_kernel): gw[m][c] = inv_scale * sum_n gy[n][m] x[n][c], an outer-product
// sum over the 64 ... 192 batch rows.  lane = c (x[n][.] is one coalesced load), a block owns eight rows m (gy[n][m .. m + 7] is
// wave-uniform: one scalar load) and its four waves a quarter of the batch each, plain fp32 FMAs, no slab; one partial of
// <unscaled gw, W_bar> per block.
// OnePix (hw > 0): the layer maps its whole H x W input to ONE output pixel (the discriminator's last 5x5 s2 conv on a 2 x 2
// map, its 3x3 head on a 1 x 1 map: 6.5 M of D's 11.6 M parameters).  Only the taps that meet the input carry a gradient -
// 4 of 25, 1 of 9 - and that gradient is the same outer-product sum over the batch with x viewed as [B, C H W]: the kernel
// below with its columns scattered to their taps and the other taps zeroed (the general kernel multiplies through all 25 taps'
// columns on the fp32 MFMA - these layers' OW is odd - for 21 exact zeros out of 25).
struct OnePix {
    int hw, W, KH, KW, pad_h, pad_w, Cw;
};

#define SKW_MT 8          // gradient rows per block (narrow layers)
#define SKW_MT_WIDE 32    // ... of layers with >= SKW_WIDE_M rows: x is re-read by a quarter as many blocks
#define SKW_WIDE_M 128
static inline int skw_mt(int M) { return M >= SKW_WIDE_M ? SKW_MT_WIDE : SKW_MT; }
#define SKW_NC 32         // batch rows per load batch

// one finished element (row m, column j) of the gradient: scattered to its tap for a one-pixel layer; its <G, W_bar> term
__device__ __forceinline__ void skw_store(const OnePix& op, float* __restrict__ gw, const float* __restrict__ w_ref, int C, int m, int j,
                                          float v, float sc, double& dot) {
    long long o = (long long)m * C + j;
    bool inside = true;
    if (op.hw > 0) {           // column j = (c, iy, ix) of a whole input map: tap (iy + pad_h, ix + pad_w) of weight row (m, c)
        const int c = j / op.hw, pix = j - c * op.hw;
        const int iy = pix / op.W, ix = pix - iy * op.W;
        const int kh = iy + op.pad_h, kw = ix + op.pad_w;
        inside = kh < op.KH && kw < op.KW;           // pixels no tap of the single output position reaches
        o = (((long long)m * op.Cw + c) * op.KH + kh) * op.KW + kw;
    }
    if (inside) {
        if (w_ref) dot += (double)v * (double)w_ref[o];
        gw[o] = v * sc;
    }
}

// The taps no input pixel reaches get their zeros here: the block owns rows i0 .. i0 + mt - 1 of the channels its 64 columns
// span - contiguous runs of gw - and walks them with consecutive lanes on consecutive addresses, skipping the taps skw_store
// wrote (disjoint addresses: no ordering needed).  A channel whose pixels straddle two blocks is zeroed by the block that
// holds its pixel 0.
__device__ __forceinline__ void skw_zero_taps(const OnePix& op, float* __restrict__ gw, int M, int i0, int mt, int bx) {
    const int H = op.hw / op.W, taps = op.KH * op.KW;
    const int first_col = bx * 64;
    const int c_first = (first_col + op.hw - 1) / op.hw;
    int c_last = (first_col + 63) / op.hw;
    if (c_last > op.Cw - 1) c_last = op.Cw - 1;
    const int span = (c_last - c_first + 1) * taps;
    for (int t = 0; t < mt; ++t) {
        if (i0 + t >= M) break;
        float* row = gw + ((long long)(i0 + t) * op.Cw + c_first) * taps;
        for (int e = threadIdx.x; e < span; e += blockDim.x) {
            const int tap = e % taps, kh = tap / op.KW, kw = tap - kh * op.KW;
            if (!(kh >= op.pad_h && kh - op.pad_h < H && kw >= op.pad_w && kw - op.pad_w < op.W)) row[e] = 0.0f;
        }
    }
}

template <int MT>
__device__ __forceinline__ void skinny_wgrad_body(const float* __restrict__ x, long long x_bs, const float* __restrict__ gy,
                                                  long long gy_bs, float* __restrict__ gw, const float* __restrict__ w_ref,
                                                  const float* __restrict__ inv_scale, int scale_bg, int scale_stride,
                                                  double* __restrict__ partial, int N, int M, int C, const OnePix& op, int bx, int by,
                                                  int grid_x) {
    __shared__ double scratch[16];
    __shared__ float red[4][MT][64];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int j = bx * 64 + lane;
    const int i0 = by * MT;
    const bool jok = j < C;
    const float* __restrict__ xc = x + (jok ? j : 0);
    float acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = 0.0f;
    // the four waves take a quarter of the batch rows each; their partial sums are added in wave order below
    const int nq = (N + 3) / 4, nlo = wid * nq, nhi = nlo + nq < N ? nlo + nq : N;
    for (int nb = nlo; nb < nhi; nb += SKW_NC) {
        float xv[SKW_NC];
#pragma unroll
        for (int q = 0; q < SKW_NC; ++q) xv[q] = (jok && nb + q < nhi) ? xc[(long long)(nb + q) * x_bs] : 0.0f;
#pragma unroll
        for (int q = 0; q < SKW_NC; ++q) {
            if (nb + q < nhi) {
                const float* __restrict__ g = gy + (long long)(nb + q) * gy_bs + i0;          // wave-uniform: scalar loads
                // a stacked call's 1 / sigma_k goes onto the x value (one multiply per batch row instead of one per row and m)
                const float xs = scale_bg ? xv[q] * inv_scale[((nb + q) / scale_bg) * scale_stride] : xv[q];
                if (i0 + MT <= M) {
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[t] = fmaf(g[t], xs, acc[t]);
                } else {
#pragma unroll
                    for (int t = 0; t < MT; ++t) acc[t] = fmaf(i0 + t < M ? g[t] : 0.0f, xs, acc[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) red[wid][t][lane] = acc[t];
    __syncthreads();
    const float sc = (!scale_bg && inv_scale) ? inv_scale[0] : 1.0f;
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < MT / 4; ++q) {          // wave w finishes rows (MT / 4) w ... (MT / 4) (w + 1) - 1
        const int t = wid * (MT / 4) + q;
        if (jok && i0 + t < M) {
            const float v = ((red[0][t][lane] + red[1][t][lane]) + red[2][t][lane]) + red[3][t][lane];
            skw_store(op, gw, w_ref, C, i0 + t, j, v, sc, dot);
        }
    }
    if (op.hw > 0) skw_zero_taps(op, gw, M, i0, MT, bx);
    if (partial) {
        dot = block_sum<double>(dot, scratch);
        if (threadIdx.x == 0) partial[by * grid_x + bx] = dot;
    }
}

// Layers of SKW_WIDE_M rows or more: a 32 x 64 tile of the gradient per block, both operands staged through LDS in runs of
// SKW_WN batch rows with coalesced loads (the narrow form's per-row scalar loads of gy cost a round trip per batch row and block),
// 2 x 4 results per thread, the batch rows summed in order by ONE thread per result (no cross-wave combination).
#define SKW_WN 96
__device__ __forceinline__ void skinny_wgrad_wide(const float* __restrict__ x, long long x_bs, const float* __restrict__ gy,
                                                  long long gy_bs, float* __restrict__ gw, const float* __restrict__ w_ref,
                                                  const float* __restrict__ inv_scale, int scale_bg, int scale_stride,
                                                  double* __restrict__ partial, int N, int M, int C, const OnePix& op, int bx, int by,
                                                  int grid_x) {
    __shared__ double wscratch[16];
    __shared__ __attribute__((aligned(16))) float wbuf[SKW_WN * (SKW_MT_WIDE + 64)];          // operand stages, then the output rows of a one-pixel layer
    float (*gs)[SKW_MT_WIDE] = reinterpret_cast<float (*)[SKW_MT_WIDE]>(wbuf);
    float (*xs)[64] = reinterpret_cast<float (*)[64]>(wbuf + SKW_WN * SKW_MT_WIDE);
    const int tid = threadIdx.x;
    const int i0 = by * SKW_MT_WIDE, j0 = bx * 64;
    const int tm = tid >> 4, tc = tid & 15;              // rows i0 + 2 tm + {0, 1}, columns j0 + 4 tc + {0 .. 3}
    const int gm = tid & 31, gr = tid >> 5;              // staging: gy column / first row of this thread
    const int xc = tid & 63, xr = tid >> 6;
    const bool gok = i0 + gm < M, xok = j0 + xc < C;
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int n0 = 0; n0 < N; n0 += SKW_WN) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SKW_WN / 8; ++r) {
            const int n = n0 + gr + 8 * r;
            float v = 0.0f;
            if (gok && n < N) {
                v = gy[(long long)n * gy_bs + i0 + gm];
                if (scale_bg) v *= inv_scale[(n / scale_bg) * scale_stride];
            }
            gs[gr + 8 * r][gm] = v;
        }
#pragma unroll
        for (int r = 0; r < SKW_WN / 4; ++r) {
            const int n = n0 + xr + 4 * r;
            xs[xr + 4 * r][xc] = (xok && n < N) ? x[(long long)n * x_bs + j0 + xc] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < SKW_WN; ++k) {
            const float2 g = *reinterpret_cast<const float2*>(&gs[k][2 * tm]);
            const float4 xv = *reinterpret_cast<const float4*>(&xs[k][4 * tc]);
            acc[0][0] = fmaf(g.x, xv.x, acc[0][0]); acc[0][1] = fmaf(g.x, xv.y, acc[0][1]);
            acc[0][2] = fmaf(g.x, xv.z, acc[0][2]); acc[0][3] = fmaf(g.x, xv.w, acc[0][3]);
            acc[1][0] = fmaf(g.y, xv.x, acc[1][0]); acc[1][1] = fmaf(g.y, xv.y, acc[1][1]);
            acc[1][2] = fmaf(g.y, xv.z, acc[1][2]); acc[1][3] = fmaf(g.y, xv.w, acc[1][3]);
        }
    }
    const float sc = (!scale_bg && inv_scale) ? inv_scale[0] : 1.0f;
    double dot = 0.0;
    const int taps = op.KH * op.KW;
    // One-pixel layer whose 64 columns are whole channels (hw | 64) and whose weight rows take 16-byte stores: the block's output
    // - 64 / hw channels x taps floats per row, contiguous in gw - is assembled in LDS (zeros, then the useful taps scattered in)
    // and streamed out with full-width stores, a few rows per pass: scattered 4-byte stores plus a separate zeroing walk cost
    // more than the arithmetic (26 MB of D's last 5x5 layer: 61 -> measured below).
    const int cpb = op.hw > 0 && (64 % op.hw) == 0 ? 64 / op.hw : 0;
    const int c0 = bx * cpb;
    const int nch = cpb > 0 ? (c0 + cpb <= op.Cw ? cpb : op.Cw - c0) : 0;
    const int rowlen = nch * taps;
    const bool staged = cpb > 0 && nch > 0 && (rowlen & 3) == 0 && (((long long)op.Cw * taps) & 3) == 0 && (((long long)c0 * taps) & 3) == 0 &&
                        rowlen * 2 <= SKW_WN * (SKW_MT_WIDE + 64) && (reinterpret_cast<uintptr_t>(gw) & 15) == 0;
    if (staged) {
        int rpp = (SKW_WN * (SKW_MT_WIDE + 64)) / rowlen;          // rows per pass: even (a thread's two rows stay together)
        rpp = rpp > SKW_MT_WIDE ? SKW_MT_WIDE : (rpp & ~1);
        const DivU32 dq((unsigned)(rowlen / 4));
        for (int r0 = 0; r0 < SKW_MT_WIDE && i0 + r0 < M; r0 += rpp) {
            __syncthreads();
            for (int e = tid; e < rpp * rowlen / 4; e += 256) reinterpret_cast<float4*>(wbuf)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int row = 2 * tm + a;
                if (row >= r0 && row < r0 + rpp && i0 + row < M) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int jl = 4 * tc + b, cl = jl / op.hw, pix = jl - cl * op.hw;
                        const int iy = pix / op.W, ix = pix - iy * op.W;
                        const int kh = iy + op.pad_h, kw = ix + op.pad_w;
                        if (cl < nch && kh < op.KH && kw < op.KW) {
                            const int t = cl * taps + kh * op.KW + kw;
                            const float v = acc[a][b];
                            if (w_ref) dot += (double)v * (double)w_ref[((long long)(i0 + row) * op.Cw + c0) * taps + t];
                            wbuf[(row - r0) * rowlen + t] = v * sc;
                        }
                    }
                }
            }
            __syncthreads();
            int rows = M - (i0 + r0);
            if (rows > rpp) rows = rpp;
            if (rows > SKW_MT_WIDE - r0) rows = SKW_MT_WIDE - r0;
            for (int e = tid; e < rows * rowlen / 4; e += 256) {
                unsigned r, q;
                dq.divmod((unsigned)e, r, q);
                reinterpret_cast<float4*>(gw + ((long long)(i0 + r0 + (int)r) * op.Cw + c0) * taps)[q] = reinterpret_cast<const float4*>(wbuf)[e];
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int m = i0 + 2 * tm + a, j = j0 + 4 * tc + b;
                if (m < M && j < C) skw_store(op, gw, w_ref, C, m, j, acc[a][b], sc, dot);
            }
        if (op.hw > 0) skw_zero_taps(op, gw, M, i0, SKW_MT_WIDE, bx);
    }
    if (partial) {
        dot = block_sum<double>(dot, wscratch);
        if (threadIdx.x == 0) partial[by * grid_x + bx] = dot;
    }
}

__global__ void __launch_bounds__(256) skinny_wgrad_kernel(const float* __restrict__ x, long long x_bs, const float* __restrict__ gy,
                                                           long long gy_bs, float* __restrict__ gw, const float* __restrict__ w_ref,
                                                           const float* __restrict__ inv_scale, int scale_bg, int scale_stride,
                                                           double* __restrict__ partial, int N, int M, int C, OnePix op) {
    if (M >= SKW_WIDE_M)
        skinny_wgrad_wide(x, x_bs, gy, gy_bs, gw, w_ref, inv_scale, scale_bg, scale_stride, partial, N, M, C, op, blockIdx.x, blockIdx.y,
                          gridDim.x);
    else
        skinny_wgrad_body<SKW_MT>(x, x_bs, gy, gy_bs, gw, w_ref, inv_scale, scale_bg, scale_stride, partial, N, M, C, op, blockIdx.x,
                                  blockIdx.y, gridDim.x);
}

// The same for ALL such layers of one backward pass in ONE launch (the style chain's links, the channel gates' squeeze convs,
// the discriminator's 1x1-map layers, its last 5x5 conv and its head): records by value in the kernel arguments like the other
// end-of-pass finalisers (finalise.hip) - every one of these launches is a ten-microsecond walk over the batch rows by a
// handful of blocks; together they fill the chip once.  Arithmetic and summation order per layer are those of the single
// launch (same body, same block shape).
struct SkwRec {
    const float* x; const float* gy; float* gw; const float* w_ref; const float* inv_scale; double* partial;
    long long x_bs, gy_bs;
    int scale_bg, scale_stride, N, M, C, grid_x, block0;
    OnePix op;
};
#define SKW_MAX 24
struct SkwBatch {
    SkwRec r[SKW_MAX];
};

__global__ void __launch_bounds__(256) skinny_wgrad_batch_kernel(const SkwBatch b, int n) {
    int k = 0;
    for (int i = 1; i < n; ++i)
        if ((int)blockIdx.x >= b.r[i].block0) k = i;          // block0 ascending
    const SkwRec& r = b.r[k];
    const int local = (int)blockIdx.x - r.block0;
    const int by = local / r.grid_x, bx = local - by * r.grid_x;
    if (r.M >= SKW_WIDE_M)
        skinny_wgrad_wide(r.x, r.x_bs, r.gy, r.gy_bs, r.gw, r.w_ref, r.inv_scale, r.scale_bg, r.scale_stride, r.partial, r.N, r.M, r.C,
                          r.op, bx, by, r.grid_x);
    else
        skinny_wgrad_body<SKW_MT>(r.x, r.x_bs, r.gy, r.gy_bs, r.gw, r.w_ref, r.inv_scale, r.scale_bg, r.scale_stride, r.partial, r.N, r.M,
                                  r.C, r.op, bx, by, r.grid_x);
}

static bool skinny_wgrad_ok(const ConvGeom& g) {
    return !path_disabled("skinny") && g.KH == 1 && g.KW == 1 && g.stride == 1 && g.pad_h == 0 && g.pad_w == 0 && g.H == 1 &&
           g.W == 1 && g.OH == 1 && g.OW == 1;
}
static dim3 skinny_wgrad_grid(const ConvGeom& g) { return dim3((g.C + 63) / 64, (g.M + skw_mt(g.M) - 1) / skw_mt(g.M)); }
// one output pixel, a kernel larger than 1x1 (see OnePix); the input map is small by construction (it fits under the kernel)
static bool onepix_wgrad_ok(const ConvGeom& g) {
    return !path_disabled("skinny") && !skinny_wgrad_ok(g) && g.OH == 1 && g.OW == 1 && (long long)g.C * g.H * g.W < (1 << 24);
}
static dim3 onepix_wgrad_grid(const ConvGeom& g) { return dim3((g.C * g.H * g.W + 63) / 64, (g.M + skw_mt(g.M) - 1) / skw_mt(g.M)); }

// The ONE plan of a weight gradient: which kernel family this geometry takes and what that launch looks like.  The size queries
// (workspace bytes, partial counts), the batch records and the launch itself all ask this function and nothing else, so the
// workspace Python sized is the workspace the kernels write.  It decides on the geometry alone: operands a route cannot take
// (alignment, strides) are an error at launch, never a switch to another route with its different workspace layout.
// groups: the stacked calls whose per-call <G_k / sigma_k, W_bar> the split reduction is to emit (2 .. 4 calls that divide the
// batch; anything else plans the single call); `dots` tells whether this geometry can emit them.
enum WgradKind { WG_MAP1X1, WG_ONEPIX, WG_POINTWISE, WG_TILED };
struct WgradRoute {
    WgradKind kind;
    dim3 grid;
    int bm;                    // tiled kernels: block-tile height
    PwPlan pw;                 // pointwise kernel: wave tile and steps
    int nsplit, chunk, zper;   // slabs in all (1: the kernel writes gw itself), reduction elements (pointwise: 16-pixel steps per
                               // wave) per slab, slabs per stacked call
    int64_t n;                 // elements of gw
    int partials;              // doubles written to inner_partial; with slabs also the grid of their reduction
    size_t ws_bytes;           // the slabs
    bool dots;
};

static WgradRoute wgrad_route(const ConvGeom& g, int groups) {
    WgradRoute r;
    const bool stacked = groups >= 2 && groups <= 4 && g.B % groups == 0;
    if (!stacked) groups = 0;
    r.bm = 0; r.nsplit = 1; r.chunk = 0; r.zper = 1; r.partials = 0; r.ws_bytes = 0; r.dots = false;
    r.n = (int64_t)g.M * g.C * g.KH * g.KW;
    const bool map1x1 = skinny_wgrad_ok(g);
    if (map1x1 || onepix_wgrad_ok(g)) {                       // no slabs; one partial per block
        r.kind = map1x1 ? WG_MAP1X1 : WG_ONEPIX;
        r.grid = map1x1 ? skinny_wgrad_grid(g) : onepix_wgrad_grid(g);
        r.partials = (int)(r.grid.x * r.grid.y);
        return r;
    }
    r.pw = pw_plan(g, groups);
    if (r.pw.ok) {                                            // always through slabs
        r.kind = WG_POINTWISE;
        if (stacked && r.pw.zper == 0) return r;              // (call lengths that do not divide into whole slabs: no plan, no dots)
        r.nsplit = r.pw.nslab; r.chunk = r.pw.chunk; r.zper = r.pw.zper;
        r.grid = dim3(r.pw.nslab, r.pw.tiles_m * r.pw.tiles_c);
        r.dots = stacked;
    } else {
        r.kind = WG_TILED;
        int tiles;
        wgrad_plan(g, groups, &r.bm, &r.nsplit, &r.chunk, &r.zper, &tiles);
        r.grid = dim3((g.C * g.KH * g.KW + 127) / 128, (g.M + r.bm - 1) / r.bm, r.nsplit);
        r.dots = stacked && (long long)g.B * g.OH * g.OW < (1ll << 31);
        if (r.nsplit == 1) { r.partials = tiles; return r; }
    }
    r.partials = wgrad_reduce_grid(r.n, r.nsplit);
    r.ws_bytes = (size_t)r.nsplit * r.n * sizeof(float);
    return r;
}

LOCATE_API size_t locate_conv_wgrad_workspace_bytes(const int* geom) { return wgrad_route(make_geom(geom), 0).ws_bytes; }

// number of doubles written to `inner_partial` by locate_conv_wgrad for this geometry
LOCATE_API int locate_conv_wgrad_partials(const int* geom) { return wgrad_route(make_geom(geom), 0).partials; }

// What locate_conv_wgrad requires of an operand of this geometry (which: 0 = x, 1 = gy): its address and its batch stride are
// multiples of the returned number of bytes - 16 for both operands of the narrow 1x1 route, 8 for gy on the 192-row plan, 4 (any
// fp32 tensor) everywhere else.  The route is fixed by the geometry, so an operand that does not meet it is refused at launch; a
// caller that may hold such a view (a slice of a flat buffer) asks here and copies it first.
LOCATE_API int locate_conv_wgrad_operand_align(const int* geom, int which) {
    const ConvGeom g = make_geom(geom);
    if (geom_check(g, "locate_conv_wgrad_operand_align")) return 4;
    const WgradRoute r = wgrad_route(g, 0);
    if (r.kind == WG_POINTWISE) return 16;
    if (r.kind == WG_TILED && r.bm == 192 && which == 1) return 8;
    return 4;
}

// ---- the small weight gradients of a pass in one launch (SkwRec above) ----
LOCATE_API size_t locate_wgrad_batch_record_bytes(void) { return sizeof(SkwRec); }
LOCATE_API int locate_wgrad_batch_max(void) { return SKW_MAX; }
// Fills `record` (locate_wgrad_batch_record_bytes() bytes, host memory) with the launch of locate_conv_wgrad for this geometry
// and these operands and returns its number of blocks - or 0 when the geometry is not one of the small-map layers (1x1 maps,
// one output pixel), which the caller then launches on its own.  Same argument meaning as locate_conv_wgrad.
LOCATE_API int locate_wgrad_batch_record(const int* geom, const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw,
                                         const float* w_ref, const float* inv_scale, int scale_group_batch, int scale_stride,
                                         double* inner_partial, void* record) {
    const ConvGeom g = make_geom(geom);
    if (geom_check(g, "locate_wgrad_batch_record") || !record || !x || !gy || !gw) return 0;
    if (inner_partial && !w_ref) return 0;
    if (scale_group_batch < 0 || (scale_group_batch > 0 && (!inv_scale || g.B % scale_group_batch != 0 || g.B / scale_group_batch > 4 ||
                                                            w_ref || inner_partial))) return 0;
    const WgradRoute route = wgrad_route(g, 0);
    if (route.kind != WG_MAP1X1 && route.kind != WG_ONEPIX) return 0;
    const bool skinny = route.kind == WG_MAP1X1;
    const dim3 grid = route.grid;
    SkwRec r;
    r.x = x; r.gy = gy; r.gw = gw; r.w_ref = w_ref; r.inv_scale = inv_scale; r.partial = inner_partial;
    r.x_bs = x_bs; r.gy_bs = gy_bs;
    r.scale_bg = scale_group_batch; r.scale_stride = scale_stride; r.N = g.B; r.M = g.M; r.C = skinny ? g.C : g.C * g.H * g.W;
    r.grid_x = (int)grid.x; r.block0 = 0;
    r.op = skinny ? OnePix{0, 0, 0, 0, 0, 0, 0} : OnePix{g.H * g.W, g.W, g.KH, g.KW, g.pad_h, g.pad_w, g.C};
    memcpy(record, &r, sizeof(r));
    return (int)(grid.x * grid.y);
}
// Launches n records (filled by locate_wgrad_batch_record, in host memory, packed) in one grid.
LOCATE_API int locate_wgrad_batch(const void* records, int n, void* stream) {
    LOCATE_REQUIRE(records && n > 0 && n <= SKW_MAX, "locate_wgrad_batch: 1 .. locate_wgrad_batch_max() records");
    SkwBatch b;
    memcpy(b.r, records, (size_t)n * sizeof(SkwRec));
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const SkwRec& r = b.r[i];
        LOCATE_REQUIRE(r.x && r.gy && r.gw && r.grid_x > 0 && r.M > 0 && r.C > 0 && r.N > 0, "locate_wgrad_batch: bad record");
        b.r[i].block0 = (int)blocks;
        blocks += (long long)r.grid_x * ((r.M + skw_mt(r.M) - 1) / skw_mt(r.M));
    }
    LOCATE_REQUIRE(blocks < (1ll << 31), "locate_wgrad_batch: too many blocks");
    skinny_wgrad_batch_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(b, n);
    LOCATE_LAUNCH_CHECK("locate_wgrad_batch");
    return LOCATE_OK;
}

// Stacked calls with the per-call <G_k / sigma_k, W_bar> partials out of the split reduction (locate_conv_wgrad with
// scale_group_batch > 0 AND w_ref + inner_partial): partials PER CALL for this geometry split into `groups` calls - inner_partial
// then holds groups x that many doubles, [call][partial] - or 0 when this geometry cannot emit them (layers on 1x1 maps / with one
// output pixel, call lengths that do not divide into whole slabs: take <gy_k, y_k - bias> on the activation side instead,
// locate_fin_sn_dots).  The workspace of that mode has its own size.
LOCATE_API int locate_conv_wgrad_group_partials(const int* geom, int groups) {
    const ConvGeom g = make_geom(geom);
    if (geom_check(g, "locate_conv_wgrad_group_partials")) return 0;
    const WgradRoute r = wgrad_route(g, groups);
    return r.dots ? r.partials : 0;
}
LOCATE_API size_t locate_conv_wgrad_group_workspace_bytes(const int* geom, int groups) {
    const ConvGeom g = make_geom(geom);
    if (geom_check(g, "locate_conv_wgrad_group_workspace_bytes")) return 0;
    const WgradRoute r = wgrad_route(g, groups);
    return r.dots ? r.ws_bytes : 0;
}

// NP: the operand form of conv_wgrad_bx6_kernel (1: bf16 operands, 2: two scaled fp16 pieces, 3: three bf16 pieces, 4: fp8)
template <int NP>
static void launch_wgrad_bx6(const WgParams& p, dim3 grid, int bm, hipStream_t st) {
    with_tile<true>(bm, [&](auto t) { using T = decltype(t); conv_wgrad_bx6_kernel<T::wgm, T::wgn, T::tm, T::tn, NP><<<grid, 256, 0, st>>>(p); });
}

// gw[m,c,kh,kw] = inv_scale * sum_{b,oh,ow} gy[b,m,oh,ow] x[b,c,oh*s-ph+kh,ow*s-pw+kw]          (overwritten)
// With w_ref (= W_bar, same layout as gw) and inner_partial: the partial sums of <UNSCALED gw, W_bar> the
// spectral-norm backward needs come out of the same pass (locate_conv_wgrad_partials(geom) doubles).
// scale_group_batch > 0: gy of batch element b is weighted by inv_scale[(b / scale_group_batch) * scale_stride] instead
// (stacked forwards; at most 4 groups; w_ref / inner_partial must then be null - see locate_sn_group_dsigma).
// deferred_reduce (nullable, host memory of locate_slab_reduce_record_bytes() bytes): the split reduction - when this geometry has
// one - is NOT launched; its launch is written there instead and gw / inner_partial are complete only after
// locate_slab_reduce_batch() has run that record (the workspace must stay untouched until then).  The record's block count is
// locate_slab_reduce_record_blocks(record): 0 = nothing pending (gw is complete when this launch is).
LOCATE_API int locate_conv_wgrad(const int* geom, const float* x, int64_t x_bs, const float* gy, int64_t gy_bs, float* gw,
                                 const float* w_ref, const float* inv_scale, int scale_group_batch, int scale_stride,
                                 double* inner_partial, void* workspace, int precision, const void* x_absmax, const void* gy_absmax,
                                 void* deferred_reduce, void* stream) {
    const ConvGeom g = make_geom(geom);
    if (int e = geom_check(g, "locate_conv_wgrad")) return e;
    LOCATE_REQUIRE(precision >= 0 && precision <= 3, "locate_conv_wgrad: precision must be 0 (fp32-faithful, bf16 pieces), 1 (bf16 operands), 2 (fp32-faithful, fp16 pieces) or 3 (fp8 operands)");
    LOCATE_REQUIRE(precision < 2 || (x_absmax && gy_absmax), "locate_conv_wgrad: precisions 2 and 3 need the absmax words of x and gy");
    LOCATE_REQUIRE(x && gy && gw, "locate_conv_wgrad: null pointer");
    LOCATE_REQUIRE(!inner_partial || w_ref, "locate_conv_wgrad: inner_partial needs w_ref");
    // stacked calls with w_ref + inner_partial: the per-call dots come out of the split reduction (locate_conv_wgrad_group_partials)
    const int gd = (scale_group_batch > 0 && w_ref && inner_partial && g.B % scale_group_batch == 0) ? g.B / scale_group_batch : 0;
    const WgradRoute r = wgrad_route(g, gd);
    LOCATE_REQUIRE(scale_group_batch >= 0 && (scale_group_batch == 0 || (inv_scale && g.B % scale_group_batch == 0 &&
                   g.B / scale_group_batch <= 4 && ((!w_ref && !inner_partial) || r.dots))),
                   "locate_conv_wgrad: bad group scaling arguments (per-call partials: see locate_conv_wgrad_group_partials)");
    hipStream_t st = as_stream(stream);
    if (deferred_reduce) memset(deferred_reduce, 0, sizeof(SlabRec));
    // the split reduction of the routes that go through slabs
    auto reduce = [&](const float* slab, const float* scale, const char* who) -> int {
        const int64_t n = r.n;
        const int nsplit = r.nsplit, zper = r.zper, rg = r.partials;
        const int zp = wgrad_reduce_zp(nsplit, n);
        if (deferred_reduce) {
            SlabRec rec;
            rec.slab = slab; rec.out = gw; rec.w_ref = w_ref; rec.inv_scale = scale; rec.partial = inner_partial;
            rec.n = n; rec.nsplit = nsplit; rec.zp = zp; rec.grid = rg; rec.block0 = 0; rec.groups = gd; rec.zper = zper;
            memcpy(deferred_reduce, &rec, sizeof(rec));
            return LOCATE_OK;
        }
        if (zp == 16) slab_reduce_kernel<16><<<rg, 256, 0, st>>>(slab, gw, n, nsplit, w_ref, scale, inner_partial, gd, zper);
        else if (zp == 4) slab_reduce_kernel<4><<<rg, 256, 0, st>>>(slab, gw, n, nsplit, w_ref, scale, inner_partial, gd, zper);
        else slab_reduce_kernel<1><<<rg, 256, 0, st>>>(slab, gw, n, nsplit, w_ref, scale, inner_partial, gd, zper);
        LOCATE_LAUNCH_CHECK(who);
        return LOCATE_OK;
    };
    if (r.kind == WG_MAP1X1) {          // 1x1 maps: plain fp32 FMAs at either precision setting (see skinny_rows_kernel)
        skinny_wgrad_kernel<<<r.grid, 256, 0, st>>>(x, x_bs, gy, gy_bs, gw, w_ref, inv_scale, scale_group_batch, scale_stride,
                                                   inner_partial, g.B, g.M, g.C, OnePix{0, 0, 0, 0, 0, 0, 0});
        LOCATE_LAUNCH_CHECK("locate_conv_wgrad(1x1 map)");
        return LOCATE_OK;
    }
    if (r.kind == WG_ONEPIX) {          // one output pixel: the useful taps only; the kernel zeroes the others itself (see OnePix)
        const OnePix op = {g.H * g.W, g.W, g.KH, g.KW, g.pad_h, g.pad_w, g.C};
        skinny_wgrad_kernel<<<r.grid, 256, 0, st>>>(x, x_bs, gy, gy_bs, gw, w_ref, inv_scale, scale_group_batch, scale_stride,
                                                   inner_partial, g.B, g.M, g.C * g.H * g.W, op);
        LOCATE_LAUNCH_CHECK("locate_conv_wgrad(one output pixel)");
        return LOCATE_OK;
    }
    const dim3 grid = r.grid;
    if (r.kind == WG_POINTWISE) {
        const PwPlan& pq = r.pw;
        // the route is decided on the geometry alone (wgrad_route), so the pointwise plan is binding here: operands it cannot take
        // are an error, never a silent switch to the general plan with its different workspace layout
        LOCATE_REQUIRE((x_bs & 3) == 0 && (gy_bs & 3) == 0 &&
                       ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy)) & 15) == 0,
                       "locate_conv_wgrad: narrow 1x1 layers need 16-byte aligned x / gy and batch strides that are multiples of 4");
        LOCATE_REQUIRE(workspace, "locate_conv_wgrad: the split reduction needs a workspace");
        PwParams q;
        q.x = x; q.gy = gy; q.slab = static_cast<float*>(workspace); q.x_bs = x_bs; q.gy_bs = gy_bs;
        q.B = g.B; q.C = g.C; q.M = g.M; q.P = g.H * g.W; q.N = g.B * g.H * g.W; q.steps = pq.steps; q.chunk = pq.chunk;
        q.tiles_c = pq.tiles_c;
        const bool grouped = scale_group_batch > 0;
        q.inv_scale = grouped ? inv_scale : nullptr; q.gscale_bg = scale_group_batch; q.gscale_stride = scale_stride;
        const int key = (pq.tm - 1) * 2 + (pq.tn - 1);
        q.x_absmax = static_cast<const unsigned*>(x_absmax);
        q.g_absmax = static_cast<const unsigned*>(gy_absmax);
        if (precision == 2 && x_absmax && gy_absmax && !grouped) {
            // (stacked calls weight gy by 1 / sigma_k while it is loaded: its largest magnitude no longer bounds the scaled value -
            // they keep the three-piece form, which needs no range)
            if (key == 0) pw_wgrad_kernel<1, 1, 2><<<grid, 256, 0, st>>>(q);
            else if (key == 1) pw_wgrad_kernel<1, 2, 2><<<grid, 256, 0, st>>>(q);
            else if (key == 2) pw_wgrad_kernel<2, 1, 2><<<grid, 256, 0, st>>>(q);
            else pw_wgrad_kernel<2, 2, 2><<<grid, 256, 0, st>>>(q);
        } else if (precision == 1) {
            if (key == 0) pw_wgrad_kernel<1, 1, 1><<<grid, 256, 0, st>>>(q);
            else if (key == 1) pw_wgrad_kernel<1, 2, 1><<<grid, 256, 0, st>>>(q);
            else if (key == 2) pw_wgrad_kernel<2, 1, 1><<<grid, 256, 0, st>>>(q);
            else pw_wgrad_kernel<2, 2, 1><<<grid, 256, 0, st>>>(q);
        } else {
            if (key == 0) pw_wgrad_kernel<1, 1, 3><<<grid, 256, 0, st>>>(q);
            else if (key == 1) pw_wgrad_kernel<1, 2, 3><<<grid, 256, 0, st>>>(q);
            else if (key == 2) pw_wgrad_kernel<2, 1, 3><<<grid, 256, 0, st>>>(q);
            else pw_wgrad_kernel<2, 2, 3><<<grid, 256, 0, st>>>(q);
        }
        LOCATE_LAUNCH_CHECK("locate_conv_wgrad(pointwise)");
        return reduce(q.slab, grouped ? nullptr : inv_scale, "locate_conv_wgrad(pointwise reduce)");
    }
    const int bm = r.bm, nsplit = r.nsplit, chunk = r.chunk, zper = r.zper;
    LOCATE_REQUIRE(nsplit == 1 || workspace, "locate_conv_wgrad: split reduction needs a workspace");
    WgParams p;
    p.x = x; p.gy = gy; p.slab = static_cast<float*>(workspace); p.x_bs = x_bs; p.gy_bs = gy_bs;
    p.B = g.B; p.C = g.C; p.H = g.H; p.W = g.W; p.M = g.M; p.OH = g.OH; p.OW = g.OW; p.KH = g.KH; p.KW = g.KW;
    p.stride = g.stride; p.pad_h = g.pad_h; p.pad_w = g.pad_w;
    p.R = g.C * g.KH * g.KW; p.N = g.B * g.OH * g.OW; p.chunk = chunk;
    p.zper = zper; p.Ng = gd > 1 ? p.N / gd : p.N;
    fastdiv_make((unsigned)(g.OH * g.OW), &p.q_mul, &p.q_s1, &p.q_s2);
    fastdiv_make((unsigned)g.OW, &p.ow_mul, &p.ow_s1, &p.ow_s2);
    const bool direct = nsplit == 1;
    const bool grouped = scale_group_batch > 0;
    p.gscale_bg = scale_group_batch; p.gscale_stride = scale_stride;
    p.x_absmax = static_cast<const unsigned*>(x_absmax);
    p.g_absmax = static_cast<const unsigned*>(gy_absmax);
    p.direct_out = direct ? gw : nullptr;
    p.w_ref = direct ? w_ref : nullptr;
    p.inv_scale = (direct || grouped) ? inv_scale : nullptr;
    p.partial = direct ? inner_partial : nullptr;
    const long long x_extent = 4ll * ((long long)(g.B - 1) * x_bs + (long long)g.C * g.H * g.W);
    p.x_bytes = (unsigned)x_extent;
    // pairs of adjacent reduction elements: same image and same output row, 8-byte aligned in gy
    const bool pairs_ok = ((g.OH * g.OW) & 1) == 0 && (g.OW & 1) == 0 && (gy_bs & 1) == 0 && (chunk & 1) == 0 &&
                          (reinterpret_cast<uintptr_t>(gy) & 7) == 0 && x_extent > 0 && x_extent < (1ll << 31) - (1 << 20);
    LOCATE_REQUIRE(bm != 192 || pairs_ok, "locate_conv_wgrad: layers with M %% 192 == 0 on even maps take the paired-load kernels - gy must be 8-byte aligned with an even batch stride");
    const bool bx6 = pairs_ok && (precision == 1 || precision == 3 || !path_disabled("wbx6"));
    if (bx6 && precision == 3) launch_wgrad_bx6<4>(p, grid, bm, st);
    else if (bx6 && precision == 1) launch_wgrad_bx6<1>(p, grid, bm, st);
    else if (bx6 && precision == 2) launch_wgrad_bx6<2>(p, grid, bm, st);
    else if (bx6) launch_wgrad_bx6<3>(p, grid, bm, st);
    else          // odd output maps (and the debug library's reference path): the exact fp32-MFMA kernel, at every precision setting
        with_tile<false>(bm, [&](auto t) { using T = decltype(t); conv_wgrad_kernel<T::wgm, T::wgn, T::tm, T::tn><<<grid, 256, 0, st>>>(p); });
    LOCATE_LAUNCH_CHECK("locate_conv_wgrad(gemm)");
    if (!direct) return reduce(p.slab, grouped ? nullptr : inv_scale, "locate_conv_wgrad(reduce)");
    return LOCATE_OK;
}

LOCATE_API size_t locate_slab_reduce_record_bytes(void) { return sizeof(SlabRec); }
LOCATE_API int locate_slab_reduce_max(void) { return SLAB_MAX; }
LOCATE_API int locate_slab_reduce_record_blocks(const void* record) {
    if (!record) return 0;
    SlabRec r;
    memcpy(&r, record, sizeof(r));
    return r.grid;
}
// Runs n deferred split reductions (records written by locate_conv_wgrad(deferred_reduce), packed, host memory) in one grid.
LOCATE_API int locate_slab_reduce_batch(const void* records, int n, void* stream) {
    LOCATE_REQUIRE(records && n > 0 && n <= SLAB_MAX, "locate_slab_reduce_batch: 1 .. locate_slab_reduce_max() records");
    SlabBatch b;
    memcpy(b.r, records, (size_t)n * sizeof(SlabRec));
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const SlabRec& r = b.r[i];
        LOCATE_REQUIRE(r.slab && r.out && r.n > 0 && r.nsplit > 0 && r.grid > 0 && (r.zp == 1 || r.zp == 4 || r.zp == 16),
                       "locate_slab_reduce_batch: bad record");
        b.r[i].block0 = (int)blocks;
        blocks += r.grid;
    }
    slab_reduce_batch_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(b, n);
    LOCATE_LAUNCH_CHECK("locate_slab_reduce_batch");
    return LOCATE_OK;
}
