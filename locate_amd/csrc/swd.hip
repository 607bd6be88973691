// Sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al., "Progressive Growing of GANs", section 5):
// the one quality metric of a generator that needs no pretrained network.  The arithmetic of the metric, stage by stage:
//   pyr_down     : G_{l+1} = the 5 x 5 binomial filter outer([1,4,6,4,1], [1,4,6,4,1]) / 256 at every second position, borders
//                  mirrored without repeating the edge sample (-1 -> 1, H -> H - 2);
//   pyr_residual : G_l - up(G_{l+1}), up = zero-stuffing to twice the size and the same filter times 4, in its polyphase form (even
//                  outputs see (1, 6, 1) / 8 of the coarse map, odd outputs (4, 4) / 8, per axis): the upsampled map is never stored;
//   swd_stats    : mean and 1 / population deviation per channel over every value of every 7 x 7 x 3 descriptor (patches overlap:
//                  not the statistic of the map), fp64 sums in a fixed order;
//   swd_project  : proj[d, j] = sum_k dirs[k, d] (v_jk - mu_c) r_c, the contraction: descriptors gathered straight from the level
//                  into LDS (normalised on the way), K = 147 (zero rows up to 160) on v_mfma_f32_32x32x2_f32 - exact fp32, a
//                  k-ordered fmaf chain;
//   swd_distance : mean |a - b| of two sorted projection sets, |a - b| in fp32, fp64 sums in a fixed order.
// The sort between the last two is the caller's (a radix sort moves keys and computes nothing).
// Nothing here uses an atomic; every result is the same bits from call to call.  Every operation of the two stencils is spelled
// out (fmaf / __fadd_rn / __fmul_rn), as in common.h's RootTanh pieces, so that a variant of either kernel agrees bit for bit.
#include "common.h"

#define SWD_THREADS 256
#define SWD_PATCH 7
#define SWD_K (3 * SWD_PATCH * SWD_PATCH)          // 147
#define SWD_TILE 128                               // descriptors and directions per block of the contraction
#define SWD_PARTIAL_BLOCKS_MAX 1024

// ---- the two stencils ---------------------------------------------------------------------------------------------------------
// mirror without repeating the edge sample; the final clamp only keeps the lanes of a ragged strip (whose outputs are not
// stored) inside the plane
__device__ __forceinline__ int pyr_mirror(int i, int S) {
    i = i < 0 ? -i : i;
    i = i >= S ? 2 * (S - 1) - i : i;
    return min(max(i, 0), S - 1);
}
// (a0 + a4) + 4 (a1 + a3) + 6 a2: the weights are exact, three roundings
__device__ __forceinline__ float pyr_tap5(float a0, float a1, float a2, float a3, float a4) {
    return fmaf(6.0f, a2, fmaf(4.0f, __fadd_rn(a1, a3), __fadd_rn(a0, a4)));
}

// one thread: 4 consecutive outputs of one row.  Horizontal pass over the five source rows first (12 source columns each), then
// the vertical one, then / 256 (exact).  VEC: S is a multiple of 8 and x 16-byte aligned - the 8 inner columns are two 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(SWD_THREADS) void pyr_down_kernel(const float* __restrict__ x, int planes, int S, float* __restrict__ out) {
    const int So = S >> 1, strips = (So + 3) >> 2;
    const unsigned total = (unsigned)planes * (unsigned)So * (unsigned)strips;
    const DivU32 by_strips((unsigned)strips), by_rows((unsigned)So);
    for (unsigned t = blockIdx.x * SWD_THREADS + threadIdx.x; t < total; t += gridDim.x * SWD_THREADS) {
        unsigned rowid, q, plane, i;
        by_strips.divmod(t, rowid, q);
        by_rows.divmod(rowid, plane, i);
        const float* px = x + (size_t)plane * S * S;
        const int c0 = 8 * (int)q;
        float h[5][4];
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const float* row = px + pyr_mirror(2 * (int)i + a - 2, S) * S;
            float v[12];
            if (VEC) {
                const float4 lo = *reinterpret_cast<const float4*>(row + c0), hi = *reinterpret_cast<const float4*>(row + c0 + 4);
                v[2] = lo.x; v[3] = lo.y; v[4] = lo.z; v[5] = lo.w; v[6] = hi.x; v[7] = hi.y; v[8] = hi.z; v[9] = hi.w;
                v[0] = row[pyr_mirror(c0 - 2, S)]; v[1] = row[pyr_mirror(c0 - 1, S)];
                v[10] = row[pyr_mirror(c0 + 8, S)]; v[11] = row[pyr_mirror(c0 + 9, S)];
            } else {
#pragma unroll
                for (int b = 0; b < 12; ++b) v[b] = row[pyr_mirror(c0 + b - 2, S)];
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) h[a][o] = pyr_tap5(v[2 * o], v[2 * o + 1], v[2 * o + 2], v[2 * o + 3], v[2 * o + 4]);
        }
        float r[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) r[o] = __fmul_rn(pyr_tap5(h[0][o], h[1][o], h[2][o], h[3][o], h[4][o]), 1.0f / 256.0f);
        float* po = out + ((size_t)plane * So + i) * So + 4 * q;
        if (VEC) {
            *reinterpret_cast<float4*>(po) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (4 * (int)q + o < So) po[o] = r[o];
        }
    }
}

// polyphase upsampling, one axis: even output 2p = (y[p-1] + 6 y[p] + y[p+1]) / 8, odd output 2p + 1 = (y[p] + y[p+1]) / 2.
// The mirror acts on the DOUBLED grid: position -2 is 2 (coarse 1), position S is S - 2 (coarse Sc - 1, the sample itself).
__device__ __forceinline__ float up_even(float lo, float mid, float hi) { return __fmul_rn(fmaf(6.0f, mid, __fadd_rn(lo, hi)), 0.125f); }
__device__ __forceinline__ float up_odd(float mid, float hi) { return __fmul_rn(__fadd_rn(mid, hi), 0.5f); }

// one thread: coarse row p, coarse columns 4q .. 4q + 3 -> the 2 x 8 patch of out = x - up(coarse).  Vertical pass first (three
// coarse rows, six columns), then the horizontal one.  x and out may be the same buffer: a thread reads the sixteen values of x
// it overwrites and nothing else of x.
template <bool VEC>
__global__ __launch_bounds__(SWD_THREADS) void pyr_residual_kernel(const float* x, const float* __restrict__ coarse, int planes, int S, float* out) {
    const int Sc = S >> 1, strips = (Sc + 3) >> 2;
    const unsigned total = (unsigned)planes * (unsigned)Sc * (unsigned)strips;
    const DivU32 by_strips((unsigned)strips), by_rows((unsigned)Sc);
    for (unsigned t = blockIdx.x * SWD_THREADS + threadIdx.x; t < total; t += gridDim.x * SWD_THREADS) {
        unsigned rowid, q, plane, p;
        by_strips.divmod(t, rowid, q);
        by_rows.divmod(rowid, plane, p);
        const float* pc = coarse + (size_t)plane * Sc * Sc;
        const int rlo = p == 0 ? 1 : (int)p - 1, rhi = (int)p + 1 == Sc ? Sc - 1 : (int)p + 1;
        const int q0 = 4 * (int)q;
        float ve[6], vo[6];          // the even and the odd output row, still at coarse columns q0 - 1 .. q0 + 4
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            int c = q0 + b - 1;
            c = c < 0 ? 1 : c;
            c = c >= Sc ? Sc - 1 : c;          // q0 + 4 == Sc: the sample itself; beyond (ragged strip): not stored
            const float lo = pc[rlo * Sc + c], mid = pc[(int)p * Sc + c], hi = pc[rhi * Sc + c];
            ve[b] = up_even(lo, mid, hi);
            vo[b] = up_odd(mid, hi);
        }
        float u[2][8];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            u[0][2 * o] = up_even(ve[o], ve[o + 1], ve[o + 2]); u[0][2 * o + 1] = up_odd(ve[o + 1], ve[o + 2]);
            u[1][2 * o] = up_even(vo[o], vo[o + 1], vo[o + 2]); u[1][2 * o + 1] = up_odd(vo[o + 1], vo[o + 2]);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const size_t at = ((size_t)plane * S + 2 * p + a) * S + 8 * q;
            if (VEC) {
                const float4 f = *reinterpret_cast<const float4*>(x + at), g = *reinterpret_cast<const float4*>(x + at + 4);
                *reinterpret_cast<float4*>(out + at) = make_float4(__fsub_rn(f.x, u[a][0]), __fsub_rn(f.y, u[a][1]), __fsub_rn(f.z, u[a][2]), __fsub_rn(f.w, u[a][3]));
                *reinterpret_cast<float4*>(out + at + 4) = make_float4(__fsub_rn(g.x, u[a][4]), __fsub_rn(g.y, u[a][5]), __fsub_rn(g.z, u[a][6]), __fsub_rn(g.w, u[a][7]));
            } else {
#pragma unroll
                for (int o = 0; o < 8; ++o)
                    if (8 * (int)q + o < S) out[at + o] = __fsub_rn(x[at + o], u[a][o]);
            }
        }
    }
}

static int pyr_check(const char* name, const void* a, const void* b, const void* c, int planes, int S) {
    LOCATE_REQUIRE(a && b && c, "%s: null pointer", name);
    LOCATE_REQUIRE(planes >= 1 && S >= 8 && S % 2 == 0 && S <= 16384, "%s: planes = %d, S = %d (S even, 8 .. 16384)", name, planes, S);
    LOCATE_REQUIRE((int64_t)planes * S * S < ((int64_t)1 << 31), "%s: %d planes of %d x %d exceed 2^31 elements", name, planes, S, S);
    LOCATE_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0, "%s: pointers must be 4-byte aligned", name);
    return LOCATE_OK;
}

LOCATE_API int locate_pyr_down(const float* x, int planes, int S, float* out, void* stream) {
    if (int e = pyr_check("locate_pyr_down", x, out, out, planes, S)) return e;
    const int64_t work = (int64_t)planes * (S / 2) * ((S / 2 + 3) / 4);
    const bool vec = S % 8 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const int grid = stream_grid(work, SWD_THREADS);
    if (vec) pyr_down_kernel<true><<<grid, SWD_THREADS, 0, as_stream(stream)>>>(x, planes, S, out);
    else pyr_down_kernel<false><<<grid, SWD_THREADS, 0, as_stream(stream)>>>(x, planes, S, out);
    LOCATE_LAUNCH_CHECK("locate_pyr_down");
    return LOCATE_OK;
}

LOCATE_API int locate_pyr_residual(const float* x, const float* coarse, int planes, int S, float* out, void* stream) {
    if (int e = pyr_check("locate_pyr_residual", x, coarse, out, planes, S)) return e;
    const int64_t work = (int64_t)planes * (S / 2) * ((S / 2 + 3) / 4);
    const bool vec = S % 8 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const int grid = stream_grid(work, SWD_THREADS);
    if (vec) pyr_residual_kernel<true><<<grid, SWD_THREADS, 0, as_stream(stream)>>>(x, coarse, planes, S, out);
    else pyr_residual_kernel<false><<<grid, SWD_THREADS, 0, as_stream(stream)>>>(x, coarse, planes, S, out);
    LOCATE_LAUNCH_CHECK("locate_pyr_residual");
    return LOCATE_OK;
}

// ---- descriptor statistics -----------------------------------------------------------------------------------------------------
// one thread per descriptor (grid-strided): its 49 values of each channel into that channel's sum and sum of squares, fp64; the
// block's six totals (block_sum: a fixed tree) go to the workspace, a second launch adds the blocks' totals in a fixed order.
__global__ __launch_bounds__(SWD_THREADS) void swd_stats_partial_kernel(const float* __restrict__ level, int n, int S, const int2* __restrict__ pos, int P,
                                                                        double* __restrict__ partials) {
    __shared__ double scratch[16];
    double s[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    const DivU32 by_p((unsigned)P);
    const int plane = S * S;
    for (unsigned j = blockIdx.x * SWD_THREADS + threadIdx.x; j < (unsigned)n; j += gridDim.x * SWD_THREADS) {
        const int2 yx = pos[j];
        const int y = min(max(yx.x, 0), S - SWD_PATCH), x0 = min(max(yx.y, 0), S - SWD_PATCH);          // a bad record cannot leave the image
        const float* base = level + (size_t)by_p.div(j) * 3 * plane + y * S + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int dy = 0; dy < SWD_PATCH; ++dy)
#pragma unroll
                for (int dx = 0; dx < SWD_PATCH; ++dx) {
                    const double v = (double)base[c * plane + dy * S + dx];
                    s[c] += v;
                    q[c] = fma(v, v, q[c]);
                }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double ts = block_sum<double>(s[c], scratch), tq = block_sum<double>(q[c], scratch);
        if (threadIdx.x == 0) {
            partials[blockIdx.x * 6 + c] = ts;
            partials[blockIdx.x * 6 + 3 + c] = tq;
        }
    }
}

__global__ __launch_bounds__(SWD_THREADS) void swd_stats_final_kernel(const double* __restrict__ partials, int nblk, double count, float* __restrict__ stats) {
    __shared__ double scratch[16];
    double t[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nblk; b += SWD_THREADS) a += partials[b * 6 + w];
        t[w] = block_sum<double>(a, scratch);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double mu = t[c] / count;
            const double var = t[3 + c] / count - mu * mu;          // fp64: |mu| = 50 sigma still leaves 1e-12 of sigma^2
            stats[c] = (float)mu;
            stats[3 + c] = (float)(1.0 / sqrt(var));                // a constant channel: not finite, by contract
        }
    }
}

static int swd_check(const char* name, const void* level, const void* pos, int N, int S, int P) {
    LOCATE_REQUIRE(level && pos, "%s: null pointer", name);
    LOCATE_REQUIRE(N >= 1 && P >= 1 && S >= SWD_PATCH && S <= 16384, "%s: N = %d, S = %d, P = %d", name, N, S, P);
    LOCATE_REQUIRE((int64_t)N * 3 * S * S < ((int64_t)1 << 31) && (int64_t)N * P < ((int64_t)1 << 31), "%s: N = %d, S = %d, P = %d exceed 2^31 elements", name, N, S, P);
    LOCATE_REQUIRE(((uintptr_t)level & 3) == 0 && ((uintptr_t)pos & 7) == 0, "%s: level must be 4-byte, pos 8-byte aligned", name);
    return LOCATE_OK;
}

LOCATE_API size_t locate_swd_stats_workspace_bytes(void) { return (size_t)SWD_PARTIAL_BLOCKS_MAX * 6 * sizeof(double); }

LOCATE_API int locate_swd_stats(const float* level, int N, int S, const int32_t* pos, int P, float* stats, void* workspace, void* stream) {
    if (int e = swd_check("locate_swd_stats", level, pos, N, S, P)) return e;
    LOCATE_REQUIRE(stats && workspace && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "locate_swd_stats: stats / workspace null or misaligned");
    const int n = N * P;
    int nblk = (int)cdiv64(n, SWD_THREADS);
    if (nblk > SWD_PARTIAL_BLOCKS_MAX) nblk = SWD_PARTIAL_BLOCKS_MAX;
    hipStream_t st = as_stream(stream);
    swd_stats_partial_kernel<<<nblk, SWD_THREADS, 0, st>>>(level, n, S, reinterpret_cast<const int2*>(pos), P, static_cast<double*>(workspace));
    LOCATE_LAUNCH_CHECK("locate_swd_stats (block sums)");
    swd_stats_final_kernel<<<1, SWD_THREADS, 0, st>>>(static_cast<const double*>(workspace), nblk, (double)n * (SWD_PATCH * SWD_PATCH), stats);
    LOCATE_LAUNCH_CHECK("locate_swd_stats");
    return LOCATE_OK;
}

// ---- the contraction -----------------------------------------------------------------------------------------------------------
// Block: 128 directions (rows of the product) x 128 descriptors (columns), four waves of 64 x 64 (2 x 2 instructions of 32 x 32).
// The descriptors are the product's columns because the accumulator has its column on the lane: a wave stores runs of 32
// consecutive j of one direction (128 bytes).  The reduction (147, padded with zero rows to 160) runs in five stages of 32 rows,
// double-buffered: [2][32][128] fp32 per operand, 64 KB, two blocks per CU; the loads of stage s are issued before the matrix
// instructions of stage s - 1 and written to LDS after them, one barrier per stage.  K is small enough for both WHOLE-K tiles
// ([148][128] each, 148 KB of CDNA4's 160 KB: one fill, one barrier, one block per CU); that form was built and measured at
// 0.60 of this one's rate, same bits - nothing hides its fill (profiles/notes_swd.md).
// Fill: thread t gathers descriptor t & 127 (one position record, one image) at k = t >> 7, + 2, ...: consecutive lanes write
// consecutive LDS words (no bank conflict), the gather itself hits L2 (the P descriptors of an image are consecutive rows, so a
// tile reads one or two images).  (v - mu) r is formed while the value goes to LDS: subtract first, by contract.
#define SWD_KC 32
#define SWD_STAGES ((SWD_K + SWD_KC - 1) / SWD_KC)
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(SWD_THREADS, 2) void swd_project_kernel(const float* __restrict__ level, int n, int S, const int2* __restrict__ pos, int P,
                                                                     const float* __restrict__ dirs, int D, const float* __restrict__ stats,
                                                                     float* __restrict__ proj) {
    __shared__ float Ds[2][SWD_KC][SWD_TILE];          // [stage buffer][k][direction]
    __shared__ float Vs[2][SWD_KC][SWD_TILE];          // [stage buffer][k][descriptor]
    const int tid = threadIdx.x, col = tid & (SWD_TILE - 1), khalf = tid >> 7;
    const int j0 = blockIdx.x * SWD_TILE, d0 = blockIdx.y * SWD_TILE;
    const bool dir_ok = d0 + col < D, desc_ok = j0 + col < n;
    const int plane = S * S;
    const float* base = level;
    if (desc_ok) {
        const int2 yx = pos[j0 + col];
        const int y = min(max(yx.x, 0), S - SWD_PATCH), x0 = min(max(yx.y, 0), S - SWD_PATCH);          // a bad record cannot leave the image
        base = level + (size_t)((j0 + col) / P) * 3 * plane + y * S + x0;
    }
    const float mu0 = stats[0], mu1 = stats[1], mu2 = stats[2], r0 = stats[3], r1 = stats[4], r2 = stats[5];
    const int lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;          // wave (wm, wn): directions 64 wm .., descriptors 64 wn ..
    const int lrow = lane >> 5, lcol = lane & 31;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][jj][e] = 0.0f;
    // pass s: the loads of stage s into registers, the matrix instructions of stage s - 1 (buffer (s - 1) & 1), the registers
    // into buffer s & 1 - whose last readers, stage s - 2, passed the barrier of the pass before - and one barrier
    for (int s = 0; s <= SWD_STAGES; ++s) {
        float dv[SWD_KC / 2], vv[SWD_KC / 2];
        if (s < SWD_STAGES) {          // rows k of dirs [147, D] and of the descriptors; zero beyond K, D and n
#pragma unroll
            for (int i = 0; i < SWD_KC / 2; ++i) {
                const int k = s * SWD_KC + khalf + 2 * i;
                const int c = k / (SWD_PATCH * SWD_PATCH), rem = k - c * (SWD_PATCH * SWD_PATCH), dy = rem / SWD_PATCH, dx = rem - dy * SWD_PATCH;
                dv[i] = (dir_ok && k < SWD_K) ? dirs[(size_t)k * D + d0 + col] : 0.0f;
                float v = 0.0f;
                if (desc_ok && k < SWD_K) {
                    const float m = c == 0 ? mu0 : c == 1 ? mu1 : mu2, rr = c == 0 ? r0 : c == 1 ? r1 : r2;
                    v = __fmul_rn(__fsub_rn(base[c * plane + dy * S + dx], m), rr);
                }
                vv[i] = v;
            }
        }
        if (s > 0) {
            const int buf = (s - 1) & 1;
#pragma unroll
            for (int k2 = 0; k2 < SWD_KC / 2; ++k2) {
                float a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = Ds[buf][2 * k2 + lrow][(wm * 2 + i) * 32 + lcol];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) b[jj] = Vs[buf][2 * k2 + lrow][(wn * 2 + jj) * 32 + lcol];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[jj], acc[i][jj], 0, 0, 0);
            }
        }
        if (s < SWD_STAGES) {
#pragma unroll
            for (int i = 0; i < SWD_KC / 2; ++i) {
                Ds[s & 1][khalf + 2 * i][col] = dv[i];
                Vs[s & 1][khalf + 2 * i][col] = vv[i];
            }
        }
        __syncthreads();
    }
    // accumulator element e of lane (lrow, lcol): row (e & 3) + 8 (e >> 2) + 4 lrow, column lcol
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = j0 + (wn * 2 + jj) * 32 + lcol;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int d = d0 + (wm * 2 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lrow;
                if (d < D && j < n) proj[(size_t)d * n + j] = acc[i][jj][e];
            }
        }
}

LOCATE_API int locate_swd_project(const float* level, int N, int S, const int32_t* pos, int P, const float* dirs, int D, const float* stats,
                                  float* proj, void* stream) {
    if (int e = swd_check("locate_swd_project", level, pos, N, S, P)) return e;
    LOCATE_REQUIRE(dirs && stats && proj && (((uintptr_t)dirs | (uintptr_t)stats | (uintptr_t)proj) & 3) == 0, "locate_swd_project: dirs / stats / proj null or misaligned");
    LOCATE_REQUIRE(D >= 1 && D <= SWD_TILE * 65535, "locate_swd_project: D = %d", D);
    const int n = N * P;
    const dim3 grid((unsigned)cdiv64(n, SWD_TILE), (unsigned)cdiv64(D, SWD_TILE));
    swd_project_kernel<<<grid, SWD_THREADS, 0, as_stream(stream)>>>(level, n, S, reinterpret_cast<const int2*>(pos), P, dirs, D, stats, proj);
    LOCATE_LAUNCH_CHECK("locate_swd_project");
    return LOCATE_OK;
}

// ---- mean |a - b| ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SWD_THREADS) void swd_distance_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t count, int vec,
                                                                           double* __restrict__ partials) {
    __shared__ double scratch[16];
    const int64_t tid = (int64_t)blockIdx.x * SWD_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * SWD_THREADS;
    double s = 0.0;
    const int64_t n4 = vec ? count >> 2 : 0;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 p = a4[i], q = b4[i];
        s += (double)fabsf(__fsub_rn(p.x, q.x));
        s += (double)fabsf(__fsub_rn(p.y, q.y));
        s += (double)fabsf(__fsub_rn(p.z, q.z));
        s += (double)fabsf(__fsub_rn(p.w, q.w));
    }
    for (int64_t i = 4 * n4 + tid; i < count; i += stride) s += (double)fabsf(__fsub_rn(a[i], b[i]));
    s = block_sum<double>(s, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(SWD_THREADS) void swd_distance_final_kernel(const double* __restrict__ partials, int nblk, double count, float* __restrict__ out) {
    __shared__ double scratch[16];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += SWD_THREADS) s += partials[b];
    s = block_sum<double>(s, scratch);
    if (threadIdx.x == 0) out[0] = (float)(s / count);
}

LOCATE_API size_t locate_swd_distance_workspace_bytes(void) { return (size_t)SWD_PARTIAL_BLOCKS_MAX * sizeof(double); }

LOCATE_API int locate_swd_distance(const float* a, const float* b, int64_t count, float* out, void* workspace, void* stream) {
    LOCATE_REQUIRE(a && b && out && workspace, "locate_swd_distance: null pointer");
    LOCATE_REQUIRE(count > 0, "locate_swd_distance: empty input");
    LOCATE_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "locate_swd_distance: misaligned pointer");
    int64_t nblk = cdiv64(count, (int64_t)SWD_THREADS * 16);          // ~16 values (four 16-byte loads per input) per thread
    nblk = nblk < 1 ? 1 : nblk > SWD_PARTIAL_BLOCKS_MAX ? SWD_PARTIAL_BLOCKS_MAX : nblk;
    hipStream_t st = as_stream(stream);
    swd_distance_partial_kernel<<<(int)nblk, SWD_THREADS, 0, st>>>(a, b, count, (((uintptr_t)a | (uintptr_t)b) & 15) == 0, static_cast<double*>(workspace));
    LOCATE_LAUNCH_CHECK("locate_swd_distance (block sums)");
    swd_distance_final_kernel<<<1, SWD_THREADS, 0, st>>>(static_cast<const double*>(workspace), (int)nblk, (double)count, out);
    LOCATE_LAUNCH_CHECK("locate_swd_distance");
    return LOCATE_OK;
}
