// Radial (azimuthally averaged) power spectrum of image planes: the instrument for the spectral artefacts of up-convolutions
// (Durall et al. 2020, "Watch your Up-Convolution"; Odena et al. 2016) - an excess at the high end of the spectrum and a
// checkerboard at (Nyquist, Nyquist).  The arithmetic, per plane x fp32 [S, S], S in {32, 64, 128, 256}, H = S / 2:
//   tables  : C[k][j] = cos(2 pi k j / S) w[j], Sn[k][j] = sin(2 pi k j / S) w[j], fp32 [S][S], made by the caller (the window w
//             is folded in); the kernels and the float64 model read the same words;
//   stage 1 : Ar[y][k] = sum_x x[y][x] C[k][x] (k = 0 .. H), Ai[y][k] = - sum_x x[y][x] Sn[k][x] (k = 1 .. H - 1; columns 0 and H
//             of Ai are identically zero and never formed): exactly S columns, one S x S x S product, kept TRANSPOSED
//             (A1[c][y], c = k for Ar and H + k for Ai) so that stage 2 reads it along its contraction;
//   stage 2 : Yr[a][k] = sum_y C[a][y] Ar[y][k] + Sn[a][y] Ai[y][k], Yi[a][k] = sum_y C[a][y] Ai[y][k] - Sn[a][y] Ar[y][k],
//             a = 0 .. S - 1, k = 0 .. H: per 16 x 16 tile of (a, k) two accumulators that share the stage-1 operand;
//   power   : ((double) Yr^2 + (double) Yi^2) m[k] / S^4, m = 1 for k in {0, H} and 2 otherwise, written to slot[a][k] of a list
//             in which the frequencies of one radial bin are consecutive (the caller's bin table in its sorted form);
//   bins    : spectrum[r] = the sum of list[start[r] .. start[r + 1]), float64, four interleaved partial sums added as
//             (p0 + p1) + (p2 + p3).
// Both products run on v_mfma_f32_16x16x4_f32 (exact fp32, fmaf chains).  A lane loads 16 bytes of each operand row - elements
// 4 g .. 4 g + 3 (g = lane >> 4) of 16 consecutive contraction indices - and the s-th of four instructions contracts element
// 4 g + s of every group: a permutation of the contraction index, the same for both operands.
// S <= 64: one block per plane, the plane, both tables and A1 in LDS (rows padded by four words), the power list over the plane
// once stage 1 is done; one global read of the plane, one write of R doubles.  S >= 128: the same three steps as three launches,
// operands read from global memory (the tables stay in L2), A1 and the power list in the caller's workspace.
// No atomics; a plane's result depends on its values and the tables alone - not on its neighbours in the call, nor on alignment.
#include "common.h"

#define SPEC_THREADS 256
#define SPEC_WAVES (SPEC_THREADS / 64)
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 spec_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// T1 row c: C[c] for c <= H, - Sn[c - H] beyond.  Tile (yt, ct) of A1[c][y] = sum_x X[y][x] T1[c][x]; two chains over alternate
// groups of 16, added at the end.  X, Ct, St: rows of LD words; A1: rows of LDA words.
template <int S, int LD, int LDA>
__device__ __forceinline__ void spec_stage1_tile(const float* X, const float* Ct, const float* St, int yt, int ct, float* A1, int lane) {
    constexpr int H = S / 2;
    const int i = lane & 15, g = lane >> 4;
    const int c = 16 * ct + i;
    const bool im = c > H;
    const float* trow = (im ? St + (c - H) * LD : Ct + c * LD) + 4 * g;
    const float* xrow = X + (16 * yt + i) * LD + 4 * g;
    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int k0 = 0; k0 < S; k0 += 32) {
        const f32x4 a0 = spec_ld4(xrow + k0), a1 = spec_ld4(xrow + k0 + 16);
        f32x4 b0 = spec_ld4(trow + k0), b1 = spec_ld4(trow + k0 + 16);
        if (im) { b0 = -b0; b1 = -b1; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], acc1, 0, 0, 0);
        }
    }
    acc0 += acc1;
    // accumulator element e of lane (g, i): y = 16 yt + 4 g + e, c = 16 ct + i
    *reinterpret_cast<f32x4*>(A1 + c * LDA + 16 * yt + 4 * g) = acc0;
}

// Tile (at, kt) of Yr / Yi and its powers.  kt = H / 16 holds column H alone (the other fifteen are computed from rows of A1 that
// exist and dropped); it and column 0 have no imaginary stage-1 part.  cells = S (H + 1).
template <int S, int LD, int LDA>
__device__ __forceinline__ void spec_stage2_tile(const float* Ct, const float* St, const float* A1, int at, int kt, const int* __restrict__ slot,
                                                 double* P, int lane) {
    constexpr int H = S / 2, cells = S * (H + 1);
    const int i = lane & 15, g = lane >> 4;
    const int a = 16 * at + i, k = 16 * kt + i;          // k <= H + 15 < S
    const bool has_im = k >= 1 && k < H;
    const bool full = kt < H / 16;                       // wave-uniform
    const float* crow = Ct + a * LD + 4 * g;
    const float* srow = St + a * LD + 4 * g;
    const float* rrow = A1 + k * LDA + 4 * g;
    const float* irow = A1 + (has_im ? H + k : 0) * LDA + 4 * g;
    f32x4 yr = {0.0f, 0.0f, 0.0f, 0.0f}, yi = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int y0 = 0; y0 < S; y0 += 16) {
        const f32x4 c4 = spec_ld4(crow + y0), s4 = spec_ld4(srow + y0), br = spec_ld4(rrow + y0);
        const f32x4 ns4 = -s4;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            yr = __builtin_amdgcn_mfma_f32_16x16x4f32(c4[s], br[s], yr, 0, 0, 0);
            yi = __builtin_amdgcn_mfma_f32_16x16x4f32(ns4[s], br[s], yi, 0, 0, 0);
        }
        if (full) {
            f32x4 bi = spec_ld4(irow + y0);
            if (!has_im) bi = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                yr = __builtin_amdgcn_mfma_f32_16x16x4f32(s4[s], bi[s], yr, 0, 0, 0);
                yi = __builtin_amdgcn_mfma_f32_16x16x4f32(c4[s], bi[s], yi, 0, 0, 0);
            }
        }
    }
    // accumulator element e of lane (g, i): a = 16 at + 4 g + e, k = 16 kt + i
    if (k <= H) {
        const double scale = ((k == 0 || k == H) ? 1.0 : 2.0) / ((double)S * S * S * S);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = 16 * at + 4 * g + e;
            const int at_slot = min(max(slot[row * (H + 1) + k], 0), cells - 1);          // a bad table cannot leave the list
            const double re = (double)yr[e], ig = (double)yi[e];
            P[at_slot] = (re * re + ig * ig) * scale;
        }
    }
}

// spectrum[r] = sum of P[start[r] .. start[r + 1]): four lanes per bin, interleaved, (p0 + p1) + (p2 + p3)
__device__ __forceinline__ void spec_bin_sums(const double* P, const int* __restrict__ start, int R, int cells, double* __restrict__ out, int tid) {
    const int q = tid & 3;
    for (int r = tid >> 2; r < R; r += SPEC_THREADS / 4) {
        const int lo = min(max(start[r], 0), cells), hi = min(max(start[r + 1], lo), cells);
        double s = 0.0;
        for (int j = lo + q; j < hi; j += 4) s += P[j];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (q == 0) out[r] = s;
    }
}

template <int S>
__global__ __launch_bounds__(SPEC_THREADS) void spectrum_fused_kernel(const float* __restrict__ x, const float* __restrict__ Ct, const float* __restrict__ St,
                                                                      const int* __restrict__ slot, const int* __restrict__ start, int R, int vec,
                                                                      double* __restrict__ out) {
    constexpr int LD = S + 4, H = S / 2, TA = S / 16, NT = H / 16 + 1;
    static_assert(S * (H + 1) * sizeof(double) <= S * LD * sizeof(float), "the power list lies over the plane");
    extern __shared__ uint4 spec_smem[];          // Xs | Cs | Ss | A1, [S][LD] fp32 each
    float* Xs = reinterpret_cast<float*>(spec_smem);
    float* Cs = Xs + S * LD;
    float* Ss = Cs + S * LD;
    float* A1 = Ss + S * LD;
    double* P = reinterpret_cast<double*>(spec_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* px = x + (size_t)blockIdx.x * S * S;
    for (int v = tid; v < S * S / 4; v += SPEC_THREADS) {
        const int row = v / (S / 4), col = 4 * (v % (S / 4));
        *reinterpret_cast<f32x4*>(Cs + row * LD + col) = spec_ld4(Ct + row * S + col);
        *reinterpret_cast<f32x4*>(Ss + row * LD + col) = spec_ld4(St + row * S + col);
        f32x4 xv;
        if (vec) {
            xv = spec_ld4(px + row * S + col);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = px[row * S + col + e];
        }
        *reinterpret_cast<f32x4*>(Xs + row * LD + col) = xv;
    }
    __syncthreads();
    for (int j = wave; j < TA * TA; j += SPEC_WAVES) spec_stage1_tile<S, LD, LD>(Xs, Cs, Ss, j % TA, j / TA, A1, lane);
    __syncthreads();          // A1 complete; nobody reads the plane any more: the power list takes its place
    for (int j = wave; j < TA * NT; j += SPEC_WAVES) spec_stage2_tile<S, LD, LD>(Cs, Ss, A1, j % TA, j / TA, slot, P, lane);
    __syncthreads();
    spec_bin_sums(P, start, R, S * (H + 1), out + (size_t)blockIdx.x * R, tid);
}

// ---- S >= 128: the three steps as three launches; blockIdx.x: the plane, blockIdx.y: four tiles (one per wave) -------------------
template <int S>
__global__ __launch_bounds__(SPEC_THREADS) void spectrum_stage1_kernel(const float* __restrict__ x, const float* __restrict__ Ct, const float* __restrict__ St,
                                                                       float* __restrict__ a1) {
    constexpr int TA = S / 16;
    const int j = blockIdx.y * SPEC_WAVES + (threadIdx.x >> 6);
    if (j < TA * TA)
        spec_stage1_tile<S, S, S>(x + (size_t)blockIdx.x * S * S, Ct, St, j % TA, j / TA, a1 + (size_t)blockIdx.x * S * S, threadIdx.x & 63);
}

template <int S>
__global__ __launch_bounds__(SPEC_THREADS) void spectrum_stage2_kernel(const float* __restrict__ Ct, const float* __restrict__ St, const float* __restrict__ a1,
                                                                       const int* __restrict__ slot, double* __restrict__ power) {
    constexpr int H = S / 2, TA = S / 16, NT = H / 16 + 1;
    const int j = blockIdx.y * SPEC_WAVES + (threadIdx.x >> 6);
    if (j < TA * NT)
        spec_stage2_tile<S, S, S>(Ct, St, a1 + (size_t)blockIdx.x * S * S, j % TA, j / TA, slot, power + (size_t)blockIdx.x * S * (H + 1), threadIdx.x & 63);
}

__global__ __launch_bounds__(SPEC_THREADS) void spectrum_bins_kernel(const double* __restrict__ power, const int* __restrict__ start, int R, int cells,
                                                                     double* __restrict__ out) {
    spec_bin_sums(power + (size_t)blockIdx.x * cells, start, R, cells, out + (size_t)blockIdx.x * R, threadIdx.x);
}

static bool spec_size_ok(int S) { return S == 32 || S == 64 || S == 128 || S == 256; }

// S <= 64: nothing.  Beyond: per plane A1 fp32 [S][S], then per plane the power list float64 [S (S / 2 + 1)].
LOCATE_API size_t locate_spectrum_workspace_bytes(int planes, int S) {
    if (planes < 1 || !spec_size_ok(S) || S <= 64) return 0;
    return (size_t)planes * ((size_t)S * S * sizeof(float) + (size_t)S * (S / 2 + 1) * sizeof(double));
}

template <int S>
static void spec_launch_fused(const float* x, int planes, const float* Ct, const float* St, const int* slot, const int* start, int R, double* out,
                              hipStream_t st) {
    constexpr size_t lds = (size_t)4 * S * (S + 4) * sizeof(float);          // 18 KB at 32, 68 KB at 64: above the default limit
    auto k = spectrum_fused_kernel<S>;
    static bool enabled = false;
    if (!enabled) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); enabled = true; }
    k<<<planes, SPEC_THREADS, lds, st>>>(x, Ct, St, slot, start, R, ((uintptr_t)x & 15) == 0, out);
}

template <int S>
static int spec_launch_staged(const float* x, int planes, const float* Ct, const float* St, const int* slot, const int* start, int R, double* out,
                              void* workspace, hipStream_t st) {
    constexpr int H = S / 2, TA = S / 16, NT = H / 16 + 1, cells = S * (H + 1);
    float* a1 = static_cast<float*>(workspace);
    double* power = reinterpret_cast<double*>(a1 + (size_t)planes * S * S);
    spectrum_stage1_kernel<S><<<dim3(planes, TA * TA / SPEC_WAVES), SPEC_THREADS, 0, st>>>(x, Ct, St, a1);
    LOCATE_LAUNCH_CHECK("locate_spectrum_planes (stage 1)");
    spectrum_stage2_kernel<S><<<dim3(planes, TA * NT / SPEC_WAVES), SPEC_THREADS, 0, st>>>(Ct, St, a1, slot, power);
    LOCATE_LAUNCH_CHECK("locate_spectrum_planes (stage 2)");
    spectrum_bins_kernel<<<planes, SPEC_THREADS, 0, st>>>(power, start, R, cells, out);
    return LOCATE_OK;
}

LOCATE_API int locate_spectrum_planes(const float* x, int planes, int S, const float* cos_table, const float* sin_table, const int32_t* slot,
                                      const int32_t* start, int R, double* spectra, void* workspace, void* stream) {
    LOCATE_REQUIRE(x && cos_table && sin_table && slot && start && spectra, "locate_spectrum_planes: null pointer");
    LOCATE_REQUIRE(spec_size_ok(S), "locate_spectrum_planes: S = %d (32, 64, 128 or 256)", S);
    LOCATE_REQUIRE(planes >= 1 && (int64_t)planes * S * S < ((int64_t)1 << 31), "locate_spectrum_planes: %d planes of %d x %d (1 .. 2^31 - 1 elements)", planes, S, S);
    LOCATE_REQUIRE(R >= 1 && R <= S * (S / 2 + 1), "locate_spectrum_planes: R = %d", R);
    LOCATE_REQUIRE(((uintptr_t)x & 3) == 0 && (((uintptr_t)cos_table | (uintptr_t)sin_table) & 15) == 0 && (((uintptr_t)slot | (uintptr_t)start) & 3) == 0 &&
                   ((uintptr_t)spectra & 7) == 0, "locate_spectrum_planes: x / slot / start must be 4-byte, the tables 16-byte, spectra 8-byte aligned");
    hipStream_t st = as_stream(stream);
    if (S <= 64) {
        if (S == 32) spec_launch_fused<32>(x, planes, cos_table, sin_table, slot, start, R, spectra, st);
        else spec_launch_fused<64>(x, planes, cos_table, sin_table, slot, start, R, spectra, st);
    } else {
        // the staged kernels load 16 bytes per lane straight from the plane
        LOCATE_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)x & 15) == 0,
                       "locate_spectrum_planes: S = %d needs a 16-byte aligned workspace and 16-byte aligned planes", S);
        if (int e = S == 128 ? spec_launch_staged<128>(x, planes, cos_table, sin_table, slot, start, R, spectra, workspace, st)
                             : spec_launch_staged<256>(x, planes, cos_table, sin_table, slot, start, R, spectra, workspace, st)) return e;
    }
    LOCATE_LAUNCH_CHECK("locate_spectrum_planes");
    return LOCATE_OK;
}

// ---- the set summary ---------------------------------------------------------------------------------------------------------------
// flags[p] = 1 where plane p's spectrum holds a NaN or an Inf: one wave per plane, its lanes across the bins
__global__ __launch_bounds__(SPEC_THREADS) void spectrum_flags_kernel(const double* __restrict__ spectra, int planes, int R, int* __restrict__ flags) {
    const int p = blockIdx.x * SPEC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= planes) return;          // wave-uniform
    int bad = 0;
    for (int r = lane; r < R; r += 64) bad |= !isfinite(spectra[(size_t)p * R + r]);
    bad = __any(bad);
    if (lane == 0) flags[p] = bad;
}

// block (r, c): over the images in ascending order, the sum and the sum of squares of spectrum / count[r] of the finite planes of
// channel c; the blocks of bin 0 also count the channel's planes that are not finite
__global__ __launch_bounds__(SPEC_THREADS) void spectrum_sums_kernel(const double* __restrict__ spectra, int n, int C, int R, const double* __restrict__ count,
                                                                     const int* __restrict__ flags, double* __restrict__ sums, int* __restrict__ nonfinite) {
    __shared__ double scratch[16];
    __shared__ int iscratch[16];
    const int r = blockIdx.x, c = blockIdx.y;
    const double cnt = count[r];
    double s = 0.0, q = 0.0;
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += SPEC_THREADS) {
        const size_t p = (size_t)i * C + c;
        if (flags[p]) {
            ++bad;
        } else {
            const double v = spectra[p * R + r] / cnt;
            s += v;
            q += v * v;
        }
    }
    s = block_sum<double>(s, scratch);
    q = block_sum<double>(q, scratch);
    bad = block_sum<int>(bad, iscratch);
    if (threadIdx.x == 0) {
        sums[(size_t)c * R + r] = s;
        sums[(size_t)(C + c) * R + r] = q;
        if (r == 0) nonfinite[c] = bad;
    }
}

LOCATE_API size_t locate_spectrum_summary_workspace_bytes(int planes) { return planes < 1 ? 0 : (size_t)planes * sizeof(int); }

LOCATE_API int locate_spectrum_summary(const double* spectra, int n, int channels, int R, const double* count, double* sums, int32_t* nonfinite,
                                       void* workspace, void* stream) {
    LOCATE_REQUIRE(spectra && count && sums && nonfinite && workspace, "locate_spectrum_summary: null pointer");
    LOCATE_REQUIRE(n >= 1 && channels >= 1 && channels <= 65535 && R >= 1 && (int64_t)n * channels * R < ((int64_t)1 << 31),
                   "locate_spectrum_summary: n = %d, channels = %d, R = %d", n, channels, R);
    LOCATE_REQUIRE((((uintptr_t)spectra | (uintptr_t)count | (uintptr_t)sums) & 7) == 0 && (((uintptr_t)nonfinite | (uintptr_t)workspace) & 3) == 0,
                   "locate_spectrum_summary: misaligned pointer");
    hipStream_t st = as_stream(stream);
    const int planes = n * channels;
    spectrum_flags_kernel<<<(int)cdiv64(planes, SPEC_WAVES), SPEC_THREADS, 0, st>>>(spectra, planes, R, static_cast<int*>(workspace));
    LOCATE_LAUNCH_CHECK("locate_spectrum_summary (flags)");
    spectrum_sums_kernel<<<dim3(R, channels), SPEC_THREADS, 0, st>>>(spectra, n, channels, R, count, static_cast<const int*>(workspace), sums, nonfinite);
    LOCATE_LAUNCH_CHECK("locate_spectrum_summary");
    return LOCATE_OK;
}
