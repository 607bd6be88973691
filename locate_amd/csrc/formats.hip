// What a reduced-precision format would do to a contraction operand (locate_amd/formats.py): for every tensor VIEW of a call
//   base    {uint64 n, zeros, nonfinite, calls; double sumsq; uint32 absmax, pad; uint64 hist[32]}
//           sumsq: the sum of (double) x * (double) x over the FINITE elements (mt_take's arithmetic: every square exact, only the
//           additions round); absmax: the bit pattern of the largest finite magnitude; hist over the finite non-zero elements:
//           bin j counts those whose fp32 exponent field (a field of 0 counted as 1) lies j below that of absmax, bin 31 takes
//           everything lower.  Non-finite elements are counted and otherwise left out of everything;
//   format  {double err_sumsq; uint64 flushed, subnormal, clamped}, once per format of the table below:
//           err_sumsq  the float64 sum of e * e, e = (double) x - (double) q * 2^-scale taken in double (exact: e has at most 24
//                      significant bits, so its square is exact too);
//           flushed    x finite and non-zero, q == 0;   subnormal  q != 0 and |q| below the grid's smallest normal;
//           clamped    the rounded magnitude exceeded the grid's maximum (q is then that maximum).
// Like the statistics (stats.hip) a kernel of its own that only READS what the step left.  The reference has nothing of the kind.
//
//   id  name          grid (mantissa bits, smallest normal, max)   scale
//   0   e4m3_tensor   3, 2^-6,  448                                 one 2^k per tensor, k = f8_scale_exp(absmax): --dtype fp8's rule
//   1   e5m2_tensor   2, 2^-14, 57344                               one 2^k per tensor, k = scale_exp_below(14, absmax, 0)
//   2   mxfp8_e4m3    3, 2^-6,  448                                 per 32-block 2^X, X = clamp(max(field(A), 1) - 127 - 8, -127, 127),
//                                                                   A the block's largest finite magnitude (OCP MX v1.0)
//   3   mxfp4_e2m1    1, 2^0,   6                                   the same with - 2
//   4   bf16          7, 2^-126, 0x7f7f0000                         none
// Every quantiser rounds to nearest even onto the grid, subnormals included, and |q| is clamped to the maximum HERE - the
// conversion instructions never see a magnitude above it, so nothing depends on the hardware's overflow mode.  Formats 0 and 2 go
// through v_cvt_pk_fp8_f32 and back through v_cvt_f32_fp8, format 1 through the bf8 pair - the instructions the fp8 contractions
// use (convfp8.hip), not a lookalike; 3 and 4 are integer / v_rndne arithmetic.  Scaling is an fp32 multiplication by a power
// of two (never a denormal one: |k| <= 126, -125 <= -X <= 127): a product that is not exact lies below 2^-126 and quantises to
// zero on every grid.
//
// A view is {x, B, C, P, batch_stride, axis}: element (b, c, p) at x[b * batch_stride + c * P + p], the 32-element scale blocks
// along c (axis 1: stride P, at fixed (b, p)) or along p (axis 2: consecutive, at fixed (b, c)); a line's last block may be
// partial.  Up to FMT_MAX_VIEWS views travel BY VALUE in the launch arguments (finalise.hip's way): the tap of
// locate_amd/formats.py calls this hundreds of times per audited iteration with transient operands.
//
// Four launches.  (1) pass 1 over the views' TILES: {sumsq, absmax, nonfinite, zeros} per tile to the workspace.  (2) one block
// per view ADDS its tiles' partials, in a fixed order, into the caller's row and leaves this call's absmax in the workspace.
// (3) pass 2 reads that absmax, quantises, and leaves {err_sumsq, counters}[5] and a histogram per tile.  (4) one block per view
// adds those.  A tile is a fixed piece of a view's index space and an element has a fixed thread in it -
//   axis 1: 256 scale blocks, thread t takes block (b, cb, p) = unravel(256 tile + t) over [B, ceil(C / 32), P]: neighbouring
//           threads read neighbouring p (coalesced), a thread its 32 c in ascending order;
//   axis 2: 128 scale blocks, eight threads per block with four consecutive elements each (a 16-byte load where the address is
//           16-byte aligned, the same elements by 4-byte loads where not), four blocks per thread;
// - and every sum has multitensor.h's one order (mt_block_total, mt_add_partials), so a view's contribution depends on its
// contents and (B, C, P, axis) alone: not on alignment, batch_stride, the other views of the call or the grid.  No host read, no
// allocation, no floating-point atomics (the histogram and nothing else uses LDS integer atomics: order-free): legal under capture.
#include "multitensor.h"
#include "igemm.h"

#define FMT_MAX_VIEWS 8
#define FMT_COUNT 5
#define FMT_BLOCK 32          // elements per scale block
#define FMT_HIST 32

struct FmtView {
    const float* x;
    int B, C, P;
    long long batch_stride;
    int axis;
};
static_assert(sizeof(FmtView) == 40, "FmtView is part of the C ABI");

struct FmtBase {
    unsigned long long n, zeros, nonfinite, calls;
    double sumsq;
    unsigned absmax, pad;
    unsigned long long hist[FMT_HIST];
};
struct FmtFormat {
    double err_sumsq;
    unsigned long long flushed, subnormal, clamped;
};
struct FmtSlot {          // one view's place in the caller's rows
    FmtBase base;
    FmtFormat fmt[FMT_COUNT];
};
static_assert(sizeof(FmtBase) == 304 && sizeof(FmtFormat) == 32 && sizeof(FmtSlot) == 464, "the row layout is part of the C ABI");

struct FmtBatch {
    FmtView v[FMT_MAX_VIEWS];
    int tile0[FMT_MAX_VIEWS + 1];          // first tile of every view; [n] is the total
    int slot[FMT_MAX_VIEWS];
    int n;
};

// ---- partial records ------------------------------------------------------------------------------------------------------------------
struct Fmt1Tile {          // pass 1, one per tile
    double sumsq;
    unsigned absmax, nonfinite, zeros, pad;
    __device__ __forceinline__ void add(const Fmt1Tile& q) {
        sumsq += q.sumsq;
        absmax = q.absmax > absmax ? q.absmax : absmax;
        nonfinite += q.nonfinite;
        zeros += q.zeros;
    }
};
struct Fmt1Total {          // a view's total: 64-bit counts
    double sumsq;
    unsigned long long nonfinite, zeros;
    unsigned absmax, pad;
    __device__ __forceinline__ void add(const Fmt1Tile& q) {
        sumsq += q.sumsq;
        absmax = q.absmax > absmax ? q.absmax : absmax;
        nonfinite += q.nonfinite;
        zeros += q.zeros;
    }
    __device__ __forceinline__ void add(const Fmt1Total& q) {
        sumsq += q.sumsq;
        absmax = q.absmax > absmax ? q.absmax : absmax;
        nonfinite += q.nonfinite;
        zeros += q.zeros;
    }
};
struct Fmt2Tile {          // pass 2, one per tile: cnt[3 f + {0, 1, 2}] = flushed, subnormal, clamped of format f
    double err[FMT_COUNT];
    unsigned cnt[3 * FMT_COUNT], pad;
    __device__ __forceinline__ void add(const Fmt2Tile& q) {
#pragma unroll
        for (int f = 0; f < FMT_COUNT; ++f) err[f] += q.err[f];
#pragma unroll
        for (int i = 0; i < 3 * FMT_COUNT; ++i) cnt[i] += q.cnt[i];
    }
};
struct Fmt2Total {
    double err[FMT_COUNT];
    unsigned long long cnt[3 * FMT_COUNT];
    template <typename Q>
    __device__ __forceinline__ void add(const Q& q) {
#pragma unroll
        for (int f = 0; f < FMT_COUNT; ++f) err[f] += q.err[f];
#pragma unroll
        for (int i = 0; i < 3 * FMT_COUNT; ++i) cnt[i] += q.cnt[i];
    }
};

// ---- workspace: [this call's absmax per view: 64 bytes][Fmt1Tile x tiles][Fmt2Tile x tiles][unsigned hist[32] x tiles] --------------
#define FMT_WS_HEAD 64
static inline size_t fmt_ws_tiles1(void) { return FMT_WS_HEAD; }
static inline size_t fmt_ws_tiles2(long long tiles) { return FMT_WS_HEAD + (size_t)tiles * sizeof(Fmt1Tile); }
static inline size_t fmt_ws_hist(long long tiles) { return fmt_ws_tiles2(tiles) + (size_t)tiles * sizeof(Fmt2Tile); }
static inline size_t fmt_ws_bytes(long long tiles) { return fmt_ws_hist(tiles) + (size_t)tiles * FMT_HIST * sizeof(unsigned); }

// scale blocks and tiles of a view (host)
static inline long long fmt_blocks(const FmtView& v) {
    return v.axis == 1 ? (long long)v.B * ((v.C + FMT_BLOCK - 1) / FMT_BLOCK) * v.P : (long long)v.B * v.C * ((v.P + FMT_BLOCK - 1) / FMT_BLOCK);
}
static inline long long fmt_tiles(const FmtView& v) {
    const long long per = v.axis == 1 ? MT_THREADS : MT_THREADS / 2;
    return (fmt_blocks(v) + per - 1) / per;
}

static const char* const FMT_NAMES[FMT_COUNT] = {"e4m3_tensor", "e5m2_tensor", "mxfp8_e4m3", "mxfp4_e2m1", "bf16"};

// ---- a thread's elements ----------------------------------------------------------------------------------------------------------------
// axis 1: ONE scale block per thread and tile, N = 32 elements;  axis 2: FOUR blocks per thread and tile, N = 4 elements of each,
// eight neighbouring threads share a block.  `ok` has bit i set where element i exists; the others read as +0.0f and are never
// touched in memory.
template <int AXIS>
struct FmtShape {
    static constexpr int N = AXIS == 1 ? FMT_BLOCK : 4;
    static constexpr int ITEMS = AXIS == 1 ? 1 : 4;
};

__device__ __forceinline__ unsigned fmt_load_axis1(const FmtView& V, unsigned tile, float (&v)[FMT_BLOCK]) {
    const unsigned nb = (unsigned)(V.C + FMT_BLOCK - 1) / FMT_BLOCK;
    const unsigned blocks = (unsigned)V.B * nb * (unsigned)V.P;          // < 2^31: the entry checked it
    const unsigned i = tile * MT_THREADS + threadIdx.x;
    unsigned ok = 0u;
    if (i < blocks) {
        const unsigned p = i % (unsigned)V.P, r = i / (unsigned)V.P;
        const unsigned cb = r % nb, b = r / nb;
        const int c0 = (int)cb * FMT_BLOCK;
        const int len = V.C - c0 < FMT_BLOCK ? V.C - c0 : FMT_BLOCK;
        const float* src = V.x + (long long)b * V.batch_stride + (long long)c0 * V.P + p;
        ok = len == FMT_BLOCK ? 0xffffffffu : (1u << len) - 1u;
#pragma unroll
        for (int k = 0; k < FMT_BLOCK; ++k) v[k] = k < len ? src[(long long)k * V.P] : 0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < FMT_BLOCK; ++k) v[k] = 0.0f;
    }
    return ok;
}

__device__ __forceinline__ unsigned fmt_load_axis2(const FmtView& V, unsigned tile, int item, float (&v)[4]) {
    const unsigned nb = (unsigned)(V.P + FMT_BLOCK - 1) / FMT_BLOCK;
    const unsigned blocks = (unsigned)V.B * (unsigned)V.C * nb;
    const unsigned i = tile * (MT_THREADS / 2) + (unsigned)item * (MT_THREADS / 8) + (threadIdx.x >> 3);
    unsigned ok = 0u;
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (i < blocks) {
        const unsigned pb = i % nb, line = i / nb;
        const unsigned c = line % (unsigned)V.C, b = line / (unsigned)V.C;
        const int p0 = (int)pb * FMT_BLOCK + 4 * (int)(threadIdx.x & 7);
        const int len = V.P - p0;          // elements of the line from p0 on (<= 0: none of this thread's four)
        const float* src = V.x + (long long)b * V.batch_stride + (long long)c * V.P + p0;
        if (len >= 4 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            ok = 15u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < len) {
                    v[k] = src[k];
                    ok |= 1u << k;
                }
            }
        }
    }
    return ok;
}

// ---- pass 1 -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fmt_take1(float x, bool ok, Fmt1Tile& r) {
    mt_take(x, r.sumsq, r.absmax, r.nonfinite);          // a missing element is +0.0f: adds nothing to any of the three
    r.zeros += ok && (__float_as_uint(x) & 0x7fffffffu) == 0u ? 1u : 0u;
}

__device__ __forceinline__ int fmt_view_of(const FmtBatch& batch, int tile) {
    int vi = 0;
    for (int k = 1; k < batch.n; ++k)
        if (tile >= batch.tile0[k]) vi = k;
    return vi;
}

__global__ void __launch_bounds__(MT_THREADS) locate_formats_pass1_kernel(const FmtBatch batch, Fmt1Tile* __restrict__ tiles) {
    __shared__ Fmt1Tile lds[MT_WAVES];
    const int total = batch.tile0[batch.n];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int vi = fmt_view_of(batch, t);
        const FmtView& V = batch.v[vi];
        const unsigned tile = (unsigned)(t - batch.tile0[vi]);
        Fmt1Tile r = {0.0, 0u, 0u, 0u, 0u};
        if (V.axis == 1) {
            float v[FMT_BLOCK];
            const unsigned ok = fmt_load_axis1(V, tile, v);
#pragma unroll
            for (int k = 0; k < FMT_BLOCK; ++k) fmt_take1(v[k], (ok >> k) & 1u, r);
        } else {
            float v[4][4];
            unsigned ok[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) ok[it] = fmt_load_axis2(V, tile, it, v[it]);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
#pragma unroll
                for (int k = 0; k < 4; ++k) fmt_take1(v[it][k], (ok[it] >> k) & 1u, r);
            }
        }
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) tiles[t] = r;          // t < total: inside the workspace
    }
}

// one block per view: this call's totals ADDED to the row; this call's absmax left for pass 2
__global__ void __launch_bounds__(MT_THREADS) locate_formats_total1_kernel(const FmtBatch batch, const Fmt1Tile* __restrict__ tiles,
                                                                            unsigned* __restrict__ call_absmax, FmtSlot* __restrict__ rows) {
    __shared__ Fmt1Total lds[MT_WAVES];
    const int vi = blockIdx.x;
    const FmtView& V = batch.v[vi];
    Fmt1Total r = {0.0, 0ull, 0ull, 0u, 0u};
    mt_add_partials(tiles + batch.tile0[vi], batch.tile0[vi + 1] - batch.tile0[vi], r);
    r = mt_block_total(r, lds);
    if (threadIdx.x == 0) {
        FmtBase& B = rows[batch.slot[vi]].base;
        B.n += (unsigned long long)V.B * (unsigned long long)V.C * (unsigned long long)V.P;
        B.zeros += r.zeros;
        B.nonfinite += r.nonfinite;
        B.calls += 1ull;
        B.sumsq += r.sumsq;
        B.absmax = r.absmax > B.absmax ? r.absmax : B.absmax;
        call_absmax[vi] = r.absmax;
    }
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fmt_pow2d(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }          // |k| <= 1022

struct FmtScales {          // what one tensor's (per-tensor formats) or one block's (MX formats) exponent turns into
    float mul;          // x -> the grid's units
    double back;          // q -> x's units
};
__device__ __forceinline__ FmtScales fmt_scales(int k) {          // multiply by 2^k, -126 <= k <= 127
    FmtScales s;
    s.mul = pow2f(k);
    s.back = fmt_pow2d(-k);
    return s;
}

__device__ __forceinline__ void fmt_account(int f, float x, float q, bool counted, bool clamped, float smallest_normal, double back, Fmt2Tile& r) {
    const double e = (double)x - (double)q * back;
    r.err[f] = fma(e, e, r.err[f]);
    const unsigned qm = __float_as_uint(q) & 0x7fffffffu;          // compared as bits: bf16's subnormals are fp32 denormals
    r.cnt[3 * f + 0] += counted && qm == 0u ? 1u : 0u;
    r.cnt[3 * f + 1] += qm != 0u && qm < __float_as_uint(smallest_normal) ? 1u : 0u;
    r.cnt[3 * f + 2] += clamped ? 1u : 0u;
}

// e4m3 (BF8 false: max 448 = 1.110b x 2^8, the tie at 464 goes DOWN to it) / e5m2 (BF8 true: max 57344 = 1.11b x 2^15, the tie
// at 61440 goes UP past it) through the conversion instructions.  xs: x in the grid's units, finite.
template <bool BF8>
__device__ __forceinline__ float fmt_hw_quantise(float xs, bool& clamped) {
    const float top = BF8 ? 57344.0f : 448.0f;
    const float a = fabsf(xs);
    clamped = BF8 ? a >= 61440.0f : a > 464.0f;
    const float in = copysignf(fminf(a, top), xs);
    if (BF8) return __builtin_amdgcn_cvt_f32_bf8(__builtin_amdgcn_cvt_pk_bf8_f32(in, 0.0f, 0, false), 0);
    return __builtin_amdgcn_cvt_f32_fp8(__builtin_amdgcn_cvt_pk_fp8_f32(in, 0.0f, 0, false), 0);
}

// e2m1: 0, 0.5 (subnormal), 1, 1.5, 2, 3, 4, 6.  The step of a's binade (that of [1, 2) below 1), v_rndne on the multiple: ties go
// to the even multiple, which is the even mantissa.  7 is the tie between 6 and the absent 8 and goes up: clamped.
__device__ __forceinline__ float fmt_e2m1_quantise(float xs, bool& clamped) {
    const float a = fabsf(xs);
    int e = (int)(__float_as_uint(a) >> 23) - 127;
    e = e < 0 ? 0 : (e > 3 ? 3 : e);          // a < 8 by the MX scale rule; the clamp keeps pow2f in range whatever comes
    float q = rintf(a * pow2f(1 - e)) * pow2f(e - 1);
    clamped = q > 6.0f;
    q = clamped ? 6.0f : q;
    return copysignf(q, xs);
}

// bf16 on the bits: round to nearest even into the upper 16, the carry runs into the exponent; denormals are bf16's own subnormals
__device__ __forceinline__ float fmt_bf16_quantise(float x, bool& clamped) {
    const unsigned bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
    unsigned q = (mag + 0x7fffu + ((mag >> 16) & 1u)) & 0xffff0000u;
    clamped = q >= 0x7f800000u;
    q = clamped ? 0x7f7f0000u : q;
    return __uint_as_float(q | (bits & 0x80000000u));
}

// X of OCP MX v1.0 for element grids whose largest binade is 2^emax
__device__ __forceinline__ int fmt_mx_exp(unsigned block_absmax, int emax) {
    const int field = (int)(block_absmax >> 23);
    const int X = (field < 1 ? 1 : field) - 127 - emax;
    return X < -127 ? -127 : (X > 127 ? 127 : X);
}

struct FmtTensorScales {
    FmtScales f0, f1;
    int top_field;          // max(field(absmax), 1)
};

__device__ __forceinline__ void fmt_take2(float x, bool ok, const FmtTensorScales& T, const FmtScales& m8, const FmtScales& m4, Fmt2Tile& r,
                                          unsigned* __restrict__ hist) {
    const unsigned mag = __float_as_uint(x) & 0x7fffffffu;
    const bool counted = ok && mag != 0u && mag < 0x7f800000u;          // finite and non-zero
    const float xv = mag < 0x7f800000u ? x : 0.0f;          // a non-finite element is left out: it enters as a zero that counts nowhere
    if (counted) {
        const int field = (int)(mag >> 23);
        const int j = T.top_field - (field < 1 ? 1 : field);
        atomicAdd(&hist[j > FMT_HIST - 1 ? FMT_HIST - 1 : j], 1u);
    }
    bool cl;
    float q = fmt_hw_quantise<false>(xv * T.f0.mul, cl);
    fmt_account(0, xv, q, counted, cl, 0.015625f, T.f0.back, r);
    q = fmt_hw_quantise<true>(xv * T.f1.mul, cl);
    fmt_account(1, xv, q, counted, cl, 6.103515625e-05f, T.f1.back, r);
    q = fmt_hw_quantise<false>(xv * m8.mul, cl);
    fmt_account(2, xv, q, counted, cl, 0.015625f, m8.back, r);
    q = fmt_e2m1_quantise(xv * m4.mul, cl);
    fmt_account(3, xv, q, counted, cl, 1.0f, m4.back, r);
    q = fmt_bf16_quantise(xv, cl);
    fmt_account(4, xv, q, counted, cl, 1.17549435e-38f, 1.0, r);
}

__device__ __forceinline__ unsigned fmt_finite_mag(float x) {
    const unsigned mag = __float_as_uint(x) & 0x7fffffffu;
    return mag < 0x7f800000u ? mag : 0u;
}

__global__ void __launch_bounds__(MT_THREADS) locate_formats_pass2_kernel(const FmtBatch batch, const unsigned* __restrict__ call_absmax,
                                                                           Fmt2Tile* __restrict__ tiles, unsigned* __restrict__ hists) {
    __shared__ Fmt2Tile lds[MT_WAVES];
    __shared__ unsigned hist[FMT_HIST];
    const int total = batch.tile0[batch.n];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int vi = fmt_view_of(batch, t);
        const FmtView& V = batch.v[vi];
        const unsigned tile = (unsigned)(t - batch.tile0[vi]);
        const unsigned amax = call_absmax[vi];
        FmtTensorScales T;
        T.f0 = fmt_scales(f8_scale_exp(amax));
        T.f1 = fmt_scales(scale_exp_below(14, amax, 0u));
        T.top_field = (int)(amax >> 23) < 1 ? 1 : (int)(amax >> 23);
        if (threadIdx.x < FMT_HIST) hist[threadIdx.x] = 0u;
        __syncthreads();
        Fmt2Tile r;
#pragma unroll
        for (int f = 0; f < FMT_COUNT; ++f) r.err[f] = 0.0;
#pragma unroll
        for (int i = 0; i < 3 * FMT_COUNT; ++i) r.cnt[i] = 0u;
        r.pad = 0u;
        if (V.axis == 1) {
            float v[FMT_BLOCK];
            const unsigned ok = fmt_load_axis1(V, tile, v);
            unsigned a = 0u;
#pragma unroll
            for (int k = 0; k < FMT_BLOCK; ++k) {
                const unsigned m = fmt_finite_mag(v[k]);
                a = m > a ? m : a;
            }
            const FmtScales m8 = fmt_scales(-fmt_mx_exp(a, 8)), m4 = fmt_scales(-fmt_mx_exp(a, 2));
#pragma unroll
            for (int k = 0; k < FMT_BLOCK; ++k) fmt_take2(v[k], (ok >> k) & 1u, T, m8, m4, r, hist);
        } else {
            float v[4][4];
            unsigned ok[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) ok[it] = fmt_load_axis2(V, tile, it, v[it]);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                unsigned a = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned m = fmt_finite_mag(v[it][k]);
                    a = m > a ? m : a;
                }
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) {          // the block's eight threads are neighbours in one wave
                    const unsigned w = (unsigned)__shfl_xor((int)a, o, 64);
                    a = w > a ? w : a;
                }
                const FmtScales m8 = fmt_scales(-fmt_mx_exp(a, 8)), m4 = fmt_scales(-fmt_mx_exp(a, 2));
#pragma unroll
                for (int k = 0; k < 4; ++k) fmt_take2(v[it][k], (ok[it] >> k) & 1u, T, m8, m4, r, hist);
            }
        }
        r = mt_block_total(r, lds);          // its first barrier also closes the histogram
        if (threadIdx.x == 0) tiles[t] = r;
        if (threadIdx.x < FMT_HIST) hists[(size_t)t * FMT_HIST + threadIdx.x] = hist[threadIdx.x];
    }
}

__global__ void __launch_bounds__(MT_THREADS) locate_formats_total2_kernel(const FmtBatch batch, const Fmt2Tile* __restrict__ tiles,
                                                                            const unsigned* __restrict__ hists, FmtSlot* __restrict__ rows) {
    __shared__ Fmt2Total lds[MT_WAVES];
    __shared__ unsigned long long hsum[MT_THREADS];
    const int vi = blockIdx.x;
    const int first = batch.tile0[vi], nt = batch.tile0[vi + 1] - first;
    Fmt2Total r;
#pragma unroll
    for (int f = 0; f < FMT_COUNT; ++f) r.err[f] = 0.0;
#pragma unroll
    for (int i = 0; i < 3 * FMT_COUNT; ++i) r.cnt[i] = 0ull;
    mt_add_partials(tiles + first, nt, r);
    r = mt_block_total(r, lds);
    // the histogram: integer sums, any order.  Thread t adds bin t % 32 of every eighth tile
    // - eight of its loads in flight at once: one after the other, a large view's 576 dependent round trips per thread took as
    // long as the whole second pass (profiles/notes_formats.md)
    constexpr int STEP = MT_THREADS / FMT_HIST;
    const unsigned* hp = hists + (size_t)first * FMT_HIST + (threadIdx.x & (FMT_HIST - 1));
    unsigned long long h = 0ull;
    int i = threadIdx.x >> 5;
    for (; i + 7 * STEP < nt; i += 8 * STEP) {
        unsigned w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = hp[(size_t)(i + u * STEP) * FMT_HIST];
#pragma unroll
        for (int u = 0; u < 8; ++u) h += w[u];
    }
    for (; i < nt; i += STEP) h += hp[(size_t)i * FMT_HIST];
    hsum[threadIdx.x] = h;
    __syncthreads();
    FmtSlot& S = rows[batch.slot[vi]];
    if (threadIdx.x < FMT_HIST) {
        unsigned long long s = 0ull;
        for (int k = 0; k < MT_THREADS / FMT_HIST; ++k) s += hsum[threadIdx.x + k * FMT_HIST];
        S.base.hist[threadIdx.x] += s;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < FMT_COUNT; ++f) {
            S.fmt[f].err_sumsq += r.err[f];
            S.fmt[f].flushed += r.cnt[3 * f + 0];
            S.fmt[f].subnormal += r.cnt[3 * f + 1];
            S.fmt[f].clamped += r.cnt[3 * f + 2];
        }
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
LOCATE_API int locate_formats_count(void) { return FMT_COUNT; }
LOCATE_API const char* locate_formats_name(int i) { return i >= 0 && i < FMT_COUNT ? FMT_NAMES[i] : nullptr; }
LOCATE_API int locate_formats_max_views(void) { return FMT_MAX_VIEWS; }
LOCATE_API size_t locate_formats_view_record_bytes(void) { return sizeof(FmtView); }
LOCATE_API size_t locate_formats_base_record_bytes(void) { return sizeof(FmtBase); }
LOCATE_API size_t locate_formats_format_record_bytes(void) { return sizeof(FmtFormat); }

// fills the batch from the host records; the status of a damaged argument
static int fmt_batch(const void* host_views, int n_views, const int* row_slots, FmtBatch& b, const char* who) {
    LOCATE_REQUIRE(host_views && n_views >= 1 && n_views <= FMT_MAX_VIEWS, "%s: 1 to %d views, got %d", who, FMT_MAX_VIEWS, n_views);
    const FmtView* views = static_cast<const FmtView*>(host_views);
    long long tiles = 0;
    b = FmtBatch{};
    for (int i = 0; i < n_views; ++i) {
        const FmtView& v = views[i];
        LOCATE_REQUIRE(v.x && (reinterpret_cast<uintptr_t>(v.x) & 3) == 0, "%s: view %d needs a 4-byte aligned address", who, i);
        LOCATE_REQUIRE(v.axis == 1 || v.axis == 2, "%s: view %d: axis %d is neither 1 nor 2", who, i, v.axis);
        LOCATE_REQUIRE(v.B > 0 && v.C > 0 && v.P > 0, "%s: view %d: non-positive extent [%d, %d, %d]", who, i, v.B, v.C, v.P);
        LOCATE_REQUIRE((long long)v.B * v.C * v.P < (1ll << 31), "%s: view %d holds 2^31 elements or more", who, i);
        LOCATE_REQUIRE(v.batch_stride >= (long long)v.C * v.P, "%s: view %d: batch stride %lld below C * P = %lld", who, i, v.batch_stride,
                       (long long)v.C * v.P);
        LOCATE_REQUIRE(!row_slots || row_slots[i] >= 0, "%s: view %d: negative row slot", who, i);
        b.v[i] = v;
        b.tile0[i] = (int)tiles;
        b.slot[i] = row_slots ? row_slots[i] : 0;
        tiles += fmt_tiles(v);          // < 2^31 / 128 each
    }
    b.tile0[n_views] = (int)tiles;
    b.n = n_views;
    return LOCATE_OK;
}

// bytes of workspace a call with these views needs; 0 for damaged arguments (locate_last_error says which)
LOCATE_API size_t locate_formats_workspace_bytes(const void* host_views, int n_views) {
    FmtBatch b;
    if (fmt_batch(host_views, n_views, nullptr, b, "locate_formats_workspace_bytes") != LOCATE_OK) return 0;
    return fmt_ws_bytes(b.tile0[n_views]);
}

// host_views: HOST array of n_views FmtView; row_slots: HOST array, view i ADDS into slot row_slots[i] of `rows` (DEVICE, 464-byte
// slots {base, format[5]}, 8-byte aligned, zeroed by the caller before a row's first call; two views of one call must not share a
// slot).  workspace: DEVICE, locate_formats_workspace_bytes(host_views, n_views) bytes, 8-byte aligned, need not be zeroed.
// Writes the named slots and the workspace, nothing else.  A damaged argument returns an error status and launches nothing.
LOCATE_API int locate_formats_audit(const void* host_views, int n_views, const int* row_slots, void* rows, void* workspace, void* stream) {
    LOCATE_REQUIRE(row_slots && rows && workspace, "locate_formats_audit: bad arguments");
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                   "locate_formats_audit: rows and workspace need 8-byte alignment");
    FmtBatch b;
    const int bad = fmt_batch(host_views, n_views, row_slots, b, "locate_formats_audit");
    if (bad != LOCATE_OK) return bad;
    for (int i = 0; i < n_views; ++i)
        for (int j = 0; j < i; ++j) LOCATE_REQUIRE(b.slot[i] != b.slot[j], "locate_formats_audit: views %d and %d share row slot %d", j, i, b.slot[i]);
    const int tiles = b.tile0[n_views];
    char* ws = static_cast<char*>(workspace);
    unsigned* call_absmax = reinterpret_cast<unsigned*>(ws);
    Fmt1Tile* t1 = reinterpret_cast<Fmt1Tile*>(ws + fmt_ws_tiles1());
    Fmt2Tile* t2 = reinterpret_cast<Fmt2Tile*>(ws + fmt_ws_tiles2(tiles));
    unsigned* hists = reinterpret_cast<unsigned*>(ws + fmt_ws_hist(tiles));
    FmtSlot* R = static_cast<FmtSlot*>(rows);
    hipStream_t st = as_stream(stream);
    locate_formats_pass1_kernel<<<mt_grid(tiles), MT_THREADS, 0, st>>>(b, t1);
    LOCATE_LAUNCH_CHECK("locate_formats_audit(pass 1)");
    locate_formats_total1_kernel<<<n_views, MT_THREADS, 0, st>>>(b, t1, call_absmax, R);
    LOCATE_LAUNCH_CHECK("locate_formats_audit(total 1)");
    locate_formats_pass2_kernel<<<mt_grid(tiles), MT_THREADS, 0, st>>>(b, call_absmax, t2, hists);
    LOCATE_LAUNCH_CHECK("locate_formats_audit(pass 2)");
    locate_formats_total2_kernel<<<n_views, MT_THREADS, 0, st>>>(b, t2, hists, R);
    LOCATE_LAUNCH_CHECK("locate_formats_audit(total 2)");
    return LOCATE_OK;
}
