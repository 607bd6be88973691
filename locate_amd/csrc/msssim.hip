// Multi-scale SSIM of image pairs in the 8-bit domain (Wang et al. 2003; the pair diversity number of Karras et al. 2018, table 1).
// The definition is stated once, in float64 numpy, in tests/helpers/msssim_model.py.  Per pair of code rows (csrc/neighbours.hip:
// c, y, x order, value u = code + 128), S in {32, 64, 128, 256}, five levels of side S >> l:
//   planes  : level 0 is u as fp32; level l + 1 the 2 x 2 mean ((p00 + p01) + (p10 + p11)) * 0.25 of level l - multiples of 4^-l
//             below 256, at most 16 significant bits: EXACT in fp32.  Their pairwise products have at most 32 bits: exact in float64;
//   rows    : per level the n = min(11, side) taps g of the caller's table, "valid": for every row r and output column x the five
//             sums over j = 0 .. n - 1, in that order, acc = fma(g[j], p, acc) with p = a, b, a a, b b, a b (a, b the two planes'
//             values at (r, x + j); the three products go through ONE inlined function, so the arithmetic is symmetric in a and b);
//   columns : per output (r, x) the same n-tap fma chain down the five row sums: mx, my, exx, eyy, exy; then - no contraction, every
//             operation rounded on its own - sxx = exx - mx mx, syy = eyy - my my, sxy = exy - mx my, v1 = 2 sxy + C2,
//             v2 = (sxx + syy) + C2, cs = v1 / v2, ssim = ((2 mx my + C1) v1) / (((mx mx + my my) + C1) v2);
//   means   : a thread adds the values of its outputs in ascending order, the block adds its threads (wave butterfly, the waves in
//             order), channel after channel; the level's two numbers are the totals / (3 o^2).
// An image against itself gives 1.0 in all ten places, and (a, b) the bits of (b, a).  No atomics; a pair's ten numbers depend on
// its two rows alone.
// Launches.  Planes of side <= 64 run in ONE launch, a block per pair: both planes of a channel in LDS (the levels ping-pong between
// two areas), the row sums in a ring of 16 rows - 11 live ones and the next band's - so that a row is filtered once: 75.5 KB at 64,
// above the default limit of 64 KB, opted in at every launch (cheap, and right on every device).  Sides 256 and 128 go through a
// tiled launch first - a block per 22 x 32 outputs of one channel, its 32 x 44 inputs in LDS - which writes the tile's two sums and
// the 2 x 2 means of the inputs it owns, as fp32, to the workspace; the launch for side 64 then reads those planes instead of codes
// and adds the tiles' sums in tile order.
#include "common.h"
#pragma clang fp contract(off)

#define MS_THREADS 256
#define MS_LEVELS 5
#define MS_TAPS 11
#define MS_RING 16          // rows of row sums held at a time: MS_TAPS - 1 live ones and a band of MS_RING - n + 1 new ones
#define MS_TILE_R 22        // the tiled launch: outputs per tile
#define MS_TILE_C 32
#define MS_TILE_IN_R 32     // MS_TILE_R + MS_TAPS - 1
#define MS_TILE_IN_C 44     // MS_TILE_C + MS_TAPS - 1 rounded up to four
#define MS_C1 ((0.01 * 255.0) * (0.01 * 255.0))          // folded by the compiler: the words the float64 model has
#define MS_C2 ((0.03 * 255.0) * (0.03 * 255.0))

__device__ __forceinline__ double ms_acc(double g, double p, double q, double acc) { return fma(g, p * q, acc); }          // p q is exact

// row sums of rows [ra, rb) at output columns [0, w): A, B rows of ld floats; H[(r % ring) * 5 + m][x], rows of hw doubles
__device__ __forceinline__ void ms_rows(const float* A, const float* B, int ld, int ra, int rb, int w, int n, const double* g, double* H, int hw,
                                        int ring, int tid) {
    for (int item = tid; item < (rb - ra) * w; item += MS_THREADS) {
        const int r = ra + item / w, x = item % w;
        const float* pa = A + r * ld + x;
        const float* pb = B + r * ld + x;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
        for (int j = 0; j < n; ++j) {
            const double a = (double)pa[j], b = (double)pb[j], t = g[j];
            mx = fma(t, a, mx);
            my = fma(t, b, my);
            xx = ms_acc(t, a, a, xx);
            yy = ms_acc(t, b, b, yy);
            xy = ms_acc(t, a, b, xy);
        }
        double* h = H + (size_t)((r % ring) * 5) * hw + x;
        h[0] = mx; h[hw] = my; h[2 * hw] = xx; h[3 * hw] = yy; h[4 * hw] = xy;
    }
}

// the outputs of rows [ra, rb), columns [0, w), from the row sums; a thread's ssim and cs values added to s and c in ascending order
__device__ __forceinline__ void ms_cols(const double* H, int hw, int ring, int ra, int rb, int w, int n, const double* g, int tid, double& s, double& c) {
    for (int item = tid; item < (rb - ra) * w; item += MS_THREADS) {
        const int r = ra + item / w, x = item % w;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < n; ++j) {
            const double* h = H + (size_t)(((r + j) % ring) * 5) * hw + x;
            const double t = g[j];
#pragma unroll
            for (int k = 0; k < 5; ++k) m[k] = fma(t, h[k * hw], m[k]);
        }
        const double mx = m[0], my = m[1];
        const double sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
        const double v1 = 2.0 * sxy + MS_C2, v2 = (sxx + syy) + MS_C2;
        c += v1 / v2;
        s += ((2.0 * mx * my + MS_C1) * v1) / (((mx * mx + my * my) + MS_C1) * v2);
    }
}

__device__ __forceinline__ void ms_load4(const int8_t* p, float* o) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)((int)(int8_t)((w >> (8 * e)) & 0xff) + 128);
}
__device__ __forceinline__ void ms_load4(const float* p, float* o) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

__device__ __forceinline__ bool ms_flagged(const int32_t* aflags, const int32_t* bflags, int pair) {
    return (aflags && aflags[pair] != 0) || (bflags && bflags[pair] != 0);
}

// ---- planes of side S0 <= 64: a block per pair, levels first .. 4 -----------------------------------------------------------------------
// FROM_PLANES: the top planes are fp32 [pair][2][3][S0][S0] (the tiled launch's means), else code rows.  `first`: the level the top
// plane is (0, or 1 / 2 behind the tiled launches, whose tile sums are parts [pair][first][3][tiles[l]][2]).
template <int S0, bool FROM_PLANES>
__global__ __launch_bounds__(MS_THREADS) void msssim_small_kernel(const int8_t* __restrict__ a, const int32_t* __restrict__ aflags, const int8_t* __restrict__ b,
                                                                  const int32_t* __restrict__ bflags, int row_bytes, const float* __restrict__ planes,
                                                                  const double* __restrict__ parts0, const double* __restrict__ parts1, int tiles0, int tiles1,
                                                                  int first, const double* __restrict__ taps, double* __restrict__ out) {
    constexpr int HW = S0 - MS_TAPS + 1;          // the widest row of row sums
    extern __shared__ double ms_smem[];          // H | taps | totals | scratch | level areas
    double* H = ms_smem;
    double* G = H + MS_RING * 5 * HW;
    double* total = G + MS_LEVELS * MS_TAPS + 1;          // [5][2], kept by thread 0
    double* scratch = total + 2 * MS_LEVELS;          // 16
    float* area0 = reinterpret_cast<float*>(scratch + 16);          // a | b of side S0, later of side S0 / 4, S0 / 16
    float* area1 = area0 + 2 * S0 * S0;          // a | b of side S0 / 2, S0 / 8
    const int tid = threadIdx.x, pair = blockIdx.x;
    double* res = out + (size_t)pair * 2 * MS_LEVELS;
    if (ms_flagged(aflags, bflags, pair)) {          // block-uniform
        if (tid < 2 * MS_LEVELS) res[tid] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    if (tid < MS_LEVELS * MS_TAPS) G[tid] = taps[tid];
    if (tid < 2 * MS_LEVELS) total[tid] = 0.0;
    // the levels of the tiled launches: the tiles' sums, channel by channel, a thread's in ascending tile order
    for (int l = 0; l < first; ++l) {
        const double* parts = (l == 0 ? parts0 : parts1) + (size_t)pair * 3 * (l == 0 ? tiles0 : tiles1) * 2;
        const int count = 3 * (l == 0 ? tiles0 : tiles1);
        double s = 0.0, c = 0.0;
        for (int i = tid; i < count; i += MS_THREADS) { s += parts[2 * i]; c += parts[2 * i + 1]; }
        s = block_sum<double>(s, scratch);
        c = block_sum<double>(c, scratch);
        if (tid == 0) { total[2 * l] = s; total[2 * l + 1] = c; }
    }
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();          // the areas are free
        for (int v = tid; v < 2 * S0 * S0 / 4; v += MS_THREADS) {
            const int side = v / (S0 * S0 / 4), at = 4 * (v % (S0 * S0 / 4));
            float o[4];
            if (FROM_PLANES) ms_load4(planes + ((size_t)(pair * 2 + side) * 3 + ch) * S0 * S0 + at, o);
            else ms_load4((side ? b : a) + (size_t)pair * row_bytes + ch * S0 * S0 + at, o);
            *reinterpret_cast<float4*>(area0 + side * S0 * S0 + at) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
        float* cur = area0;
        float* nxt = area1;
        int side = S0;
        for (int l = first; l < MS_LEVELS; ++l) {
            const int n = side < MS_TAPS ? side : MS_TAPS, o = side - n + 1, band = MS_RING - n + 1;
            const double* g = G + l * MS_TAPS;
            const float* A = cur;
            const float* B = cur + side * side;
            double s = 0.0, c = 0.0;
            int filtered = 0;
            for (int r0 = 0; r0 < o; r0 += band) {
                const int r1 = r0 + band < o ? r0 + band : o;
                ms_rows(A, B, side, filtered, r1 + n - 1, o, n, g, H, HW, MS_RING, tid);
                filtered = r1 + n - 1;
                __syncthreads();
                ms_cols(H, HW, MS_RING, r0, r1, o, n, g, tid, s, c);
                __syncthreads();
            }
            if (l + 1 < MS_LEVELS) {          // the next level's planes: exact in fp32
                const int half = side / 2;
                for (int i = tid; i < 2 * half * half; i += MS_THREADS) {
                    const int which = i / (half * half), y = (i % (half * half)) / half, x = i % half;
                    const float* p = cur + which * side * side + 2 * y * side + 2 * x;
                    nxt[which * half * half + y * half + x] = ((p[0] + p[1]) + (p[side] + p[side + 1])) * 0.25f;
                }
            }
            s = block_sum<double>(s, scratch);          // its barriers also order the means above against the next level's reads
            c = block_sum<double>(c, scratch);
            if (tid == 0) { total[2 * l] += s; total[2 * l + 1] += c; }
            float* t = cur; cur = nxt; nxt = t;
            side /= 2;
        }
    }
    __syncthreads();
    if (tid < 2 * MS_LEVELS) {
        const int l = tid >> 1, side = (S0 << first) >> l;
        const int n = side < MS_TAPS ? side : MS_TAPS, o = side - n + 1;
        res[(tid & 1) * MS_LEVELS + l] = total[tid] / (double)(3 * o * o);
    }
}

// ---- a plane of side s = 256 or 128: a block per tile (blockIdx.x), channel (.y) and pair (.z) ---------------------------------------------
// src: code rows (SrcT = int8_t; a and b) or fp32 planes [pair][2][3][s][s] (a; b unused).  Writes parts[pair][ch][tile][2] and the
// 2 x 2 means of the inputs the tile owns to next[pair][2][3][s / 2][s / 2].
template <typename SrcT>
__global__ __launch_bounds__(MS_THREADS) void msssim_tile_kernel(const SrcT* __restrict__ a, const int32_t* __restrict__ aflags, const SrcT* __restrict__ b,
                                                                 const int32_t* __restrict__ bflags, int row_bytes, int s, int level,
                                                                 const double* __restrict__ taps, double* __restrict__ parts, float* __restrict__ next) {
    __shared__ double H[MS_TILE_IN_R * 5 * MS_TILE_C];
    __shared__ __attribute__((aligned(16))) float tile[2][MS_TILE_IN_R * MS_TILE_IN_C];
    __shared__ double G[MS_TAPS];
    __shared__ double scratch[16];
    const int tid = threadIdx.x, ch = blockIdx.y, pair = blockIdx.z;
    if (ms_flagged(aflags, bflags, pair)) return;          // block-uniform; the last launch writes the NaNs
    const int o = s - MS_TAPS + 1;
    const int bands = (o + MS_TILE_R - 1) / MS_TILE_R, strips = (o + MS_TILE_C - 1) / MS_TILE_C;
    const int band = blockIdx.x / strips, strip = blockIdx.x % strips;
    const int r0 = band * MS_TILE_R, c0 = strip * MS_TILE_C;
    const int in_r = min(MS_TILE_IN_R, s - r0), in_c = min(MS_TILE_IN_C, s - c0);          // in_c: a multiple of four
    const int out_r = min(MS_TILE_R, o - r0), out_c = min(MS_TILE_C, o - c0);
    if (tid < MS_TAPS) G[tid] = taps[level * MS_TAPS + tid];
    const int groups = in_c / 4;
    for (int v = tid; v < 2 * in_r * groups; v += MS_THREADS) {
        const int side = v / (in_r * groups), r = (v % (in_r * groups)) / groups, x = 4 * (v % groups);
        const size_t at = (size_t)ch * s * s + (size_t)(r0 + r) * s + c0 + x;
        float w[4];
        if constexpr (sizeof(SrcT) == 1) ms_load4((side ? b : a) + (size_t)pair * row_bytes + at, w);
        else ms_load4(a + (size_t)(pair * 2 + side) * 3 * s * s + at, w);
        *reinterpret_cast<float4*>(&tile[side][r * MS_TILE_IN_C + x]) = make_float4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    ms_rows(tile[0], tile[1], MS_TILE_IN_C, 0, out_r + MS_TAPS - 1, out_c, MS_TAPS, G, H, MS_TILE_C, MS_TILE_IN_R, tid);
    // the inputs this tile owns: rows [r0, r0 + 22) and columns [c0, c0 + 32), the last band and strip through to the edge
    const int own_r = (band == bands - 1 ? s - r0 : MS_TILE_R) / 2, own_c = (strip == strips - 1 ? s - c0 : MS_TILE_C) / 2, half = s / 2;
    for (int i = tid; i < 2 * own_r * own_c; i += MS_THREADS) {
        const int side = i / (own_r * own_c), y = (i % (own_r * own_c)) / own_c, x = i % own_c;
        const float* p = &tile[side][2 * y * MS_TILE_IN_C + 2 * x];
        next[((size_t)(pair * 2 + side) * 3 + ch) * half * half + (size_t)(r0 / 2 + y) * half + c0 / 2 + x] =
            ((p[0] + p[1]) + (p[MS_TILE_IN_C] + p[MS_TILE_IN_C + 1])) * 0.25f;
    }
    __syncthreads();
    double sum = 0.0, csum = 0.0;
    ms_cols(H, MS_TILE_C, MS_TILE_IN_R, 0, out_r, out_c, MS_TAPS, G, tid, sum, csum);
    sum = block_sum<double>(sum, scratch);
    csum = block_sum<double>(csum, scratch);
    if (tid == 0) {
        double* p = parts + (((size_t)pair * 3 + ch) * (bands * strips) + blockIdx.x) * 2;
        p[0] = sum;
        p[1] = csum;
    }
}

static bool ms_size_ok(int S) { return S == 32 || S == 64 || S == 128 || S == 256; }
static int ms_tiles(int s) {
    const int o = s - MS_TAPS + 1;
    return ((o + MS_TILE_R - 1) / MS_TILE_R) * ((o + MS_TILE_C - 1) / MS_TILE_C);
}
static size_t ms_planes_bytes(int pairs, int s) { return (size_t)pairs * 6 * s * s * sizeof(float); }
static size_t ms_parts_bytes(int pairs, int s) { return (size_t)pairs * 3 * ms_tiles(s) * 2 * sizeof(double); }

// S <= 64: nothing.  128: the planes of side 64, the tile sums of level 0.  256: the planes of side 128 and 64, the tile sums of levels 0, 1.
LOCATE_API size_t locate_msssim_workspace_bytes(int pairs, int S) {
    if (pairs < 1 || !ms_size_ok(S) || S <= 64) return 0;
    size_t bytes = ms_planes_bytes(pairs, 64) + ms_parts_bytes(pairs, 128);
    if (S == 256) bytes += ms_planes_bytes(pairs, 128) + ms_parts_bytes(pairs, 256);
    return bytes;
}

template <int S0, bool FROM_PLANES>
static void ms_launch_small(const int8_t* a, const int32_t* aflags, const int8_t* b, const int32_t* bflags, int pairs, int row_bytes, const float* planes,
                            const double* parts0, const double* parts1, int tiles0, int tiles1, int first, const double* taps, double* out, hipStream_t st) {
    constexpr size_t lds = (size_t)(MS_RING * 5 * (S0 - MS_TAPS + 1) + MS_LEVELS * MS_TAPS + 1 + 2 * MS_LEVELS + 16) * sizeof(double) +
                           (size_t)(2 * S0 * S0 + 2 * (S0 / 2) * (S0 / 2)) * sizeof(float);          // 25 KB at 32, 75.5 KB at 64
    auto k = msssim_small_kernel<S0, FROM_PLANES>;
    // above 64 KB a kernel has to opt in, per device: asked for at every launch, which costs nothing beside the launch
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    k<<<pairs, MS_THREADS, lds, st>>>(a, aflags, b, bflags, row_bytes, planes, parts0, parts1, tiles0, tiles1, first, taps, out);
}

LOCATE_API int locate_msssim_pairs(const int8_t* a, const int32_t* aflags, const int8_t* b, const int32_t* bflags, int pairs, int row_bytes, int S,
                                   const double* taps, double* out, void* workspace, void* stream) {
    LOCATE_REQUIRE(a && b && taps && out, "locate_msssim_pairs: null pointer");
    LOCATE_REQUIRE(ms_size_ok(S), "locate_msssim_pairs: S = %d (32, 64, 128 or 256)", S);
    LOCATE_REQUIRE(row_bytes >= 3 * S * S && row_bytes % 16 == 0 && row_bytes <= (1 << 20), "locate_msssim_pairs: row_bytes = %d for S = %d", row_bytes, S);
    LOCATE_REQUIRE(pairs >= 1 && (int64_t)pairs * row_bytes < ((int64_t)1 << 40), "locate_msssim_pairs: %d pairs", pairs);
    LOCATE_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0 && (((uintptr_t)taps | (uintptr_t)out) & 7) == 0 &&
                   (((uintptr_t)aflags | (uintptr_t)bflags) & 3) == 0,
                   "locate_msssim_pairs: the code rows must be 16-byte, taps and out 8-byte, the flags 4-byte aligned");
    hipStream_t st = as_stream(stream);
    if (S == 32) {
        ms_launch_small<32, false>(a, aflags, b, bflags, pairs, row_bytes, nullptr, nullptr, nullptr, 0, 0, 0, taps, out, st);
    } else if (S == 64) {
        ms_launch_small<64, false>(a, aflags, b, bflags, pairs, row_bytes, nullptr, nullptr, nullptr, 0, 0, 0, taps, out, st);
    } else {
        LOCATE_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "locate_msssim_pairs: S = %d needs a 16-byte aligned workspace", S);
        LOCATE_REQUIRE(pairs <= 65535, "locate_msssim_pairs: at most 65535 pairs of S = %d a call, got %d", S, pairs);
        char* ws = static_cast<char*>(workspace);
        float* planes64 = reinterpret_cast<float*>(ws);
        ws += ms_planes_bytes(pairs, 64);
        double* parts128 = reinterpret_cast<double*>(ws);
        ws += ms_parts_bytes(pairs, 128);
        if (S == 128) {
            msssim_tile_kernel<int8_t><<<dim3(ms_tiles(128), 3, pairs), MS_THREADS, 0, st>>>(a, aflags, b, bflags, row_bytes, 128, 0, taps, parts128, planes64);
            LOCATE_LAUNCH_CHECK("locate_msssim_pairs (tiles of 128)");
            ms_launch_small<64, true>(a, aflags, b, bflags, pairs, row_bytes, planes64, parts128, nullptr, ms_tiles(128), 0, 1, taps, out, st);
        } else {
            float* planes128 = reinterpret_cast<float*>(ws);
            ws += ms_planes_bytes(pairs, 128);
            double* parts256 = reinterpret_cast<double*>(ws);
            msssim_tile_kernel<int8_t><<<dim3(ms_tiles(256), 3, pairs), MS_THREADS, 0, st>>>(a, aflags, b, bflags, row_bytes, 256, 0, taps, parts256, planes128);
            LOCATE_LAUNCH_CHECK("locate_msssim_pairs (tiles of 256)");
            msssim_tile_kernel<float><<<dim3(ms_tiles(128), 3, pairs), MS_THREADS, 0, st>>>(planes128, aflags, nullptr, bflags, 0, 128, 1, taps, parts128, planes64);
            LOCATE_LAUNCH_CHECK("locate_msssim_pairs (tiles of 128)");
            ms_launch_small<64, true>(a, aflags, b, bflags, pairs, row_bytes, planes64, parts256, parts128, ms_tiles(256), ms_tiles(128), 2, taps, out, st);
        }
    }
    LOCATE_LAUNCH_CHECK("locate_msssim_pairs");
    return LOCATE_OK;
}
