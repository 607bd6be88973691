// Device-side input pipeline: the reference's two torchvision / PIL transform chains (libs/utils.py:88-113) on a uint8 image store
// that is resident in device memory, in Pillow's own arithmetic (bit for bit):
//   flip -> colour jitter (brightness / contrast / saturation in a per-sample order) -> square crop -> antialiased bilinear resize
//   to S x S (22-bit fixed-point taps, horizontal pass, uint8, vertical pass) -> (u8 / 255 - 0.5) / 0.5 as fp32 NCHW.
// Two launches per batch pair: the contrast pass (integer sum of L over each jittered sample's WHOLE source image - Pillow's
// contrast degenerate is the image mean before the crop) and the transform pass (one block = one sample x a band of output rows).
// Everything a kernel computes is integer or pinned fp32 arithmetic; the resize taps and the 256 output values come from the host.
//
// Source pixels are 3 bytes, so no row and no image starts on a 16-byte boundary in general.  The STORE does, and 48 bytes = three
// 16-byte words = 16 whole pixels: the kernels read the store in such groups (three aligned 16-byte loads, pixels unpacked from
// registers) and mask the pixels of a group that lie outside the span they want.
#include "common.h"

struct InputParam {          // one record per output sample (locate_input_param_record_bytes() = 32)
    int32_t flip;            // != 0: columns reversed before everything else
    int32_t order;           // four 4-bit op codes, first op in the low bits: 0 brightness, 1 contrast, 2 saturation, others: nothing
    float f[3];              // brightness, contrast, saturation factors
    int32_t top, left, side; // square crop of the (flipped) image
};
static_assert(sizeof(InputParam) == 32, "InputParam is part of the C ABI");

#define IN_THREADS 256
#define IN_BAND 8                       // output rows per block of the transform pass (halved until the rows fit IN_LDS_BYTES)
#define IN_LDS_BYTES (64 * 1024)
#define IN_MAX_TAPS 32
#define IN_MEAN_BLOCKS_MAX 16
#define IN_FIX 22                       // Pillow's PRECISION_BITS for 8-bit channels

// Image.blend(degenerate, image, f) on one channel: fp32, a multiply and an add that stay two roundings, clip, truncate.
// common.h's __fmul_rn / __fadd_rn spelling is not enough here: the two calls inline to a multiply feeding an add, which the
// compiler's default contraction turns into one v_fma_f32 (one rounding - a level off from Pillow on some pixels).  The pragma
// takes the contraction permission off exactly these operations; it travels with them wherever the function is inlined.
__device__ __forceinline__ int blend8(int d, int p, float f) {
#pragma clang fp contract(off)
    const float fd = (float)d;
    const float diff = (float)p - fd;                  // exact: integers below 2^24
    const float prod = f * diff;
    float t = fd + prod;
    t = fminf(fmaxf(t, 0.0f), 255.0f);
    return (int)t;
}
__device__ __forceinline__ int luma8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ bool order_has_contrast(int order) {
    bool has = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) has = has || ((order >> (4 * k)) & 15) == 1;
    return has;
}

// the jitter chain on one pixel; UNTIL_CONTRAST: only the ops in front of the contrast op (what its mean is taken over)
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_pixel(int& r, int& g, int& b, const InputParam& P, int mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = (P.order >> (4 * k)) & 15;          // block-uniform
        if (op == 0) {
            r = blend8(0, r, P.f[0]); g = blend8(0, g, P.f[0]); b = blend8(0, b, P.f[0]);
        } else if (op == 1) {
            if (UNTIL_CONTRAST) return;
            r = blend8(mean, r, P.f[1]); g = blend8(mean, g, P.f[1]); b = blend8(mean, b, P.f[1]);
        } else if (op == 2) {
            const int l = luma8(r, g, b);
            r = blend8(l, r, P.f[2]); g = blend8(l, g, P.f[2]); b = blend8(l, b, P.f[2]);
        }
    }
}

// 16-byte word `wi` of the store; only the store's last, partial word (at most one in the whole store) is assembled from bytes
__device__ __forceinline__ uint4 load_store_word(const uint8_t* __restrict__ store, int64_t wi, int64_t total_bytes) {
    const int64_t at = wi * 16;
    if (at + 16 <= total_bytes) return reinterpret_cast<const uint4*>(store)[wi];
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (at + i < total_bytes) w[i >> 2] |= (unsigned)store[at + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// pixels 16 g ... 16 g + 15 of the store (counted over all images) as 12 words
__device__ __forceinline__ void load_group(const uint8_t* __restrict__ store, int64_t g, int64_t total_bytes, unsigned (&w)[12]) {
    const uint4 a = load_store_word(store, 3 * g, total_bytes), b = load_store_word(store, 3 * g + 1, total_bytes),
                c = load_store_word(store, 3 * g + 2, total_bytes);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
}
#define GROUP_BYTE(w, i) ((int)(((w)[(i) >> 2] >> (8 * ((i) & 3))) & 255u))

// ---- contrast pass: partials[sample][block] = sum of L over this block's share of the sample's source image, after the ops
//      that precede contrast in the sample's order (the flip does not change a sum).  Integer: exact in any order. ----
__global__ __launch_bounds__(IN_THREADS) void input_contrast_sum_kernel(const uint8_t* __restrict__ store, int N, int H, int W, int64_t total_bytes,
                                                                       const int32_t* __restrict__ idx, const InputParam* __restrict__ params,
                                                                       int* __restrict__ partials) {
    __shared__ int scratch[16];
    const int sample = blockIdx.y, nblk = gridDim.x;
    const InputParam P = params[sample];
    const int id = idx[sample];
    int sum = 0;
    if (order_has_contrast(P.order) && id >= 0 && id < N) {              // block-uniform
        const int64_t hw = (int64_t)H * W, p0 = id * hw, p1 = p0 + hw, g1 = (p1 + 15) >> 4;
        for (int64_t g = (p0 >> 4) + (int64_t)blockIdx.x * IN_THREADS + threadIdx.x; g < g1; g += (int64_t)nblk * IN_THREADS) {
            unsigned w[12];
            load_group(store, g, total_bytes, w);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t p = g * 16 + j;
                int r = GROUP_BYTE(w, 3 * j), gg = GROUP_BYTE(w, 3 * j + 1), b = GROUP_BYTE(w, 3 * j + 2);
                jitter_pixel<true>(r, gg, b, P, 0);
                sum += (p >= p0 && p < p1) ? luma8(r, gg, b) : 0;
            }
        }
    }
    sum = block_sum<int>(sum, scratch);
    if (threadIdx.x == 0) partials[sample * nblk + blockIdx.x] = sum;
}

// ---- transform pass.  Dynamic LDS: lut[256] | taps of this sample's crop side [S][2 + ktaps] | src rows [max_rows][pitch] |
//      horizontally resized rows [max_rows][S]; a pixel is one word (r | g << 8 | b << 16). ----
struct TapRange { int first, count; };
__device__ __forceinline__ TapRange tap_range(const int* __restrict__ taps, int i, int stride, int ktaps, int side) {
    TapRange t;                                                         // clamped: a bad table may give wrong pixels, never a wild address
    t.first = min(max(taps[i * stride], 0), side - 1);
    t.count = min(max(taps[i * stride + 1], 1), min(ktaps, side - t.first));
    return t;
}
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(IN_THREADS) void input_transform_kernel(const uint8_t* __restrict__ store, int N, int H, int W, int64_t total_bytes,
                                                                    const int32_t* __restrict__ idx, const InputParam* __restrict__ params, int n_first,
                                                                    const int32_t* __restrict__ coef, int side_lo, int side_hi, int ktaps,
                                                                    const float* __restrict__ lut, const int* __restrict__ partials, int nblk,
                                                                    int S, int band, int max_rows, float* __restrict__ out_first,
                                                                    float* __restrict__ out_rest) {
    extern __shared__ uint4 smem4[];
    const int tid = threadIdx.x, sample = blockIdx.y, stride = 2 + ktaps, pitch = side_hi;
    float* lutS = reinterpret_cast<float*>(smem4);
    int* tapS = reinterpret_cast<int*>(lutS + 256);
    unsigned* srcS = reinterpret_cast<unsigned*>(tapS + ((S * stride + 3) & ~3));
    unsigned* horS = srcS + (((int64_t)max_rows * pitch + 3) & ~3);

    const InputParam P = params[sample];
    const int id = idx[sample], side = P.side;
    // the caller validates the records (a device table cannot be checked on the host side of this library); a record that is out
    // of range all the same leaves its output untouched instead of reading outside the store
    if (id < 0 || id >= N || side < side_lo || side > side_hi || P.top < 0 || P.left < 0 || P.top + side > H || P.left + side > W) return;

    for (int i = tid; i < 256; i += IN_THREADS) lutS[i] = lut[i];
    const int32_t* my_taps = coef + (int64_t)(side - side_lo) * S * stride;
    for (int i = tid; i < S * stride; i += IN_THREADS) tapS[i] = my_taps[i];
    int mean = 0;
    if (order_has_contrast(P.order)) {
        unsigned long long sum = 0;
        for (int j = 0; j < nblk; ++j) sum += (unsigned)partials[sample * nblk + j];
        const unsigned long long n = (unsigned long long)H * W;
        mean = (int)((2 * sum + n) / (2 * n));                        // ImageStat mean of L, rounded half up
    }
    __syncthreads();

    const int y0 = blockIdx.x * band, y1 = min(y0 + band, S);
    const TapRange ta = tap_range(tapS, y0, stride, ktaps, side), tb = tap_range(tapS, y1 - 1, stride, ktaps, side);
    const int row_a = ta.first, nrows = min(max(tb.first + tb.count - row_a, 1), max_rows);

    // 1. the band's source rows, crop columns only, jittered and flipped on the way in
    {
        const int c0 = P.flip ? W - P.left - side : P.left;              // first source column of the crop
        const int ng = ((side + 15) >> 4) + 1;                            // groups that can touch `side` pixels at any alignment
        for (int it = tid; it < nrows * ng; it += IN_THREADS) {
            const int r = it / ng, gi = it - r * ng;
            const int64_t p0 = ((int64_t)id * H + P.top + row_a + r) * W + c0, p1 = p0 + side, g = (p0 >> 4) + gi;
            if (g * 16 >= p1) continue;
            unsigned w[12];
            load_group(store, g, total_bytes, w);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t p = g * 16 + j;
                if (p < p0 || p >= p1) continue;
                int rr = GROUP_BYTE(w, 3 * j), gg = GROUP_BYTE(w, 3 * j + 1), bb = GROUP_BYTE(w, 3 * j + 2);
                jitter_pixel<false>(rr, gg, bb, P, mean);
                const int x = (int)(p - p0);
                srcS[r * pitch + (P.flip ? side - 1 - x : x)] = (unsigned)rr | (unsigned)gg << 8 | (unsigned)bb << 16;
            }
        }
    }
    __syncthreads();

    // 2. horizontal pass: every staged row to S pixels, quantised to uint8
    for (int it = tid; it < nrows * S; it += IN_THREADS) {
        const int r = it / S, x = it - r * S;
        const TapRange t = tap_range(tapS, x, stride, ktaps, side);
        const int* k = tapS + x * stride + 2;
        const unsigned* row = srcS + r * pitch + t.first;
        int a0 = 1 << (IN_FIX - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < t.count; ++j) {
            const unsigned px = row[j];
            const int kj = k[j];
            a0 += kj * (int)(px & 255u); a1 += kj * (int)((px >> 8) & 255u); a2 += kj * (int)((px >> 16) & 255u);
        }
        horS[r * S + x] = (unsigned)clip8(a0 >> IN_FIX) | (unsigned)clip8(a1 >> IN_FIX) << 8 | (unsigned)clip8(a2 >> IN_FIX) << 16;
    }
    __syncthreads();

    // 3. vertical pass, four pixels per thread, three 16-byte stores (one per channel plane)
    const int S4 = S >> 2;
    float* out = sample < n_first ? out_first + (int64_t)sample * 3 * S * S : out_rest + (int64_t)(sample - n_first) * 3 * S * S;
    for (int it = tid; it < (y1 - y0) * S4; it += IN_THREADS) {
        const int yy = it / S4, x4 = it - yy * S4, y = y0 + yy;
        TapRange t = tap_range(tapS, y, stride, ktaps, side);
        const int* k = tapS + y * stride + 2;
        const int r0 = min(max(t.first - row_a, 0), nrows - 1);
        t.count = min(t.count, nrows - r0);
        int acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 1 << (IN_FIX - 1);
        for (int j = 0; j < t.count; ++j) {
            const uint4 q = *reinterpret_cast<const uint4*>(horS + (r0 + j) * S + 4 * x4);
            const unsigned px[4] = {q.x, q.y, q.z, q.w};
            const int kj = k[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i] += kj * (int)(px[i] & 255u);
                acc[4 + i] += kj * (int)((px[i] >> 8) & 255u);
                acc[8 + i] += kj * (int)((px[i] >> 16) & 255u);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 v;
            v.x = lutS[clip8(acc[4 * c] >> IN_FIX)]; v.y = lutS[clip8(acc[4 * c + 1] >> IN_FIX)];
            v.z = lutS[clip8(acc[4 * c + 2] >> IN_FIX)]; v.w = lutS[clip8(acc[4 * c + 3] >> IN_FIX)];
            *reinterpret_cast<float4*>(out + ((int64_t)c * S + y) * S + 4 * x4) = v;
        }
    }
}

static int mean_blocks(int H, int W) {
    const int64_t groups = cdiv64((int64_t)H * W, 16) + 1;
    int64_t b = cdiv64(groups, IN_THREADS);
    return (int)(b < 1 ? 1 : b > IN_MEAN_BLOCKS_MAX ? IN_MEAN_BLOCKS_MAX : b);
}
// source rows a band of `band` output rows can need: taps of output y span [c - fs + 0.5 - 1, c + fs + 0.5), c = (y + 0.5) scale
static int band_max_rows(int band, int side_hi, int S) {
    const double scale = (double)side_hi / S, fs = scale > 1.0 ? scale : 1.0;
    const int rows = (int)((band - 1) * scale + 2.0 * fs + 1.0) + 1;
    return rows < side_hi ? rows : side_hi;
}
static size_t transform_lds_bytes(int band, int side_hi, int S, int ktaps) {
    const size_t rows = (size_t)band_max_rows(band, side_hi, S);
    return 4 * (256 + (((size_t)S * (2 + ktaps) + 3) & ~(size_t)3) + ((rows * side_hi + 3) & ~(size_t)3) + rows * S);
}

LOCATE_API size_t locate_input_param_record_bytes(void) { return sizeof(InputParam); }
LOCATE_API int locate_input_mean_blocks(int H, int W) { return H > 0 && W > 0 ? mean_blocks(H, W) : 0; }
LOCATE_API size_t locate_input_workspace_bytes(int n, int H, int W) {
    return n > 0 && H > 0 && W > 0 ? (size_t)n * mean_blocks(H, W) * sizeof(int) : 0;
}

LOCATE_API int locate_input_transform(const void* store, int N, int H, int W, const int32_t* idx, const void* params, int n, int n_first,
                                      const int32_t* coef, int side_lo, int side_hi, int ktaps, const float* lut, int S,
                                      float* out_first, float* out_rest, void* workspace, void* stream) {
    LOCATE_REQUIRE(store && idx && params && coef && lut && workspace, "locate_input_transform: null pointer");
    LOCATE_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)H * W <= (1 << 23), "locate_input_transform: bad store shape %d x %d x %d", N, H, W);
    LOCATE_REQUIRE(n > 0 && n <= 65535 && n_first >= 0 && n_first <= n, "locate_input_transform: bad sample counts %d / %d", n_first, n);
    LOCATE_REQUIRE((n_first == 0 || out_first) && (n_first == n || out_rest), "locate_input_transform: null output");
    LOCATE_REQUIRE(S >= 4 && (S & 3) == 0 && S <= 4096, "locate_input_transform: S = %d must be a multiple of 4", S);
    LOCATE_REQUIRE(side_lo >= 1 && side_lo <= side_hi && side_hi <= (H < W ? H : W), "locate_input_transform: bad crop sides [%d, %d]", side_lo,
                   side_hi);
    LOCATE_REQUIRE(ktaps >= 1 && ktaps <= IN_MAX_TAPS, "locate_input_transform: bad tap count %d", ktaps);
    LOCATE_REQUIRE(((uintptr_t)store & 15) == 0 && ((uintptr_t)out_first & 15) == 0 && ((uintptr_t)out_rest & 15) == 0,
                   "locate_input_transform: store and outputs must be 16-byte aligned");
    int band = IN_BAND < S ? IN_BAND : S;
    while (band > 1 && transform_lds_bytes(band, side_hi, S, ktaps) > IN_LDS_BYTES) band >>= 1;
    const size_t lds = transform_lds_bytes(band, side_hi, S, ktaps);
    LOCATE_REQUIRE(lds <= IN_LDS_BYTES, "locate_input_transform: a crop side of %d at S = %d does not fit LDS", side_hi, S);
    const int64_t total_bytes = (int64_t)N * H * W * 3;
    const int nblk = mean_blocks(H, W);
    hipStream_t st = as_stream(stream);
    input_contrast_sum_kernel<<<dim3(nblk, n), IN_THREADS, 0, st>>>(static_cast<const uint8_t*>(store), N, H, W, total_bytes, idx,
                                                                   static_cast<const InputParam*>(params), static_cast<int*>(workspace));
    LOCATE_LAUNCH_CHECK("locate_input_transform (contrast sums)");
    input_transform_kernel<<<dim3((unsigned)cdiv64(S, band), n), IN_THREADS, lds, st>>>(
        static_cast<const uint8_t*>(store), N, H, W, total_bytes, idx, static_cast<const InputParam*>(params), n_first, coef, side_lo, side_hi,
        ktaps, lut, static_cast<const int*>(workspace), nblk, S, band, band_max_rows(band, side_hi, S), out_first, out_rest);
    LOCATE_LAUNCH_CHECK("locate_input_transform");
    return LOCATE_OK;
}
