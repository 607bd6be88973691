// Training monitor: the reference's sample picture (main.py:194-225) rendered on the device.  The reference takes a batch of
// generated images to the host, tiles and normalises it with torchvision's make_grid(padding, normalize=True) and hands the
// result to matplotlib's imsave, which turns it into RGBA bytes with (x * 255).astype(uint8).  Here the same bytes come from
//   range pass   : lo = min(x), hi = max(x) over the whole batch - a per-block (lo, hi) pair into the workspace, then one small
//                  block that folds the pairs (min and max do not depend on order: exact, no atomics on values);
//   compose pass : one thread per grid pixel: pad_value outside the images, ((clamp(x, lo, hi) - lo) / d) inside, as the fp32
//                  grid make_grid returns and / or as the RGBA bytes imsave gives the PNG encoder.
// Every operation of the value chain is a single fp32 IEEE operation in the reference's order (subtract, divide, multiply by 255,
// truncate); nothing may be fused or replaced by a reciprocal, so the functions that hold it switch contraction off.
#include "common.h"

#define GRID_THREADS 256
#define GRID_RANGE_BLOCKS_MAX 1024
#define GRID_RANGE_WORDS 3              // per block: lo, hi, 1.0f if the block saw a NaN

__device__ __forceinline__ float block_min(float v, float* scratch) { return -block_max(-v, scratch); }          // negation is exact

__device__ __forceinline__ void range_take(float v, float& lo, float& hi, float& bad) {
    lo = fminf(lo, v);                  // fminf / fmaxf skip a NaN operand: the NaN is carried by `bad` instead
    hi = fmaxf(hi, v);
    bad = v != v ? 1.0f : bad;
}

__global__ __launch_bounds__(GRID_THREADS) void image_range_partial_kernel(const float* __restrict__ x, int64_t n_elems, int vec,
                                                                           float* __restrict__ partials) {
    __shared__ float scratch[16];
    const int64_t tid = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * GRID_THREADS;
    float lo = INFINITY, hi = -INFINITY, bad = 0.0f;
    const int64_t n4 = vec ? n_elems >> 2 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 q = x4[i];
        range_take(q.x, lo, hi, bad); range_take(q.y, lo, hi, bad); range_take(q.z, lo, hi, bad); range_take(q.w, lo, hi, bad);
    }
    for (int64_t i = 4 * n4 + tid; i < n_elems; i += stride) range_take(x[i], lo, hi, bad);
    lo = block_min(lo, scratch);
    hi = block_max(hi, scratch);
    bad = block_max(bad, scratch);
    if (threadIdx.x == 0) {
        float* p = partials + (int64_t)blockIdx.x * GRID_RANGE_WORDS;
        p[0] = lo; p[1] = hi; p[2] = bad;
    }
}

// one block: the pairs of the launch before it (stream order makes them visible) into range = {lo, hi}; a NaN anywhere in x
// makes both NaN, as torch's min() / max() do, so that the caller can see it
__global__ __launch_bounds__(GRID_THREADS) void image_range_final_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ range) {
    __shared__ float scratch[16];
    float lo = INFINITY, hi = -INFINITY, bad = 0.0f;
    for (int b = threadIdx.x; b < nblk; b += GRID_THREADS) {
        const float* p = partials + (int64_t)b * GRID_RANGE_WORDS;
        lo = fminf(lo, p[0]); hi = fmaxf(hi, p[1]); bad = fmaxf(bad, p[2]);
    }
    lo = block_min(lo, scratch);
    hi = block_max(hi, scratch);
    bad = block_max(bad, scratch);
    if (threadIdx.x == 0) {
        range[0] = bad > 0.0f ? NAN : lo;
        range[1] = bad > 0.0f ? NAN : hi;
    }
}

// make_grid's norm_range on one value: clamp to [lo, hi], subtract lo, divide by max(hi - lo, 1e-5) (the divisor `d`)
__device__ __forceinline__ float grid_normalise(float x, float lo, float hi, float d) {
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(x, lo), hi);
    const float s = c - lo;
    return s / d;
}
// imsave's (x * 255).astype(uint8) on one value of the grid.  The values are in [0, 1]; the clamp only gives a non-finite input
// (unspecified bytes, by contract) a defined result.
__device__ __forceinline__ unsigned grid_byte(float v) {
#pragma clang fp contract(off)
    const float t = v * 255.0f;
    return (unsigned)min(max((int)t, 0), 255);
}

__global__ __launch_bounds__(GRID_THREADS) void image_grid_kernel(const float* __restrict__ x, int n, int S, int xmaps, int padding, float pad_value,
                                                                  const float* __restrict__ range, float divisor, int GH, int GW,
                                                                  float* __restrict__ grid_f32, uchar4* __restrict__ grid_u8) {
    const int gx = blockIdx.x * GRID_THREADS + threadIdx.x;
    if (gx >= GW) return;
    const float lo = range[0], hi = range[1];
    // hi - lo as Python takes it (two doubles), floored at 1e-5, rounded ONCE to the fp32 divisor
    const float d = divisor != 0.0f ? divisor : (float)fmax((double)hi - (double)lo, 1e-5);
    const int cell = S + padding, xs = gx - padding;
    const int col = xs >= 0 ? xs / cell : -1, ix = xs - col * cell;
    const bool in_x = xs >= 0 && ix < S && col < xmaps;
    const unsigned pad_byte = grid_byte(pad_value);
    const int64_t plane = (int64_t)S * S, gplane = (int64_t)GH * GW;
    for (int gy = blockIdx.y; gy < GH; gy += gridDim.y) {
        const int ys = gy - padding;
        const int row = ys >= 0 ? ys / cell : -1, iy = ys - row * cell;
        const int k = row * xmaps + col;
        float r = pad_value, g = pad_value, b = pad_value;
        unsigned br = pad_byte, bg = pad_byte, bb = pad_byte;
        if (in_x && ys >= 0 && iy < S && k < n) {
            const float* px = x + (int64_t)k * 3 * plane + (int64_t)iy * S + ix;
            r = grid_normalise(px[0], lo, hi, d); g = grid_normalise(px[plane], lo, hi, d); b = grid_normalise(px[2 * plane], lo, hi, d);
            br = grid_byte(r); bg = grid_byte(g); bb = grid_byte(b);
        }
        const int64_t at = (int64_t)gy * GW + gx;
        if (grid_f32 != nullptr) { grid_f32[at] = r; grid_f32[gplane + at] = g; grid_f32[2 * gplane + at] = b; }
        if (grid_u8 != nullptr) grid_u8[at] = make_uchar4((unsigned char)br, (unsigned char)bg, (unsigned char)bb, 255);
    }
}

static int range_blocks(int64_t n_elems) {
    const int64_t b = cdiv64(n_elems, (int64_t)GRID_THREADS * 16);          // ~16 elements (four 16-byte loads) per thread
    return (int)(b < 1 ? 1 : b > GRID_RANGE_BLOCKS_MAX ? GRID_RANGE_BLOCKS_MAX : b);
}

LOCATE_API size_t locate_image_range_workspace_bytes(void) { return (size_t)GRID_RANGE_BLOCKS_MAX * GRID_RANGE_WORDS * sizeof(float); }

LOCATE_API int locate_image_range(const float* x, int64_t n_elems, float* range, void* workspace, void* stream) {
    LOCATE_REQUIRE(x && range && workspace, "locate_image_range: null pointer");
    LOCATE_REQUIRE(n_elems > 0, "locate_image_range: empty input");
    LOCATE_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)range & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                   "locate_image_range: pointers must be 4-byte aligned");
    const int nblk = range_blocks(n_elems);
    hipStream_t st = as_stream(stream);
    image_range_partial_kernel<<<nblk, GRID_THREADS, 0, st>>>(x, n_elems, ((uintptr_t)x & 15) == 0, static_cast<float*>(workspace));
    LOCATE_LAUNCH_CHECK("locate_image_range (block pairs)");
    image_range_final_kernel<<<1, GRID_THREADS, 0, st>>>(static_cast<const float*>(workspace), nblk, range);
    LOCATE_LAUNCH_CHECK("locate_image_range");
    return LOCATE_OK;
}

LOCATE_API int locate_image_grid(const float* x, int n, int S, int nrow, int padding, float pad_value, const float* range, float divisor,
                                 float* grid_f32, uint8_t* grid_u8, void* stream) {
    LOCATE_REQUIRE(x && range, "locate_image_grid: null pointer");
    LOCATE_REQUIRE(grid_f32 || grid_u8, "locate_image_grid: no output");
    LOCATE_REQUIRE(n >= 1 && n <= 65535 && S >= 1 && S <= 4096 && nrow >= 1 && padding >= 0 && padding <= 4096,
                   "locate_image_grid: bad geometry n = %d, S = %d, nrow = %d, padding = %d", n, S, nrow, padding);
    LOCATE_REQUIRE(divisor >= 0.0f, "locate_image_grid: the divisor is positive, or 0 to have it computed from the range");
    const int xmaps = nrow < n ? nrow : n, ymaps = (n + xmaps - 1) / xmaps;
    const int64_t GH = (int64_t)(S + padding) * ymaps + padding, GW = (int64_t)(S + padding) * xmaps + padding;
    LOCATE_REQUIRE(GH * GW <= ((int64_t)1 << 28) && (int64_t)n * 3 * S * S < ((int64_t)1 << 31), "locate_image_grid: a grid of %lld x %lld is too large",
                   (long long)GH, (long long)GW);
    LOCATE_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)range & 3) == 0 && ((uintptr_t)grid_f32 & 3) == 0 && ((uintptr_t)grid_u8 & 3) == 0,
                   "locate_image_grid: pointers must be 4-byte aligned");
    const dim3 grid((unsigned)cdiv64(GW, GRID_THREADS), (unsigned)(GH < 65535 ? GH : 65535));
    image_grid_kernel<<<grid, GRID_THREADS, 0, as_stream(stream)>>>(x, n, S, xmaps, padding, pad_value, range, divisor, (int)GH, (int)GW, grid_f32,
                                                                    reinterpret_cast<uchar4*>(grid_u8));
    LOCATE_LAUNCH_CHECK("locate_image_grid");
    return LOCATE_OK;
}
