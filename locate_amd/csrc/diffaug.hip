// Differentiable augmentation (Zhao et al. 2020) of an image batch and its adjoint (locate_amd/augment.py; the definition in float64
// numpy: tests/helpers/diffaug_model.py).  Every image the discriminator sees passes through one random transform T - colour, then
// translation, then cutout - whose parameters arrive as a row of DA_PARAMS fp32 words per image, drawn on the host:
//   word 0 b, 1 s, 2 c (brightness offset, saturation and contrast factors), 3 ty, 4 tx (shift), 5 y0, 6 y1, 7 x0, 8 x1 (cut
//   rectangle [y0, y1) x [x0, x1)); the integers are small exact integers stored as fp32; word 9 is the per-image op mask (below; 0: every op of the policy runs); words 10 and 11 are zero.
// Forward, per image x [3, S, S] with mu[p] = mean_c x[c, p] and M = mean(x):
//   z[c, p] = c (s (x[c, p] - mu[p]) + mu[p] - M) + M + b,   w[c, i, j] = z[c, i - ty, j - tx] inside the frame and exactly 0.0
//   elsewhere (a gather, nothing is multiplied),   y = keep * w with keep = 0.0f inside the rectangle and 1.0f outside (an fp32
//   multiplication: a NaN or Inf under the cut stays non-finite).
// Backward: gz[c, p] = keep[p + t] * gy[c, p + t] inside the frame, else 0;
//   gx[c, p] = c s gz[c, p] + c (1 - s) mean_c gz[:, p] + (1 - c) mean(gz).
// The policy is STATIC: its three bits select one of eight instantiations, and an op that is off executes none of its arithmetic -
// without DA_COLOR the output is the input shifted and masked, bit for bit, whatever the row's colour words hold.
//
// Both directions are one reduction (M, mean(gz)) and one apply.
//   S <= 64: ONE launch, a block per image.  The image (12 / 48 KiB) is staged into LDS, by 16-byte loads where the buffer allows
//   them; the mean is taken from the registers that staged it; the shifted reads come from LDS, so the stores stay 16-byte
//   whatever tx is.  One read and one write of the batch.
//   S = 128, 256: an image does not fit LDS.  Launch 1 writes a float64 partial sum per (image, slab of MT_CHUNK elements) into
//   the workspace; launch 2 adds an image's partials in ascending order and streams the image.  Without DA_COLOR launch 1 is
//   not run.
// The sums are float64 sums of the fp32 values in one fixed order (multitensor.h: a thread's elements in index order, a wave by
// a butterfly, the four waves in order; slabs ascending), divided by 3 S^2 in float64 and rounded once to fp32; no atomics.  An
// element belongs to the same thread whatever the buffer's alignment, so an image's output depends on that image and its row
// alone.  Every other operation is one IEEE fp32 operation spelled out below under `fp contract(off)`, with fmaf where a fused
// multiply-add is meant.
//
// PER-IMAGE OP MASK (adaptive augmentation, csrc/ada.hip).  Word 9 of a row is a small exact integer: bit k set switches op k off
// for THIS image; 0 is the behaviour above.  The ops that run are OPS = POLICY & ~mask, and every kernel below branches once per
// block on OPS into the body instantiated for exactly that subset, so an image's output under policy P and mask m is, bit for bit,
// what the instantiation P & ~m writes for the same row: a masked op executes none of its arithmetic (no colour chain, ty = tx = 0,
// no multiplication by keep).  The mask is the same in every thread of a block (blockIdx.x / blockIdx.y names the image): the branch
// is wave-uniform.  The image loads of the one-launch form and of launch 1 are issued BEFORE the branch, so that an unmasked image
// waits for nothing it did not wait for before.  OPS == 0 is a plain copy: no LDS, no reduction, 16-byte loads and stores where each
// side allows them.  At S >= 128 launch 1 leaves an image whose colour is masked as soon as the mask has arrived - it adds nothing
// and writes no partial - and launch 2 then reads none.
#include "multitensor.h"

#define DA_PARAMS 12
#define DA_COLOR 1
#define DA_TRANSLATION 2
#define DA_CUTOUT 4
#define DA_MASK_WORD 9          // bit k set: op k is off for this image
#define DA_SMALL_MAX 64         // largest S of the one-launch form

struct DaSum {
    double s;
    __device__ __forceinline__ void add(const DaSum& q) { s += q.s; }
};

struct DaRow {          // an image's parameter row, decoded
    float b, s, c;
    int ty, tx, y0, y1, x0, x1;
};

template <int POLICY>
__device__ __forceinline__ DaRow da_row(const float* __restrict__ params, int img) {
    const float* p = params + (size_t)img * DA_PARAMS;
    DaRow r;
    r.b = 0.0f; r.s = 1.0f; r.c = 1.0f;
    r.ty = r.tx = 0;
    r.y0 = r.y1 = r.x0 = r.x1 = 0;
    if (POLICY & DA_COLOR) { r.b = p[0]; r.s = p[1]; r.c = p[2]; }
    if (POLICY & DA_TRANSLATION) { r.ty = (int)p[3]; r.tx = (int)p[4]; }
    if (POLICY & DA_CUTOUT) { r.y0 = (int)p[5]; r.y1 = (int)p[6]; r.x0 = (int)p[7]; r.x1 = (int)p[8]; }
    return r;
}

// The ops that run for image `img`: the static policy without the bits of the row's mask word; the same value in every lane (the
// word's address is the block's, so it arrives in a scalar register, which the "s" operand below insists on).  In two steps, so
// that a kernel can ask for the word first, issue its image loads, and only then wait for the word.
__device__ __forceinline__ float da_mask_word(const float* __restrict__ params, int img) {
    return params[(size_t)img * DA_PARAMS + DA_MASK_WORD];
}

template <int POLICY>
__device__ __forceinline__ int da_ops(float mask_word) {
    // The empty statement pins the conversion, and with it the wait for the word, where this call stands: left to itself the
    // compiler lifts both to the top of the kernel, in front of the image loads.
    unsigned bits = __float_as_uint(mask_word);
    asm volatile("" : "+s"(bits));
    const float word = __uint_as_float(bits);
    return POLICY & ~(int)word;
}

// `ops` is a subset of POLICY: run BODY with the compile-time constant OPS equal to it (1 .. 7; 0 is the callers' copy path)
#define DA_CASE(POLICY, K, BODY)                   \
    case K:                                        \
        if constexpr (((POLICY) & (K)) == (K)) {   \
            constexpr int OPS = K;                 \
            BODY;                                  \
        }                                          \
        break;
#define DA_DISPATCH(POLICY, ops, BODY)                                                                              \
    switch (ops) {                                                                                                  \
        DA_CASE(POLICY, 1, BODY) DA_CASE(POLICY, 2, BODY) DA_CASE(POLICY, 3, BODY) DA_CASE(POLICY, 4, BODY)         \
        DA_CASE(POLICY, 5, BODY) DA_CASE(POLICY, 6, BODY) DA_CASE(POLICY, 7, BODY)                                  \
        default: break;                                                                                             \
    }

__device__ __forceinline__ float da_keep(const DaRow& r, int i, int j) {
    return (i >= r.y0 && i < r.y1 && j >= r.x0 && j < r.x1) ? 0.0f : 1.0f;
}

// ---- the fp32 arithmetic, pinned ------------------------------------------------------------------------------------------------------
struct DaColour {          // per image: forward {s, c, M, M + b}; backward {c s, c (1 - s), (1 - c) mean(gz)}
    float k0, k1, k2, k3;
};

__device__ __forceinline__ DaColour da_colour_fwd(const DaRow& r, float M) {
#pragma clang fp contract(off)
    DaColour k;
    k.k0 = r.s; k.k1 = r.c; k.k2 = M;
    k.k3 = M + r.b;
    return k;
}

__device__ __forceinline__ DaColour da_colour_bwd(const DaRow& r, float G) {
#pragma clang fp contract(off)
    DaColour k;
    k.k0 = r.c * r.s;
    const float oms = 1.0f - r.s;
    k.k1 = r.c * oms;
    const float omc = 1.0f - r.c;
    k.k2 = omc * G;
    k.k3 = 0.0f;
    return k;
}

// z[c] = fma(c, fma(s, x[c] - mu, mu) - M, M + b), mu = ((x0 + x1) + x2) / 3
__device__ __forceinline__ void da_pixel_fwd(const DaColour& k, float& a0, float& a1, float& a2) {
#pragma clang fp contract(off)
    const float sum = (a0 + a1) + a2;
    const float mu = sum / 3.0f;
    const float d0 = a0 - mu, d1 = a1 - mu, d2 = a2 - mu;
    const float t0 = fmaf(k.k0, d0, mu) - k.k2, t1 = fmaf(k.k0, d1, mu) - k.k2, t2 = fmaf(k.k0, d2, mu) - k.k2;
    a0 = fmaf(k.k1, t0, k.k3);
    a1 = fmaf(k.k1, t1, k.k3);
    a2 = fmaf(k.k1, t2, k.k3);
}

// gx[c] = fma(c s, gz[c], fma(c (1 - s), m, (1 - c) G)), m = ((gz0 + gz1) + gz2) / 3
__device__ __forceinline__ void da_pixel_bwd(const DaColour& k, float& a0, float& a1, float& a2) {
#pragma clang fp contract(off)
    const float sum = (a0 + a1) + a2;
    const float m = sum / 3.0f;
    const float r = fmaf(k.k1, m, k.k2);
    a0 = fmaf(k.k0, a0, r);
    a1 = fmaf(k.k0, a1, r);
    a2 = fmaf(k.k0, a2, r);
}

__device__ __forceinline__ float da_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// ---- one output pixel, all three channels ---------------------------------------------------------------------------------------------
// src: the image's base (LDS or global), planes of S * S.  Output pixel (i, j).  Forward reads the source pixel (i - ty, j - tx),
// applies the colour there and masks at (i, j); backward reads (i + ty, j + tx), masks THERE and applies the colour adjoint at
// (i, j).  A source pixel outside the frame is never read.  COLOUR_NOW false: the backward's reduction, which wants gz itself.
template <int POLICY, bool BWD, bool COLOUR_NOW>
__device__ __forceinline__ void da_pixel(const float* src, int S, const DaRow& r, const DaColour& k, int i, int j, float& a0, float& a1,
                                         float& a2) {
    const int si = BWD ? i + r.ty : i - r.ty, sj = BWD ? j + r.tx : j - r.tx;
    const bool inside = (unsigned)si < (unsigned)S && (unsigned)sj < (unsigned)S;
    a0 = a1 = a2 = 0.0f;
    if (inside) {
        const int o = si * S + sj, plane = S * S;
        a0 = src[o];
        a1 = src[o + plane];
        a2 = src[o + 2 * plane];
        if (BWD) {
            if (POLICY & DA_CUTOUT) {
                const float keep = da_keep(r, si, sj);
                a0 = da_mul(keep, a0); a1 = da_mul(keep, a1); a2 = da_mul(keep, a2);
            }
        } else {
            if ((POLICY & DA_COLOR) && COLOUR_NOW) da_pixel_fwd(k, a0, a1, a2);
            if (POLICY & DA_CUTOUT) {
                const float keep = da_keep(r, i, j);
                a0 = da_mul(keep, a0); a1 = da_mul(keep, a1); a2 = da_mul(keep, a2);
            }
        }
    }
    if (BWD && (POLICY & DA_COLOR) && COLOUR_NOW) da_pixel_bwd(k, a0, a1, a2);          // the border's gz is 0, its gx is not
}

// four neighbouring output pixels (i, j .. j + 3) of the three planes, stored by 16-byte words where dst allows it
template <int POLICY, bool BWD>
__device__ __forceinline__ void da_quad(const float* src, float* dst, bool dst_vec, int S, const DaRow& r, const DaColour& k, int i, int j) {
    float4 q[3];
    da_pixel<POLICY, BWD, true>(src, S, r, k, i, j, q[0].x, q[1].x, q[2].x);
    da_pixel<POLICY, BWD, true>(src, S, r, k, i, j + 1, q[0].y, q[1].y, q[2].y);
    da_pixel<POLICY, BWD, true>(src, S, r, k, i, j + 2, q[0].z, q[1].z, q[2].z);
    da_pixel<POLICY, BWD, true>(src, S, r, k, i, j + 3, q[0].w, q[1].w, q[2].w);
    const int o = i * S + j, plane = S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* d = dst + o + c * plane;
        if (dst_vec) {
            *reinterpret_cast<float4*>(d) = q[c];
        } else {
            d[0] = q[c].x; d[1] = q[c].y; d[2] = q[c].z; d[3] = q[c].w;
        }
    }
}

__device__ __forceinline__ float da_mean(double total, int S) { return (float)(total / (double)(3 * S * S)); }

// ---- an image without an op: a plain copy ----------------------------------------------------------------------------------------------
// one 16-byte word (four neighbouring elements), by a 16-byte access where that side allows it
__device__ __forceinline__ float4 da_load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    float4 v;
    v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    return v;
}

__device__ __forceinline__ void da_store4(float* p, bool vec, const float4& v) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// ---- S <= 64: a block per image, the image in LDS --------------------------------------------------------------------------------------
// what follows the staging for the ops OPS (not 0): the reduction, if colour runs, and the apply
template <int OPS, bool BWD>
__device__ __forceinline__ void da_small_apply(const float* __restrict__ params, const float* img, float* dst, bool dst_vec, int S, DaSum acc,
                                               DaSum* red, float* mean_sh) {
    const DaRow r = da_row<OPS>(params, blockIdx.x);
    const int quads_per_row = S >> 2, n_quads = S * quads_per_row;
    DaColour k = {0.0f, 0.0f, 0.0f, 0.0f};
    if (OPS & DA_COLOR) {
        if (BWD) {          // mean(gz): the masked, shifted gradient, in the order of the output's pixel quads
            for (int q = threadIdx.x; q < n_quads; q += MT_THREADS) {
                const int i = q / quads_per_row, j = (q - i * quads_per_row) << 2;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float a0, a1, a2;
                    da_pixel<OPS, true, false>(img, S, r, k, i, j + u, a0, a1, a2);
                    acc.s = ((acc.s + (double)a0) + (double)a1) + (double)a2;
                }
            }
        }
        const DaSum total = mt_block_total(acc, red);
        if (threadIdx.x == 0) *mean_sh = da_mean(total.s, S);
        __syncthreads();
        k = BWD ? da_colour_bwd(r, *mean_sh) : da_colour_fwd(r, *mean_sh);
    }
    for (int q = threadIdx.x; q < n_quads; q += MT_THREADS) {
        const int i = q / quads_per_row, j = (q - i * quads_per_row) << 2;
        da_quad<OPS, BWD>(img, dst, dst_vec, S, r, k, i, j);
    }
}

template <int POLICY, bool BWD>
__global__ void __launch_bounds__(MT_THREADS) diffaug_small_kernel(const float* __restrict__ in, const float* __restrict__ params,
                                                                    float* __restrict__ out, int S) {
    __shared__ float4 img4[3 * DA_SMALL_MAX * DA_SMALL_MAX / 4];
    __shared__ DaSum red[MT_WAVES];
    __shared__ float mean_sh;
    float* img = reinterpret_cast<float*>(img4);
    const int n_el = 3 * S * S, n4 = n_el >> 2;          // S is a multiple of 4
    const float* src = in + (size_t)blockIdx.x * n_el;
    float* dst = out + (size_t)blockIdx.x * n_el;
    const bool src_vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0, dst_vec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const float mask_word = da_mask_word(params, blockIdx.x);

    // stage: 16-byte word w of the image belongs to thread w % 256 whatever the alignment.  The first round's loads are issued
    // BEFORE the mask word is looked at (its wait would otherwise stand in front of them: +0.5 us at 192 x 3 x 64 x 64,
    // profiles/notes_ada.md); what is done with the loaded words depends on it: an image without an op goes straight to dst.  The
    // forward's sum is taken under the STATIC policy (a masked colour leaves it unused: da_small_apply<OPS> never looks at it).
    DaSum acc = {0.0};
    int ops;
    if (src_vec) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int w = u * MT_THREADS + threadIdx.x;
            if (w < n4) v[u] = reinterpret_cast<const float4*>(src)[w];
        }
        ops = da_ops<POLICY>(mask_word);
        for (int w0 = 0; w0 < n4; w0 += 4 * MT_THREADS) {
            if (w0 > 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int w = w0 + u * MT_THREADS + threadIdx.x;
                    if (w < n4) v[u] = reinterpret_cast<const float4*>(src)[w];
                }
            }
            if (ops == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int w = w0 + u * MT_THREADS + threadIdx.x;
                    if (w < n4) da_store4(dst + 4 * w, dst_vec, v[u]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int w = w0 + u * MT_THREADS + threadIdx.x;
                    if (w < n4) {
                        img4[w] = v[u];
                        if ((POLICY & DA_COLOR) && !BWD) acc.s = (((acc.s + (double)v[u].x) + (double)v[u].y) + (double)v[u].z) + (double)v[u].w;
                    }
                }
            }
        }
    } else {
        ops = da_ops<POLICY>(mask_word);
        for (int w = threadIdx.x; w < n4; w += MT_THREADS) {
            float4 v;
            v.x = src[4 * w]; v.y = src[4 * w + 1]; v.z = src[4 * w + 2]; v.w = src[4 * w + 3];
            if (ops == 0) {
                da_store4(dst + 4 * w, dst_vec, v);
            } else {
                img4[w] = v;
                if ((POLICY & DA_COLOR) && !BWD) acc.s = (((acc.s + (double)v.x) + (double)v.y) + (double)v.z) + (double)v.w;
            }
        }
    }
    if (ops == 0) return;          // the whole block: `ops` is the image's
    __syncthreads();
    DA_DISPATCH(POLICY, ops, (da_small_apply<OPS, BWD>(params, img, dst, dst_vec, S, acc, red, &mean_sh)))
}

// ---- S >= 128, launch 1: a float64 partial per (image, slab) ---------------------------------------------------------------------------
template <int OPS, bool BWD>
__device__ __forceinline__ void da_partial(const float* __restrict__ params, const float4 (&v)[MT_PER_THREAD], double* __restrict__ partials,
                                           int S, DaSum* red) {
    const int n_el = 3 * S * S, slabs = n_el / MT_CHUNK;          // S >= 128: a whole number of slabs
    const int slab = blockIdx.x, image = blockIdx.y;
    const DaRow r = da_row<OPS>(params, image);
    DaSum acc = {0.0};
#pragma unroll
    for (int u = 0; u < MT_PER_THREAD; ++u) {
        float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        if (BWD) {          // gz is gy masked where it is read and dropped where its target leaves the frame
            const int at = slab * MT_CHUNK + 4 * (threadIdx.x + u * MT_THREADS);          // the four share a row: S is a multiple of 4
            const int pix = at & (S * S - 1), si = pix / S, sj = pix - si * S;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool lands = (unsigned)(si - r.ty) < (unsigned)S && (unsigned)(sj + t - r.tx) < (unsigned)S;
                if (OPS & DA_CUTOUT) e[t] = da_mul(da_keep(r, si, sj + t), e[t]);
                e[t] = lands ? e[t] : 0.0f;
            }
        }
        acc.s = (((acc.s + (double)e[0]) + (double)e[1]) + (double)e[2]) + (double)e[3];
    }
    const DaSum total = mt_block_total(acc, red);
    if (threadIdx.x == 0) partials[(size_t)image * slabs + slab] = total.s;
}

template <int POLICY, bool BWD>
__global__ void __launch_bounds__(MT_THREADS) diffaug_partial_kernel(const float* __restrict__ in, const float* __restrict__ params,
                                                                      double* __restrict__ partials, int S) {
    __shared__ DaSum red[MT_WAVES];
    const int n_el = 3 * S * S;
    const int slab = blockIdx.x, image = blockIdx.y;
    const float* src = in + (size_t)image * n_el + (size_t)slab * MT_CHUNK;
    const float mask_word = da_mask_word(params, image);
    float4 v[MT_PER_THREAD];
    mt_read_lanes(src, MT_CHUNK, v);          // issued before the mask word is looked at: its wait does not stand in front of them
    const int ops = da_ops<POLICY>(mask_word);
    if (!(ops & DA_COLOR)) return;          // colour is masked for this image: no partial is written, and launch 2 reads none
    DA_DISPATCH(POLICY, ops, (da_partial<OPS, BWD>(params, v, partials, S, red)))
}

// ---- S >= 128, launch 2: the image streamed; a thread per pixel quad ------------------------------------------------------------------
template <int OPS, bool BWD>
__device__ __forceinline__ void da_apply(const float* src, const float* __restrict__ params, float* dst, bool dst_vec,
                                         const double* __restrict__ partials, int S, int image, int i, int j) {
    const int slabs = 3 * S * S / MT_CHUNK;
    const DaRow r = da_row<OPS>(params, image);
    DaColour k = {0.0f, 0.0f, 0.0f, 0.0f};
    if (OPS & DA_COLOR) {
        double total = 0.0;
        for (int s = 0; s < slabs; ++s) total += partials[(size_t)image * slabs + s];          // ascending, the same in every thread
        const float mean = da_mean(total, S);
        k = BWD ? da_colour_bwd(r, mean) : da_colour_fwd(r, mean);
    }
    da_quad<OPS, BWD>(src, dst, dst_vec, S, r, k, i, j);
}

template <int POLICY, bool BWD>
__global__ void __launch_bounds__(MT_THREADS) diffaug_apply_kernel(const float* __restrict__ in, const float* __restrict__ params,
                                                                    float* __restrict__ out, const double* __restrict__ partials, int S) {
    const int n_el = 3 * S * S, image = blockIdx.y;
    const float* src = in + (size_t)image * n_el;
    float* dst = out + (size_t)image * n_el;
    const bool src_vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0, dst_vec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const int ops = da_ops<POLICY>(da_mask_word(params, image));
    const int quads_per_row = S >> 2, q = blockIdx.x * MT_THREADS + threadIdx.x;
    if (q >= S * quads_per_row) return;
    const int i = q / quads_per_row, j = (q - i * quads_per_row) << 2;
    if (ops == 0) {          // the quad of each plane, copied
        const int o = i * S + j, plane = S * S;
        float4 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = da_load4(src + o + c * plane, src_vec);
#pragma unroll
        for (int c = 0; c < 3; ++c) da_store4(dst + o + c * plane, dst_vec, v[c]);
        return;
    }
    DA_DISPATCH(POLICY, ops, (da_apply<OPS, BWD>(src, params, dst, dst_vec, partials, S, image, i, j)))
}

// ---- host entries ---------------------------------------------------------------------------------------------------------------------
static bool da_size_ok(int S) { return S == 32 || S == 64 || S == 128 || S == 256; }

template <int POLICY, bool BWD>
static void da_launch(const float* in, const float* params, float* out, int n, int S, double* partials, hipStream_t st) {
    if (S <= DA_SMALL_MAX) {
        diffaug_small_kernel<POLICY, BWD><<<n, MT_THREADS, 0, st>>>(in, params, out, S);
        return;
    }
    const int slabs = 3 * S * S / MT_CHUNK;
    if (POLICY & DA_COLOR) diffaug_partial_kernel<POLICY, BWD><<<dim3(slabs, n), MT_THREADS, 0, st>>>(in, params, partials, S);
    diffaug_apply_kernel<POLICY, BWD><<<dim3(S * S / 4 / MT_THREADS, n), MT_THREADS, 0, st>>>(in, params, out, partials, S);
}

template <bool BWD>
static int da_run(const char* name, const float* in, const float* params, float* out, int n, int S, int policy, void* workspace, void* stream) {
    LOCATE_REQUIRE(in && params && out && in != out, "%s: null or aliased buffers", name);
    LOCATE_REQUIRE(da_size_ok(S), "%s: S = %d is not one of 32, 64, 128, 256", name, S);
    LOCATE_REQUIRE(n > 0 && n <= 65535, "%s: n = %d is not in 1 .. 65535", name, n);
    LOCATE_REQUIRE(policy >= 0 && policy < 8, "%s: policy %d has bits beyond colour | translation | cutout", name, policy);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params)) & 3) == 0,
                   "%s: buffers must be 4-byte aligned", name);
    const bool two = S > DA_SMALL_MAX && (policy & DA_COLOR);
    LOCATE_REQUIRE(!two || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0), "%s: S = %d needs an 8-byte aligned workspace", name, S);
    double* partials = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    switch (policy) {
        case 0: da_launch<0, BWD>(in, params, out, n, S, partials, st); break;
        case 1: da_launch<1, BWD>(in, params, out, n, S, partials, st); break;
        case 2: da_launch<2, BWD>(in, params, out, n, S, partials, st); break;
        case 3: da_launch<3, BWD>(in, params, out, n, S, partials, st); break;
        case 4: da_launch<4, BWD>(in, params, out, n, S, partials, st); break;
        case 5: da_launch<5, BWD>(in, params, out, n, S, partials, st); break;
        case 6: da_launch<6, BWD>(in, params, out, n, S, partials, st); break;
        default: da_launch<7, BWD>(in, params, out, n, S, partials, st); break;
    }
    LOCATE_LAUNCH_CHECK(name);
    return LOCATE_OK;
}

LOCATE_API int locate_diffaug_param_floats(void) { return DA_PARAMS; }

// 0 for the one-launch sizes (the workspace may then be null)
LOCATE_API size_t locate_diffaug_workspace_bytes(int n, int S) {
    if (n <= 0 || !da_size_ok(S) || S <= DA_SMALL_MAX) return 0;
    return (size_t)n * (size_t)(3 * S * S / MT_CHUNK) * sizeof(double);
}

// No allocation, no host read, no synchronisation: legal under stream capture.  Writes [y, y + 3 n S^2) and, for S >= 128 with
// colour, the workspace; nothing else.
LOCATE_API int locate_diffaug_fwd(const float* x, const float* params, float* y, int n, int S, int policy, void* workspace, void* stream) {
    return da_run<false>("locate_diffaug_fwd", x, params, y, n, S, policy, workspace, stream);
}

LOCATE_API int locate_diffaug_bwd(const float* gy, const float* params, float* gx, int n, int S, int policy, void* workspace, void* stream) {
    return da_run<true>("locate_diffaug_bwd", gy, params, gx, n, S, policy, workspace, stream);
}
