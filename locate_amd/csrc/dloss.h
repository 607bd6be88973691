// The D-step's hinge and consistency-penalty arithmetic, shared by csrc/loss.hip (locate_d_loss) and csrc/lecam.hip
// (locate_d_loss_lecam, whose inactive path has to return locate_d_loss's bits): the sums of one pass over the logits, the scalars
// derived from them and the plain gradients, each spelled ONCE here.
//
// Every fp32 operation is rounded once and written in the order the kernel has always executed it (`fp contract(off)`), with the
// single fused operation spelled as fmaf: the total is d_error + gamma * delta * delta evaluated as fma(delta, gamma * delta,
// d_error), so losses[2] is NOT always the fp32 sum of losses[0] and losses[1].  (That is what the backend made of the plain
// expression under the default contraction mode; writing it out keeps the bits where another file inlines the same code.)
#pragma once
#include "common.h"

// clamp(v, min=0) as ATen computes it: a NaN argument stays NaN (fmaxf would return the 0 and a NaN discriminator output would
// leave the printed loss finite); its gradient mask (v >= 0) is false there, as ATen's.
__device__ __forceinline__ float hinge_clamp(float v) { return v < 0.0f ? 0.0f : v; }

struct DLossScalars {
    float invB;          // 1 / B
    float delta;         // mean t - mean a
    float pen_g;         // d penalty / d t_i = ((2 gamma) delta) / B
    float d_error;       // mean hinge
    float pen;           // (gamma delta) delta
};

// hs, ts, as: the block's float64 sums of relu(1 - t) + relu(1 + f), of t and of a
__device__ __forceinline__ DLossScalars d_loss_scalars(double hs, double ts, double as, int B, float gamma) {
#pragma clang fp contract(off)
    DLossScalars s;
    s.invB = 1.0f / (float)B;
    s.delta = (float)(ts / B) - (float)(as / B);
    s.pen_g = 2.0f * gamma * s.delta * s.invB;
    s.d_error = (float)(hs / B);
    s.pen = gamma * s.delta * s.delta;
    return s;
}

// d_error + penalty as locate_d_loss has always returned it: one fused multiply-add on the penalty's last product
__device__ __forceinline__ float d_loss_total(const DLossScalars& s, float gamma) {
#pragma clang fp contract(off)
    return fmaf(s.delta, gamma * s.delta, s.d_error);
}

__device__ __forceinline__ double d_hinge_term(float t, float f) { return (double)hinge_clamp(1.0f - t) + (double)hinge_clamp(1.0f + f); }

__device__ __forceinline__ float d_grad_true(float t, const DLossScalars& s) {
#pragma clang fp contract(off)
    return ((1.0f - t) >= 0.0f ? -s.invB : 0.0f) + s.pen_g;
}
__device__ __forceinline__ float d_grad_fake(float f, const DLossScalars& s) { return (1.0f + f) >= 0.0f ? s.invB : 0.0f; }

// The whole of locate_d_loss's kernel for one block of 256 threads; scratch: 16 doubles of LDS.
__device__ __forceinline__ void d_loss_plain(const float* __restrict__ t, const float* __restrict__ f, const float* __restrict__ a, int B,
                                             float gamma, float* __restrict__ losses, float* __restrict__ gt, float* __restrict__ gf,
                                             float* __restrict__ ga, double* scratch) {
    double hs = 0.0, ts = 0.0, as = 0.0;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        hs += d_hinge_term(t[i], f[i]);
        ts += t[i];
        as += a[i];
    }
    hs = block_sum<double>(hs, scratch);
    ts = block_sum<double>(ts, scratch);
    as = block_sum<double>(as, scratch);
    const DLossScalars s = d_loss_scalars(hs, ts, as, B, gamma);
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        gt[i] = d_grad_true(t[i], s);
        gf[i] = d_grad_fake(f[i], s);
        ga[i] = -s.pen_g;
    }
    if (threadIdx.x == 0) {
        losses[0] = s.d_error;
        losses[1] = s.pen;
        losses[2] = d_loss_total(s, gamma);
    }
}
