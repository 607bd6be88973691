// The Nadam schedule and update bodies, instantiated twice: plain (nadam.hip) and behind a verdict (guard.hip).  Both steps run this
// one source, so a guard that has nothing to do is Nadam bit for bit by construction (tests/test_gpu_guard.py holds the two
// instantiations against each other, tests/golden/p01_nadam_bits.npz both against the past).
#pragma once
#include "multitensor.h"

struct NadamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    double* sched;     // [2]: step count, m_schedule
    long long n;
    unsigned* absmax;  // nullable: AMAX_WORDS words that receive the largest magnitude of the UPDATED tensor (bit pattern,
                       // spread like every other absmax slot, common.h) - what the fp16-piece weight panels are scaled by;
                       // re-packing them then needs no pass of its own over the weights (convpack.hip, direct packing)
};

struct NadamCoef {
    float c_grad, c_mom, bias2, pad;
};

// One thread per tensor.  `take` false (a skipped guarded step) leaves (step, m_schedule) alone and writes no coefficients; the
// largest-magnitude words are cleared either way: the update kernel folds the maximum in, skipped or not.
__device__ __forceinline__ void nadam_schedule(const NadamTensor* __restrict__ tensors, NadamCoef* __restrict__ coef, int n_tensors,
                                               double lr, double b1, double b2, double sd, bool take) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tensors) return;
    double* st = tensors[i].sched;
    const double t = st[0] + 1.0;
    const double ms = st[0] == 0.0 ? 1.0 : st[1];
    const double mc_t = b1 * (1.0 - 0.5 * pow(0.96, t * sd));
    const double mc_t1 = b1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * sd));
    const double ms_new = ms * mc_t;
    const double ms_next = ms_new * mc_t1;
    if (take) {
        st[0] = t;
        st[1] = ms_new;
    }
    if (tensors[i].absmax)
        for (int k = 0; k < AMAX_LINES; ++k) tensors[i].absmax[k * AMAX_STRIDE] = 0u;
    NadamCoef c;
    c.c_grad = (float)(-lr * (1.0 - mc_t) / (1.0 - ms_new));
    c.c_mom = (float)(-lr * mc_t1 / (1.0 - ms_next));
    c.bias2 = (float)(1.0 - pow(b2, t));
    c.pad = 0.0f;
    if (take) coef[i] = c;
}

// One element of the update, every rounding spelled out (common.h's rule for arithmetic shared between kernels: with the compiler
// free to contract a * b + c per call site, the same source inlined into two kernels rounds differently):
//   g' = rn(g * scale)   SCALED only, one rounding of its own;  g' = fma(wd, p, g') with weight decay (nadam.py:65-66)
//   m  = fma(1 - b1, g', rn(b1 * m))                     v = rn(rn(rn((1 - b2) * g') * g') + rn(b2 * v))
//   p  = rn(rn(p + rn(c_grad * rn(g' / denom))) + rn(c_mom * rn(m / denom))),  denom = rn(sqrt(rn(v / bias2)) + eps)
template <bool SCALED>
__device__ __forceinline__ void nadam_element(float& p, float gin, float& m, float& v, float scale, float wd, float b1, float b2,
                                              float omb1, float omb2, float eps, const NadamCoef& c) {
#pragma clang fp contract(off)
    const float gs = SCALED ? gin * scale : gin;
    const float g = wd != 0.0f ? fmaf(wd, p, gs) : gs;
    const float mb = m * b1;
    m = fmaf(omb1, g, mb);
    const float vb = v * b2;
    const float og = omb2 * g;
    v = og * g + vb;
    const float denom = sqrtf(v / c.bias2) + eps;
    p = p + c.c_grad * (g / denom);
    p = p + c.c_mom * (m / denom);
}

// One block per chunk-table entry.  GUARDED: `skip` (block-uniform) streams p alone to fold max |p| into the words again and
// writes nothing else; otherwise every gradient element is multiplied by `scale` first.
template <bool GUARDED>
__device__ __forceinline__ void nadam_update(const NadamTensor* __restrict__ tensors, const NadamCoef* __restrict__ coef,
                                             const int2* __restrict__ chunks, float b1, float b2, float eps, float wd, int skip, float scale) {
    const int2 ch = chunks[blockIdx.x];
    NadamTensor T;
    long long begin;
    int len;
    if (!mt_decode(tensors, MT_ANY_TENSOR, ch, T, begin, len)) return;          // block-uniform
    const long long end = begin + len;
    __shared__ float scratch[16];
    float amax = 0.0f;
    if (GUARDED && skip) {
        if (!T.absmax) return;
        for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) amax = fmaxf(amax, fabsf(T.p[i]));
        absmax_publish(amax, scratch, T.absmax);
        return;
    }
    const NadamCoef c = coef[ch.x];
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) {
        float p = T.p[i], m = T.m[i], v = T.v[i];
        nadam_element<GUARDED>(p, T.g[i], m, v, scale, wd, b1, b2, omb1, omb2, eps, c);
        T.m[i] = m;
        T.v[i] = v;
        T.p[i] = p;
        amax = fmaxf(amax, fabsf(p));
    }
    if (T.absmax) absmax_publish(amax, scratch, T.absmax);          // wave-uniform condition: every thread of the block takes it
}
