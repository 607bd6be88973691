// Device code of InPlaceNorm's backward dx term, shared by its own element-wise kernel (norm_bwd_dx_kernel, norm.hip) and by the
// gate backward kernels that form the same value on the fly (gate_bwd_*_kernel with an incoming-gradient term, elementwise.hip):
// one definition, so that the folded and the separate form cannot round differently.
#pragma once
#include "common.h"

#define NORM_MAX_GROUPS 4

// The incoming-gradient term of locate_gate_bwd_term (LocateGateTerm of include/locate_hip.h, passed by value).
struct LocateGateTerm {
    int32_t kind;                   // GATE_TERM_NONE / _NORM / _ROOTTANH
    int32_t with_act;               // norm: the forward returned RootTanh(norm(out)) - the kernels' GATE_TERM_NORM_ACT
    int32_t per_sample;             // norm: scale is [B*C]
    int32_t has_share;              // norm: g of the gate call holds the other consumer's share, added AFTER the term (o + share)
    const float* go;                // norm: gradient w.r.t. the norm's output [planes * hw]
    const float* stats;             // norm: groups x {mean, std}
    const float* scale;
    const float* bias;
    const double* partial;          // norm: the plane pass's per-block group sums [npartial][NORM_MAX_GROUPS][2]
    int32_t npartial, B, C, groups;
};
enum { GATE_TERM_NONE = 0, GATE_TERM_NORM = 1, GATE_TERM_ROOTTANH = 2, GATE_TERM_NORM_ACT = 3 /* kernel instantiations only */ };

#ifdef __HIPCC__
// a * b rounded as a product of its own.  hipcc contracts a multiplication into the addition that consumes it wherever it sees
// both (-ffp-contract=fast; to it __fmul_rn is a plain `*`), and a gate's stored output is such a product: the kernels that
// recompute it and go on to subtract a mean must not fold the two into one fma.  The empty asm hides the product from that.
__device__ __forceinline__ float mul_pinned(float a, float b) {
    float r = a * b;
    asm("" : "+v"(r));
    return r;
}

template <bool ACT>
__device__ __forceinline__ float norm_go(float xv, float gv, float mu, float inv_s, float y, float b) {
    if (!ACT) return gv;
    const float o = fmaf(xv - mu, y * inv_s, b);          // the same expression as the forward's norm_apply_fused_kernel
    return roottanh_grad_f(o, gv);
}

// { mean(y go / s), dz / ((N - 1) s) } of group `grp` from the plane pass's per-block partials: ONE wave (lane = 0 .. 63), fp64,
// fixed order; lane 0 writes consts[0 .. 1].  n = elements per group, s = the group's std.
__device__ __forceinline__ void norm_group_consts(const double* __restrict__ partial, int npartial, int grp, float s, int64_t n,
                                                  int lane, float* consts) {
    double a = 0.0, b2 = 0.0;
    for (int i = lane; i < npartial; i += 64) {
        a += partial[((int64_t)i * NORM_MAX_GROUPS + grp) * 2];
        b2 += partial[((int64_t)i * NORM_MAX_GROUPS + grp) * 2 + 1];
    }
    a = wave_sum_d(a);
    b2 = wave_sum_d(b2);
    if (lane == 0) {
        const double sd = (double)s, nn = (double)n;
        consts[0] = (float)(a / sd / nn);
        consts[1] = (float)(-b2 / (sd * sd) / ((nn - 1.0) * sd));
    }
}

// dx of one element: y go' / s - m + k (x - mu), go' = go (or go * RootTanh'(norm(x)) with ACT)
template <bool ACT>
__device__ __forceinline__ float norm_dx(float xv, float gv, float mu, float inv_s, float y, float b, float k, float m) {
    const float go = norm_go<ACT>(xv, gv, mu, inv_s, y, b);
    return fmaf(y * inv_s, go, fmaf(k, xv - mu, -m));
}
#endif
