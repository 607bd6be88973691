// LeCam regularisation of the discriminator (Tseng et al. 2021, "Regularizing Generative Adversarial Networks under Limited Data"):
// exponential moving averages of D's mean prediction on real and on generated images - the anchors - and a penalty on D's real
// predictions for moving away from the generated anchor and the other way round.  Two single-block kernels (locate_amd/lecam.py,
// LeCam; the definition in numpy, which both kernels equal with ==: tests/helpers/lecam_model.py).
//
//   d_loss:  locate_d_loss's launch with the regulariser added to the total and to the gradients - or, while the regulariser is
//            inactive, locate_d_loss's own arithmetic (dloss.h) and nothing else;
//   observe: runs BESIDE the training step, once after an iteration: the batch means of D(real) and D(G(z)) into the anchors.
//
// The state is one record of LECAM_STATE_WORDS 32-bit words at a fixed device address:
//   0 alpha_R, the anchor of mean D(real) (fp32)   1 alpha_F, the anchor of mean D(G(z)) (fp32)   2 observations accepted
//   3 observations in all   4 observations refused as non-finite   5 ring rows written in all   6 m_R and 7 m_F of the last
//   observation (fp32)   8 .. 15 zero.       (counters mod 2^32)
// A ring row: LECAM_RING_WORDS words {iteration, alpha_R, alpha_F, m_R, m_F, 1 if the observation was accepted else 0, 0, 0}, the
// anchors as the observation left them.
// Both kernels: no allocation, no host read, no atomics, values written by ordinary vector stores; legal under stream capture
// (observe's `iteration` is a launch argument: a captured launch would repeat it).  Whether the regulariser is active is decided
// on the device from word 2, so a replayed graph switches it on by itself.
#include "dloss.h"

#define LECAM_STATE_WORDS 16
#define LECAM_RING_WORDS 8
#define LECAM_THREADS 256

// ---- the regulariser --------------------------------------------------------------------------------------------------------------------
//   d_i = t_i - alpha_F,  e_i = alpha_R - f_i;  one_sided: both through hinge_clamp (a NaN stays NaN)
//   R = (float)(sum d_i^2 / B) + (float)(sum e_i^2 / B)      float64 products and sums, block_sum's order
//   total = (d_error + penalty) + weight * R                  here d_error + penalty is ONE rounded fp32 addition, not dloss.h's fma
//   g_true[i] = plain + q,  q = c * d_i;   g_fake[i] = plain + (-(c * e_i));   c = (2 weight) / B
// one_sided: an element whose unclamped difference is not >= 0 (negative, or a NaN) adds +0.0f instead - clamp's gradient mask.
struct LecamTerm {
    float value;          // d_i or e_i as it enters R
    bool passes;          // the gradient mask
};

__device__ __forceinline__ LecamTerm lecam_term(float minuend, float subtrahend, bool one_sided) {
#pragma clang fp contract(off)
    const float raw = minuend - subtrahend;
    LecamTerm out;
    out.value = one_sided ? hinge_clamp(raw) : raw;
    out.passes = !one_sided || raw >= 0.0f;
    return out;
}

__device__ __forceinline__ float lecam_grad(float plain, float c, LecamTerm term, bool negate) {
#pragma clang fp contract(off)
    float q = c * term.value;
    if (negate) q = -q;
    return plain + (term.passes ? q : 0.0f);
}

__device__ __forceinline__ float lecam_total(float d_error, float pen, float weight, float R) {
#pragma clang fp contract(off)
    const float plain = d_error + pen;
    const float wr = weight * R;
    return plain + wr;
}

// the sums of one pass behind ONE pair of barriers (common.h, block_sums; csrc/topk.hip shares it): every sum has block_sum's bits
template <int N>
__device__ __forceinline__ void lecam_block_sums(double (&v)[N], double* scratch) {
    block_sums<N, LECAM_THREADS / 64>(v, scratch);
}

__global__ void __launch_bounds__(LECAM_THREADS) d_loss_lecam_kernel(const float* __restrict__ t, const float* __restrict__ f,
                                                                     const float* __restrict__ a, int B, float gamma,
                                                                     const unsigned* __restrict__ state, float weight, int one_sided,
                                                                     unsigned warmup, float* __restrict__ losses, float* __restrict__ gt,
                                                                     float* __restrict__ gf, float* __restrict__ ga) {
    __shared__ double scratch[5 * LECAM_THREADS / 64];
    // the three words in one request ahead of the branch: behind a cold cache every dependent load is another trip to memory
    const unsigned word_r = state[0], word_f = state[1], accepted = state[2];
    const bool active = weight != 0.0f && accepted >= (warmup > 1u ? warmup : 1u);          // uniform over the block
    if (!active) {
        d_loss_plain(t, f, a, B, gamma, losses, gt, gf, ga, scratch);
        if (threadIdx.x == 0) losses[3] = 0.0f;
        return;
    }
    const float alpha_r = __uint_as_float(word_r), alpha_f = __uint_as_float(word_f);
    const bool clamp = one_sided != 0;
    double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // hinge, t, a, d^2, e^2
    for (int i = threadIdx.x; i < B; i += LECAM_THREADS) {
        const float ti = t[i], fi = f[i];
        sums[0] += d_hinge_term(ti, fi);
        sums[1] += ti;
        sums[2] += a[i];
        const double d = (double)lecam_term(ti, alpha_f, clamp).value, e = (double)lecam_term(alpha_r, fi, clamp).value;
        sums[3] += d * d;          // a product of two fp32 is exact in float64: nothing to contract
        sums[4] += e * e;
    }
    lecam_block_sums<5>(sums, scratch);
    const double hs = sums[0], ts = sums[1], as = sums[2], ds = sums[3], es = sums[4];
    const DLossScalars s = d_loss_scalars(hs, ts, as, B, gamma);
    const float c = 2.0f * weight * s.invB;
    for (int i = threadIdx.x; i < B; i += LECAM_THREADS) {
        const float ti = t[i], fi = f[i];
        gt[i] = lecam_grad(d_grad_true(ti, s), c, lecam_term(ti, alpha_f, clamp), false);
        gf[i] = lecam_grad(d_grad_fake(fi, s), c, lecam_term(alpha_r, fi, clamp), true);
        ga[i] = -s.pen_g;
    }
    if (threadIdx.x == 0) {
        const float R = (float)(ds / B) + (float)(es / B);
        losses[0] = s.d_error;
        losses[1] = s.pen;
        losses[2] = lecam_total(s.d_error, s.pen, weight, R);
        losses[3] = R;
    }
}

// ---- observe: one block -----------------------------------------------------------------------------------------------------------------
// m_R = (float)(sum t_i / B), m_F = (float)(sum -g_i / B) for g = the step's out["d_gen"] = -f (the negation is exact).  Both finite:
// the first accepted observation SETS the anchors, later ones move them by rate * (m - alpha), three fp32 operations as
// csrc/average.hip's.  A non-finite mean, or an update that would leave an anchor non-finite, moves nothing and counts one refusal.
__device__ __forceinline__ float lecam_ema(float a, float m, float w) {
#pragma clang fp contract(off)
    const float d = m - a;
    const float wd = w * d;
    return a + wd;
}

__device__ __forceinline__ bool lecam_finite(float v) { return fabsf(v) <= 3.402823466e38f; }          // false for a NaN

__global__ void __launch_bounds__(LECAM_THREADS) lecam_observe_kernel(const float* __restrict__ t, const float* __restrict__ g, int B,
                                                                      int iteration, unsigned* __restrict__ state,
                                                                      unsigned* __restrict__ ring, int capacity, float rate) {
    __shared__ double scratch[2 * LECAM_THREADS / 64];
    double sums[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < B; i += LECAM_THREADS) {
        sums[0] += t[i];
        sums[1] += -g[i];
    }
    lecam_block_sums<2>(sums, scratch);
    if (threadIdx.x != 0) return;
    const float m_r = (float)(sums[0] / B), m_f = (float)(sums[1] / B);
    float alpha_r = __uint_as_float(state[0]), alpha_f = __uint_as_float(state[1]);
    unsigned accepted = state[2], refused = state[4];
    const unsigned rows = state[5];
    unsigned took = 0u;
    if (lecam_finite(m_r) && lecam_finite(m_f)) {
        const float new_r = accepted == 0u ? m_r : lecam_ema(alpha_r, m_r, rate);
        const float new_f = accepted == 0u ? m_f : lecam_ema(alpha_f, m_f, rate);
        if (lecam_finite(new_r) && lecam_finite(new_f)) {
            alpha_r = new_r;
            alpha_f = new_f;
            took = 1u;
        }
    }
    accepted += took;
    refused += 1u - took;
    unsigned* row = ring + (size_t)(rows % (unsigned)capacity) * LECAM_RING_WORDS;
    row[0] = (unsigned)iteration;
    row[1] = __float_as_uint(alpha_r);
    row[2] = __float_as_uint(alpha_f);
    row[3] = __float_as_uint(m_r);
    row[4] = __float_as_uint(m_f);
    row[5] = took;
    row[6] = 0u;
    row[7] = 0u;
    state[0] = __float_as_uint(alpha_r);
    state[1] = __float_as_uint(alpha_f);
    state[2] = accepted;
    state[3] = state[3] + 1u;
    state[4] = refused;
    state[5] = rows + 1u;
    state[6] = __float_as_uint(m_r);
    state[7] = __float_as_uint(m_f);
}

// ---- host entries -----------------------------------------------------------------------------------------------------------------------
static bool lecam_finite_host(float v) { return v == v && v - v == 0.0f; }

// d_true, d_fake, d_aug: fp32 [B] raw logits; state: the record above (read only); losses: 4 floats {d_error, penalty, total, R};
// g_*: [B] gradients of the total w.r.t. each D output.  Active iff weight != 0 and word 2 of the record >= max(warmup, 1).
// Writes losses[0 .. 4) and the three gradients and nothing else.
LOCATE_API int locate_d_loss_lecam(const float* d_true, const float* d_fake, const float* d_aug, int B, float gamma, const void* state,
                                   float weight, int one_sided, int warmup, float* losses, float* g_true, float* g_fake, float* g_aug,
                                   void* stream) {
    LOCATE_REQUIRE(d_true && d_fake && d_aug && state && losses && g_true && g_fake && g_aug, "locate_d_loss_lecam: null buffers");
    LOCATE_REQUIRE(B > 0 && warmup >= 0, "locate_d_loss_lecam: B = %d must be positive, warmup = %d not negative", B, warmup);
    LOCATE_REQUIRE(lecam_finite_host(weight), "locate_d_loss_lecam: weight %g must be finite", (double)weight);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(d_true) | reinterpret_cast<uintptr_t>(d_fake) | reinterpret_cast<uintptr_t>(d_aug) |
                     reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(losses) | reinterpret_cast<uintptr_t>(g_true) |
                     reinterpret_cast<uintptr_t>(g_fake) | reinterpret_cast<uintptr_t>(g_aug)) & 3) == 0,
                   "locate_d_loss_lecam: buffers must be 4-byte aligned");
    d_loss_lecam_kernel<<<1, LECAM_THREADS, 0, as_stream(stream)>>>(d_true, d_fake, d_aug, B, gamma, static_cast<const unsigned*>(state), weight,
                                                                    one_sided, (unsigned)warmup, losses, g_true, g_fake, g_aug);
    LOCATE_LAUNCH_CHECK("locate_d_loss_lecam");
    return LOCATE_OK;
}

// d_true: fp32 [B], D(real); d_gen: fp32 [B], MINUS D(G(z)) (the step's out["d_gen"]); ring: `capacity` rows of 8 words; rate:
// fp32(1 - decay).  Writes the state record and one ring row.
LOCATE_API int locate_lecam_observe(const float* d_true, const float* d_gen, int B, int iteration, void* state, void* ring, int capacity,
                                    float rate, void* stream) {
    LOCATE_REQUIRE(d_true && d_gen && state && ring, "locate_lecam_observe: null buffers");
    LOCATE_REQUIRE(B > 0 && capacity > 0, "locate_lecam_observe: B = %d, capacity = %d must be positive", B, capacity);
    LOCATE_REQUIRE(lecam_finite_host(rate) && rate >= 0.0f && rate <= 1.0f, "locate_lecam_observe: rate %g must be in [0, 1]", (double)rate);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(d_true) | reinterpret_cast<uintptr_t>(d_gen) | reinterpret_cast<uintptr_t>(state) |
                     reinterpret_cast<uintptr_t>(ring)) & 3) == 0,
                   "locate_lecam_observe: buffers must be 4-byte aligned");
    lecam_observe_kernel<<<1, LECAM_THREADS, 0, as_stream(stream)>>>(d_true, d_gen, B, iteration, static_cast<unsigned*>(state),
                                                                     static_cast<unsigned*>(ring), capacity, rate);
    LOCATE_LAUNCH_CHECK("locate_lecam_observe");
    return LOCATE_OK;
}
