// Adaptive discriminator augmentation (Karras et al. 2020, "Training Generative Adversarial Networks with Limited Data") around the
// differentiable augmentation of csrc/diffaug.hip: two small kernels that run BESIDE the training step (locate_amd/augment.py,
// AdaptiveDiffAugment; the definition in numpy, which both kernels equal with ==: tests/helpers/ada_model.py).
//
//   observe: the overfitting indicator r_t = E[sign(D(real))] over a window of `interval` batches, and the controller that moves the
//            augmentation probability p towards keeping r_t at `target`;
//   gate:    turns the host's uniforms into the per-image op mask that the diffaug kernels read from word 9 of a parameter row.
//
// The state is one record of ADA_STATE_WORDS 32-bit words at a fixed device address:
//   0 p (fp32)   1 r of the last closed window that counted a logit (fp32)   2 window sum (int32)   3 logits counted in the window
//   4 observations in the window   5 windows closed   6 ups   7 downs   8 NaN logits seen in all (mod 2^32)   9 ring rows written
//   in all (mod 2^32)   10 .. 15 zero.
// Both kernels: no allocation, no host read, no atomics, values written by ordinary vector stores; legal under stream capture
// (observe's `iteration` is a launch argument: a captured launch would repeat it).
#include "common.h"

#define ADA_ROW_WORDS 12          // a parameter row (diffaug.hip, DA_PARAMS)
#define ADA_GATE_WORD 9           // raw row: the uniforms of op 0, 1, 2 in words 9, 10, 11; gated row: the mask in word 9, then zeros
#define ADA_STATE_WORDS 16
#define ADA_RING_WORDS 4          // {iteration, r, p, logits counted in the window}
#define ADA_THREADS 256

// ---- gate: a thread per word of the output ------------------------------------------------------------------------------------------
// Words 0 .. 8 are copied as bit patterns.  Op k of the policy is applied iff g_k < p - strictly, so p = 0 applies nothing and a
// NaN uniform applies nothing; bit k of the mask is set where op k is in the policy and is NOT applied.
__global__ void __launch_bounds__(ADA_THREADS) ada_gate_kernel(const unsigned* __restrict__ raw, const unsigned* __restrict__ state,
                                                               unsigned* __restrict__ out, int n_words, int policy) {
    const int at = blockIdx.x * ADA_THREADS + threadIdx.x;
    if (at >= n_words) return;
    const int row = at / ADA_ROW_WORDS, word = at - row * ADA_ROW_WORDS;
    unsigned v = 0u;
    if (word < ADA_GATE_WORD) {
        v = raw[at];
    } else if (word == ADA_GATE_WORD) {
        const float p = __uint_as_float(state[0]);
        int mask = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float g = __uint_as_float(raw[at + k]);
            if ((policy >> k & 1) && !(g < p)) mask |= 1 << k;
        }
        v = __float_as_uint((float)mask);          // 0 .. 7: exact
    }
    out[at] = v;
}

// ---- observe: one block ---------------------------------------------------------------------------------------------------------------
// Adds #(x > 0) - #(x < 0) over the B logits to the window (+-0.0 count 0, +-Inf count as their sign, a NaN counts nowhere: it is
// left out of the sum and of the denominator), in integers: exact and independent of the order.  The interval-th observation closes
// the window: r = (float)((double)sum / (double)counted) if anything was counted; p moves by `step` towards the side r lies on, one
// fp32 addition clamped to [0, p_max] (p stays where it is for r == target and for a window without a counted logit); {iteration,
// r, p, counted} goes into the ring at row (rows written) % capacity; the window starts empty.
__device__ __forceinline__ float ada_move(float p, float step, float p_max) {
#pragma clang fp contract(off)
    const float q = p + step;
    return fminf(fmaxf(q, 0.0f), p_max);
}

__global__ void __launch_bounds__(ADA_THREADS) ada_observe_kernel(const float* __restrict__ logits, int B, int iteration,
                                                                  unsigned* __restrict__ state, unsigned* __restrict__ ring, int capacity,
                                                                  int interval, float target, float step, float p_max) {
    __shared__ int scratch[16];
    int sign_sum = 0, nans = 0;
    for (int i = threadIdx.x; i < B; i += ADA_THREADS) {
        const float x = logits[i];
        sign_sum += (x > 0.0f ? 1 : 0) - (x < 0.0f ? 1 : 0);
        nans += x != x ? 1 : 0;
    }
    sign_sum = block_sum<int>(sign_sum, scratch);
    nans = block_sum<int>(nans, scratch);
    if (threadIdx.x != 0) return;
    float p = __uint_as_float(state[0]), r = __uint_as_float(state[1]);
    int sum = (int)state[2] + sign_sum, counted = (int)state[3] + (B - nans), seen = (int)state[4] + 1;
    unsigned closed = state[5], ups = state[6], downs = state[7], rows = state[9];
    const unsigned nan_total = state[8] + (unsigned)nans;
    if (seen >= interval) {
        if (counted > 0) {
            r = (float)((double)sum / (double)counted);
            if (r > target) {
                p = ada_move(p, step, p_max);
                ups += 1u;
            } else if (r < target) {
                p = ada_move(p, -step, p_max);
                downs += 1u;
            }
        }
        unsigned* row = ring + (size_t)(rows % (unsigned)capacity) * ADA_RING_WORDS;
        row[0] = (unsigned)iteration;
        row[1] = __float_as_uint(r);
        row[2] = __float_as_uint(p);
        row[3] = (unsigned)counted;
        rows += 1u;
        closed += 1u;
        sum = counted = seen = 0;
    }
    state[0] = __float_as_uint(p);
    state[1] = __float_as_uint(r);
    state[2] = (unsigned)sum;
    state[3] = (unsigned)counted;
    state[4] = (unsigned)seen;
    state[5] = closed;
    state[6] = ups;
    state[7] = downs;
    state[8] = nan_total;
    state[9] = rows;
}

// ---- host entries ---------------------------------------------------------------------------------------------------------------------
// raw_rows, out_rows: fp32 [n, 12], distinct, 4-byte aligned; state: the record above.  Writes [out_rows, out_rows + 12 n) and
// nothing else.
LOCATE_API int locate_ada_gate(const float* raw_rows, const void* state, float* out_rows, int n, int policy, void* stream) {
    LOCATE_REQUIRE(raw_rows && state && out_rows && raw_rows != out_rows, "locate_ada_gate: null or aliased buffers");
    LOCATE_REQUIRE(n > 0 && n <= (1 << 24), "locate_ada_gate: n = %d is not in 1 .. 2^24", n);
    LOCATE_REQUIRE(policy >= 0 && policy < 8, "locate_ada_gate: policy %d has bits beyond colour | translation | cutout", policy);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(raw_rows) | reinterpret_cast<uintptr_t>(out_rows) | reinterpret_cast<uintptr_t>(state)) & 3) == 0,
                   "locate_ada_gate: buffers must be 4-byte aligned");
    const int n_words = n * ADA_ROW_WORDS;
    ada_gate_kernel<<<(n_words + ADA_THREADS - 1) / ADA_THREADS, ADA_THREADS, 0, as_stream(stream)>>>(
        reinterpret_cast<const unsigned*>(raw_rows), static_cast<const unsigned*>(state), reinterpret_cast<unsigned*>(out_rows), n_words, policy);
    LOCATE_LAUNCH_CHECK("locate_ada_gate");
    return LOCATE_OK;
}

// d_true: fp32 [B]; ring: `capacity` rows of 4 words.  B * interval < 2^31 keeps the window's integers exact.  Writes the state
// record and at most one ring row.
LOCATE_API int locate_ada_observe(const float* d_true, int B, int iteration, void* state, void* ring, int capacity, int interval, float target,
                                  float step, float p_max, void* stream) {
    LOCATE_REQUIRE(d_true && state && ring, "locate_ada_observe: null buffers");
    LOCATE_REQUIRE(B > 0 && interval > 0 && capacity > 0, "locate_ada_observe: B = %d, interval = %d, capacity = %d must be positive", B, interval,
                   capacity);
    LOCATE_REQUIRE((long long)B * (long long)interval < (1ll << 31), "locate_ada_observe: B * interval = %lld does not fit the window's int32",
                   (long long)B * (long long)interval);
    LOCATE_REQUIRE(target == target && step >= 0.0f && step < 1e30f && p_max > 0.0f && p_max <= 1.0f,
                   "locate_ada_observe: target %g, step %g, p_max %g: target must be a number, step finite and >= 0, p_max in (0, 1]", (double)target,
                   (double)step, (double)p_max);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(d_true) | reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(ring)) & 3) == 0,
                   "locate_ada_observe: buffers must be 4-byte aligned");
    ada_observe_kernel<<<1, ADA_THREADS, 0, as_stream(stream)>>>(d_true, B, iteration, static_cast<unsigned*>(state), static_cast<unsigned*>(ring),
                                                                  capacity, interval, target, step, p_max);
    LOCATE_LAUNCH_CHECK("locate_ada_observe");
    return LOCATE_OK;
}
