// Guarded Nadam step (locate_amd/guard.py): the multi-tensor Nadam step of nadam.hip behind a verdict that is taken ON THE DEVICE
// from the gradients the step is about to consume - skip the step when a gradient holds NaN or Inf, scale the gradients down when
// their global norm exceeds a limit.  One stream, no host read, no allocation: the whole step can sit inside a captured hipGraph and
// the decision is taken anew at every replay.  The reference has nothing of the kind; nadam.hip stays the default.
//
// The unit is one optimizer, all its parameter groups together.  Per step:
//   (1) guard_reduce_kernel    one pass over every gradient, driven by a chunk table (multitensor.h): a block per 4096-element
//                              chunk (at most 2048 blocks stride over the chunk table) writes the float64 sum of the exact squares
//                              of the chunk's FINITE elements and the count of elements whose exponent field is all ones to
//                              partials[chunk position];
//   (2) guard_verdict_kernel   one block adds the partials in a fixed order and writes the verdict record (GuardVerdict below);
//   (3) guarded_schedule_kernel / guarded_update_kernel, once per parameter group: nadam.hip's pair, reading the verdict.
// No floating-point atomics: every sum has a fixed order (multitensor.h's mt_block_total and mt_add_partials), so two steps over
// the same gradients at the same addresses reach the same verdict bit for bit.  Unlike the statistics' records the sum DOES depend
// on a tensor's alignment: a chunk is read split at the 16-byte boundaries (multitensor.h's mt_read_split: a tensor that is only
// 4-byte aligned, as the data-parallel bucket views are, is read with 16-byte loads between a per-word head and tail), so the
// 16-byte words fall on other elements than in an aligned tensor and the additions associate differently (within n 2^-52
// relative either way).
//
// The update: g' = g * scale is ONE separately rounded fp32 multiply (never fused into the operations behind it), then Nadam's
// arithmetic runs on g': both steps instantiate the one spelled-out element of nadam_step.h.  Weight decay is added after the scaling,
// as torch's clip_grad_norm_ followed by an optimizer step does.  scale == 1.0f leaves every g as it is, so an idle guard is Nadam bit
// for bit.  The gradient itself is only read.  A skipped step writes nothing but the largest-magnitude words (common.h): the schedule
// kernel clears them and the update kernel streams p to fold max |p| in again, so the words hold the maximum of the parameter version
// the step stamps, as after every Nadam step.
#include "nadam_step.h"

struct GuardTensor {
    const float* g;
    long long n;
};

struct GuardVerdict {               // 64 bytes, 8-byte aligned; the counters run from the record's zero state
    double norm;                    // sqrt of the sum of squares of the finite gradient elements
    unsigned long long nonfinite;   // gradient elements that are NaN or +-Inf
    float scale;                    // what every gradient is multiplied by: max_norm / norm, or exactly 1
    int skip;                       // 1: this step writes no weight and no state
    long long steps;                // verdicts taken
    long long skipped;              // ... of which skip == 1
    long long clipped;              // ... of which scale came from max_norm / norm
    long long consecutive_skips;    // skipped steps since the last step that was taken
    double sumsq;                   // the total norm is the root of
};

// MtPartial's layout with an add() that leaves the maximum out: the verdict never reads it, carrying it cost the step 2.2 us
// (multitensor.h, mt_take), and the partials' absmax stays 0
struct GuardPartial {
    double sumsq;
    unsigned absmax;
    unsigned nonfinite;
    __device__ __forceinline__ void add(const GuardPartial& q) {
        sumsq += q.sumsq;
        nonfinite += q.nonfinite;
    }
};
static_assert(sizeof(GuardPartial) == sizeof(MtPartial), "the guard's workspace holds MtPartial-sized records");

struct GuardTotal {          // the count is kept in 64 bits from the verdict on (a chunk's fits 32)
    double sumsq;
    unsigned long long nonfinite;
    __device__ __forceinline__ void add(const GuardPartial& q) {
        sumsq += q.sumsq;
        nonfinite += q.nonfinite;
    }
    __device__ __forceinline__ void add(const GuardTotal& q) {
        sumsq += q.sumsq;
        nonfinite += q.nonfinite;
    }
};

__global__ void __launch_bounds__(MT_THREADS) guard_reduce_kernel(const GuardTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                 int n_tensors, int n_chunks, GuardPartial* __restrict__ partials) {
    __shared__ GuardPartial lds[MT_WAVES];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        GuardPartial r = {0.0, 0u, 0u};
        GuardTensor T;
        long long begin;
        int len;
        // a damaged table entry contributes nothing (and reads nothing); its partial is still written: the verdict adds them all
        if (mt_decode(tensors, n_tensors, chunks[c], T, begin, len)) {
            const float* x = T.g + begin;
            mt_word4<float> v[MT_PER_THREAD];
            float h, t;
            mt_read_split(x, mt_split(x, len), v, h, t);          // +0.0 where the chunk has no word: it changes neither result
            mt_take<false>(h, r.sumsq, r.absmax, r.nonfinite);
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) mt_take4<false>(v[k], r.sumsq, r.absmax, r.nonfinite);
            mt_take<false>(t, r.sumsq, r.absmax, r.nonfinite);
        }
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) partials[c] = r;          // c < n_chunks: inside the workspace
    }
}

__global__ void __launch_bounds__(MT_THREADS) guard_verdict_kernel(const GuardPartial* __restrict__ partials, int n_chunks,
                                                                  GuardVerdict* __restrict__ verdict, double max_norm, int skip_nonfinite) {
    __shared__ GuardTotal lds[MT_WAVES];
    GuardTotal total = {0.0, 0ull};
    mt_add_partials(partials, n_chunks, total);
    total = mt_block_total(total, lds);
    if (threadIdx.x != 0) return;
    const double s = total.sumsq;
    const unsigned long long cnt = total.nonfinite;
    GuardVerdict V = *verdict;
    const double norm = sqrt(s);
    const int skip = skip_nonfinite && cnt > 0ull ? 1 : 0;
    const bool clip = max_norm > 0.0 && norm > max_norm && !skip;
    V.norm = norm;
    V.sumsq = s;
    V.nonfinite = cnt;
    V.skip = skip;
    V.scale = clip ? (float)(max_norm / norm) : 1.0f;
    V.steps += 1;
    V.skipped += skip;
    V.clipped += clip ? 1 : 0;
    V.consecutive_skips = skip ? V.consecutive_skips + 1 : 0;
    *verdict = V;
}

// nadam_step.h's pair behind the verdict
__global__ void __launch_bounds__(64) guarded_schedule_kernel(const NadamTensor* __restrict__ tensors, NadamCoef* __restrict__ coef,
                                                              int n_tensors, double lr, double b1, double b2, double sd,
                                                              const GuardVerdict* __restrict__ verdict) {
    nadam_schedule(tensors, coef, n_tensors, lr, b1, b2, sd, verdict->skip == 0);
}

__global__ void __launch_bounds__(256) guarded_update_kernel(const NadamTensor* __restrict__ tensors, const NadamCoef* __restrict__ coef,
                                                             const int2* __restrict__ chunks, float b1, float b2, float eps, float wd,
                                                             const GuardVerdict* __restrict__ verdict) {
    nadam_update<true>(tensors, coef, chunks, b1, b2, eps, wd, verdict->skip, verdict->scale);
}

LOCATE_API size_t locate_guard_tensor_record_bytes(void) { return sizeof(GuardTensor); }
LOCATE_API size_t locate_guard_verdict_bytes(void) { return sizeof(GuardVerdict); }
LOCATE_API int locate_guard_chunk_elems(void) { return MT_CHUNK; }
LOCATE_API int locate_guard_max_blocks(void) { return mt_grid(0x7fffffff); }
LOCATE_API size_t locate_guard_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(GuardPartial) : 0; }

// One optimizer step behind a verdict.
//   grads / grad_chunks: DEVICE array of n_grads {const float* g; int64 n} records over EVERY gradient of the optimizer, and the
//     n_grad_chunks (tensor index, chunk index) int pairs that cover them in locate_guard_chunk_elems() pieces.  With n_grads > 0 the
//     reduce and the verdict run first; with n_grads == 0 (grads, grad_chunks and workspace NULL, n_grad_chunks 0) the verdict the
//     record already holds is applied - the second and later parameter groups of the same step.
//   workspace: locate_guard_workspace_bytes(n_grad_chunks) bytes, 8-byte aligned, need not be zeroed.
//   verdict: locate_guard_verdict_bytes() = 64 bytes, 8-byte aligned, zeroed once by the caller; read and written.
//   max_norm: 0 = no clipping; skip_nonfinite: 0 = take the step whatever the gradients hold.
//   tensors, coef, chunks, n_tensors, n_chunks and the hyper-parameters: as locate_nadam_step, for ONE parameter group.
LOCATE_API int locate_guarded_nadam_step(const void* grads, const void* grad_chunks, int n_grads, int n_grad_chunks, void* workspace,
                                         void* verdict, double max_norm, int skip_nonfinite, const void* tensors, void* coef,
                                         const void* chunks, int n_tensors, int n_chunks, double lr, double beta1, double beta2, double eps,
                                         double schedule_decay, double weight_decay, void* stream) {
    LOCATE_REQUIRE(tensors && coef && chunks && verdict && n_tensors > 0 && n_chunks > 0, "locate_guarded_nadam_step: bad arguments");
    LOCATE_REQUIRE(n_grads >= 0 && (n_grads > 0 ? grads && grad_chunks && workspace && n_grad_chunks > 0
                                                : !grads && !grad_chunks && !workspace && n_grad_chunks == 0),
                   "locate_guarded_nadam_step: the gradient table, its chunks and the workspace come together with positive counts, or not at all");
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(verdict) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                   "locate_guarded_nadam_step: the verdict record and the workspace need 8-byte alignment");
    LOCATE_REQUIRE(max_norm >= 0.0 && max_norm <= 1.7976931348623157e308, "locate_guarded_nadam_step: max_norm must be finite and >= 0");
    hipStream_t st = as_stream(stream);
    GuardVerdict* V = static_cast<GuardVerdict*>(verdict);
    if (n_grads > 0) {
        guard_reduce_kernel<<<mt_grid(n_grad_chunks), MT_THREADS, 0, st>>>(static_cast<const GuardTensor*>(grads), static_cast<const int2*>(grad_chunks),
                                                                           n_grads, n_grad_chunks, static_cast<GuardPartial*>(workspace));
        LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(reduce)");
        guard_verdict_kernel<<<1, MT_THREADS, 0, st>>>(static_cast<const GuardPartial*>(workspace), n_grad_chunks, V, max_norm, skip_nonfinite);
        LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(verdict)");
    }
    guarded_schedule_kernel<<<(n_tensors + 63) / 64, 64, 0, st>>>(static_cast<const NadamTensor*>(tensors), static_cast<NadamCoef*>(coef),
                                                                  n_tensors, lr, beta1, beta2, schedule_decay, V);
    LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(schedule)");
    guarded_update_kernel<<<n_chunks, 256, 0, st>>>(static_cast<const NadamTensor*>(tensors), static_cast<const NadamCoef*>(coef),
                                                    static_cast<const int2*>(chunks), (float)beta1, (float)beta2, (float)eps, (float)weight_decay, V);
    LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(update)");
    return LOCATE_OK;
}
