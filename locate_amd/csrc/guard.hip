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
// No floating-point atomics: every sum has a fixed order (multitensor.h's reduction, shared with stats.hip), so two steps over the
// same gradients at the same addresses reach the same verdict bit for bit.  Unlike stats.hip's records the sum DOES depend on a
// tensor's alignment: a tensor that is only 4-byte aligned (the data-parallel bucket views) is read with 16-byte loads between a
// scalar head and tail, so the 16-byte words fall on other elements than in an aligned tensor and the additions associate
// differently (within n 2^-52 relative either way).
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

__global__ void __launch_bounds__(MT_THREADS) guard_reduce_kernel(const GuardTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                 int n_tensors, int n_chunks, MtPartial* __restrict__ partials) {
    __shared__ MtPartial lds[MT_WAVES];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        double s = 0.0;
        unsigned amax = 0u, cnt = 0u;          // the shared reduction without its maximum: the partials' absmax stays 0
        GuardTensor T;
        long long begin;
        int len;
        // a damaged table entry contributes nothing (and reads nothing); its partial is still written: the verdict adds them all
        if (mt_decode(tensors, n_tensors, chunks[c], T, begin, len)) {
            const float* x = T.g + begin;
            // elements up to the first 16-byte boundary (0 .. 3 of them), 16-byte words, the rest (0 .. 3)
            int head = (int)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2;
            if (head > len) head = len;
            const int n4 = (len - head) >> 2;
            const int tail = len - head - 4 * n4;
            const float4* x4 = reinterpret_cast<const float4*>(x + head);
            const float* xt = x + head + 4 * n4;
            float4 v[MT_PER_THREAD];
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) {          // every load issued before the first use
                const int w = threadIdx.x + k * MT_THREADS;
                v[k] = w < n4 ? x4[w] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // +0.0 changes neither result
            }
            const float h = (int)threadIdx.x < head ? x[threadIdx.x] : 0.0f;
            const float t = (int)threadIdx.x < tail ? xt[threadIdx.x] : 0.0f;
            mt_take<false>(h, s, amax, cnt);
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) mt_take4<false>(v[k], s, amax, cnt);
            mt_take<false>(t, s, amax, cnt);
        }
        const MtPartial r = mt_block_reduce<false>(s, amax, cnt, lds);
        if (threadIdx.x == 0) partials[c] = r;          // c < n_chunks: inside the workspace
    }
}

// the count is kept in 64 bits from here on (a chunk's fits 32), so the block's last stage is this kernel's own
__global__ void __launch_bounds__(MT_THREADS) guard_verdict_kernel(const MtPartial* __restrict__ partials, int n_chunks,
                                                                  GuardVerdict* __restrict__ verdict, double max_norm, int skip_nonfinite) {
    __shared__ double lds_s[MT_WAVES];
    __shared__ unsigned long long lds_c[MT_WAVES];
    double s = 0.0;
    unsigned amax = 0u;
    unsigned long long cnt = 0ull;
    mt_add_partials(partials, n_chunks, s, amax, cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        cnt += (unsigned long long)__shfl_xor((long long)cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        lds_s[threadIdx.x >> 6] = s;
        lds_c[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    s = lds_s[0];
    cnt = lds_c[0];
#pragma unroll
    for (int w = 1; w < MT_WAVES; ++w) {
        s += lds_s[w];
        cnt += lds_c[w];
    }
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
LOCATE_API size_t locate_guard_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(MtPartial) : 0; }

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
                                                                           n_grads, n_grad_chunks, static_cast<MtPartial*>(workspace));
        LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(reduce)");
        guard_verdict_kernel<<<1, MT_THREADS, 0, st>>>(static_cast<const MtPartial*>(workspace), n_grad_chunks, V, max_norm, skip_nonfinite);
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
