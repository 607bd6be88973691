// Guarded Nadam step (locate_amd/guard.py): the multi-tensor Nadam step of nadam.hip behind a verdict that is taken ON THE DEVICE
// from the gradients the step is about to consume - skip the step when a gradient holds NaN or Inf, scale the gradients down when
// their global norm exceeds a limit.  One stream, no host read, no allocation: the whole step can sit inside a captured hipGraph and
// the decision is taken anew at every replay.  The reference has nothing of the kind; nadam.hip stays the default and is untouched.
//
// The unit is one optimizer, all its parameter groups together.  Per step:
//   (1) guard_reduce_kernel    one pass over every gradient, driven by a device table: a block per 4096-element chunk (at most 2048
//                              blocks stride over the chunk table) writes the float64 sum of the exact squares of the chunk's FINITE
//                              elements and the count of elements whose exponent field is all ones to partials[chunk position];
//   (2) guard_verdict_kernel   one block adds the partials in a fixed order and writes the verdict record (GuardVerdict below);
//   (3) guarded_schedule_kernel / guarded_update_kernel, once per parameter group: nadam.hip's pair, reading the verdict.
// No floating-point atomics: every sum has a fixed order (a thread's elements in index order, a wave by a butterfly, the block's four
// waves in order, partial p on thread p % 256 in ascending order), so two steps over the same gradients at the same addresses reach
// the same verdict bit for bit.  Unlike stats.hip's records the sum DOES depend on a tensor's alignment: a tensor that is only 4-byte
// aligned (the data-parallel bucket views) is read with 16-byte loads between a scalar head and tail, so the 16-byte words fall on
// other elements than in an aligned tensor and the additions associate differently (within n 2^-52 relative either way).
//
// The update: g' = g * scale is ONE separately rounded fp32 multiply (never fused into the operations behind it), then nadam.hip's
// arithmetic runs on g', rounding for rounding (guarded_nadam_element below); weight decay is added after the scaling, as torch's
// clip_grad_norm_ followed by an optimizer step does.  scale == 1.0f leaves every g as it is, so an idle guard is Nadam bit for bit.
// The gradient itself is only read.  A skipped step writes nothing but the largest-magnitude words (common.h): the schedule kernel
// clears them and the update kernel streams p to fold max |p| in again, so the words hold the maximum of the parameter version the
// step stamps, as after every Nadam step.
#include "common.h"

struct GuardTensor {
    const float* g;
    long long n;
};

struct GuardPartial {
    double sumsq;
    unsigned nonfinite;
    unsigned pad;
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

// same layout as nadam.hip's records: the Python side builds one table format for both steps
struct GuardedNadamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    double* sched;     // [2]: step count, m_schedule
    long long n;
    unsigned* absmax;  // nullable, see nadam.hip
};

struct GuardedNadamCoef {
    float c_grad, c_mom, bias2, pad;
};

#define GUARD_CHUNK 4096
#define GUARD_THREADS 256
#define GUARD_WAVES (GUARD_THREADS / 64)
#define GUARD_PER_THREAD (GUARD_CHUNK / 4 / GUARD_THREADS)          // 16-byte words per thread in a full chunk
#define GUARD_MAX_BLOCKS 2048

__device__ __forceinline__ void guard_take(float x, double& s, unsigned& c) {
    const bool finite = (__float_as_uint(x) & 0x7fffffffu) < 0x7f800000u;
    const double d = finite ? (double)x : 0.0;
    s = fma(d, d, s);          // d * d is exact in fp64: one rounding, that of the addition
    c += finite ? 0u : 1u;
}

// the block's total in thread 0 (other threads: unspecified); `lds` holds GUARD_WAVES partials
__device__ __forceinline__ GuardPartial guard_block_reduce(double s, unsigned c, GuardPartial* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        c += (unsigned)__shfl_xor((int)c, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();          // lds may still be read from the previous chunk
    if (lane == 0) {
        lds[wid].sumsq = s;
        lds[wid].nonfinite = c;
    }
    __syncthreads();
    GuardPartial r = lds[0];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < GUARD_WAVES; ++w) {
            r.sumsq += lds[w].sumsq;
            r.nonfinite += lds[w].nonfinite;
        }
    }
    r.pad = 0u;
    return r;
}

__global__ void __launch_bounds__(GUARD_THREADS) guard_reduce_kernel(const GuardTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                    int n_tensors, int n_chunks, GuardPartial* __restrict__ partials) {
    __shared__ GuardPartial lds[GUARD_WAVES];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int2 ch = chunks[c];
        double s = 0.0;
        unsigned cnt = 0u;
        // a damaged table entry contributes nothing (and reads nothing); its partial is still written: the verdict adds them all
        if ((unsigned)ch.x < (unsigned)n_tensors && ch.y >= 0) {
            const GuardTensor T = tensors[ch.x];
            const long long begin = (long long)ch.y * GUARD_CHUNK;
            if (begin < T.n) {
                const int len = T.n - begin < GUARD_CHUNK ? (int)(T.n - begin) : GUARD_CHUNK;
                const float* x = T.g + begin;
                // elements up to the first 16-byte boundary (0 .. 3 of them), 16-byte words, the rest (0 .. 3)
                int head = (int)((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2;
                if (head > len) head = len;
                const int n4 = (len - head) >> 2;
                const int tail = len - head - 4 * n4;
                const float4* x4 = reinterpret_cast<const float4*>(x + head);
                const float* xt = x + head + 4 * n4;
                float4 v[GUARD_PER_THREAD];
#pragma unroll
                for (int k = 0; k < GUARD_PER_THREAD; ++k) {          // every load issued before the first use
                    const int w = threadIdx.x + k * GUARD_THREADS;
                    v[k] = w < n4 ? x4[w] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // +0.0 changes neither result
                }
                const float h = (int)threadIdx.x < head ? x[threadIdx.x] : 0.0f;
                const float t = (int)threadIdx.x < tail ? xt[threadIdx.x] : 0.0f;
                guard_take(h, s, cnt);
#pragma unroll
                for (int k = 0; k < GUARD_PER_THREAD; ++k) {
                    guard_take(v[k].x, s, cnt);
                    guard_take(v[k].y, s, cnt);
                    guard_take(v[k].z, s, cnt);
                    guard_take(v[k].w, s, cnt);
                }
                guard_take(t, s, cnt);
            }
        }
        const GuardPartial r = guard_block_reduce(s, cnt, lds);
        if (threadIdx.x == 0) partials[c] = r;          // c < n_chunks: inside the workspace
    }
}

__global__ void __launch_bounds__(GUARD_THREADS) guard_verdict_kernel(const GuardPartial* __restrict__ partials, int n_chunks,
                                                                     GuardVerdict* __restrict__ verdict, double max_norm, int skip_nonfinite) {
    __shared__ double lds_s[GUARD_WAVES];
    __shared__ unsigned long long lds_c[GUARD_WAVES];
    double s = 0.0;
    unsigned long long cnt = 0ull;
    for (int i = threadIdx.x; i < n_chunks; i += GUARD_THREADS) {
        s += partials[i].sumsq;
        cnt += partials[i].nonfinite;
    }
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
    for (int w = 1; w < GUARD_WAVES; ++w) {
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

// nadam_schedule_kernel behind the verdict: a skipped step leaves (step, m_schedule) alone and writes no coefficients
__global__ void __launch_bounds__(64) guarded_schedule_kernel(const GuardedNadamTensor* __restrict__ tensors, GuardedNadamCoef* __restrict__ coef,
                                                              int n_tensors, double lr, double b1, double b2, double sd,
                                                              const GuardVerdict* __restrict__ verdict) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tensors) return;
    const bool take = verdict->skip == 0;
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
        for (int k = 0; k < AMAX_LINES; ++k) tensors[i].absmax[k * AMAX_STRIDE] = 0u;      // the update kernel folds the maximum in, skipped or not
    GuardedNadamCoef c;
    c.c_grad = (float)(-lr * (1.0 - mc_t) / (1.0 - ms_new));
    c.c_mom = (float)(-lr * mc_t1 / (1.0 - ms_next));
    c.bias2 = (float)(1.0 - pow(b2, t));
    c.pad = 0.0f;
    if (take) coef[i] = c;
}

// One element of the update, every rounding spelled out.  nadam.hip leaves the contraction of its expressions to the compiler, and the
// same source inlined behind the scaling multiply was contracted another way (b1 * m fused, (1 - b1) * g rounded, instead of the
// reverse): the moments then differed from Nadam's in the last bit.  So this is nadam_update_kernel's arithmetic AS ITS OBJECT CODE
// COMPUTES IT, written under `fp contract(off)` with fmaf where that code fuses:
//   g' = rn(g * scale)                                   one rounding of its own;  g' = fma(wd, p, g') with weight decay
//   m  = fma(1 - b1, g', rn(b1 * m))                     v = rn(rn(rn((1 - b2) * g') * g') + rn(b2 * v))
//   p  = rn(rn(p + rn(c_grad * rn(g' / denom))) + rn(c_mom * rn(m / denom))),  denom = rn(sqrt(rn(v / bias2)) + eps)
// tests/test_gpu_guard.py holds it to Nadam's bits; should a compiler contract nadam.hip differently one day, that test says so.
__device__ __forceinline__ void guarded_nadam_element(float& p, float gin, float& m, float& v, float scale, float wd, float b1, float b2,
                                                      float omb1, float omb2, float eps, const GuardedNadamCoef& c) {
#pragma clang fp contract(off)
    const float gs = gin * scale;
    const float g = wd != 0.0f ? fmaf(wd, p, gs) : gs;          // nadam.py:65-66: grad + weight_decay * p
    const float mb = m * b1;
    m = fmaf(omb1, g, mb);
    const float vb = v * b2;
    const float og = omb2 * g;
    v = og * g + vb;
    const float denom = sqrtf(v / c.bias2) + eps;
    p = p + c.c_grad * (g / denom);
    p = p + c.c_mom * (m / denom);
}

__global__ void __launch_bounds__(256) guarded_update_kernel(const GuardedNadamTensor* __restrict__ tensors,
                                                             const GuardedNadamCoef* __restrict__ coef, const int2* __restrict__ chunks,
                                                             float b1, float b2, float eps, float wd, const GuardVerdict* __restrict__ verdict) {
    const int2 ch = chunks[blockIdx.x];
    const GuardedNadamTensor T = tensors[ch.x];
    const long long begin = (long long)ch.y * GUARD_CHUNK;
    long long end = begin + GUARD_CHUNK;
    if (end > T.n) end = T.n;
    __shared__ float scratch[16];
    float amax = 0.0f;
    if (verdict->skip) {          // block-uniform.  Only p is read, and only the words are written
        if (!T.absmax) return;
        for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) amax = fmaxf(amax, fabsf(T.p[i]));
        absmax_publish(amax, scratch, T.absmax);
        return;
    }
    const float scale = verdict->scale;
    const GuardedNadamCoef c = coef[ch.x];
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) {
        float p = T.p[i], m = T.m[i], v = T.v[i];
        guarded_nadam_element(p, T.g[i], m, v, scale, wd, b1, b2, omb1, omb2, eps, c);
        T.m[i] = m;
        T.v[i] = v;
        T.p[i] = p;
        amax = fmaxf(amax, fabsf(p));
    }
    if (T.absmax) absmax_publish(amax, scratch, T.absmax);          // wave-uniform condition: every thread of the block takes it
}

LOCATE_API size_t locate_guard_tensor_record_bytes(void) { return sizeof(GuardTensor); }
LOCATE_API size_t locate_guard_verdict_bytes(void) { return sizeof(GuardVerdict); }
LOCATE_API int locate_guard_chunk_elems(void) { return GUARD_CHUNK; }
LOCATE_API int locate_guard_max_blocks(void) { return GUARD_MAX_BLOCKS; }
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
        const int grid = n_grad_chunks < GUARD_MAX_BLOCKS ? n_grad_chunks : GUARD_MAX_BLOCKS;
        guard_reduce_kernel<<<grid, GUARD_THREADS, 0, st>>>(static_cast<const GuardTensor*>(grads), static_cast<const int2*>(grad_chunks), n_grads,
                                                            n_grad_chunks, static_cast<GuardPartial*>(workspace));
        LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(reduce)");
        guard_verdict_kernel<<<1, GUARD_THREADS, 0, st>>>(static_cast<const GuardPartial*>(workspace), n_grad_chunks, V, max_norm, skip_nonfinite);
        LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(verdict)");
    }
    guarded_schedule_kernel<<<(n_tensors + 63) / 64, 64, 0, st>>>(static_cast<const GuardedNadamTensor*>(tensors), static_cast<GuardedNadamCoef*>(coef),
                                                                  n_tensors, lr, beta1, beta2, schedule_decay, V);
    LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(schedule)");
    guarded_update_kernel<<<n_chunks, 256, 0, st>>>(static_cast<const GuardedNadamTensor*>(tensors), static_cast<const GuardedNadamCoef*>(coef),
                                                    static_cast<const int2*>(chunks), (float)beta1, (float)beta2, (float)eps, (float)weight_decay, V);
    LOCATE_LAUNCH_CHECK("locate_guarded_nadam_step(update)");
    return LOCATE_OK;
}
