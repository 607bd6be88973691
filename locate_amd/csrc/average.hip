// Exponential moving average of a network's weights (locate_amd/average.py): avg <- avg + (1 - beta) (src - avg) for every tensor
// of a network in ONE launch driven by a chunk table (multitensor.h) - a kernel of its own that runs BETWEEN two training
// iterations, so nothing the training step runs is touched.  The reference has no averaged generator.
//
// The arithmetic is pinned: three IEEE fp32 operations, each rounded once, never contracted into an fma - so
//   d = src - avg;  d = w * d;  avg = avg + d      (numpy float32, tests/helpers/average_model.py)
// reproduces the kernel bit for bit.  A tensor whose weight w = 1 - beta is exactly 1 is COPIED bit for bit (a + (s - a) is not s
// in floating point; NaN and Inf payloads survive): the spectral-norm u / v of the average follow the live network that way.
//
// A pure bandwidth kernel (12 bytes per element, 3 operations): 16-byte loads and stores, a full chunk's eight loads in flight
// per thread before the first use, at most 2048 blocks (256 CUs x 8) that stride over the chunk table.
#include "multitensor.h"

struct AverageTensor {
    float* avg;
    const float* src;
    long long n;
    float one_minus_beta;          // == 1.0f: exact copy
};

// __fadd_rn(a, __fmul_rn(w, __fsub_rn(s, a))) - written with the plain operators under `fp contract(off)`: the __f*_rn wrappers are
// plain operators compiled in the header's contraction mode, and the backend fused their multiply and add into one fma here.
__device__ __forceinline__ float ema_f(float a, float s, float w) {
#pragma clang fp contract(off)
    const float d = s - a;
    const float wd = w * d;
    return a + wd;
}

__device__ __forceinline__ float4 ema_f4(float4 a, float4 s, float w) {
    return make_float4(ema_f(a.x, s.x, w), ema_f(a.y, s.y, w), ema_f(a.z, s.z, w), ema_f(a.w, s.w, w));
}

__global__ void __launch_bounds__(MT_THREADS) average_update_kernel(const AverageTensor* __restrict__ tensors,
                                                                     const int2* __restrict__ chunks, int n_tensors, int n_chunks) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        AverageTensor T;
        long long begin;
        int len;
        if (!mt_decode(tensors, n_tensors, chunks[c], T, begin, len)) continue;          // a damaged table writes nothing
        const long long end = begin + len;
        const float w = T.one_minus_beta;
        const bool copy = w == 1.0f;          // uniform per tensor
        float* avg = T.avg;
        const float* src = T.src;
        // chunk starts are multiples of 16 bytes: the chunk is aligned where both base pointers are
        const bool vec = ((reinterpret_cast<uintptr_t>(avg + begin) | reinterpret_cast<uintptr_t>(src + begin)) & 15) == 0;
        if (!vec) {
            if (copy) {
                const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
                unsigned* a1 = reinterpret_cast<unsigned*>(avg);
                for (long long i = begin + threadIdx.x; i < end; i += MT_THREADS) a1[i] = s1[i];
            } else {
                for (long long i = begin + threadIdx.x; i < end; i += MT_THREADS) avg[i] = ema_f(avg[i], src[i], w);
            }
            continue;
        }
        const int n4 = len >> 2;
        if (copy) {
            const uint4* s4 = reinterpret_cast<const uint4*>(src + begin);
            uint4* a4 = reinterpret_cast<uint4*>(avg + begin);
            for (int i = threadIdx.x; i < n4; i += MT_THREADS) a4[i] = s4[i];
            const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
            unsigned* a1 = reinterpret_cast<unsigned*>(avg);
            for (long long i = begin + ((long long)n4 << 2) + threadIdx.x; i < end; i += MT_THREADS) a1[i] = s1[i];
            continue;
        }
        const float4* s4 = reinterpret_cast<const float4*>(src + begin);
        float4* a4 = reinterpret_cast<float4*>(avg + begin);
        if (n4 == MT_CHUNK / 4) {          // a full chunk: every load issued before the first use
            float4 a[MT_PER_THREAD], s[MT_PER_THREAD];
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) {
                a[k] = a4[threadIdx.x + k * MT_THREADS];
                s[k] = s4[threadIdx.x + k * MT_THREADS];
            }
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) a4[threadIdx.x + k * MT_THREADS] = ema_f4(a[k], s[k], w);
            continue;
        }
        for (int i = threadIdx.x; i < n4; i += MT_THREADS) a4[i] = ema_f4(a4[i], s4[i], w);
        for (long long i = begin + ((long long)n4 << 2) + threadIdx.x; i < end; i += MT_THREADS) avg[i] = ema_f(avg[i], src[i], w);
    }
}

LOCATE_API size_t locate_average_record_bytes(void) { return sizeof(AverageTensor); }
LOCATE_API int locate_average_chunk_elems(void) { return MT_CHUNK; }

// tensors: DEVICE array of n_tensors records {avg, src, n, one_minus_beta}; chunks: DEVICE array of n_chunks (tensor index,
// chunk index) int pairs covering every tensor in locate_average_chunk_elems() pieces.  No allocation, no host read, no
// synchronisation: legal under stream capture.  Writes [avg, avg + n) of every record and nothing else.
LOCATE_API int locate_average_update(const void* tensors, const void* chunks, int n_tensors, int n_chunks, void* stream) {
    LOCATE_REQUIRE(tensors && chunks && n_tensors > 0 && n_chunks > 0, "locate_average_update: bad arguments");
    average_update_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(static_cast<const AverageTensor*>(tensors),
                                                                       static_cast<const int2*>(chunks), n_tensors, n_chunks);
    LOCATE_LAUNCH_CHECK("locate_average_update");
    return LOCATE_OK;
}
