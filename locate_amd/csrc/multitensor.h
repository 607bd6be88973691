// What the kernels driven by a device chunk table share (nadam.hip, guard.hip, average.hip, stats.hip, parallel.hip): a table of
// per-tensor records (each kernel's own struct, with the element count in a member `n`) and a list of int2 {tensor, chunk} entries
// that covers every tensor in MT_CHUNK-element pieces (locate_amd/_tables.py builds both).  Here: the chunk size, the decode of an
// entry, the grid cap, and the fixed-order reduction the statistics and the guard are built from.
#pragma once
#include "common.h"

#define MT_CHUNK 4096
#define MT_THREADS 256
#define MT_WAVES (MT_THREADS / 64)
#define MT_PER_THREAD (MT_CHUNK / 4 / MT_THREADS)          // 16-byte words per thread in a full chunk
#define MT_ANY_TENSOR 0x7fffffff          // n_tensors of a kernel whose entry point carries no tensor count: any index >= 0 passes

// at most 2048 blocks (256 CUs x 8) that stride over the chunk table
static inline int mt_grid(int n_chunks) { return stream_grid(n_chunks, 1); }

#ifdef __HIPCC__
// Entry `ch` -> its tensor's record and the elements [begin, begin + len) of it, 0 < len <= MT_CHUNK.  false for a damaged entry
// (no such tensor, a negative chunk, a chunk past the tensor's end): nothing was read through it and nothing may be written.
template <typename Rec>
__device__ __forceinline__ bool mt_decode(const Rec* __restrict__ tensors, int n_tensors, int2 ch, Rec& T, long long& begin, int& len) {
    if ((unsigned)ch.x >= (unsigned)n_tensors || ch.y < 0) return false;
    T = tensors[ch.x];
    begin = (long long)ch.y * MT_CHUNK;
    if (begin >= T.n) return false;
    len = T.n - begin < MT_CHUNK ? (int)(T.n - begin) : MT_CHUNK;
    return true;
}

// ---- the reduction: sum of exact squares of the finite elements, their largest magnitude, the count of the others ----------------
// Every sum has one order - a thread's elements in index order, a wave by a butterfly, the block's four waves in order, partial p
// on thread p % 256 in ascending order - and no floating-point atomics: the determinism stats.hip and guard.hip document rests on
// these three functions.
struct MtPartial {          // a chunk's partial and a tensor's record alike
    double sumsq;
    unsigned absmax;          // bit pattern of a non-negative finite fp32
    unsigned nonfinite;
};

// WITH_MAX false leaves the maximum out (m stays what it was): the guard, which has no use for it, ran its two steps 2.2 us slower
// behind an iteration with the maximum carried along, against 0.6 us between the parent's own runs (profiles/notes_multitensor.md).
template <bool WITH_MAX = true>
__device__ __forceinline__ void mt_take(float x, double& s, unsigned& m, unsigned& c) {
    const unsigned mag = __float_as_uint(x) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    const double d = finite ? (double)x : 0.0;
    s = fma(d, d, s);          // d * d is exact in fp64: one rounding, that of the addition
    if (WITH_MAX) m = finite && mag > m ? mag : m;
    c += finite ? 0u : 1u;
}

template <bool WITH_MAX = true>
__device__ __forceinline__ void mt_take4(float4 v, double& s, unsigned& m, unsigned& c) {
    mt_take<WITH_MAX>(v.x, s, m, c);
    mt_take<WITH_MAX>(v.y, s, m, c);
    mt_take<WITH_MAX>(v.z, s, m, c);
    mt_take<WITH_MAX>(v.w, s, m, c);
}

// the block's total in thread 0 (other threads: unspecified); `lds` holds MT_WAVES records
template <bool WITH_MAX = true>
__device__ __forceinline__ MtPartial mt_block_reduce(double s, unsigned m, unsigned c, MtPartial* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        if (WITH_MAX) {
            const unsigned om = (unsigned)__shfl_xor((int)m, o, 64);
            m = om > m ? om : m;
        }
        c += (unsigned)__shfl_xor((int)c, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();          // lds may still be read from the previous chunk
    if (lane == 0) {
        lds[wid].sumsq = s;
        lds[wid].absmax = m;
        lds[wid].nonfinite = c;
    }
    __syncthreads();
    MtPartial r = lds[0];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MT_WAVES; ++w) {
            r.sumsq += lds[w].sumsq;
            if (WITH_MAX) r.absmax = lds[w].absmax > r.absmax ? lds[w].absmax : r.absmax;
            r.nonfinite += lds[w].nonfinite;
        }
    }
    return r;
}

// this thread's share of n partials: p[threadIdx.x], p[threadIdx.x + 256], ... added in ascending order
template <typename Count>
__device__ __forceinline__ void mt_add_partials(const MtPartial* __restrict__ p, int n, double& s, unsigned& m, Count& c) {
    for (int i = threadIdx.x; i < n; i += MT_THREADS) {
        const MtPartial q = p[i];
        s += q.sumsq;
        m = q.absmax > m ? q.absmax : m;
        c += q.nonfinite;
    }
}
#endif
