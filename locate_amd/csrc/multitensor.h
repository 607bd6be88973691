// What the kernels driven by a device chunk table share (nadam.hip, guard.hip, average.hip, stats.hip, dynamics.hip, digest.hip,
// snapshot.hip, parallel.hip): a table of per-tensor records (each kernel's own struct, with the element count in a member `n`) and
// a list of int2 {tensor, chunk} entries that covers every tensor in MT_CHUNK-element pieces (locate_amd/_tables.py builds both).
// Here:
//   - the chunk size, the decode of an entry (mt_decode) and the grid cap (mt_grid);
//   - the two ways a block reads a chunk, every load issued before the first use: in FIXED LANES (mt_read_lanes / mt_write_lanes:
//     an element belongs to the same thread whatever the base's alignment) and SPLIT at the 16-byte boundaries (mt_split /
//     mt_read_split: a per-word head, 16-byte words, a per-word tail);
//   - the fixed-order sum of any record of 32-bit words with an add(): a block's total (mt_block_total) and a thread's share of a
//     run of partials (mt_add_partials);
//   - the record {sumsq, absmax, nonfinite} of the statistics and what one element adds to it (MtPartial, mt_take).
// These kernels take raw addresses for every tensor of a run: the tail arithmetic below is the only copy there is.
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

// ---- a chunk in fixed lanes ---------------------------------------------------------------------------------------------------------
// Elements [0, len) of the chunk at x, 0 < len <= MT_CHUNK: thread t holds elements 4 (t + 256 k) + j in v[k] (k, j < 4) whether
// they arrive by a 16-byte load (x 16-byte aligned) or by 4-byte loads, so what a kernel computes from v does not depend on the
// alignment.  Elements at or past len read as +0.0f and are never touched in memory.
// N operands are read together - 16-byte loads where ALL of them are aligned - so that a full chunk's N * 4 loads sit in one basic
// block: read one after the other through branches of their own, the second operand's loads waited for the first's (dynamics.hip's
// recording pass then ran 0.6 - 2.8 us longer, profiles/notes_multitensor.md).
template <int N>
__device__ __forceinline__ void mt_read_lanes(const float* const (&x)[N], int len, float4 (&v)[N][MT_PER_THREAD]) {
    uintptr_t bits = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) bits |= reinterpret_cast<uintptr_t>(x[i]);
    const bool vec = (bits & 15) == 0;
    if (vec && len == MT_CHUNK) {          // a full chunk: every load issued before the first use
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) v[i][k] = reinterpret_cast<const float4*>(x[i])[threadIdx.x + k * MT_THREADS];
        }
    } else if (vec) {
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) {
            const int e = 4 * (threadIdx.x + k * MT_THREADS);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (e + 4 <= len) {
                    v[i][k] = reinterpret_cast<const float4*>(x[i])[threadIdx.x + k * MT_THREADS];
                } else {
                    v[i][k].x = e < len ? x[i][e] : 0.0f;
                    v[i][k].y = e + 1 < len ? x[i][e + 1] : 0.0f;
                    v[i][k].z = e + 2 < len ? x[i][e + 2] : 0.0f;
                    v[i][k].w = 0.0f;          // e + 3 < len would have taken the 16-byte load
                }
            }
        }
    } else {          // a base that is not 16-byte aligned: the same elements per thread through 4-byte loads
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) {
            const int e = 4 * (threadIdx.x + k * MT_THREADS);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                v[i][k].x = e < len ? x[i][e] : 0.0f;
                v[i][k].y = e + 1 < len ? x[i][e + 1] : 0.0f;
                v[i][k].z = e + 2 < len ? x[i][e + 2] : 0.0f;
                v[i][k].w = e + 3 < len ? x[i][e + 3] : 0.0f;
            }
        }
    }
}

__device__ __forceinline__ void mt_read_lanes(const float* x, int len, float4 (&v)[MT_PER_THREAD]) {
    const float* const one[1] = {x};
    mt_read_lanes(one, len, reinterpret_cast<float4 (&)[1][MT_PER_THREAD]>(v));
}

// the same elements back: exactly [x, x + len) is written
__device__ __forceinline__ void mt_write_lanes(float* x, int len, const float4 (&v)[MT_PER_THREAD]) {
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    float4* x4 = reinterpret_cast<float4*>(x);
    if (vec && len == MT_CHUNK) {
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) x4[threadIdx.x + k * MT_THREADS] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) {
            const int e = 4 * (threadIdx.x + k * MT_THREADS);
            if (vec && e + 4 <= len) {
                x4[threadIdx.x + k * MT_THREADS] = v[k];
            } else {
                if (e < len) x[e] = v[k].x;
                if (e + 1 < len) x[e + 1] = v[k].y;
                if (e + 2 < len) x[e + 2] = v[k].z;
                if (e + 3 < len) x[e + 3] = v[k].w;
            }
        }
    }
}

// ---- a chunk split at the 16-byte boundaries ----------------------------------------------------------------------------------------
// Words [0, len) of the chunk at p (4-byte words, 0 < len <= MT_CHUNK): `head` words up to p's first 16-byte boundary (0 .. 3, at
// most len), n4 16-byte words, `tail` words behind them (0 .. 3).  Word j of 16-byte word w is word head + 4 w + j of the chunk.
struct MtSplit {
    int head, n4, tail;
};

template <typename W>
__device__ __forceinline__ MtSplit mt_split(const W* p, int len) {
    static_assert(sizeof(W) == 4, "a chunk is split in 4-byte words");
    MtSplit s;
    s.head = (int)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
    s.head = s.head > len ? len : s.head;
    s.n4 = (len - s.head) >> 2;
    s.tail = len - s.head - 4 * s.n4;
    return s;
}

template <typename W>
using mt_word4 = W __attribute__((ext_vector_type(4)));

// This thread's part of the chunk: 16-byte words t + 256 k in v[k], head word t in h, tail word t in t_ - zero where the chunk has
// none, and nothing outside [p, p + len) is touched.  Every load is issued before the first use.
template <typename W>
__device__ __forceinline__ void mt_read_split(const W* p, const MtSplit& s, mt_word4<W> (&v)[MT_PER_THREAD], W& h, W& t_) {
    const int tid = threadIdx.x;
    const mt_word4<W>* p4 = reinterpret_cast<const mt_word4<W>*>(p + s.head);
#pragma unroll
    for (int k = 0; k < MT_PER_THREAD; ++k) {
        const int w = tid + k * MT_THREADS;
        v[k] = w < s.n4 ? p4[w] : mt_word4<W>{0, 0, 0, 0};
    }
    h = tid < s.head ? p[tid] : W(0);
    t_ = tid < s.tail ? p[s.head + 4 * s.n4 + tid] : W(0);
}

// ---- the fixed-order sum ------------------------------------------------------------------------------------------------------------
// Every sum has one order - a thread's elements in index order, a wave by a butterfly, the block's four waves in order, partial p
// on thread p % 256 in ascending order - and no floating-point atomics: the determinism that stats.hip, guard.hip and dynamics.hip
// document rests on these two functions.  R: any record that is a whole number of 32-bit words and has add(const R&).

// the block's total in thread 0 (other threads: unspecified); `lds` holds MT_WAVES records
template <typename R>
__device__ __forceinline__ R mt_block_total(R r, R* lds) {
    static_assert(sizeof(R) % 4 == 0, "a record is shuffled word by word");
    constexpr int WORDS = sizeof(R) / 4;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        int mine[WORDS], theirs[WORDS];
        __builtin_memcpy(mine, &r, sizeof(R));
#pragma unroll
        for (int i = 0; i < WORDS; ++i) theirs[i] = __shfl_xor(mine[i], o, 64);
        R q;
        __builtin_memcpy(&q, theirs, sizeof(R));
        r.add(q);
    }
    __syncthreads();          // lds may still be read from the previous chunk
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = r;
    __syncthreads();
    R total = lds[0];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MT_WAVES; ++w) total.add(lds[w]);
    }
    return total;
}

// this thread's share of n partials: p[threadIdx.x], p[threadIdx.x + 256], ... added to r in ascending order
template <typename R, typename P>
__device__ __forceinline__ void mt_add_partials(const P* __restrict__ p, int n, R& r) {
    for (int i = threadIdx.x; i < n; i += MT_THREADS) r.add(p[i]);
}

// ---- sum of exact squares of the finite elements, their largest magnitude, the count of the others ---------------------------------
struct MtPartial {          // a chunk's partial and a tensor's record alike
    double sumsq;
    unsigned absmax;          // bit pattern of a non-negative finite fp32
    unsigned nonfinite;
    __device__ __forceinline__ void add(const MtPartial& q) {
        sumsq += q.sumsq;
        absmax = q.absmax > absmax ? q.absmax : absmax;
        nonfinite += q.nonfinite;
    }
};

// WITH_MAX false leaves the maximum out (m stays what it was): the guard, which has no use for it, ran its two steps 2.2 us slower
// behind an iteration with the maximum carried along, against 0.6 us between the parent's own runs (profiles/notes_multitensor.md).
// Its record (guard.hip, GuardPartial) has MtPartial's layout and an add() that skips the maximum for the same reason.
template <bool WITH_MAX = true>
__device__ __forceinline__ void mt_take(float x, double& s, unsigned& m, unsigned& c) {
    const unsigned mag = __float_as_uint(x) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    const double d = finite ? (double)x : 0.0;
    s = fma(d, d, s);          // d * d is exact in fp64: one rounding, that of the addition
    if (WITH_MAX) m = finite && mag > m ? mag : m;
    c += finite ? 0u : 1u;
}

template <bool WITH_MAX = true, typename V4>
__device__ __forceinline__ void mt_take4(V4 v, double& s, unsigned& m, unsigned& c) {
    mt_take<WITH_MAX>(v.x, s, m, c);
    mt_take<WITH_MAX>(v.y, s, m, c);
    mt_take<WITH_MAX>(v.z, s, m, c);
    mt_take<WITH_MAX>(v.w, s, m, c);
}
#endif
