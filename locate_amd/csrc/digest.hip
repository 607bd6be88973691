// A 128-bit digest of every tensor of a device table (locate_amd/spill.py), over 4-byte words w_0 .. w_{n-1}, all arithmetic
// modulo 2^64 on unsigned integers:
//   A = sum_i w_i                               changes with any single bit;
//   B = sum_i ((i + 1) mod 2^32) * w_i          changes when two unequal words swap places or a block moves.
// The mod 2^32 is deliberate: a word costs one 32 x 32 + 64 multiply-add and one 64-bit add.  Both are commutative integer sums,
// so a digest depends only on its tensor's words and their order - not on the grid, on the tensor's place in the table, on what
// else the table holds, nor on the tensor's alignment.  The snapshot's spill to disk (spill.py) runs it over a committed slot on a
// side stream and compares the result with the same sums taken on the host from the bytes that arrived there; like the
// statistics and the snapshot it only READS what the step left and runs BETWEEN two iterations.  The reference has nothing of the kind.
//
// Two launches on the chunk-table layer of multitensor.h.  (1) digest_partial_kernel: blocks stride over
// the int2 {tensor, chunk} list and write one {A, B} partial per entry to partials[position of the entry]; a damaged entry
// (mt_decode false) writes a zero partial, so every word of partials[0 .. n_chunks) is written by every call.
// (2) digest_combine_kernel: one block per tensor adds the partials of [first[t], first[t + 1]) into out[t]; a tensor without
// chunks (n = 0) or with a damaged range gets {0, 0}.  No atomics, nothing to clear between calls.
//
// A bandwidth kernel (4 bytes per word): a chunk is read split at the 16-byte boundaries (multitensor.h's mt_read_split), every
// load issued before the first use; the sums are multitensor.h's mt_block_total and mt_add_partials; at most 2048 blocks.
#include "multitensor.h"

typedef unsigned long long u64;

struct DigestTensor {          // 16 bytes
    const unsigned* p;         // 4-byte aligned
    long long n;               // 4-byte words
};

struct DigestPair {            // a chunk's partial and a tensor's digest alike
    u64 a;
    u64 b;
    __device__ __forceinline__ void add(const DigestPair& q) {
        a += q.a;
        b += q.b;
    }
};

__device__ __forceinline__ void digest_take(unsigned w, unsigned index, u64& a, u64& b) {
    a += (u64)w;
    b += (u64)index * (u64)w;          // 32 x 32 -> 64, added modulo 2^64
}

__global__ void __launch_bounds__(MT_THREADS) digest_partial_kernel(const DigestTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                   int n_tensors, int n_chunks, DigestPair* __restrict__ partials) {
    __shared__ DigestPair lds[MT_WAVES];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        DigestTensor T;
        long long begin;
        int len;
        if (!mt_decode(tensors, n_tensors, chunks[c], T, begin, len)) {          // nothing was read through it
            if (tid == 0) partials[c] = DigestPair{0ull, 0ull};
            continue;
        }
        const unsigned* src = T.p + begin;
        const MtSplit sp = mt_split(src, len);
        const int head = sp.head, n4 = sp.n4;
        mt_word4<unsigned> v[MT_PER_THREAD];
        unsigned h, t;
        mt_read_split(src, sp, v, h, t);
        // word j of the chunk is word begin + j of its tensor: its factor is (begin + j + 1) mod 2^32.  A zero word adds nothing,
        // so the loads that were not taken need no branch here.
        const unsigned base = (unsigned)(begin + 1);
        u64 a = 0ull, b = 0ull;
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) {
            const unsigned at = base + (unsigned)(head + 4 * (tid + k * MT_THREADS));
            digest_take(v[k].x, at, a, b);
            digest_take(v[k].y, at + 1u, a, b);
            digest_take(v[k].z, at + 2u, a, b);
            digest_take(v[k].w, at + 3u, a, b);
        }
        digest_take(h, base + (unsigned)tid, a, b);
        digest_take(t, base + (unsigned)(head + 4 * n4 + tid), a, b);
        const DigestPair r = mt_block_total(DigestPair{a, b}, lds);
        if (tid == 0) partials[c] = r;          // c < n_chunks: inside the workspace
    }
}

__global__ void __launch_bounds__(MT_THREADS) digest_combine_kernel(const int* __restrict__ first, int n_tensors, int n_chunks,
                                                                   const DigestPair* __restrict__ partials, DigestPair* __restrict__ out) {
    __shared__ DigestPair lds[MT_WAVES];
    for (int t = blockIdx.x; t < n_tensors; t += gridDim.x) {
        const int lo = first[t], hi = first[t + 1];
        DigestPair r = {0ull, 0ull};
        if (lo >= 0 && lo <= hi && hi <= n_chunks) mt_add_partials(partials + lo, hi - lo, r);          // a damaged range reads nothing
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) out[t] = r;
    }
}

LOCATE_API size_t locate_digest_record_bytes(void) { return sizeof(DigestTensor); }
LOCATE_API int locate_digest_chunk_elems(void) { return MT_CHUNK; }

// records: DEVICE array of n_tensors {const uint32* p; int64 n} records; chunks: DEVICE (tensor index, chunk index) int pairs in
// pieces of locate_digest_chunk_elems() words, a tensor's chunks consecutive; first: DEVICE int[n_tensors + 1], the position of
// each tensor's first pair and n_chunks at the end.  Writes partials[0 .. n_chunks) and out[0 .. n_tensors), 16 bytes each, and
// nothing else.  No allocation, no host read, no synchronisation, no atomics: legal under stream capture.
LOCATE_API int locate_digest(const void* records, const void* chunks, const void* first, int n_tensors, int n_chunks, void* partials, void* out,
                             void* stream) {
    LOCATE_REQUIRE(records && chunks && first && partials && out && n_tensors > 0 && n_chunks > 0, "locate_digest: bad arguments");
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(out)) & 7) == 0,
                   "locate_digest: partials and out need 8-byte alignment");
    digest_partial_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(static_cast<const DigestTensor*>(records),
                                                                                  static_cast<const int2*>(chunks), n_tensors, n_chunks,
                                                                                  static_cast<DigestPair*>(partials));
    LOCATE_LAUNCH_CHECK("locate_digest");
    digest_combine_kernel<<<mt_grid(n_tensors), MT_THREADS, 0, as_stream(stream)>>>(static_cast<const int*>(first), n_tensors, n_chunks,
                                                                                   static_cast<const DigestPair*>(partials),
                                                                                   static_cast<DigestPair*>(out));
    LOCATE_LAUNCH_CHECK("locate_digest");
    return LOCATE_OK;
}
