// A last-good copy of a training state in device memory (locate_amd/snapshot.py): every tensor of a table is copied into one of
// two preallocated slots in ONE pass that also classifies every word it copies, and a one-block launch behind it commits the slot
// only when every copied word was finite.  Kernels of their own that run BETWEEN two training iterations, like the average and the
// statistics: nothing the training step runs is touched.  The reference has nothing of the kind.
//
// The unit of work is the 4-byte word, so one kernel serves fp32 tensors and the float64 (step, m_schedule) pairs of Nadam.  A
// record's `kind` says how its words are judged: 0 never, 1 as fp32 (exponent field all ones), 2 as fp64 (n even; the exponent
// field of the HIGH word - the odd word of a little-endian pair - all ones; the low word is never looked at).  The copy itself is
// bit for bit whatever the kind: NaN payloads, denormals and -0.0 survive.  A record whose live pointer is null stands for a
// tensor that does not exist yet (Nadam creates its state lazily): its four fill words, repeating, are written instead and
// nothing is judged (four, not two: the fresh (0.0, 1.0) pair of doubles is the words 0, 0, 0, 0x3ff00000).
//
// The count is kept in integers only and goes to the commit record by ONE atomicAdd and ONE atomicMin (lowest tensor index with
// a bad word) PER BLOCK, issued only by blocks that found something: a clean take issues no atomic at all, integer vector atomics
// commute, so the record does not depend on the order of arrival.  The commit launch reads both, decides, and clears them: the
// record is ready for the next take.
//
// A pure bandwidth kernel (8 bytes per word): 16-byte loads and stores where the live pointer is 16-byte aligned at the chunk
// (slot offsets are multiples of 16, so only the live side varies), otherwise 16-byte accesses on the live side between a
// per-word head and tail and per-word accesses on the slot side: the split is multitensor.h's (mt_split), the loads and the
// stores are this file's.  Every load of a chunk is issued before its first store; at most 2048 blocks (256 CUs x 8) stride over
// the chunk table.  A block's count is multitensor.h's mt_block_total.
//
// SNAPSHOT_NONTEMPORAL: the destination slot is not read again for hundreds of iterations, and a take pushes a slot's worth of
// stores through the Infinity Cache the next iteration's weights sit in.  Both store forms are compiled.  Measured, the take PLUS
// the iteration behind it does not tell them apart (profiles/notes_snapshot.md): nontemporal was 9 - 12 us shorter in two
// sessions and 6 us longer in a third, all inside that iteration's own run-to-run spread; the take itself is 8 - 9 us slower
// with it.  The product library uses nontemporal stores - the mean of the three sessions and the reasoning point the same way,
// and nothing measured speaks against it.  The debug variant of the library (igemm.h's knobs) reads LOCATE_SNAPSHOT_NT = 0 / 1
// at every call so that tools/bench_snapshot.py can time both.
#include <limits.h>
#include "igemm.h"
#include "multitensor.h"

#define SNAPSHOT_NONTEMPORAL 1

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct SnapshotTensor {          // 48 bytes
    unsigned* live;              // null: the tensor does not exist yet
    long long offset;            // BYTES into a slot, a multiple of 16
    long long n;                 // 4-byte words
    int kind;                    // 0 raw, 1 fp32, 2 fp64
    unsigned fill[4];            // written, repeating from fill[0], where live is null: one 16-byte word of the slot
    int pad;
};

struct SnapshotCommit {          // 64 bytes, 8-byte aligned
    int good;                    // -1: no slot committed yet; else the slot that holds the last good state
    int bad_tensor;              // of the take in flight: lowest tensor index with a bad word (INT_MAX between takes)
    unsigned long long bad_words;            // of the take in flight: words that are non-finite for their kind (0 between takes)
    long long iteration;         // of the good slot
    long long taken;             // takes committed
    long long rejected;          // takes that were not
    long long last_rejected_iteration;
    long long last_rejected_count;
    int last_rejected_tensor;    // -1: none yet
    int pad;
};

__device__ __forceinline__ unsigned snap_bad(unsigned w, int kind, int odd) {
    const unsigned mask = kind == 2 ? 0x7ff00000u : 0x7f800000u;
    const bool judged = kind == 1 || (kind == 2 && odd);
    return judged && (w & mask) == mask ? 1u : 0u;
}

template <bool NT>
__device__ __forceinline__ void snap_store(unsigned* p, unsigned w) {
    if (NT) __builtin_nontemporal_store(w, p);
    else *p = w;
}

// 16 bytes to p: one store where p is 16-byte aligned (`vec`), four otherwise
template <bool NT>
__device__ __forceinline__ void snap_store4(unsigned* p, u32x4 v, bool vec) {
    if (vec) {
        if (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
        else *reinterpret_cast<u32x4*>(p) = v;
    } else {
        snap_store<NT>(p, v.x);
        snap_store<NT>(p + 1, v.y);
        snap_store<NT>(p + 2, v.z);
        snap_store<NT>(p + 3, v.w);
    }
}

__device__ __forceinline__ u32x4 snap_load4(const unsigned* p, bool vec) {
    if (vec) return *reinterpret_cast<const u32x4*>(p);
    u32x4 v;
    v.x = p[0];
    v.y = p[1];
    v.z = p[2];
    v.w = p[3];
    return v;
}

// Words [0, len) of a chunk from src to dst in multitensor.h's split `s` of the LIVE side: head words, 16-byte words, the rest.
// src_vec / dst_vec: whether that side is 16-byte aligned at src + head / dst + head (the live side always is, the slot side only
// when head == 0).  Every load before the first store.  Returns this thread's count of words that are non-finite for `kind`; the
// chunk starts at an even word of its tensor.  The loads are this file's own, not mt_read_split: with the shared read the copy
// kernel went from 90 to 58 VGPRs and the restore ran 46 us longer (profiles/notes_multitensor.md).
template <bool NT, bool JUDGE>
__device__ __forceinline__ unsigned snap_copy_chunk(const unsigned* __restrict__ src, unsigned* __restrict__ dst, const MtSplit& s,
                                                    bool src_vec, bool dst_vec, int kind) {
    const int tid = threadIdx.x, head = s.head, n4 = s.n4, tail = s.tail;
    u32x4 v[MT_PER_THREAD];
#pragma unroll
    for (int k = 0; k < MT_PER_THREAD; ++k) {
        const int w = tid + k * MT_THREADS;
        if (w < n4) v[k] = snap_load4(src + head + 4 * w, src_vec);
    }
    const unsigned h = tid < head ? src[tid] : 0u;
    const unsigned t = tid < tail ? src[head + 4 * n4 + tid] : 0u;
    unsigned bad = 0u;
#pragma unroll
    for (int k = 0; k < MT_PER_THREAD; ++k) {
        const int w = tid + k * MT_THREADS;
        if (w < n4) {
            snap_store4<NT>(dst + head + 4 * w, v[k], dst_vec);
            if (JUDGE) {          // word index head + 4 w + j: its parity is that of head + j
                bad += snap_bad(v[k].x, kind, head & 1) + snap_bad(v[k].y, kind, (head + 1) & 1) + snap_bad(v[k].z, kind, head & 1) +
                       snap_bad(v[k].w, kind, (head + 1) & 1);
            }
        }
    }
    if (tid < head) {
        snap_store<NT>(dst + tid, h);
        if (JUDGE) bad += snap_bad(h, kind, tid & 1);
    }
    if (tid < tail) {
        snap_store<NT>(dst + head + 4 * n4 + tid, t);
        if (JUDGE) bad += snap_bad(t, kind, (head + tid) & 1);          // 4 n4 is even
    }
    return bad;
}

// what a take found: words that are non-finite for their kind, and the lowest tensor index that has one.  32 bits hold a block's
// count: a thread sees at most 18 words per chunk and a block at most 1 / 2048 of a table that fits the device's memory.
struct SnapBad {
    unsigned count;
    int first;
    __device__ __forceinline__ void add(const SnapBad& q) {
        count += q.count;
        first = q.first < first ? q.first : first;
    }
};

template <bool NT>
__global__ void __launch_bounds__(MT_THREADS) snapshot_copy_kernel(const SnapshotTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                  int n_tensors, int n_chunks, unsigned* slot0, unsigned* slot1,
                                                                  SnapshotCommit* commit) {
    __shared__ SnapBad lds[MT_WAVES];
    unsigned* slot = commit->good == 0 ? slot1 : slot0;          // the slot that is NOT the good one; uniform
    SnapBad found = {0u, INT_MAX};
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        SnapshotTensor T;
        long long begin;
        int len;
        const int2 ch = chunks[c];
        if (!mt_decode(tensors, n_tensors, ch, T, begin, len)) continue;          // a damaged table writes nothing
        unsigned* dst = slot + (T.offset >> 2) + begin;          // 16-byte aligned: offset and 4 * begin are multiples of 16
        if (T.live == nullptr) {
            const int n4 = len >> 2;
            u32x4 f;
            f.x = T.fill[0];
            f.y = T.fill[1];
            f.z = T.fill[2];
            f.w = T.fill[3];
            for (int w = threadIdx.x; w < n4; w += MT_THREADS) snap_store4<NT>(dst + 4 * w, f, true);
            const int i = 4 * n4 + threadIdx.x;
            if (i < len) snap_store<NT>(dst + i, T.fill[i & 3]);
            continue;
        }
        const unsigned* src = T.live + begin;
        const MtSplit s = mt_split(src, len);
        const unsigned bad = snap_copy_chunk<NT, true>(src, dst, s, true, s.head == 0, T.kind);
        found.count += bad;
        found.first = bad != 0u && ch.x < found.first ? ch.x : found.first;
    }
    found = mt_block_total(found, lds);
    if (threadIdx.x == 0 && found.count != 0u) {
        atomicAdd(&commit->bad_words, (unsigned long long)found.count);
        atomicMin(&commit->bad_tensor, found.first);
    }
}

__global__ void __launch_bounds__(64) snapshot_commit_kernel(SnapshotCommit* commit, long long iteration) {
    if (threadIdx.x != 0) return;
    SnapshotCommit C = *commit;
    if (C.bad_words == 0ull) {
        C.good = C.good == 0 ? 1 : 0;          // the slot the copy just wrote
        C.iteration = iteration;
        C.taken += 1;
    } else {
        C.rejected += 1;
        C.last_rejected_iteration = iteration;
        C.last_rejected_count = (long long)C.bad_words;
        C.last_rejected_tensor = C.bad_tensor;
    }
    C.bad_words = 0ull;
    C.bad_tensor = INT_MAX;
    *commit = C;
}

__global__ void __launch_bounds__(MT_THREADS) snapshot_restore_kernel(const SnapshotTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                     int n_tensors, int n_chunks, const unsigned* __restrict__ slot) {
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        SnapshotTensor T;
        long long begin;
        int len;
        if (!mt_decode(tensors, n_tensors, chunks[c], T, begin, len) || T.live == nullptr) continue;
        unsigned* dst = T.live + begin;
        const MtSplit s = mt_split(dst, len);
        (void)snap_copy_chunk<false, false>(slot + (T.offset >> 2) + begin, dst, s, s.head == 0, true, 0);
    }
}

LOCATE_API size_t locate_snapshot_record_bytes(void) { return sizeof(SnapshotTensor); }
LOCATE_API size_t locate_snapshot_commit_bytes(void) { return sizeof(SnapshotCommit); }
LOCATE_API int locate_snapshot_chunk_elems(void) { return MT_CHUNK; }

static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// records: DEVICE array of n_tensors SnapshotTensor; chunks: DEVICE (tensor index, chunk index) int pairs in pieces of
// locate_snapshot_chunk_elems() WORDS; slot0 / slot1: 16-byte aligned, each at least max(offset + 4 n) bytes; commit: the 64-byte
// record.  Two launches, no allocation, no host read, no synchronisation: legal under stream capture, where the decision is
// taken at every replay.  Writes the slot that is not `good` and the commit record and nothing else.
LOCATE_API int locate_snapshot_take(const void* records, const void* chunks, int n_tensors, int n_chunks, void* slot0, void* slot1, void* commit,
                                    long long iteration, void* stream) {
    LOCATE_REQUIRE(records && chunks && n_tensors > 0 && n_chunks > 0, "locate_snapshot_take: bad arguments");
    LOCATE_REQUIRE(slot0 && slot1 && slot0 != slot1 && aligned_to(slot0, 16) && aligned_to(slot1, 16),
                   "locate_snapshot_take: the two slots must be distinct and 16-byte aligned");
    LOCATE_REQUIRE(commit && aligned_to(commit, 8), "locate_snapshot_take: the commit record must be 8-byte aligned");
    const SnapshotTensor* rec = static_cast<const SnapshotTensor*>(records);
    const int2* ch = static_cast<const int2*>(chunks);
    unsigned* s0 = static_cast<unsigned*>(slot0);
    unsigned* s1 = static_cast<unsigned*>(slot1);
    SnapshotCommit* cm = static_cast<SnapshotCommit*>(commit);
    if (knob_int("LOCATE_SNAPSHOT_NT", SNAPSHOT_NONTEMPORAL) != 0)
        snapshot_copy_kernel<true><<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(rec, ch, n_tensors, n_chunks, s0, s1, cm);
    else
        snapshot_copy_kernel<false><<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(rec, ch, n_tensors, n_chunks, s0, s1, cm);
    LOCATE_LAUNCH_CHECK("locate_snapshot_take");
    snapshot_commit_kernel<<<1, 64, 0, as_stream(stream)>>>(cm, iteration);
    LOCATE_LAUNCH_CHECK("locate_snapshot_take");
    return LOCATE_OK;
}

// `slot` back into the live tensors: writes exactly [live, live + n) of every record whose live pointer is not null.
LOCATE_API int locate_snapshot_restore(const void* records, const void* chunks, int n_tensors, int n_chunks, const void* slot, void* stream) {
    LOCATE_REQUIRE(records && chunks && n_tensors > 0 && n_chunks > 0, "locate_snapshot_restore: bad arguments");
    LOCATE_REQUIRE(slot && aligned_to(slot, 16), "locate_snapshot_restore: the slot must be 16-byte aligned");
    snapshot_restore_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(static_cast<const SnapshotTensor*>(records),
                                                                                    static_cast<const int2*>(chunks), n_tensors, n_chunks,
                                                                                    static_cast<const unsigned*>(slot));
    LOCATE_LAUNCH_CHECK("locate_snapshot_restore");
    return LOCATE_OK;
}
