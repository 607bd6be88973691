// Binned mode coverage (NDB): the centroid update of an exact k-means in the 8-bit code domain of neighbours.hip.  The assignment
// step is nn_search with k = 1; this file is the other half, the sum of the code rows of every group of images and the rounded
// mean.  Integers throughout: the result depends on nothing but the inputs.
//   md_slab_kernel   : the grouped positions `order[0 .. M)` are cut into slabs of MD_SLAB rows, a row into column tiles of
//                      MD_THREADS 16-byte lanes.  A block walks its slab, eight 16-byte row loads in flight per lane, and unpacks
//                      every code into an int32 accumulator; wherever a group begins or ends inside the slab it stores the
//                      accumulators to a partial slot and starts again.  The bank is read once, at stream rate, however unequal
//                      the groups are.
//   md_gather_kernel : per group and 64 columns, the sum of the partial slots the group spans, sixteen slots at a time.
//   md_centroid_kernel : the rounded mean of a group's sums, floor((2 s + n) / (2 n)), beside its norm and the bytes that changed.
// Slots.  A segment is a maximal run of positions that crosses neither a slab boundary nor a value of `starts` (clamped to
// 0 .. M).  slot(p) = p / MD_SLAB + #{j : starts[j] <= p}: it is constant on a segment and grows across every boundary, so segments
// have different slots, below ceil(M / MD_SLAB) + K + 1, for ANY `starts` - decreasing, repeated, out of range.  A group is an
// interval of positions, hence a run of whole segments, and its sum is that of the used slots from slot(lo) to slot(hi - 1):
// groups that overlap (a `starts` that decreases) read the same slots twice and are right too.  Numbers that no segment has
// (where several `starts` coincide) are marked unused.  Every block counts the `starts` below and inside its slab itself: K + 1
// words from L2 per block, nothing beside the slab's rows for the hundreds of bins this is built for.
#include "common.h"

#define MD_THREADS 256
#define MD_SLAB 64                                 // rows of `order` per block of the walk
#define MD_TILE (16 * MD_THREADS)                  // bytes of a row per block of the walk
#define MD_FLIGHT 8                                // row loads in flight per lane
#define MD_ROW_MAX 262144
#define MD_M_MAX ((1 << 24) - 1)                   // 128 M < 2^31: an int32 sum cannot overflow
#define MD_K_MAX 65535
#define MD_GATHER_COLS 64                          // columns per block of the gather: 16 lanes of four int32
#define MD_GATHER_PHASES 16                        // slots it reads side by side

static inline int64_t md_slots(int M, int K) { return cdiv64(M, MD_SLAB) + K + 1; }

__device__ __forceinline__ int md_clamp(int v, int M) { return v < 0 ? 0 : v > M ? M : v; }

// acc[4 w + b] += byte b of word w, as int8
__device__ __forceinline__ void md_add16(int (&acc)[16], const int4& v) {
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[4 * i] += (int)((unsigned)w[i] << 24) >> 24;
        acc[4 * i + 1] += (int)((unsigned)w[i] << 16) >> 24;
        acc[4 * i + 2] += (int)((unsigned)w[i] << 8) >> 24;
        acc[4 * i + 3] += w[i] >> 24;
    }
}

__device__ __forceinline__ void md_flush(int (&acc)[16], int* __restrict__ partial, int64_t slot, int row_bytes, int col, bool live) {
    if (live) {
        int4* p = reinterpret_cast<int4*>(partial + slot * row_bytes + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = make_int4(acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
}

// the 16 bytes at pc of the MD_FLIGHT rows row[0 ..]; -1 (no image): row 0
__device__ __forceinline__ void md_load(int4 (&v)[MD_FLIGHT], const int8_t* __restrict__ pc, const int* row, int row_bytes) {
#pragma unroll
    for (int r = 0; r < MD_FLIGHT; ++r) {
        const int idx = row[r];
        v[r] = *reinterpret_cast<const int4*>(pc + (size_t)(idx < 0 ? 0 : idx) * row_bytes);
    }
}

// grid (slabs, column tiles).  used [slots], first / last [K + 1]: written by the blocks of column tile 0 - first[j] = slot(starts[j])
// where starts[j] < M, last[j] = slot(starts[j] - 1) where starts[j] >= 1: all that a group that is not empty needs.
__global__ __launch_bounds__(MD_THREADS) void md_slab_kernel(const int8_t* __restrict__ codes, int N, int row_bytes, const int* __restrict__ order, int M,
                                                             const int* __restrict__ starts, int K, int* __restrict__ partial, int* __restrict__ used,
                                                             int* __restrict__ first, int* __restrict__ last) {
    __shared__ int s_row[MD_SLAB + MD_FLIGHT];     // the image of each position, -1: none (outside 0 .. N - 1, past M, past the slab)
    __shared__ int s_inc[MD_SLAB];                 // the `starts` equal to base + i
    __shared__ int s_pre[MD_SLAB + 1];             // s_pre[i]: the `starts` in [base, base + i)
    __shared__ int s_scratch[16];
    const int t = threadIdx.x;
    const int base = blockIdx.x * MD_SLAB;         // < M <= MD_M_MAX
    const int nrows = M - base < MD_SLAB ? M - base : MD_SLAB;
    if (t < MD_SLAB + MD_FLIGHT) {
        const int idx = t < nrows ? order[base + t] : -1;
        s_row[t] = idx >= 0 && idx < N ? idx : -1;
    }
    if (t < MD_SLAB) s_inc[t] = 0;
    __syncthreads();
    int below = 0;
    for (int j = t; j <= K; j += MD_THREADS) {
        const int d = md_clamp(starts[j], M) - base;
        if (d < 0) below += 1;
        else if (d < MD_SLAB) atomicAdd(&s_inc[d], 1);
    }
    below = block_sum<int>(below, s_scratch);
    if (t == 0) {
        int run = 0;
        s_pre[0] = 0;
        for (int i = 0; i < MD_SLAB; ++i) {
            run += s_inc[i];
            s_pre[i + 1] = run;
        }
    }
    __syncthreads();
    const int own = blockIdx.x + below;            // slot(base + i) = own + s_pre[i + 1]; at most slabs - 1 + K + 1

    if (blockIdx.y == 0) {
        const int owned = 1 + s_pre[MD_SLAB];
        for (int u = t; u < owned; u += MD_THREADS) used[own + u] = 0;
        __syncthreads();
        if (t < nrows && (t == 0 || s_inc[t] > 0)) used[own + s_pre[t + 1]] = 1;
        for (int j = t; j <= K; j += MD_THREADS) {
            const int d = md_clamp(starts[j], M) - base;
            if (d >= 0 && d < nrows) first[j] = own + s_pre[d + 1];
            if (d >= 1 && d <= nrows) last[j] = own + s_pre[d];
        }
    }

    // Every load is unconditional, so that the compiler can count them: a position without an image reads row 0 (N >= 1) and is
    // left out when the sums are formed, a lane past the row's end reads column 0 and stores nothing.  The next eight rows are
    // requested before the current eight are unpacked; the eight past the slab's end are row 0 again, from L2.
    const int col = blockIdx.y * MD_TILE + 16 * t;
    const bool live = col < row_bytes;
    const int8_t* pc = codes + (live ? col : 0);
    int acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    int slot = own + s_pre[1];
    int4 next[MD_FLIGHT];
    md_load(next, pc, s_row, row_bytes);
    for (int i0 = 0; i0 < nrows; i0 += MD_FLIGHT) {
        int4 v[MD_FLIGHT];
#pragma unroll
        for (int r = 0; r < MD_FLIGHT; ++r) v[r] = next[r];
        md_load(next, pc, s_row + i0 + MD_FLIGHT, row_bytes);
#pragma unroll
        for (int r = 0; r < MD_FLIGHT; ++r) {
            const int i = i0 + r;
            if (i > 0 && i < nrows && s_inc[i] > 0) {
                md_flush(acc, partial, slot, row_bytes, col, live);
                slot += s_inc[i];
            }
            if (s_row[i] >= 0) md_add16(acc, v[r]);          // the same in every lane
        }
    }
    md_flush(acc, partial, slot, row_bytes, col, live);
}

// grid (row_bytes / 64, K).  Lane group t & 15 holds four columns, t >> 4 is the phase: slot first + phase, + 16, ...; an unused
// slot's words are read (they lie inside the workspace) and dropped.  The sixteen phases meet in LDS.
__global__ __launch_bounds__(MD_THREADS) void md_gather_kernel(const int* __restrict__ partial, const int* __restrict__ used, const int* __restrict__ first,
                                                               const int* __restrict__ last, const int* __restrict__ starts, int M, int row_bytes,
                                                               int slots, int* __restrict__ sums) {
    __shared__ int4 s_part[MD_GATHER_PHASES][MD_GATHER_COLS / 4];
    const int t = threadIdx.x, k = blockIdx.y;
    const int lane = t & 15, phase = t >> 4;
    const int col = blockIdx.x * MD_GATHER_COLS;
    const int lo = md_clamp(starts[k], M), hi = md_clamp(starts[k + 1], M);
    int4 a = make_int4(0, 0, 0, 0);
    if (hi > lo) {
        int f = first[k], l = last[k + 1];         // written by the walk for exactly these lo < M and hi >= 1
        f = f < 0 ? 0 : f;
        l = l < slots ? l : slots - 1;
        const int* p = partial + col + 4 * lane;
#pragma unroll 4
        for (int s = f + phase; s <= l; s += MD_GATHER_PHASES) {
            const int4 v = *reinterpret_cast<const int4*>(p + (size_t)s * row_bytes);
            if (used[s] != 0) {
                a.x += v.x;
                a.y += v.y;
                a.z += v.z;
                a.w += v.w;
            }
        }
    }
    s_part[phase][lane] = a;
    __syncthreads();
    if (t < MD_GATHER_COLS) {
        const int* w = reinterpret_cast<const int*>(&s_part[0][0]);
        int total = 0;
#pragma unroll
        for (int ph = 0; ph < MD_GATHER_PHASES; ++ph) total += w[ph * MD_GATHER_COLS + t];
        sums[(size_t)k * row_bytes + col + t] = total;
    }
}

// one block per centre, one thread per 16 bytes of its row.  a = s + 128 n lies in 0 .. 255 n < 2^32, and floor((2 s + n) / (2 n))
// + 128 = floor(a / n) + (2 (a mod n) >= n): unsigned 32-bit arithmetic, a half goes up.  `previous` may be `codes`: a thread reads
// its sixteen bytes before it writes them.
__global__ __launch_bounds__(MD_THREADS) void md_centroid_kernel(const int* __restrict__ sums, const int* __restrict__ starts, int M, int row_bytes,
                                                                 const int8_t* previous, int8_t* codes, long long* __restrict__ norms, int* __restrict__ moved) {
    __shared__ long long scratch_norm[16];
    __shared__ int scratch_moved[16];
    const int k = blockIdx.x;
    const int lo = md_clamp(starts[k], M), hi = md_clamp(starts[k + 1], M);
    const unsigned n = hi > lo ? (unsigned)(hi - lo) : 0u;
    const size_t row = (size_t)k * row_bytes;
    long long norm = 0;
    int changed = 0;
    for (int g = threadIdx.x; g < (row_bytes >> 4); g += MD_THREADS) {
        const int4 old = *reinterpret_cast<const int4*>(previous + row + 16 * g);
        int4 out = old;
        if (n > 0) {
            const int4* ps = reinterpret_cast<const int4*>(sums + row + 16 * g);
            int w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int4 s = ps[i];
                const int e[4] = {s.x, s.y, s.z, s.w};
                w[i] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const unsigned a = (unsigned)e[b] + 128u * n;
                    const unsigned q = a / n, r = a - q * n;
                    const int c = (int)(q + (2u * r >= n ? 1u : 0u)) - 128;
                    w[i] |= (c & 255) << (8 * b);
                }
            }
            out = make_int4(w[0], w[1], w[2], w[3]);
        }
        const int wo[4] = {old.x, old.y, old.z, old.w}, wn[4] = {out.x, out.y, out.z, out.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int c = (int)((unsigned)wn[i] << (24 - 8 * b)) >> 24;
                norm += c * c;
                changed += (((wn[i] ^ wo[i]) >> (8 * b)) & 255) != 0 ? 1 : 0;
            }
        }
        *reinterpret_cast<int4*>(codes + row + 16 * g) = out;
    }
    const long long tn = block_sum<long long>(norm, scratch_norm);
    const int tm = block_sum<int>(changed, scratch_moved);
    if (threadIdx.x == 0) {
        norms[k] = tn;
        moved[k] = tm;
    }
}

static int md_check(const char* name, int M, int K, int row_bytes) {
    LOCATE_REQUIRE(M >= 1 && M <= MD_M_MAX, "%s: M = %d (1 .. 2^24 - 1: an int32 sum of M codes must not overflow)", name, M);
    LOCATE_REQUIRE(K >= 1 && K <= MD_K_MAX, "%s: K = %d (1 .. %d)", name, K, MD_K_MAX);
    LOCATE_REQUIRE(row_bytes >= 64 && row_bytes % 64 == 0 && row_bytes <= MD_ROW_MAX, "%s: row_bytes = %d (a multiple of 64 up to %d)", name, row_bytes,
                   MD_ROW_MAX);
    return LOCATE_OK;
}

LOCATE_API size_t locate_nn_group_sums_workspace_bytes(int M, int K, int row_bytes) {
    if (M < 1 || M > MD_M_MAX || K < 1 || K > MD_K_MAX || row_bytes < 64 || row_bytes % 64 || row_bytes > MD_ROW_MAX) return 0;
    return 4 * ((size_t)md_slots(M, K) * ((size_t)row_bytes + 1) + 2 * ((size_t)K + 1));
}

LOCATE_API int locate_nn_group_sums(const int8_t* codes, int N, int row_bytes, const int32_t* order, int M, const int32_t* starts, int K,
                                    int32_t* sums, void* workspace, void* stream) {
    LOCATE_REQUIRE(codes && order && starts && sums && workspace, "locate_nn_group_sums: null pointer");
    if (int e = md_check("locate_nn_group_sums", M, K, row_bytes)) return e;
    LOCATE_REQUIRE(N >= 1, "locate_nn_group_sums: N = %d", N);
    LOCATE_REQUIRE((((uintptr_t)codes | (uintptr_t)workspace) & 15) == 0, "locate_nn_group_sums: codes and workspace must be 16-byte aligned");
    LOCATE_REQUIRE((((uintptr_t)order | (uintptr_t)starts | (uintptr_t)sums) & 3) == 0, "locate_nn_group_sums: order, starts and sums must be 4-byte aligned");
    const int64_t slots = md_slots(M, K);
    int* partial = static_cast<int*>(workspace);
    int* used = partial + (size_t)slots * row_bytes;
    int* first = used + slots;
    int* last = first + K + 1;
    hipStream_t st = as_stream(stream);
    const dim3 walk((unsigned)cdiv64(M, MD_SLAB), (unsigned)cdiv64(row_bytes, MD_TILE));
    md_slab_kernel<<<walk, MD_THREADS, 0, st>>>(codes, N, row_bytes, order, M, starts, K, partial, used, first, last);
    LOCATE_LAUNCH_CHECK("locate_nn_group_sums (slabs)");
    const dim3 gather((unsigned)(row_bytes / MD_GATHER_COLS), (unsigned)K);
    md_gather_kernel<<<gather, MD_THREADS, 0, st>>>(partial, used, first, last, starts, M, row_bytes, (int)slots, sums);
    LOCATE_LAUNCH_CHECK("locate_nn_group_sums");
    return LOCATE_OK;
}

LOCATE_API int locate_nn_centroids(const int32_t* sums, const int32_t* starts, int K, int M, int row_bytes, const int8_t* previous,
                                   int8_t* codes, int64_t* norms, int32_t* moved, void* stream) {
    LOCATE_REQUIRE(sums && starts && previous && codes && norms && moved, "locate_nn_centroids: null pointer");
    if (int e = md_check("locate_nn_centroids", M, K, row_bytes)) return e;
    LOCATE_REQUIRE((((uintptr_t)sums | (uintptr_t)previous | (uintptr_t)codes) & 15) == 0, "locate_nn_centroids: sums, previous and codes must be 16-byte aligned");
    LOCATE_REQUIRE(((uintptr_t)norms & 7) == 0 && (((uintptr_t)starts | (uintptr_t)moved) & 3) == 0,
                   "locate_nn_centroids: norms must be 8-byte, starts and moved 4-byte aligned");
    md_centroid_kernel<<<K, MD_THREADS, 0, as_stream(stream)>>>(sums, starts, M, row_bytes, previous, codes, reinterpret_cast<long long*>(norms), moved);
    LOCATE_LAUNCH_CHECK("locate_nn_centroids");
    return LOCATE_OK;
}
