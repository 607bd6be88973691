// Exact nearest neighbours of images in the 8-bit domain: "generated sample | its nearest training images" and the distances
// behind it - the check for memorisation and collapse that no patch statistic can make.
//   nn_encode : fp32 [n, 3, S, S] -> per image one row of int8 codes (u - 128, u the byte the value quantises to), padded with
//               zeros to a multiple of 64 bytes, beside it the int64 sum of code^2 and the number of NaN / Inf elements;
//   nn_search : per query the k references with the smallest (d2, index), d2 = sum (code_q - code_r)^2 = |q|^2 + |r|^2 - 2 q.r
//               with the dot product on v_mfma_i32_32x32x32_i8 - integers throughout, so the Gram form is EXACT and the result
//               depends on nothing but the bytes.  Two launches: a tile kernel that walks whole rows and leaves each query's best
//               of the tile in the workspace, and a merge.  No atomics.
//   nn_within : per query the number of references whose ball it lies in (d2 <= radius2[r]), per reference the number of queries
//               in its ball - the counts behind precision / recall / density / coverage.  The same tile walk with a lighter end:
//               a comparison per pair, counts per block in the workspace, and a sum.  No atomics here either.
// Order: key = d2 * 2^30 + index as an unsigned 64-bit word - the lexicographic order of (d2, index) and the tie rule (lower index
// first) in one comparison.  index < 2^30 and d2 <= 255^2 row_bytes < 2^34 for rows up to NN_ROW_MAX bytes; the all-ones word is
// larger than every key and marks an empty slot.
#include "common.h"

#define NN_THREADS 256
#define NN_TQ 64                                   // queries per block of the tile kernel
#define NN_TR 128                                  // references per block
#define NN_STAGE 128                               // bytes of every row per stage
#define NN_LD (NN_STAGE + 16)                      // LDS row stride: 36 words - 16 lanes reading 16 bytes each hit 64 different banks
#define NN_KMAX 8
#define NN_SEGMENT 65536                           // bytes of a row per int32 accumulation: |dot| <= 128^2 65536 = 2^30
#define NN_INDEX_BITS 30
#define NN_ROW_MAX 262144                          // 255^2 262144 < 2^34: the key fits 64 bits
#define NN_EMPTY 0xFFFFFFFFFFFFFFFFull
#define NN_MERGE_THREADS 64

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long nn_key;

static inline int nn_row_bytes(int S) { return (int)(((int64_t)3 * S * S + 63) / 64 * 64); }

// ---- the encoder ---------------------------------------------------------------------------------------------------------------
// t = (x + 1) 127.5 in two fp32 roundings (spelled out: a contraction would round once), clamped to [0, 255], rounded to the nearest
// integer, ties to even; a NaN or an Inf gives the code byte 0 and is counted
__device__ __forceinline__ int nn_code(float x, int& bad) {
    if (!(fabsf(x) <= 3.402823466e38f)) {
        bad += 1;
        return 0;
    }
    const float t = __fmul_rn(__fadd_rn(x, 1.0f), 127.5f);
    const float u = t < 0.0f ? 0.0f : t > 255.0f ? 255.0f : rintf(t);
    return (int)u - 128;
}

// one block per image (grid-strided), one thread per 16-byte group of the row: four 16-byte loads, one 16-byte store.
// VEC: x is 16-byte aligned and 3 S^2 a multiple of 4, so every image starts aligned and a group of four lies wholly inside or
// outside the image.
template <bool VEC>
__global__ __launch_bounds__(NN_THREADS) void nn_encode_kernel(const float* __restrict__ x, int n, int elems, int row_bytes, int8_t* __restrict__ codes,
                                                               long long* __restrict__ norms, int* __restrict__ nonfinite) {
    __shared__ long long scratch_norm[16];
    __shared__ int scratch_bad[16];
    const int groups = row_bytes >> 4;
    for (int img = blockIdx.x; img < n; img += gridDim.x) {
        const float* px = x + (size_t)img * elems;
        int8_t* pc = codes + (size_t)img * row_bytes;
        long long norm = 0;
        int bad = 0;
        for (int g = threadIdx.x; g < groups; g += NN_THREADS) {
            const int e0 = 16 * g;
            float v[16];
            bool in[16];
            if (VEC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = e0 + 4 * i < elems;
                    const float4 f = ok ? *reinterpret_cast<const float4*>(px + e0 + 4 * i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
                    in[4 * i] = in[4 * i + 1] = in[4 * i + 2] = in[4 * i + 3] = ok;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    in[i] = e0 + i < elems;
                    v[i] = in[i] ? px[e0 + i] : 0.0f;
                }
            }
            int w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = in[i] ? nn_code(v[i], bad) : 0;          // the pad: code byte 0
                norm += c * c;
                w[i >> 2] |= (c & 255) << (8 * (i & 3));
            }
            *reinterpret_cast<int4*>(pc + e0) = make_int4(w[0], w[1], w[2], w[3]);
        }
        const long long tn = block_sum<long long>(norm, scratch_norm);
        const int tb = block_sum<int>(bad, scratch_bad);
        if (threadIdx.x == 0) {
            norms[img] = tn;
            nonfinite[img] = tb;
        }
    }
}

LOCATE_API int locate_nn_row_bytes(int S) { return S >= 1 && S <= 4096 ? nn_row_bytes(S) : 0; }

LOCATE_API int locate_nn_encode(const float* x, int n, int S, int8_t* codes, int64_t* norms, int32_t* nonfinite, void* stream) {
    LOCATE_REQUIRE(x && codes && norms && nonfinite, "locate_nn_encode: null pointer");
    LOCATE_REQUIRE(n >= 1 && S >= 1 && S <= 4096, "locate_nn_encode: n = %d, S = %d", n, S);
    LOCATE_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)codes & 15) == 0 && ((uintptr_t)norms & 7) == 0 && ((uintptr_t)nonfinite & 3) == 0,
                   "locate_nn_encode: x must be 4-byte, codes 16-byte, norms 8-byte, nonfinite 4-byte aligned");
    const int elems = 3 * S * S, row_bytes = nn_row_bytes(S);
    const bool vec = ((uintptr_t)x & 15) == 0 && elems % 4 == 0;
    const int grid = n < 65535 ? n : 65535;
    if (vec) nn_encode_kernel<true><<<grid, NN_THREADS, 0, as_stream(stream)>>>(x, n, elems, row_bytes, codes, reinterpret_cast<long long*>(norms), nonfinite);
    else nn_encode_kernel<false><<<grid, NN_THREADS, 0, as_stream(stream)>>>(x, n, elems, row_bytes, codes, reinterpret_cast<long long*>(norms), nonfinite);
    LOCATE_LAUNCH_CHECK("locate_nn_encode");
    return LOCATE_OK;
}

// ---- the search ----------------------------------------------------------------------------------------------------------------
// a sorted list of the NN_KMAX smallest keys seen: the new key bubbles through
__device__ __forceinline__ void nn_insert(nn_key (&best)[NN_KMAX], nn_key x) {
    if (x < best[NN_KMAX - 1]) {
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i) {
            const nn_key lo = x < best[i] ? x : best[i];
            x = x < best[i] ? best[i] : x;
            best[i] = lo;
        }
    }
}

// Block: 128 references (rows of the product) x 64 queries (columns), four waves of 32 references x 64 queries (two instructions
// of 32 x 32 x 32 per 32 bytes of row).  The queries are the columns because the accumulator has its column on the lane: a lane
// then holds 16 candidates of ONE query per instruction tile and selects among them in registers.
// Operands: lane l of an instruction reads the 16 bytes at offset 16 (l >> 5) of the 32-byte step of row l & 31 - of a reference
// row for A, of a query row for B.  Both read the same byte offsets, so whatever order the instruction gives the 32 products of a
// step, they are products of corresponding bytes.  Accumulator element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5),
// column l & 31.
// The row is walked in stages of 128 bytes, double-buffered as in swd_project_kernel: the 16-byte global loads of stage s are issued
// before the matrix instructions of stage s - 1 and written to LDS after them, one barrier per stage.  Rows are a multiple of 64
// bytes, not of 128: the last stage's upper half is zero on both sides.  Rows beyond N and Q are zero and masked at the end.
// SEGMENTED (rows longer than NN_SEGMENT bytes): the int32 accumulators are added into int64 sums every 512 stages.
#define NN_SMEM_BYTES (2 * (NN_TR + NN_TQ) * NN_LD)          // 55296 bytes: two blocks per CU

// The stage loop, once, for every kernel over the block tile.  It leaves the dot products of the block's 128 x 64 pairs in
// registers - sum[j][e] + acc[j][e], or acc[j][e] alone when not SEGMENTED - and ends on a barrier, so the caller may reuse
// smem at once.
template <bool SEGMENTED>
__device__ __forceinline__ void nn_tile_dots(const int8_t* __restrict__ qcodes, int Q, int q0, const int8_t* __restrict__ rcodes, int N, int r0, int row_bytes,
                                             unsigned char* smem, i32x16 (&acc)[2], long long (&sum)[2][SEGMENTED ? 16 : 1]) {
    unsigned char* Rs = smem;                                  // [2][NN_TR][NN_LD]
    unsigned char* Qs = smem + 2 * NN_TR * NN_LD;              // [2][NN_TQ][NN_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    const int stages = (row_bytes + NN_STAGE - 1) / NN_STAGE;
    // fill: thread t owns the 16 bytes at (t & 7) 16 of rows (t >> 3) + 32 i - eight lanes read 128 consecutive bytes of a row
    const int crow = tid >> 3, cbyte = (tid & 7) * 16;
    const int8_t* rsrc[4];
    const int8_t* qsrc[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) rsrc[i] = r0 + crow + 32 * i < N ? rcodes + (size_t)(r0 + crow + 32 * i) * row_bytes + cbyte : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i) qsrc[i] = q0 + crow + 32 * i < Q ? qcodes + (size_t)(q0 + crow + 32 * i) * row_bytes + cbyte : nullptr;

#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0;
#pragma unroll
        for (int e = 0; e < (SEGMENTED ? 16 : 1); ++e) sum[j][e] = 0;
    }
    const i32x4 zero = {0, 0, 0, 0};
    for (int s = 0; s <= stages; ++s) {
        i32x4 rv[4], qv[2];
        if (s < stages) {
            const bool inside = s * NN_STAGE + cbyte < row_bytes;          // a 16-byte group lies wholly inside the row or outside
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[i] = (inside && rsrc[i]) ? *reinterpret_cast<const i32x4*>(rsrc[i] + (size_t)s * NN_STAGE) : zero;
#pragma unroll
            for (int i = 0; i < 2; ++i) qv[i] = (inside && qsrc[i]) ? *reinterpret_cast<const i32x4*>(qsrc[i] + (size_t)s * NN_STAGE) : zero;
        }
        if (s > 0) {
            const int buf = (s - 1) & 1;
            const unsigned char* ra = Rs + (buf * NN_TR + 32 * wave + lrow) * NN_LD + 16 * lhalf;
            const unsigned char* qb = Qs + (buf * NN_TQ + lrow) * NN_LD + 16 * lhalf;
#pragma unroll
            for (int kk = 0; kk < NN_STAGE / 32; ++kk) {
                const i32x4 a = *reinterpret_cast<const i32x4*>(ra + 32 * kk);
                const i32x4 b0 = *reinterpret_cast<const i32x4*>(qb + 32 * kk);
                const i32x4 b1 = *reinterpret_cast<const i32x4*>(qb + 32 * NN_LD + 32 * kk);
                acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b1, acc[1], 0, 0, 0);
            }
            if (SEGMENTED && (s & (NN_SEGMENT / NN_STAGE - 1)) == 0) {          // s stages = a whole number of segments done
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        sum[j][SEGMENTED ? e : 0] += acc[j][e];
                        acc[j][e] = 0;
                    }
            }
        }
        if (s < stages) {
            const int buf = s & 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<i32x4*>(Rs + (buf * NN_TR + crow + 32 * i) * NN_LD + cbyte) = rv[i];
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<i32x4*>(Qs + (buf * NN_TQ + crow + 32 * i) * NN_LD + cbyte) = qv[i];
        }
        __syncthreads();
    }
}

template <bool SEGMENTED>
__global__ __launch_bounds__(NN_THREADS, 2) void nn_tile_kernel(const int8_t* __restrict__ qcodes, const long long* __restrict__ qnorms, const int* __restrict__ qflags,
                                                                int Q, const int8_t* __restrict__ rcodes, const long long* __restrict__ rnorms,
                                                                const int* __restrict__ rflags, int N, int row_bytes, const int* __restrict__ skip, int k,
                                                                nn_key* __restrict__ ws, int tiles) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[NN_SMEM_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    const int r0 = blockIdx.x * NN_TR, q0 = blockIdx.y * NN_TQ;
    i32x16 acc[2];
    long long sum[2][SEGMENTED ? 16 : 1];
    nn_tile_dots<SEGMENTED>(qcodes, Q, q0, rcodes, N, r0, row_bytes, smem, acc, sum);

    // d2 and this lane's best per query.  A reference is a candidate if it exists, is not flagged and is not the query's `skip`;
    // a flagged query has no candidates.
    long long rn[16];
    bool rok[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        rok[e] = r < N && (rflags == nullptr || rflags[r] == 0);
        rn[e] = r < N ? rnorms[r] : 0;
    }
    nn_key* lists = reinterpret_cast<nn_key*>(smem);          // [8 lane groups][NN_KMAX][NN_TQ]: 32 KiB of the staging buffers
    const int group = 2 * wave + lhalf;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + 32 * j + lrow;
        const bool qok = q < Q && qflags[q] == 0;
        const long long nq = q < Q ? qnorms[q] : 0;
        const int sk = (skip != nullptr && q < Q) ? skip[q] : -1;
        nn_key best[NN_KMAX];
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i) best[i] = NN_EMPTY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            const long long dot = SEGMENTED ? sum[j][SEGMENTED ? e : 0] + acc[j][e] : (long long)acc[j][e];
            const long long d2 = nq + rn[e] - 2 * dot;
            if (qok && rok[e] && r != sk) nn_insert(best, ((nn_key)d2 << NN_INDEX_BITS) | (nn_key)r);
        }
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i) lists[(group * NN_KMAX + i) * NN_TQ + 32 * j + lrow] = best[i];
    }
    __syncthreads();
    if (tid < NN_TQ && q0 + tid < Q) {
        nn_key best[NN_KMAX];
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i) best[i] = NN_EMPTY;
        for (int g = 0; g < 8; ++g)
#pragma unroll
            for (int i = 0; i < NN_KMAX; ++i) nn_insert(best, lists[(g * NN_KMAX + i) * NN_TQ + tid]);
        nn_key* out = ws + ((size_t)(q0 + tid) * tiles + blockIdx.x) * k;
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i)
            if (i < k) out[i] = best[i];
    }
}

// one block of 64 lanes per query: lane l takes tiles l, l + 64, ... in ascending order, lane 0 then the lanes' lists in lane order
__global__ __launch_bounds__(NN_MERGE_THREADS) void nn_merge_kernel(const nn_key* __restrict__ ws, int tiles, int k, long long* __restrict__ d2, int* __restrict__ index) {
    __shared__ nn_key lists[NN_KMAX][NN_MERGE_THREADS];
    const int q = blockIdx.x, lane = threadIdx.x;
    nn_key best[NN_KMAX];
#pragma unroll
    for (int i = 0; i < NN_KMAX; ++i) best[i] = NN_EMPTY;
    for (int t = lane; t < tiles; t += NN_MERGE_THREADS) {
        const nn_key* in = ws + ((size_t)q * tiles + t) * k;
        for (int i = 0; i < k; ++i) nn_insert(best, in[i]);
    }
#pragma unroll
    for (int i = 0; i < NN_KMAX; ++i) lists[i][lane] = best[i];
    __syncthreads();
    if (lane == 0) {
        const int lanes = tiles < NN_MERGE_THREADS ? tiles : NN_MERGE_THREADS;
        for (int l = 1; l < lanes; ++l)
#pragma unroll
            for (int i = 0; i < NN_KMAX; ++i) nn_insert(best, lists[i][l]);
#pragma unroll
        for (int i = 0; i < NN_KMAX; ++i)
            if (i < k) {
                const bool empty = best[i] == NN_EMPTY;
                d2[(size_t)q * k + i] = empty ? -1 : (long long)(best[i] >> NN_INDEX_BITS);
                index[(size_t)q * k + i] = empty ? -1 : (int)(best[i] & ((1u << NN_INDEX_BITS) - 1));
            }
    }
}

static int nn_search_check(const char* name, int Q, int N, int k) {
    LOCATE_REQUIRE(Q >= 1 && Q <= NN_TQ * 65535, "%s: Q = %d", name, Q);
    LOCATE_REQUIRE(N >= 1 && (int64_t)N < ((int64_t)1 << NN_INDEX_BITS), "%s: N = %d (1 .. 2^30 - 1)", name, N);
    LOCATE_REQUIRE(k >= 1 && k <= NN_KMAX, "%s: k = %d (1 .. %d)", name, k, NN_KMAX);
    return LOCATE_OK;
}

LOCATE_API size_t locate_nn_search_workspace_bytes(int Q, int N, int k) {
    if (Q < 1 || N < 1 || k < 1 || k > NN_KMAX) return 0;
    return (size_t)Q * (size_t)cdiv64(N, NN_TR) * (size_t)k * sizeof(nn_key);
}

LOCATE_API int locate_nn_search(const int8_t* qcodes, const int64_t* qnorms, const int32_t* qflags, int Q, const int8_t* rcodes, const int64_t* rnorms,
                                const int32_t* rflags, int N, int row_bytes, const int32_t* skip, int k, int64_t* d2, int32_t* index, void* workspace,
                                void* stream) {
    LOCATE_REQUIRE(qcodes && qnorms && qflags && rcodes && rnorms && d2 && index && workspace, "locate_nn_search: null pointer");
    if (int e = nn_search_check("locate_nn_search", Q, N, k)) return e;
    LOCATE_REQUIRE(row_bytes >= 64 && row_bytes % 64 == 0 && row_bytes <= NN_ROW_MAX, "locate_nn_search: row_bytes = %d (a multiple of 64 up to %d)", row_bytes,
                   NN_ROW_MAX);
    LOCATE_REQUIRE((((uintptr_t)qcodes | (uintptr_t)rcodes) & 15) == 0, "locate_nn_search: the code banks must be 16-byte aligned");
    LOCATE_REQUIRE((((uintptr_t)qnorms | (uintptr_t)rnorms | (uintptr_t)d2 | (uintptr_t)workspace) & 7) == 0, "locate_nn_search: norms, d2 and workspace must be 8-byte aligned");
    LOCATE_REQUIRE((((uintptr_t)qflags | (uintptr_t)rflags | (uintptr_t)skip | (uintptr_t)index) & 3) == 0, "locate_nn_search: flags, skip and index must be 4-byte aligned");
    const int tiles = (int)cdiv64(N, NN_TR);
    const dim3 grid((unsigned)tiles, (unsigned)cdiv64(Q, NN_TQ));
    hipStream_t st = as_stream(stream);
    nn_key* ws = static_cast<nn_key*>(workspace);
    const long long* qn = reinterpret_cast<const long long*>(qnorms);
    const long long* rn = reinterpret_cast<const long long*>(rnorms);
    if (row_bytes > NN_SEGMENT) nn_tile_kernel<true><<<grid, NN_THREADS, 0, st>>>(qcodes, qn, qflags, Q, rcodes, rn, rflags, N, row_bytes, skip, k, ws, tiles);
    else nn_tile_kernel<false><<<grid, NN_THREADS, 0, st>>>(qcodes, qn, qflags, Q, rcodes, rn, rflags, N, row_bytes, skip, k, ws, tiles);
    LOCATE_LAUNCH_CHECK("locate_nn_search (tiles)");
    nn_merge_kernel<<<Q, NN_MERGE_THREADS, 0, st>>>(ws, tiles, k, reinterpret_cast<long long*>(d2), index);
    LOCATE_LAUNCH_CHECK("locate_nn_search");
    return LOCATE_OK;
}

// ---- which balls is each query in ----------------------------------------------------------------------------------------------
// The pair (q, r) counts if q is not flagged, r exists, is not flagged, has a ball (radius2[r] >= 0) and is not the query's `skip`,
// and d2 <= radius2[r] in int64.  A lane holds 2 x 16 such booleans.
//   per query     : a lane adds its 16; the 8 lane groups (4 waves x 2 halves) meet in the staging LDS and thread t adds them for
//                   query t - as the search does with its lists;
//   per reference : a reference row lives in one wave - element e of the lanes of one half - so the wave's ballot of element e
//                   holds the row of half 0 in its low word and the row of half 1 in its high word, for both query tiles: four
//                   popcounts, no LDS.  Lane 16 h + e keeps the count of element e, half h, and stores it.
// Each block writes its counts to hits_ws [Q][tiles_r] and cov_ws [N][tiles_q]; every word of both is written.
template <bool SEGMENTED>
__global__ __launch_bounds__(NN_THREADS, 2) void nn_within_kernel(const int8_t* __restrict__ qcodes, const long long* __restrict__ qnorms, const int* __restrict__ qflags,
                                                                  int Q, const int8_t* __restrict__ rcodes, const long long* __restrict__ rnorms,
                                                                  const int* __restrict__ rflags, int N, int row_bytes, const long long* __restrict__ radius2,
                                                                  const int* __restrict__ skip, int* __restrict__ hits_ws, int tiles_r,
                                                                  int* __restrict__ cov_ws, int tiles_q) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[NN_SMEM_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lhalf = lane >> 5;
    const int r0 = blockIdx.x * NN_TR, q0 = blockIdx.y * NN_TQ;
    i32x16 acc[2];
    long long sum[2][SEGMENTED ? 16 : 1];
    nn_tile_dots<SEGMENTED>(qcodes, Q, q0, rcodes, N, r0, row_bytes, smem, acc, sum);

    long long rn[16], rad[16];
    bool rok[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        rn[e] = r < N ? rnorms[r] : 0;
        rad[e] = r < N ? radius2[r] : -1;
        rok[e] = r < N && (rflags == nullptr || rflags[r] == 0) && rad[e] >= 0;
    }
    bool in[2][16];
    int* counts = reinterpret_cast<int*>(smem);          // [8 lane groups][NN_TQ]
    const int group = 2 * wave + lhalf;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + 32 * j + lrow;
        const bool qok = q < Q && qflags[q] == 0;
        const long long nq = q < Q ? qnorms[q] : 0;
        const int sk = (skip != nullptr && q < Q) ? skip[q] : -1;
        int mine = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            const long long dot = SEGMENTED ? sum[j][SEGMENTED ? e : 0] + acc[j][e] : (long long)acc[j][e];
            const long long d2 = nq + rn[e] - 2 * dot;
            in[j][e] = qok && rok[e] && r != sk && d2 <= rad[e];
            mine += in[j][e] ? 1 : 0;
        }
        counts[group * NN_TQ + 32 * j + lrow] = mine;
    }
    if (cov_ws != nullptr) {          // the same for every lane of the grid: the ballots below are of whole waves
        int kept = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned long long b0 = __ballot(in[0][e]), b1 = __ballot(in[1][e]);
            const int lo = __popc((unsigned)b0) + __popc((unsigned)b1);
            const int hi = __popc((unsigned)(b0 >> 32)) + __popc((unsigned)(b1 >> 32));
            if ((lane & 15) == e) kept = (lane & 16) ? hi : lo;
        }
        const int e = lane & 15, h = (lane >> 4) & 1;
        const int r = r0 + 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (lane < 32 && r < N) cov_ws[(size_t)r * tiles_q + blockIdx.y] = kept;
    }
    __syncthreads();
    if (tid < NN_TQ && q0 + tid < Q) {
        int total = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) total += counts[g * NN_TQ + tid];
        hits_ws[(size_t)(q0 + tid) * tiles_r + blockIdx.x] = total;
    }
}

// one thread per output word: the first Q add a query's tiles, the next N (if wanted) a reference's, in ascending tile order
__global__ __launch_bounds__(NN_THREADS) void nn_within_sum_kernel(const int* __restrict__ hits_ws, int Q, int tiles_r, int* __restrict__ hits,
                                                                   const int* __restrict__ cov_ws, int N, int tiles_q, int* __restrict__ covered) {
    const long long i = (long long)blockIdx.x * NN_THREADS + threadIdx.x;
    const bool query = i < Q;
    if (!query && (cov_ws == nullptr || i - Q >= N)) return;
    const int* in = query ? hits_ws + (size_t)i * tiles_r : cov_ws + (size_t)(i - Q) * tiles_q;
    const int tiles = query ? tiles_r : tiles_q;
    int total = 0;
    for (int t = 0; t < tiles; ++t) total += in[t];
    if (query) hits[i] = total;
    else covered[i - Q] = total;
}

LOCATE_API size_t locate_nn_within_workspace_bytes(int Q, int N, int want_covered) {
    if (Q < 1 || N < 1) return 0;
    const size_t per_query = (size_t)Q * (size_t)cdiv64(N, NN_TR) * sizeof(int32_t);
    return per_query + (want_covered ? (size_t)N * (size_t)cdiv64(Q, NN_TQ) * sizeof(int32_t) : 0);
}

LOCATE_API int locate_nn_within(const int8_t* qcodes, const int64_t* qnorms, const int32_t* qflags, int Q, const int8_t* rcodes, const int64_t* rnorms,
                                const int32_t* rflags, int N, int row_bytes, const int64_t* radius2, const int32_t* skip, int32_t* hits, int32_t* covered,
                                void* workspace, void* stream) {
    LOCATE_REQUIRE(qcodes && qnorms && qflags && rcodes && rnorms && radius2 && hits && workspace, "locate_nn_within: null pointer");
    LOCATE_REQUIRE(Q >= 1 && Q <= NN_TQ * 65535, "locate_nn_within: Q = %d", Q);
    LOCATE_REQUIRE(N >= 1 && (int64_t)N < ((int64_t)1 << NN_INDEX_BITS), "locate_nn_within: N = %d (1 .. 2^30 - 1)", N);
    LOCATE_REQUIRE(row_bytes >= 64 && row_bytes % 64 == 0 && row_bytes <= NN_ROW_MAX, "locate_nn_within: row_bytes = %d (a multiple of 64 up to %d)", row_bytes,
                   NN_ROW_MAX);
    LOCATE_REQUIRE((((uintptr_t)qcodes | (uintptr_t)rcodes) & 15) == 0, "locate_nn_within: the code banks must be 16-byte aligned");
    LOCATE_REQUIRE((((uintptr_t)qnorms | (uintptr_t)rnorms | (uintptr_t)radius2) & 7) == 0, "locate_nn_within: norms and radius2 must be 8-byte aligned");
    LOCATE_REQUIRE((((uintptr_t)qflags | (uintptr_t)rflags | (uintptr_t)skip | (uintptr_t)hits | (uintptr_t)covered | (uintptr_t)workspace) & 3) == 0,
                   "locate_nn_within: flags, skip, hits, covered and workspace must be 4-byte aligned");
    const int tiles_r = (int)cdiv64(N, NN_TR), tiles_q = (int)cdiv64(Q, NN_TQ);
    const dim3 grid((unsigned)tiles_r, (unsigned)tiles_q);
    hipStream_t st = as_stream(stream);
    int* hits_ws = static_cast<int*>(workspace);
    int* cov_ws = covered ? hits_ws + (size_t)Q * tiles_r : nullptr;
    const long long* qn = reinterpret_cast<const long long*>(qnorms);
    const long long* rn = reinterpret_cast<const long long*>(rnorms);
    const long long* rad = reinterpret_cast<const long long*>(radius2);
    if (row_bytes > NN_SEGMENT) nn_within_kernel<true><<<grid, NN_THREADS, 0, st>>>(qcodes, qn, qflags, Q, rcodes, rn, rflags, N, row_bytes, rad, skip, hits_ws, tiles_r, cov_ws, tiles_q);
    else nn_within_kernel<false><<<grid, NN_THREADS, 0, st>>>(qcodes, qn, qflags, Q, rcodes, rn, rflags, N, row_bytes, rad, skip, hits_ws, tiles_r, cov_ws, tiles_q);
    LOCATE_LAUNCH_CHECK("locate_nn_within (tiles)");
    const long long words = (long long)Q + (covered ? N : 0);
    nn_within_sum_kernel<<<(unsigned)cdiv64(words, NN_THREADS), NN_THREADS, 0, st>>>(hits_ws, Q, tiles_r, hits, cov_ws, N, tiles_q, covered);
    LOCATE_LAUNCH_CHECK("locate_nn_within");
    return LOCATE_OK;
}
