// How far one iteration moved every tensor of a network (locate_amd/dynamics.py): for every tensor of a device table the delta
// d[i] = w[i] - base[i] - ONE fp32 subtraction per element, denormals kept - against a copy `base` the caller keeps in an arena of
// its own, reduced to one 32-byte record
//   delta_sumsq  (float64)  sum of (double) d * (double) d over the FINITE d - each square is exact in fp64, only the additions round;
//   base_sumsq   (float64)  the same sum over the finite base[i];
//   delta_absmax (uint32)   bit pattern of the largest finite |d| (0 if there is none), an integer maximum of bits & 0x7fffffff;
//   unchanged    (uint32)   elements with w[i] == base[i] as an fp32 comparison: +0 == -0 counts, a NaN never does;
//   nonfinite    (uint32)   elements whose d is NaN or +-Inf; they are left out of the two delta fields;
//   pad          (uint32)   0
// and / or to the copy itself, base[i] = w[i] bit for bit (NaN payloads included), which starts the next window.  Driven by a chunk
// table (multitensor.h); a kernel of its own that runs BETWEEN two training iterations and only READS what the step left.  The
// reference has nothing of the kind.
//
// MODE (a template parameter): DYN_RECORD (1) writes the records and only reads base; DYN_REBASE (2) copies and writes no record;
// 3 does both in one pass - every thread stores after its own loads of the same elements, so the record describes the old base.
//
// Two launches on the chunk-table layer of multitensor.h.  (1) locate_dyn_partial_kernel: one block per 4096-element chunk, at
// most mt_grid blocks striding over the chunk table, writes that chunk's partial record to workspace[position of the chunk in the
// chunk table]; w and base are read together in fixed lanes (mt_read_lanes: 16-byte loads where BOTH are 16-byte aligned at the
// chunk, 4-byte ones otherwise) and the copy is written the same way (mt_write_lanes).  (2) locate_dyn_combine_kernel: one block
// per tensor adds the partials of its chunks in a fixed order and writes the record.  DYN_REBASE alone is the first launch only
// and touches neither records nor workspace.
//
// A record depends only on its tensor's contents and length - not on the grid, on the tensor's position in the table, on what else
// the table holds, nor on the alignment of w or base: an element belongs to the same thread however it was loaded, and every sum
// has the one order of multitensor.h's mt_block_total and mt_add_partials.  No floating-point atomics, no atomics at all.
// Missing elements of a short chunk enter as w = base = +0.0: they change neither sum nor the maximum nor the non-finite count,
// and thread 0 takes their number off the chunk's `unchanged`.
//
// A bandwidth kernel (8 bytes read per element in mode 1, 4 read and 4 written in mode 2): a full chunk's eight 16-byte loads in
// flight per thread before the first use.  Ordinary stores (profiles/notes_snapshot.md could not tell them from nontemporal ones).
#include "multitensor.h"

#define DYN_RECORD 1
#define DYN_REBASE 2

struct DynTensor {
    const float* w;          // the live tensor
    float* base;          // its slot in the caller's arena
    long long n;
    int first_chunk;          // position of this tensor's chunk 0 in the chunk table; its chunks follow in order
    int pad;
};

struct DynRecord {          // a chunk's partial and a tensor's record alike
    double delta_sumsq;
    double base_sumsq;
    unsigned delta_absmax;          // bit pattern of a non-negative finite fp32
    unsigned unchanged;
    unsigned nonfinite;
    unsigned pad;
    __device__ __forceinline__ void add(const DynRecord& q) {
        delta_sumsq += q.delta_sumsq;
        base_sumsq += q.base_sumsq;
        delta_absmax = q.delta_absmax > delta_absmax ? q.delta_absmax : delta_absmax;
        unchanged += q.unchanged;
        nonfinite += q.nonfinite;
    }
};

__device__ __forceinline__ void dyn_take(float w, float b, DynRecord& r) {
    const float d = __fsub_rn(w, b);
    const unsigned dmag = __float_as_uint(d) & 0x7fffffffu, bmag = __float_as_uint(b) & 0x7fffffffu;
    const bool dfin = dmag < 0x7f800000u, bfin = bmag < 0x7f800000u;
    const double dd = dfin ? (double)d : 0.0, bb = bfin ? (double)b : 0.0;
    r.delta_sumsq = fma(dd, dd, r.delta_sumsq);          // exact squares: one rounding, that of the addition
    r.base_sumsq = fma(bb, bb, r.base_sumsq);
    r.delta_absmax = dfin && dmag > r.delta_absmax ? dmag : r.delta_absmax;
    r.unchanged += w == b ? 1u : 0u;
    r.nonfinite += dfin ? 0u : 1u;
}

__device__ __forceinline__ void dyn_take4(float4 w, float4 b, DynRecord& r) {
    dyn_take(w.x, b.x, r);
    dyn_take(w.y, b.y, r);
    dyn_take(w.z, b.z, r);
    dyn_take(w.w, b.w, r);
}

template <int MODE>
__global__ void __launch_bounds__(MT_THREADS) locate_dyn_partial_kernel(const DynTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                                                                          int n_tensors, int n_chunks, DynRecord* __restrict__ partials) {
    constexpr bool REC = (MODE & DYN_RECORD) != 0, COPY = (MODE & DYN_REBASE) != 0;
    __shared__ DynRecord lds[MT_WAVES];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int2 ch = chunks[c];
        DynTensor T;
        long long begin;
        int len;
        // a damaged table writes nothing
        if (!mt_decode(tensors, n_tensors, ch, T, begin, len) || (long long)T.first_chunk + ch.y != c || !T.w || !T.base) continue;
        float4 v[2][MT_PER_THREAD];          // w, and base when recording
        const float* const src[2] = {T.w + begin, T.base + begin};
        if (REC) mt_read_lanes(src, len, v);          // the loads ahead of the store: the record describes the old base
        else mt_read_lanes(src[0], len, v[0]);
        if (COPY) mt_write_lanes(T.base + begin, len, v[0]);
        if (REC) {
            DynRecord r = {0.0, 0.0, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < MT_PER_THREAD; ++k) dyn_take4(v[0][k], v[1][k], r);
            r = mt_block_total(r, lds);
            if (threadIdx.x == 0) {
                r.unchanged -= (unsigned)(MT_CHUNK - len);          // the +0.0 == +0.0 of a short chunk's missing elements
                r.pad = 0u;
                partials[c] = r;          // c < n_chunks: inside the workspace
            }
        }
    }
}

__global__ void __launch_bounds__(MT_THREADS) locate_dyn_combine_kernel(const DynTensor* __restrict__ tensors, int n_tensors, int n_chunks,
                                                                          const DynRecord* __restrict__ partials, DynRecord* __restrict__ records) {
    __shared__ DynRecord lds[MT_WAVES];
    for (int t = blockIdx.x; t < n_tensors; t += gridDim.x) {
        const DynTensor T = tensors[t];
        if (T.n <= 0 || T.first_chunk < 0 || !T.w || !T.base) continue;          // a damaged table writes nothing
        const long long nc = (T.n + MT_CHUNK - 1) / MT_CHUNK;
        if ((long long)T.first_chunk + nc > n_chunks) continue;
        DynRecord r = {0.0, 0.0, 0u, 0u, 0u, 0u};
        mt_add_partials(partials + T.first_chunk, (int)nc, r);
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) {
            r.pad = 0u;
            records[t] = r;
        }
    }
}

LOCATE_API size_t locate_dyn_tensor_record_bytes(void) { return sizeof(DynTensor); }
LOCATE_API size_t locate_dyn_record_bytes(void) { return sizeof(DynRecord); }
LOCATE_API int locate_dyn_chunk_elems(void) { return MT_CHUNK; }
LOCATE_API int locate_dyn_max_blocks(void) { return mt_grid(0x7fffffff); }
LOCATE_API size_t locate_dyn_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(DynRecord) : 0; }

// tensors: DEVICE array of n_tensors records {w, base, n, first_chunk}; chunks: DEVICE array of n_chunks (tensor index, chunk
// index) int pairs, a tensor's chunks consecutive and in order from position first_chunk.  mode 1 writes records[0 .. n_tensors)
// and workspace[0 .. locate_dyn_workspace_bytes(n_chunks)); mode 2 writes every tensor's base[0 .. n) and takes null records and
// workspace; mode 3 writes all three.  Nothing else is written.  No allocation, no host read, no synchronisation: legal under
// stream capture.
LOCATE_API int locate_dyn_pass(const void* tensors, const void* chunks, int n_tensors, int n_chunks, int mode, void* records, void* workspace,
                               void* stream) {
    LOCATE_REQUIRE(tensors && chunks && n_tensors > 0 && n_chunks > 0, "locate_dyn_pass: bad arguments");
    LOCATE_REQUIRE(mode >= 1 && mode <= 3, "locate_dyn_pass: mode %d is none of 1 (record), 2 (rebase), 3 (both)", mode);
    if (mode & DYN_RECORD) {
        LOCATE_REQUIRE(records && workspace, "locate_dyn_pass: a recording mode needs records and a workspace");
        LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                       "locate_dyn_pass: records and workspace need 8-byte alignment");
    }
    const DynTensor* T = static_cast<const DynTensor*>(tensors);
    const int2* C = static_cast<const int2*>(chunks);
    DynRecord* P = static_cast<DynRecord*>(workspace);
    hipStream_t st = as_stream(stream);
    if (mode == DYN_RECORD) locate_dyn_partial_kernel<DYN_RECORD><<<mt_grid(n_chunks), MT_THREADS, 0, st>>>(T, C, n_tensors, n_chunks, P);
    else if (mode == DYN_REBASE) locate_dyn_partial_kernel<DYN_REBASE><<<mt_grid(n_chunks), MT_THREADS, 0, st>>>(T, C, n_tensors, n_chunks, nullptr);
    else locate_dyn_partial_kernel<DYN_RECORD | DYN_REBASE><<<mt_grid(n_chunks), MT_THREADS, 0, st>>>(T, C, n_tensors, n_chunks, P);
    LOCATE_LAUNCH_CHECK("locate_dyn_pass");
    if (mode & DYN_RECORD) {
        locate_dyn_combine_kernel<<<mt_grid(n_tensors), MT_THREADS, 0, st>>>(T, n_tensors, n_chunks, P, static_cast<DynRecord*>(records));
        LOCATE_LAUNCH_CHECK("locate_dyn_pass");
    }
    return LOCATE_OK;
}
