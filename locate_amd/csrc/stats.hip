// Per-tensor statistics of a whole network with a non-finite guard (locate_amd/stats.py): for every tensor of a device table
//   sumsq     (float64)  sum of (double) x * (double) x over the FINITE elements - the square of an fp32 value is exact in fp64,
//                        so the only roundings are those of the additions;
//   absmax    (fp32)     the largest magnitude among the finite elements (0 if there is none), taken as an integer maximum of
//                        bits & 0x7fffffff - order-preserving for finite values, so exact; denormals count;
//   nonfinite (uint32)   the elements whose exponent field is all ones: NaN of either sign and any payload, +-Inf;
// and per call one summary {uint32 total non-finite count, int32 index of the first tensor in table order that has one, or -1}.
// Driven by a chunk table (multitensor.h); like the averaged generator (average.hip) a kernel of
// its own that runs BETWEEN two training iterations and only READS what the step left.  The reference has nothing of the kind.
//
// Two launches.  (1) locate_stats_partial_kernel: one block per 4096-element chunk writes that chunk's partial {sumsq, absmax,
// count} to workspace[position of the chunk in the chunk table].  (2) locate_stats_combine_kernel: one block per tensor adds the
// partials of its chunks in a fixed order and writes the record.  A second small launch was chosen over a last-block-done stage
// inside the first: it needs no arrival counters (which would have to be zeroed before every call, by one more node on the stream),
// no release / acquire fences between blocks and no second read path for partials another XCD wrote; the price is one launch
// boundary (~2 us) behind a kernel that runs for tens of microseconds.
//
// A record depends only on its tensor's contents and length - not on the grid, on the tensor's position in the table, on what else
// the table holds, nor on the tensor's alignment: a chunk is read in multitensor.h's fixed lanes (mt_read_lanes: an element belongs
// to the same thread whether it arrived by a 16-byte or a 4-byte load) and every sum has the one order of multitensor.h's
// mt_block_total and mt_add_partials.  Missing elements of a short chunk enter as +0.0, which changes none of the three results.
// No floating-point atomics; the summary is built with integer atomics (an add and a minimum: order-free, so deterministic).
//
// A pure bandwidth kernel (4 bytes per element, ~3 operations): 16-byte loads where the chunk is 16-byte aligned, a full chunk's
// four loads in flight per thread before the first use, at most 2048 blocks (256 CUs x 8) that stride over the chunk table.
#include "multitensor.h"

struct StatsTensor {
    const float* x;
    long long n;
    int first_chunk;          // position of this tensor's chunk 0 in the chunk table; its chunks follow in order
    int pad;
};

typedef MtPartial StatsRecord;          // {sumsq, absmax, nonfinite}: a chunk's partial and a tensor's record alike

__global__ void __launch_bounds__(MT_THREADS) locate_stats_partial_kernel(const StatsTensor* __restrict__ tensors,
                                                                            const int2* __restrict__ chunks, int n_tensors, int n_chunks,
                                                                            StatsRecord* __restrict__ partials, unsigned* __restrict__ summary) {
    __shared__ StatsRecord lds[MT_WAVES];
    if (blockIdx.x == 0 && threadIdx.x == 0) {          // the combine launch behind this one adds into it
        summary[0] = 0u;
        summary[1] = 0xffffffffu;          // -1: no tensor has a non-finite element
    }
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int2 ch = chunks[c];
        StatsTensor T;
        long long begin;
        int len;
        // a damaged table writes nothing
        if (!mt_decode(tensors, n_tensors, ch, T, begin, len) || (long long)T.first_chunk + ch.y != c) continue;
        float4 v[MT_PER_THREAD];
        mt_read_lanes(T.x + begin, len, v);
        StatsRecord r = {0.0, 0u, 0u};
#pragma unroll
        for (int k = 0; k < MT_PER_THREAD; ++k) mt_take4(v[k], r.sumsq, r.absmax, r.nonfinite);
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) partials[c] = r;          // c < n_chunks: inside the workspace
    }
}

__global__ void __launch_bounds__(MT_THREADS) locate_stats_combine_kernel(const StatsTensor* __restrict__ tensors, int n_tensors, int n_chunks,
                                                                            const StatsRecord* __restrict__ partials,
                                                                            StatsRecord* __restrict__ records, unsigned* __restrict__ summary) {
    __shared__ StatsRecord lds[MT_WAVES];
    for (int t = blockIdx.x; t < n_tensors; t += gridDim.x) {
        const StatsTensor T = tensors[t];
        if (T.n <= 0 || T.first_chunk < 0) continue;          // a damaged table writes nothing
        const long long nc = (T.n + MT_CHUNK - 1) / MT_CHUNK;
        if ((long long)T.first_chunk + nc > n_chunks) continue;
        StatsRecord r = {0.0, 0u, 0u};
        mt_add_partials(partials + T.first_chunk, (int)nc, r);
        r = mt_block_total(r, lds);
        if (threadIdx.x == 0) {
            records[t] = r;
            if (r.nonfinite) {          // integer atomics: the result does not depend on the order of arrival
                atomicAdd(&summary[0], r.nonfinite);
                atomicMin(&summary[1], (unsigned)t);
            }
        }
    }
}

LOCATE_API size_t locate_stats_tensor_record_bytes(void) { return sizeof(StatsTensor); }
LOCATE_API size_t locate_stats_record_bytes(void) { return sizeof(StatsRecord); }
LOCATE_API int locate_stats_chunk_elems(void) { return MT_CHUNK; }
LOCATE_API int locate_stats_max_blocks(void) { return mt_grid(0x7fffffff); }
LOCATE_API size_t locate_stats_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(StatsRecord) : 0; }

// tensors: DEVICE array of n_tensors records {x, n, first_chunk}; chunks: DEVICE array of n_chunks (tensor index, chunk index) int
// pairs, a tensor's chunks consecutive and in order from position first_chunk.  Writes records[0 .. n_tensors), summary[0 .. 2)
// and workspace[0 .. locate_stats_workspace_bytes(n_chunks)), nothing else.  No allocation, no host read, no synchronisation:
// legal under stream capture.
LOCATE_API int locate_stats_reduce(const void* tensors, const void* chunks, int n_tensors, int n_chunks, void* records, void* summary,
                                   void* workspace, void* stream) {
    LOCATE_REQUIRE(tensors && chunks && records && summary && workspace && n_tensors > 0 && n_chunks > 0, "locate_stats_reduce: bad arguments");
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0 &&
                       (reinterpret_cast<uintptr_t>(summary) & 3) == 0, "locate_stats_reduce: records and workspace need 8-byte alignment");
    const StatsTensor* T = static_cast<const StatsTensor*>(tensors);
    locate_stats_partial_kernel<<<mt_grid(n_chunks), MT_THREADS, 0, as_stream(stream)>>>(T, static_cast<const int2*>(chunks), n_tensors, n_chunks,
                                                                             static_cast<StatsRecord*>(workspace), static_cast<unsigned*>(summary));
    LOCATE_LAUNCH_CHECK("locate_stats_reduce");
    locate_stats_combine_kernel<<<mt_grid(n_tensors), MT_THREADS, 0, as_stream(stream)>>>(T, n_tensors, n_chunks, static_cast<const StatsRecord*>(workspace),
                                                                             static_cast<StatsRecord*>(records), static_cast<unsigned*>(summary));
    LOCATE_LAUNCH_CHECK("locate_stats_reduce");
    return LOCATE_OK;
}
