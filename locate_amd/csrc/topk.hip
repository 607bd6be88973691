// Top-k training of the generator (Sinha et al. 2020, "Top-k Training of GANs: Improving GAN Performance by Throwing Away Bad
// Samples"): in the G-step only the k fakes with the highest D(G(z)) contribute to the loss and its gradient.  One single-block kernel
// (locate_amd/topk.py, TopK; the definition in numpy, which the kernel equals with ==: tests/helpers/topk_model.py): locate_g_loss's
// launch with the selection in it - values, gradients, the record's statistics and one ring row all come out of it.
//
// k comes from a record of TOPK_STATE_WORDS 32-bit words at a fixed device address, so a replayed graph follows the host's schedule:
//   0 k (int32; the host writes it, the kernel only reads it; not in 1 .. B: k_used = B, the plain loss)   1 launches
//   2 launches whose logits held a NaN or an Inf   3 k_used   4 kept elements with (1 - f) >= 0   5 threshold, the fp32 bits of the
//   kept element of rank k_used - 1   6 mean_all = (float)(sum f / B)   7 mean_kept = (float)(sum_kept f / k_used)   8 .. 15 zero.
// A ring row: TOPK_RING_WORDS words {launch ordinal (1-based), k_used, active, threshold, mean_all, mean_kept, non-finite 0 / 1, 0}
// at slot (ordinal - 1) % capacity.  The ordinal lives on the device: a captured launch cannot take an iteration number.
//
// The order: j stands before i iff f_j is a NaN and f_i is not; or both are NaNs and j < i; or neither is and f_j > f_i; or neither
// is, f_j == f_i (-0 == +0) and j < i.  rank_i = the number of elements before i; i is kept iff rank_i < k_used.  Both selection
// forms below realise it through topk_key(), an unsigned word that orders like the logit with every NaN on top and -0 folded onto +0.
// No allocation, no host read, no atomics, values written by ordinary vector stores; legal under stream capture.
#include "gloss.h"

#define TOPK_STATE_WORDS 16
#define TOPK_RING_WORDS 8
#define TOPK_THREADS 256
#define TOPK_MAX_B 4096
#define TOPK_FORM_AUTO 0
#define TOPK_FORM_RANK 1          // every element counts the elements before it: B^2 comparisons on broadcast LDS reads, no barrier
#define TOPK_FORM_SORT 2          // bitonic sort of {key, ~index}: log2(B) (log2(B) + 1) / 2 steps with a barrier each
// TOPK_FORM_AUTO sorts from this B on (profiles/notes_topk.md)
#define TOPK_SORT_FROM 512

// > 0 for every logit: the smallest is -Inf's 0x007FFFFF, so 0 pads below everything and key - 1 never wraps
__device__ __forceinline__ unsigned topk_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    const unsigned b = v == 0.0f ? 0u : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The number of elements before element i = tid + TOPK_THREADS * m.  keys: n words, n a multiple of 4 * TOPK_BATCH, zero from B on.
// For j < i equality counts (key_j > key_i - 1), for j > i it does not; both hold for a whole group of TOPK_THREADS indices below
// and above the block's own, where the bound is uniform, and in the block's own group the bound is chosen per j.  Every lane reads
// the same address (a broadcast).  The loops stay small on purpose: unrolled eight quads deep, and with the tail's four divisions in
// a row, the launch measured 0.2 - 0.4 us longer at 64 logits, where it counts (profiles/notes_topk.md).
#define TOPK_BATCH 2
__device__ __forceinline__ int topk_padded(int B) { return (B + 4 * TOPK_BATCH - 1) & ~(4 * TOPK_BATCH - 1); }
template <int OWN>
__device__ __forceinline__ unsigned topk_count(const uint4* quads, int from, int to, int i, unsigned key) {
    unsigned count = 0;
#pragma unroll 1
    for (int q = from; q < to; q += TOPK_BATCH) {
        uint4 w[TOPK_BATCH];
#pragma unroll
        for (int u = 0; u < TOPK_BATCH; ++u) w[u] = quads[q + u];
#pragma unroll
        for (int u = 0; u < TOPK_BATCH; ++u) {
            const int j = 4 * (q + u);
            const unsigned b0 = OWN ? key - (unsigned)(j < i) : key, b1 = OWN ? key - (unsigned)(j + 1 < i) : key;
            const unsigned b2 = OWN ? key - (unsigned)(j + 2 < i) : key, b3 = OWN ? key - (unsigned)(j + 3 < i) : key;
            count += (unsigned)(w[u].x > b0) + (unsigned)(w[u].y > b1) + (unsigned)(w[u].z > b2) + (unsigned)(w[u].w > b3);
        }
    }
    return count;
}

__device__ __forceinline__ unsigned topk_rank(const unsigned* keys, int n, int m, int i, unsigned key) {
    const uint4* quads = reinterpret_cast<const uint4*>(keys);
    const int lo = m * (TOPK_THREADS / 4), hi = min(lo + TOPK_THREADS / 4, n >> 2);
    return topk_count<0>(quads, 0, lo, i, key - 1u) + topk_count<1>(quads, lo, hi, i, key) + topk_count<0>(quads, hi, n >> 2, i, key);
}

template <int FORM>
__global__ void __launch_bounds__(TOPK_THREADS) g_loss_topk_kernel(const float* __restrict__ f, int B, unsigned* __restrict__ record,
                                                                   unsigned* __restrict__ ring, int capacity, float* __restrict__ losses,
                                                                   float* __restrict__ gf) {
    constexpr int WAVES = TOPK_THREADS / 64;
    __shared__ float vals[TOPK_MAX_B];
    __shared__ __attribute__((aligned(16))) unsigned keys[FORM == TOPK_FORM_RANK ? TOPK_MAX_B : 4];
    __shared__ unsigned long long sorted[FORM == TOPK_FORM_SORT ? TOPK_MAX_B : 1];
    __shared__ unsigned short rank_of[FORM == TOPK_FORM_SORT ? TOPK_MAX_B : 1];
    __shared__ double scratch[5 * WAVES];
    __shared__ unsigned threshold;
    const int tid = threadIdx.x;
    // asked for ahead of everything else: behind a cold cache every dependent load is another trip to memory
    const int k = (int)record[0];
    unsigned launches = 0u, nonfinite = 0u;
    if (tid == 0) {
        launches = record[1];
        nonfinite = record[2];
    }
    if (FORM == TOPK_FORM_RANK) {
        const int n = topk_padded(B);
        for (int i = tid; i < n; i += TOPK_THREADS) {
            const float v = i < B ? f[i] : 0.0f;
            if (i < B) vals[i] = v;
            keys[i] = i < B ? topk_key(v) : 0u;
        }
        __syncthreads();
    } else {
        int n = 2;
        while (n < B) n <<= 1;
        for (int i = tid; i < n; i += TOPK_THREADS) {
            const float v = i < B ? f[i] : 0.0f;
            if (i < B) vals[i] = v;
            sorted[i] = i < B ? ((unsigned long long)topk_key(v) << 32) | (unsigned)~i : 0ull;          // descending: lower index first
        }
        __syncthreads();
        for (int span = 2; span <= n; span <<= 1) {
            for (int j = span >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n >> 1); t += TOPK_THREADS) {
                    const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const bool descending = (a & span) == 0;
                    const unsigned long long x = sorted[a], y = sorted[b];
                    if ((x < y) == descending) {
                        sorted[a] = y;
                        sorted[b] = x;
                    }
                }
                __syncthreads();
            }
        }
        for (int p = tid; p < B; p += TOPK_THREADS) rank_of[~(unsigned)sorted[p]] = (unsigned short)p;          // the pads sort behind
        __syncthreads();
    }
    const int k_used = (k >= 1 && k <= B) ? k : B;
    const float inv = 1.0f / (float)k_used;
    double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // hinge kept, hinge all, f all, f kept, active + 65536 * non-finite
    for (int m = 0, i = tid; i < B; ++m, i += TOPK_THREADS) {
        const float v = vals[i];
        unsigned rank;
        if (FORM == TOPK_FORM_RANK) rank = topk_rank(keys, topk_padded(B), m, i, keys[i]);
        else rank = rank_of[i];
        const bool kept = rank < (unsigned)k_used;
        const double h = g_hinge_term(v);
        sums[1] += h;
        sums[2] += (double)v;
        if (kept) {
            sums[0] += h;
            sums[3] += (double)v;
            if (g_hinge_passes(v)) sums[4] += 1.0;
        }
        if (!(fabsf(v) <= 3.402823466e38f)) sums[4] += 65536.0;          // an Inf or a NaN; both counts stay exact integers
        gf[i] = kept ? g_hinge_grad(v, inv) : 0.0f;
        if (rank == (unsigned)(k_used - 1)) threshold = __float_as_uint(v);          // exactly one element: the ranks are a permutation
    }
    block_sums<5, WAVES>(sums, scratch);          // its barriers also publish `threshold`
    if (tid >= 64) return;
    // the four quotients, each (float)(sum / n) as g_hinge_mean spells it, in four lanes of one division instead of four in a row
    const double numerator = tid == 0 ? sums[0] : tid == 1 ? sums[1] : tid == 2 ? sums[2] : sums[3];
    const float quotient = g_hinge_mean(numerator, (tid == 0 || tid == 3) ? k_used : B);
    const float loss_topk = __shfl(quotient, 0, 64), loss_all = __shfl(quotient, 1, 64);
    const float mean_all = __shfl(quotient, 2, 64), mean_kept = __shfl(quotient, 3, 64);
    if (tid != 0) return;
    const unsigned counts = (unsigned)sums[4];
    const unsigned active = counts & 0xFFFFu, bad = counts >> 16 ? 1u : 0u, cut = threshold;
    losses[0] = loss_topk;
    losses[1] = loss_all;
    unsigned* row = ring + (size_t)(launches % (unsigned)capacity) * TOPK_RING_WORDS;
    row[0] = launches + 1u;
    row[1] = (unsigned)k_used;
    row[2] = active;
    row[3] = cut;
    row[4] = __float_as_uint(mean_all);
    row[5] = __float_as_uint(mean_kept);
    row[6] = bad;
    row[7] = 0u;
    record[1] = launches + 1u;
    record[2] = nonfinite + bad;
    record[3] = (unsigned)k_used;
    record[4] = active;
    record[5] = cut;
    record[6] = __float_as_uint(mean_all);
    record[7] = __float_as_uint(mean_kept);
}

// d_fake: fp32 [B] raw logits D(G(z)), 1 <= B <= 4096; record: the 16 words above (word 0 is read, words 1 .. 7 are written); ring:
// `capacity` rows of 8 words; losses: 2 floats {loss_topk, loss_all}; g_fake: [B], the gradient of loss_topk.  form: 0 chooses the
// selection by B, 1 counts ranks, 2 sorts - the same bits either way.  With k_used == B losses[0], losses[1] and g_fake are
// locate_g_loss's bits; losses[1] always is.
LOCATE_API int locate_g_loss_topk(const float* d_fake, int B, void* record, void* ring, int capacity, int form, float* losses, float* g_fake,
                                  void* stream) {
    LOCATE_REQUIRE(d_fake && record && ring && losses && g_fake, "locate_g_loss_topk: null buffers");
    LOCATE_REQUIRE(B >= 1 && B <= TOPK_MAX_B, "locate_g_loss_topk: B = %d must be in 1 .. %d", B, TOPK_MAX_B);
    LOCATE_REQUIRE(capacity > 0, "locate_g_loss_topk: capacity = %d must be positive", capacity);
    LOCATE_REQUIRE(form >= TOPK_FORM_AUTO && form <= TOPK_FORM_SORT, "locate_g_loss_topk: form = %d must be 0 (by size), 1 (rank) or 2 (sort)",
                   form);
    LOCATE_REQUIRE(((reinterpret_cast<uintptr_t>(d_fake) | reinterpret_cast<uintptr_t>(record) | reinterpret_cast<uintptr_t>(ring) |
                     reinterpret_cast<uintptr_t>(losses) | reinterpret_cast<uintptr_t>(g_fake)) & 3) == 0,
                   "locate_g_loss_topk: buffers must be 4-byte aligned");
    if (form == TOPK_FORM_AUTO) form = B >= TOPK_SORT_FROM ? TOPK_FORM_SORT : TOPK_FORM_RANK;
    if (form == TOPK_FORM_RANK)
        g_loss_topk_kernel<TOPK_FORM_RANK><<<1, TOPK_THREADS, 0, as_stream(stream)>>>(d_fake, B, static_cast<unsigned*>(record),
                                                                                      static_cast<unsigned*>(ring), capacity, losses, g_fake);
    else
        g_loss_topk_kernel<TOPK_FORM_SORT><<<1, TOPK_THREADS, 0, as_stream(stream)>>>(d_fake, B, static_cast<unsigned*>(record),
                                                                                      static_cast<unsigned*>(ring), capacity, losses, g_fake);
    LOCATE_LAUNCH_CHECK("locate_g_loss_topk");
    return LOCATE_OK;
}
