// Panel packing of the dense contractions: re-lays a weight tensor [M, C, KH, KW] out as the panel(s) conv.hip planned for it
// (conv_plan / win_finish fill one PackArgs per phase; panel layout: igemm.h) - K-major fp32 rows with the gather offset tables,
// the bf16 / fp16 / fp8 piece planes, or the window kernels' unit-ordered planes.  One panel per launch (launch_pack) or all
// panels of a network in one (locate_conv_pack_panels over the jobs locate_conv_pack_job wrote).
#include "igemm.h"

__device__ __forceinline__ void pack_tables(const PackArgs& a, int k) {
    int* koff = reinterpret_cast<int*>(a.out + (size_t)a.rows * a.ld);
    unsigned char* ktap = reinterpret_cast<unsigned char*>(koff + a.rows);
    const int T = a.TH * a.TW;
    int off = 0, tap = 31;
    if (k < a.K && T > 0) {
        const int c = k / T, t = k - c * T;
        const int th = t / a.TW, tw = t - th * a.TW;
        off = 4 * (c * a.gHW + (a.dy0 + a.dys * th) * a.gW + a.dx0 + a.dxs * tw - a.dmin);
        tap = t;
    }
    koff[k] = off;
    ktap[k] = (unsigned char)tap;
}

// fp16-piece panels: a packing block folds the largest magnitude of the weights it handled into the header word of its
// phase(s) (atomic max on the bit pattern, skipped when the word already holds as much: after the first few blocks almost
// every one).  A block of the adjoint packer handles all sub-pixel phases of its weights and reports to each of them the
// maximum over ALL its taps - an upper bound of the phase's own, which is all the scale exponent needs.
__device__ __forceinline__ void pack_publish_absmax(float m, const PackArgs* phases, int nphase, float* red) {
    m = wave_max(m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned bits = __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
        for (int i = 0; i < nphase; ++i) {
            const PackArgs& a = phases[i];
            if (!a.fmt) continue;
            unsigned* word = reinterpret_cast<unsigned*>(a.out + panel_split_offset_dev(a.rows, a.ld));
            if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                (void)__hip_atomic_fetch_max(word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#define PACK_SMEM (256 * (PACK_MAX_TAPS + 1))      // floats; also holds the 64 x 65 transpose tile

// direct form: one chunk of 8 consecutive k for one column -> the panel's planes (two scaled fp16 pieces, or three bf16 pieces)
__device__ __forceinline__ void pack_emit_chunk(const PackArgs& a, const float (&v)[8], float sc, int64_t i) {
    const int64_t plane = (int64_t)(a.rows / 8) * a.ld;
    uint4* w3 = reinterpret_cast<uint4*>(a.out + panel_split_offset_dev(a.rows, a.ld) + (a.fmt ? PANEL_HDR : 0));
    if (a.fmt == 2) {          // fp8 plane: 16-k chunks - this 8-k chunk is one half (8 bytes) of chunk (kb8 / 2, column)
        const int64_t kb8 = i / a.ld, col = i - kb8 * a.ld;
        int t0 = 0, t1 = 0;
        t0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * sc, v[1] * sc, t0, false);
        t0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * sc, v[3] * sc, t0, true);
        t1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * sc, v[5] * sc, t1, false);
        t1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * sc, v[7] * sc, t1, true);
        reinterpret_cast<uint2*>(w3)[2 * ((kb8 >> 1) * a.ld + col) + (kb8 & 1)] = make_uint2((unsigned)t0, (unsigned)t1);
    } else if (a.fmt) {
        uint4 h, l;
        split2_f16x8(v, sc, h, l);
        w3[i] = h;
        w3[plane + i] = l;
    } else {
        bf16x8 h, m, l;
        split3_bf16x8(v, h, m, l);
        w3[i] = *reinterpret_cast<uint4*>(&h);
        w3[plane + i] = *reinterpret_cast<uint4*>(&m);
        w3[2 * plane + i] = *reinterpret_cast<uint4*>(&l);
    }
}

// generic element-wise form (any tap count): virtual grid (nbx, nphase)
__device__ __forceinline__ void pack_generic_body(const PackBatch& batch, int bx, int by, int nbx, float* smem) {
    const PackArgs& a = batch.ph[by];
    const int64_t total = (int64_t)a.rows * a.ld;
    const int64_t stride = (int64_t)nbx * 256;
    const int T = a.TH * a.TW;
    float am = 0.0f;
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += stride) {
        const int k = (int)(i / a.ld), col = (int)(i - (int64_t)k * a.ld);
        float v = 0.0f;
        if (k < a.K) {
            if (a.mode == 0) {
                if (col < a.M) {
                    const int c = k / T, t = k - c * T;
                    const int th = t / a.TW, tw = t - th * a.TW;
                    v = a.w[(((int64_t)col * a.C + c) * a.KH + a.kh0 + th) * a.KW + a.kw0 + tw];
                }
            } else {
                if (col < a.C) {
                    const int m = k / T, r = k - m * T;
                    const int th = r / a.TW, tw = r - th * a.TW;
                    const int kh = a.kh0 + a.s * th, kw = a.kw0 + a.s * tw;
                    v = a.w[(((int64_t)m * a.C + col) * a.KH + kh) * a.KW + kw];
                }
            }
        }
        a.out[i] = v;
        am = fmaxf(am, fabsf(v));
    }
    for (int64_t k = (int64_t)bx * 256 + threadIdx.x; k < a.rows; k += stride) pack_tables(a, (int)k);
    if (a.fmt) pack_publish_absmax(am, &a, 1, smem);
}

// mode 0 (R forward): the panel is the transpose of W viewed as [M][K]: 64 x 64 tiles through LDS, both the read
// (along k) and the write (along m) are coalesced.  virtual grid (rows / 64, ld / 64).
__device__ __forceinline__ void pack_transpose_body(const PackArgs& a, int bx, int by, float* smem) {
    float (*tile)[65] = reinterpret_cast<float (*)[65]>(smem);
    const int k0 = bx * 64, m0 = by * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float am = 0.0f;
    // this thread's reduction index k = (c, th, tw) inside a weight row [C][KH][KW]: k itself when the panel holds every tap, else
    // the tap sub-rectangle's position (layers whose maps mostly see padding: the reads then stay inside each channel's window)
    const int k = k0 + tx, T = a.TH * a.TW;
    int src = k;
    if (T != a.KH * a.KW && k < a.K) {
        const int c = k / T, t = k - c * T;
        const int th = t / a.TW, tw = t - th * a.TW;
        src = (c * a.KH + a.kh0 + th) * a.KW + a.kw0 + tw;
    }
    const int64_t wrow = (int64_t)a.C * a.KH * a.KW;
    for (int j = ty; j < 64; j += 4) {
        const int m = m0 + j;
        const float v = (m < a.M && k < a.K) ? a.w[(int64_t)m * wrow + src] : 0.0f;
        tile[j][tx] = v;
        am = fmaxf(am, fabsf(v));
    }
    __syncthreads();
    if (a.direct) {
        // direct form: the tile's 8 k-blocks x 64 columns as piece chunks, two per thread; consecutive threads write
        // consecutive 16-byte chunks of a plane row
        const unsigned bits = a.fmt ? absmax_read(a.wmax) : 0u;
        const float sc = pow2f(a.fmt == 2 ? f8_scale_exp(bits) : f16_scale_exp(bits));
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int kb = (threadIdx.x >> 6) + 4 * q, m = m0 + tx;
            if (k0 + kb * 8 < a.rows && m < a.ld) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = tile[tx][kb * 8 + e];
                pack_emit_chunk(a, v, sc, (int64_t)(k0 / 8 + kb) * a.ld + m);
            }
        }
        if (a.fmt && bx == 0 && by == 0 && threadIdx.x == 0) *reinterpret_cast<unsigned*>(a.out + panel_split_offset_dev(a.rows, a.ld)) = bits;
        if (!a.keep_f32) return;
    }
    for (int j = ty; j < 64; j += 4) {
        const int k = k0 + j, m = m0 + tx;
        if (k < a.rows && m < a.ld) a.out[(int64_t)k * a.ld + m] = tile[tx][j];
    }
    if (a.direct) return;               // tables and header: from the panel's first (two-pass) packing / written above
    if (by == 0 && threadIdx.x < 64 && k0 + (int)threadIdx.x < a.rows) pack_tables(a, k0 + threadIdx.x);
    if (a.fmt) pack_publish_absmax(am, &a, 1, smem + 64 * 65);       // PACK_SMEM floats: room behind the tile
}

// Direct form of the adjoint packer (see PackArgs::wmax): a block stages eight weight rows m x 32 channels (all taps) in LDS
// - eight contiguous reads - and writes, for every sub-pixel phase, the chunks of 8 consecutive k = (m, tap) it now holds for
// its 32 columns: 8 T / 8 = T chunks per phase and column, 512-byte runs per plane row.  virtual grid (ld / 32, ceil(M / 8)).
#define PACKD_MB 8
static_assert(8704 >= PACK_SMEM, "direct packing reuses the packers' LDS block");
#define PACKD_SMEM 8704           // floats: 8 rows x 64 channels x up to 16 (+1) taps, or x 32 channels for up to 32 taps (34 KB:
                                  // four blocks per CU - the packers are bandwidth kernels, a larger block cost them occupancy)
static inline __host__ __device__ int packd_cs(int KK) { return PACKD_MB * 64 * (KK | 1) <= PACKD_SMEM ? 64 : 32; }
__device__ __forceinline__ void pack_adjoint_direct_body(const PackBatch& batch, int nphase, int bx, int by, float* lds) {
    const PackArgs& a0 = batch.ph[0];
    const int KK = a0.KH * a0.KW, S = KK | 1;
    const int CS = packd_cs(KK);
    const int m0 = by * PACKD_MB, c0 = bx * CS;
    const int cn = min(CS, a0.C - c0);
    const DivU32 dk((unsigned)KK);
    if (cn > 0) {
        const int run = cn * KK;
#pragma unroll
        for (int mm = 0; mm < PACKD_MB; ++mm) {
            if (m0 + mm >= a0.M) break;
            const float* src = a0.w + ((int64_t)(m0 + mm) * a0.C + c0) * KK;
            for (int idx = threadIdx.x; idx < run; idx += 256) {
                unsigned cl, t;
                dk.divmod((unsigned)idx, cl, t);
                lds[(mm * CS + (int)cl) * S + (int)t] = src[idx];
            }
        }
    }
    __syncthreads();
    const unsigned bits = a0.fmt ? absmax_read(a0.wmax) : 0u;
    const float sc = pow2f(a0.fmt == 2 ? f8_scale_exp(bits) : f16_scale_exp(bits));
    // work items (phase, chunk, column), columns fastest: T chunks of 8 rows k = (m, tap) per phase for this block's 8 m
    int tsum = 0;
    for (int ph = 0; ph < nphase; ++ph) tsum += batch.ph[ph].TH * batch.ph[ph].TW;
    const int csh = CS == 64 ? 6 : 5;
    for (int it = threadIdx.x; it < (tsum << csh); it += 256) {
        const int cl = it & (CS - 1);
        int ch = it >> csh, ph = 0;
        while (ch >= batch.ph[ph].TH * batch.ph[ph].TW) { ch -= batch.ph[ph].TH * batch.ph[ph].TW; ++ph; }
        const PackArgs& a = batch.ph[ph];
        const int T = a.TH * a.TW, col = c0 + cl;
        if (col >= a.ld || (by * T + ch) * 8 >= a.rows) continue;          // (the last row group may reach past the zero tail)
        int mm = (ch * 8) / T, r = ch * 8 - mm * T;
        int th = r / a.TW, tw = r - th * a.TW;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int t = (a.kh0 + a.s * th) * a.KW + a.kw0 + a.s * tw;
            v[e] = (m0 + mm < a.M && cl < cn) ? lds[(mm * CS + cl) * S + t] : 0.0f;
            if (++tw == a.TW) { tw = 0; if (++th == a.TH) { th = 0; ++mm; } }
        }
        pack_emit_chunk(a, v, sc, (int64_t)(by * T + ch) * a.ld + col);
        if (a.keep_f32) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a.out[(int64_t)((by * T + ch) * 8 + e) * a.ld + col] = v[e];
        }
    }
    if (a0.fmt && bx == 0 && by == 0 && threadIdx.x < nphase)
        *reinterpret_cast<unsigned*>(batch.ph[threadIdx.x].out + panel_split_offset_dev(batch.ph[threadIdx.x].rows, batch.ph[threadIdx.x].ld)) = bits;
}

// mode 1 (data adjoint, all sub-pixel phases at once): for one m, W[m] is a [C][KH*KW] matrix; a block stages 256
// channels of it in LDS (contiguous read) and writes, per tap, one 256-wide piece of the row (m, tap) of the phase
// that owns the tap.  by == M: zero tail rows and the offset tables.  virtual grid (ld / 256, M + 1).
__device__ __forceinline__ void pack_adjoint_body(const PackBatch& batch, int nphase, int bx, int by, float* lds) {
    const PackArgs& a0 = batch.ph[0];
    const int KK = a0.KH * a0.KW, S = KK | 1;
    const int m = by, c0 = bx * 256;
    const int col = c0 + threadIdx.x;
    float am = 0.0f;
    if (m < a0.M) {
        const int cn = min(256, a0.C - c0);
        if (cn > 0) {
            const float* src = a0.w + ((int64_t)m * a0.C + c0) * KK;
            const int total = cn * KK;
            for (int idx = threadIdx.x; idx < total; idx += 256) {
                const int cl = idx / KK, t = idx - cl * KK;
                const float v = src[idx];
                lds[cl * S + t] = v;
                am = fmaxf(am, fabsf(v));
            }
        }
        __syncthreads();
        for (int ph = 0; ph < nphase; ++ph) {
            const PackArgs& a = batch.ph[ph];
            if (col >= a.ld) continue;
            const int T = a.TH * a.TW;
            for (int r = 0; r < T; ++r) {
                const int th = r / a.TW, tw = r - th * a.TW;
                const int t = (a.kh0 + a.s * th) * a.KW + a.kw0 + a.s * tw;
                a.out[((int64_t)m * T + r) * a.ld + col] = (int)threadIdx.x < cn ? lds[threadIdx.x * S + t] : 0.0f;
            }
        }
        if (a0.fmt) pack_publish_absmax(am, batch.ph, nphase, lds + 256 * (PACK_MAX_TAPS + 1) - 8);
        return;
    }
    for (int ph = 0; ph < nphase; ++ph) {
        const PackArgs& a = batch.ph[ph];
        if (col < a.ld)
            for (int k = a.K; k < a.rows; ++k) a.out[(int64_t)k * a.ld + col] = 0.0f;
        if (bx == 0)
            for (int k = threadIdx.x; k < a.rows; k += 256) pack_tables(a, k);
    }
}


// second packing pass: the fp32 K-major rows of a panel -> its three bf16 planes (16-byte chunks of 8 consecutive k), or
// its two scaled fp16 planes
__device__ __forceinline__ void pack_split_body(const PackArgs& a, int bx, int nbx) {
    if (a.direct || a.win) return;     // direct form / window panels: the packing blocks wrote the planes
    const float* w = a.out;
    uint4* w3 = reinterpret_cast<uint4*>(a.out + panel_split_offset_dev(a.rows, a.ld) + (a.fmt ? PANEL_HDR : 0));
    const int64_t stride = (int64_t)nbx * 256;
    if (a.fmt == 2) {          // fp8: chunks of 16 consecutive k, e4m3 bytes of w * 2^k(absmax)
        const float sc = pow2f(f8_scale_exp(*reinterpret_cast<const unsigned*>(a.out + panel_split_offset_dev(a.rows, a.ld))));
        const int64_t total16 = (int64_t)(a.rows / 16) * a.ld;
        for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total16; i += stride) {
            const int kb = (int)(i / a.ld), col = (int)(i - (int64_t)kb * a.ld);
            unsigned wq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = w[(int64_t)(kb * 16 + 4 * q + j) * a.ld + col] * sc;
                int t = 0;
                t = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], t, false);
                t = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], t, true);
                wq[q] = (unsigned)t;
            }
            w3[i] = make_uint4(wq[0], wq[1], wq[2], wq[3]);
        }
        return;
    }
    const int64_t total = (int64_t)(a.rows / 8) * a.ld;
    if (a.fmt) {
        const float sc = pow2f(f16_scale_exp(*reinterpret_cast<const unsigned*>(a.out + panel_split_offset_dev(a.rows, a.ld))));
        for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += stride) {
            const int kb = (int)(i / a.ld), col = (int)(i - (int64_t)kb * a.ld);
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)(kb * 8 + j) * a.ld + col];
            uint4 h, l;
            split2_f16x8(v, sc, h, l);
            w3[i] = h;
            w3[total + i] = l;
        }
        return;
    }
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += stride) {
        const int kb = (int)(i / a.ld), col = (int)(i - (int64_t)kb * a.ld);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)(kb * 8 + j) * a.ld + col];
        bf16x8 h, m, l;
        split3_bf16x8(v, h, m, l);
        w3[i] = *reinterpret_cast<uint4*>(&h);
        w3[total + i] = *reinterpret_cast<uint4*>(&m);
        w3[2 * total + i] = *reinterpret_cast<uint4*>(&l);
    }
}

// ---------------------------------------------------------------------------------------------
// Window panels (PackArgs::win; convwin.hip): chunk rows in unit order u = c8g * Tp + t - the 8 reduction channels of group c8g
// at tap t - piece planes only.  A block stages RG reduction channels x CS columns x all taps of the weight tensor in LDS
// (contiguous runs: RG KK floats per column in the regular direction, CS KK floats per reduction channel in the adjoint one)
// and writes, for every phase, the chunks (t, c8) of its columns; the last row of blocks also writes the zero rows behind the
// last unit.  Always one pass: the scale of fp16-piece planes comes from the optimizer's absmax words or from the panel's own
// header (win_absmax_jobs_kernel ran first).  virtual grid (ceil(ld / CS), ceil(reduction channels / RG)).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_win_emit(const PackArgs& a, const float (&v)[8], float sc, int64_t i) {
    const int64_t plane = (int64_t)a.urows * a.ld;
    uint4* w3 = reinterpret_cast<uint4*>(a.out + PANEL_HDR);
    if (a.fmt) {
        uint4 h, l;
        split2_f16x8(v, sc, h, l);
        w3[i] = h;
        w3[plane + i] = l;
    } else {
        bf16x8 h, m, l;
        split3_bf16x8(v, h, m, l);
        w3[i] = *reinterpret_cast<uint4*>(&h);
        w3[plane + i] = *reinterpret_cast<uint4*>(&m);
        w3[2 * plane + i] = *reinterpret_cast<uint4*>(&l);
    }
}

__device__ __forceinline__ void pack_win_body(const PackBatch& batch, int nphase, int bx, int by, int gy, float* lds) {
    const PackArgs& a0 = batch.ph[0];
    const int KK = a0.KH * a0.KW, S = KK | 1;
    const int CS = KK <= 4 ? 64 : (KK <= 16 ? 32 : 16), RG = win_pack_rg(KK);
    const int Cred = a0.mode == 0 ? a0.C : a0.M, ncol = a0.mode == 0 ? a0.M : a0.C;
    const int r0 = by * RG, col0 = bx * CS;
    const int rn = min(RG, Cred - r0), cn = min(CS, ncol - col0);
    if (rn > 0 && cn > 0) {
        const DivU32 dk((unsigned)KK);
        if (a0.mode == 0) {          // w[col][r][t]: per column a run of rn KK floats
            const int run = rn * KK;
            const DivU32 dr((unsigned)run);
            for (int idx = threadIdx.x; idx < cn * run; idx += 256) {
                unsigned col, rem, r, t;
                dr.divmod((unsigned)idx, col, rem);
                dk.divmod(rem, r, t);
                lds[((int)r * CS + (int)col) * S + (int)t] = a0.w[((int64_t)(col0 + (int)col) * a0.C + r0) * KK + rem];
            }
        } else {                     // w[r][col][t]: per reduction channel a run of cn KK floats
            const int run = cn * KK;
            const DivU32 dr((unsigned)run);
            for (int idx = threadIdx.x; idx < rn * run; idx += 256) {
                unsigned r, rem, col, t;
                dr.divmod((unsigned)idx, r, rem);
                dk.divmod(rem, col, t);
                lds[((int)r * CS + (int)col) * S + (int)t] = a0.w[((int64_t)(r0 + (int)r) * a0.C + col0) * KK + rem];
            }
        }
    }
    __syncthreads();
    unsigned bits = 0u;
    if (a0.fmt) bits = a0.wmax_single ? (unsigned)__builtin_amdgcn_readfirstlane((int)*a0.wmax) : absmax_read(a0.wmax);
    const float sc = pow2f(f16_scale_exp(bits));
    const int csh = CS == 64 ? 6 : (CS == 32 ? 5 : 4);
    const int ng8 = RG / 8;
    for (int ph = 0; ph < nphase; ++ph) {
        const PackArgs& a = batch.ph[ph];
        const int T = a.TH * a.TW;
        // work items (unit row of this block, column), columns fastest
        const int nrow = ng8 * a.Tp;
        for (int it = threadIdx.x; it < (nrow << csh); it += 256) {
            const int cl = it & (CS - 1), row = it >> csh;
            const int c8 = row / a.Tp, t = row - c8 * a.Tp;
            const int col = col0 + cl;
            const int u = (r0 / 8 + c8) * a.Tp + t;
            if (col >= a.ld || u >= a.urows) continue;
            float v[8];
            const bool tap_ok = t < T && cl < cn;
            int tapidx = 0;
            if (tap_ok) {
                const int th = t / a.TW, tw = t - th * a.TW;
                tapidx = (a.kh0 + a.s * th) * a.KW + a.kw0 + a.s * tw;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (tap_ok && c8 * 8 + e < rn) ? lds[((c8 * 8 + e) * CS + cl) * S + tapidx] : 0.0f;
            pack_win_emit(a, v, sc, (int64_t)u * a.ld + col);
        }
        if (by == gy - 1) {          // zero rows behind this block's last unit (padding groups of single-tap layers, the tail)
            const int u0 = (r0 / 8 + ng8) * a.Tp;
            const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int it = threadIdx.x; it < ((a.urows - u0) << csh); it += 256) {
                const int cl = it & (CS - 1), u = u0 + (it >> csh);
                if (col0 + cl < a.ld) pack_win_emit(a, z, 1.0f, (int64_t)u * a.ld + col0 + cl);
            }
        }
        if (a.fmt && !a.wmax_single && bx == 0 && by == 0 && threadIdx.x == 0) *reinterpret_cast<unsigned*>(a.out) = bits;
    }
}

PackJob make_pack_job(const PackBatch& b, int nphase) {
    PackJob j;
    j.batch = b; j.nphase = nphase; j.block_start = 0; j.pad = 0;
    const PackArgs& a0 = b.ph[0];
    if (a0.win) {
        const int KK = a0.KH * a0.KW;
        j.kind = 4; j.gx = (a0.ld + win_pack_cs(KK) - 1) / win_pack_cs(KK);
        j.gy = ((a0.mode == 0 ? a0.C : a0.M) + win_pack_rg(KK) - 1) / win_pack_rg(KK);
    } else if (a0.mode == 0 && nphase == 1) {
        j.kind = 0; j.gx = (a0.rows + 63) / 64; j.gy = (a0.ld + 63) / 64;
    } else if (a0.mode == 1 && a0.KH * a0.KW <= PACK_MAX_TAPS && a0.direct) {
        j.kind = 3; j.gx = (a0.ld + packd_cs(a0.KH * a0.KW) - 1) / packd_cs(a0.KH * a0.KW); j.gy = (a0.M + PACKD_MB - 1) / PACKD_MB;
    } else if (a0.mode == 1 && a0.KH * a0.KW <= PACK_MAX_TAPS) {
        j.kind = 1; j.gx = (a0.ld + 255) / 256; j.gy = a0.M + 1;
    } else {
        int64_t big = 1;
        for (int i = 0; i < nphase; ++i) {
            const int64_t t = (int64_t)b.ph[i].rows * b.ph[i].ld;
            if (t > big) big = t;
        }
        j.kind = 2; j.gx = stream_grid(big, 256); j.gy = nphase;
    }
    return j;
}

__device__ __forceinline__ void pack_job_body(const PackJob& j, int local, float* smem) {
    const int bx = local % j.gx, by = local / j.gx;
    if (j.kind == 0) pack_transpose_body(j.batch.ph[0], bx, by, smem);
    else if (j.kind == 1) pack_adjoint_body(j.batch, j.nphase, bx, by, smem);
    else if (j.kind == 3) pack_adjoint_direct_body(j.batch, j.nphase, bx, by, smem);
    else if (j.kind == 4) pack_win_body(j.batch, j.nphase, bx, by, j.gy, smem);
    else pack_generic_body(j.batch, bx, by, j.gx, smem);
}

__global__ void __launch_bounds__(256) pack_job_kernel(const PackJob job) {
    __shared__ float smem[PACKD_SMEM];
    pack_job_body(job, blockIdx.x, smem);
}

#define PACK_SPLIT_BLOCKS 256
__global__ void __launch_bounds__(256) pack_split_kernel(const PackJob job) {
    if ((int)blockIdx.y < job.nphase) pack_split_body(job.batch.ph[blockIdx.y], blockIdx.x, gridDim.x);
}

// fp16-piece panels only: zero the absmax words (one thread per (job, phase)), then take the maxima
__device__ __forceinline__ void pack_clear_one(const PackJob& j, int ph) {
    if (ph < j.nphase && j.batch.ph[ph].fmt && !j.batch.ph[ph].direct) {
        const PackArgs& a = j.batch.ph[ph];
        unsigned* hdr = reinterpret_cast<unsigned*>(a.win ? a.out : a.out + panel_split_offset_dev(a.rows, a.ld));
        hdr[0] = 0u; hdr[1] = 0u; hdr[2] = 0u; hdr[3] = 0u;
    }
}
// window panels of fp16 pieces packed without the optimizer's absmax words: the largest weight magnitude goes into every phase's
// header word first (the packing blocks read it from there).  blockIdx.y = job.
__device__ __forceinline__ void win_absmax_body(const PackJob& j, int bx, int nbx) {
    const PackArgs& a0 = j.batch.ph[0];
    if (j.kind != 4 || !a0.fmt || !a0.wmax_single) return;
    __shared__ float red[16];
    const int64_t total = (int64_t)a0.M * a0.C * a0.KH * a0.KW;
    float am = 0.0f;
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += (int64_t)nbx * 256) am = fmaxf(am, fabsf(a0.w[i]));
    am = block_max(am, red);
    if (threadIdx.x == 0) {
        const unsigned bits = __float_as_uint(am);
        for (int ph = 0; ph < j.nphase; ++ph) {
            unsigned* word = reinterpret_cast<unsigned*>(j.batch.ph[ph].out);
            if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                (void)__hip_atomic_fetch_max(word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
#define WIN_ABSMAX_BLOCKS 64
__global__ void __launch_bounds__(256) win_absmax_kernel(const PackJob job) { win_absmax_body(job, blockIdx.x, gridDim.x); }
__global__ void __launch_bounds__(256) win_absmax_jobs_kernel(const PackJob* __restrict__ jobs) { win_absmax_body(jobs[blockIdx.y], blockIdx.x, gridDim.x); }
__global__ void __launch_bounds__(64) pack_clear_kernel(const PackJob job) { if (threadIdx.x < 4) pack_clear_one(job, threadIdx.x); }
__global__ void __launch_bounds__(64) pack_clear_jobs_kernel(const PackJob* __restrict__ jobs, int n_jobs) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < 4 * n_jobs) pack_clear_one(jobs[i >> 2], i & 3);
}
// blockIdx.y = job, blockIdx.z = phase
__global__ void __launch_bounds__(256) pack_split_jobs_kernel(const PackJob* __restrict__ jobs) {
    const PackJob& j = jobs[blockIdx.y];
    if ((int)blockIdx.z < j.nphase) pack_split_body(j.batch.ph[blockIdx.z], blockIdx.x, gridDim.x);
}

// many panels in one launch: `jobs` (device) sorted by block_start; a block finds its job by bisection
__global__ void __launch_bounds__(256) pack_jobs_kernel(const PackJob* __restrict__ jobs, int n_jobs) {
    __shared__ float smem[PACKD_SMEM];
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block_start <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PackJob& j = jobs[lo];
    pack_job_body(j, blockIdx.x - j.block_start, smem);
}

// all phases of one panel in a single launch
int launch_pack(const PackBatch& b, int nphase, hipStream_t st, const char* who) {
    const PackJob j = make_pack_job(b, nphase);
    if (b.ph[0].fmt) pack_clear_kernel<<<1, 64, 0, st>>>(j);      // the absmax words the packing blocks fold their maxima into
    if (b.ph[0].win) {                 // window panels: (largest magnitude into the headers,) one packing pass
        if (b.ph[0].fmt) win_absmax_kernel<<<WIN_ABSMAX_BLOCKS, 256, 0, st>>>(j);
        pack_job_kernel<<<j.gx * j.gy, 256, 0, st>>>(j);
        LOCATE_LAUNCH_CHECK(who);
        return LOCATE_OK;
    }
    pack_job_kernel<<<j.gx * j.gy, 256, 0, st>>>(j);
    LOCATE_LAUNCH_CHECK(who);
    int64_t big = 1;
    for (int i = 0; i < nphase; ++i) {
        const int64_t t = (int64_t)(b.ph[i].rows / 8) * b.ph[i].ld;
        if (t > big) big = t;
    }
    pack_split_kernel<<<dim3(stream_grid(big, 256), nphase), 256, 0, st>>>(j);
    LOCATE_LAUNCH_CHECK(who);
    return LOCATE_OK;
}

LOCATE_API size_t locate_conv_pack_job_bytes(void) { return sizeof(PackJob); }

// any_f16: some job is a TWO-PASS fp16-piece panel (its absmax header is cleared first); any_two_pass: some job is in the
// two-pass form at all (the split launch is needed) - both 0 when every job was built in the direct form: one launch.
// passes: bit 0 = some gather-kernel panel is in the two-pass form (split launch), bit 1 = some WINDOW panel of fp16 pieces has no
// absmax words (absmax pre-pass into the panel headers).
LOCATE_API int locate_conv_pack_panels(const void* jobs, int n_jobs, int total_blocks, int any_f16, int passes, void* stream) {
    LOCATE_REQUIRE(jobs && n_jobs > 0 && total_blocks > 0, "locate_conv_pack_panels: bad arguments");
    const int any_two_pass = passes & 1;
    if (any_f16)        // fp16-piece panels: zero the absmax words the packing blocks fold their maxima into
        pack_clear_jobs_kernel<<<(4 * n_jobs + 63) / 64, 64, 0, as_stream(stream)>>>(static_cast<const PackJob*>(jobs), n_jobs);
    if (passes & 2)
        win_absmax_jobs_kernel<<<dim3(WIN_ABSMAX_BLOCKS, n_jobs), 256, 0, as_stream(stream)>>>(static_cast<const PackJob*>(jobs));
    pack_jobs_kernel<<<total_blocks, 256, 0, as_stream(stream)>>>(static_cast<const PackJob*>(jobs), n_jobs);
    LOCATE_LAUNCH_CHECK("locate_conv_pack_panels");
    if (any_two_pass) {
        pack_split_jobs_kernel<<<dim3(PACK_SPLIT_BLOCKS, n_jobs, 4), 256, 0, as_stream(stream)>>>(static_cast<const PackJob*>(jobs));
        LOCATE_LAUNCH_CHECK("locate_conv_pack_panels(split)");
    }
    return LOCATE_OK;
}
// whether a job built by locate_conv_pack_job took the direct form (then it needs neither the clearing nor the split launch)
// 1 for a window panel's job (its non-direct form needs pass bit 1 of locate_conv_pack_panels, never the split launch)
LOCATE_API int locate_conv_pack_job_is_window(const void* job) {
    if (!job) return 0;
    PackJob j;
    memcpy(&j, job, sizeof(j));
    return j.kind == 4;
}
LOCATE_API int locate_conv_pack_job_is_direct(const void* job) {
    if (!job) return 0;
    PackJob j;
    memcpy(&j, job, sizeof(j));
    return j.batch.ph[0].direct;
}
