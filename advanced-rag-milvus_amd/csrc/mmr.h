// Greedy MMR diversification of a batch of fused lists on token-Jaccard similarity.
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

// Position of the first entry >= key in the ascending list t[0, n) (n when there is none).
__device__ inline int token_lower_bound(const int32_t* __restrict__ t, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// |A ∩ B| of two ascending, duplicate-free token lists by one wave: the lanes stride the shorter list and look every
// token up in the longer one (binary search, global memory); the hits of a stride are counted with one ballot.
// Every lane returns the count.
__device__ inline int token_intersection_wave(const int32_t* __restrict__ a, int la, const int32_t* __restrict__ b, int lb) {
    if (la > lb) {
        const int32_t* t = a; a = b; b = t;
        const int l = la; la = lb; lb = l;
    }
    const int lane = threadIdx.x & 63;
    int count = 0;
    for (int base = 0; base < la; base += 64) {   // la is wave-uniform: every lane takes part in every ballot
        bool hit = false;
        if (base + lane < la) {
            const int32_t key = a[base + lane];
            const int p = token_lower_bound(b, lb, key);
            hit = p < lb && b[p] == key;
        }
        count += __popcll(__ballot(hit));
    }
    return count;
}

// One block (256 threads) per query.  Restates HybridRetriever._mmr_diversify (reference
// src/advanced_rag/retrieval.py:493-516) operation for operation on the fused list of query q:
//   sim(r, s) = |A_r ∩ A_s| / (|A_r ∪ A_s| or 1)           (integers, one float64 division)
//   first pick:  val_r = score_r
//   afterwards:  val_r = lambda * score_r - (1 - lambda) * max_{s selected} sim(r, s)
//                (two float64 products and one subtraction, each rounded on its own; 1 - lambda computed once)
// every step takes the candidate with the largest val that is > -1e9; among equals the first in fused order (the
// reference scans the pool in that order and replaces its best only by a strictly larger value).  No candidate above
// -1e9 (NaN included) ends the selection.
// The maximum over the selected is kept as a running value per candidate and updated against the newest member only:
// every sim is exact, so max(running, new) equals the reference's recomputed maximum.  (sim >= 0: the running value
// starts at 0.)
// Token sets are read where they lie, in global memory: no limit on the length of a row.
__global__ __launch_bounds__(256) void mmr_select_kernel(
    const int64_t* __restrict__ ids, const double* __restrict__ scores, const int32_t* __restrict__ n_valid, int k_in,
    const int64_t* __restrict__ tok_indptr, const int32_t* __restrict__ tok, int64_t tok_rows, int64_t first_row,
    const double* __restrict__ lambdas, int k_out, int32_t* __restrict__ out_pos, int32_t* __restrict__ out_n) {
    __shared__ double sc[kFuseMax];
    __shared__ double msim[kFuseMax];      // largest similarity to a selected entry so far
    __shared__ int64_t set_lo[kFuseMax];   // the entry's tokens: tok[set_lo .. set_lo + set_len)
    __shared__ int set_len[kFuseMax];
    __shared__ int alive[kFuseMax];
    __shared__ double w_val[4];            // per-wave winners of a step
    __shared__ int w_pos[4];
    __shared__ int s_best;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = n_valid[q];
    n = n < 0 ? 0 : (n > k_in ? k_in : n);
    const int limit = n < k_out ? n : k_out;
    const double lam = lambdas[q];
    const double one_minus = __dsub_rn(1.0, lam);
    for (int i = tid; i < n; i += 256) {
        const int64_t o = (int64_t)q * k_in + i;
        const int64_t r = ids[o] - first_row;
        int64_t lo = 0;
        int len = 0;
        if (r >= 0 && r < tok_rows) {
            lo = tok_indptr[r];
            len = (int)(tok_indptr[r + 1] - lo);
        }
        sc[i] = scores[o];
        msim[i] = 0.0;
        set_lo[i] = lo;
        set_len[i] = len;
        alive[i] = 1;
    }
    for (int i = tid; i < k_out; i += 256) out_pos[(int64_t)q * k_out + i] = -1;
    __syncthreads();
    int n_sel = 0;
    for (; n_sel < limit; ++n_sel) {
        // step A: block argmax by (val desc, position asc) over the live candidates with val > -1e9
        double bv = 0.0;
        int bp = kFuseMax;   // = none
        for (int i = tid; i < n; i += 256) {
            if (!alive[i]) continue;
            const double v = n_sel ? __dsub_rn(__dmul_rn(lam, sc[i]), __dmul_rn(one_minus, msim[i])) : sc[i];
            if (v > -1e9 && (bp == kFuseMax || v > bv)) { bv = v; bp = i; }   // positions ascend per thread: > keeps the first
        }
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_down(bv, off);
            const int op = __shfl_down(bp, off);
            if (op != kFuseMax && (bp == kFuseMax || ov > bv || (ov == bv && op < bp))) { bv = ov; bp = op; }
        }
        if (lane == 0) { w_val[wave] = bv; w_pos[wave] = bp; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) {
                const double ov = w_val[w];
                const int op = w_pos[w];
                if (op != kFuseMax && (bp == kFuseMax || ov > bv || (ov == bv && op < bp))) { bv = ov; bp = op; }
            }
            s_best = bp;
            if (bp != kFuseMax) {
                alive[bp] = 0;
                out_pos[(int64_t)q * k_out + n_sel] = bp;
            }
        }
        __syncthreads();
        const int best = s_best;   // the same for every thread: the loop exit below is block-uniform
        if (best == kFuseMax) break;
        if (n_sel + 1 >= limit) continue;   // the last pick: nobody reads the similarities to it
        // step B: a wave per remaining candidate: its similarity to the new member
        const int lb = set_len[best];
        if (lb) {   // an empty member has similarity 0 / (|A| or 1) = 0 to everyone: the running maxima stay
            const int32_t* tb = tok + set_lo[best];
            for (int c = wave; c < n; c += 4) {
                if (!alive[c]) continue;
                const int la = set_len[c];
                if (!la) continue;
                const int inter = token_intersection_wave(tok + set_lo[c], la, tb, lb);
                if (lane == 0) {
                    const int uni = la + lb - inter;   // >= 1 here
                    const double sim = (double)inter / (double)uni;
                    if (sim > msim[c]) msim[c] = sim;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) out_n[q] = n_sel;
}

// ---- vector MMR (hr_mmr_select_vec_dev): the same greedy selection on the cosine of the STORED embeddings --------------
// A sibling of mmr_select_kernel, which stays instruction for instruction what it is.  include/hbmrag.h holds the
// contract; advanced_rag/mmr.py restates it on the host, bit for bit.
//
// One block (256 threads) per query.  The candidates' rows were gathered once, by get_rows_kernel, into `rows`: row-major,
// in the shard's own element type, list entry i of query q at rows + (q * k_in + i) * stride (stride a multiple of one
// 16-byte chunk; the elements at and beyond dim are never written and never read here).  An id outside the shard was
// gathered as zeros and has norm 0.
//   rel[i]  = the entry's score widened to double and normalised as decay_rerank_kernel does it (lo / hi over the valid
//             prefix, NaN scores ignored by the comparisons)
//   sim     = (double)(float)(S / sqrt(N_c * N_b)), 0 when the product is not > 0: S the k-ordered fp64 sum of the exact
//             products, N the store's norm2 — refine_dense_slot's arithmetic with the member's row as the query
//   m[i]    = the similarity to the FIRST member, afterwards the running maximum (cosine can be negative: no floor at 0)
// After each pick the newest member's row is staged in LDS (widened to fp32, exact; at most HR_MAX_DIM floats = 16 KiB) and
// every live candidate, thread = candidate, walks its own row against it: a dependent fp64 chain per pair, so the
// parallelism is across candidates.  A thread reads its row 16 bytes at a time, front to back: the lines it touches are
// its own and stay in the vector L1 until it has used them up (a list's rows are k_in * dim elements, a few hundred KiB
// at the most, all of it resident in L2 after the first pick).
// The argmax is mmr_select_kernel's: (val desc, position asc), only val > -1e9; no atomic decides anything.
template <typename STORE>
__global__ __launch_bounds__(256) void mmr_select_vec_kernel(
    const int64_t* __restrict__ ids, const void* __restrict__ scores, int score_is_f64, int norm,
    const int32_t* __restrict__ n_valid, int k_in, const STORE* __restrict__ rows, int64_t stride, int dim,
    const double* __restrict__ norm2, int64_t n_rows, int64_t first_row, const double* __restrict__ lambdas, int k_out,
    int32_t* __restrict__ out_pos, double* __restrict__ out_val, int32_t* __restrict__ out_n) {
    constexpr int E = kChunkBytes / (int)sizeof(STORE);
    __shared__ double sc[kFuseMax];        // relevance
    __shared__ double msim[kFuseMax];      // largest similarity to a selected entry so far (valid once one is selected)
    __shared__ double nrm[kFuseMax];       // the row's norm2; 0 for an id outside the shard
    __shared__ int alive[kFuseMax];
    __shared__ __attribute__((aligned(16))) float member[HR_MAX_DIM];   // the newest member's row
    __shared__ double w_lo[4], w_hi[4];
    __shared__ double w_val[4];
    __shared__ int w_pos[4];
    __shared__ int s_best;
    __shared__ double s_best_val;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = n_valid[q];
    n = n < 0 ? 0 : (n > k_in ? k_in : n);
    const int limit = n < k_out ? n : k_out;
    const double lam = lambdas[q];
    const double one_minus = __dsub_rn(1.0, lam);
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int i = tid; i < n; i += 256) {
        const int64_t o = (int64_t)q * k_in + i;
        const double s = score_is_f64 ? static_cast<const double*>(scores)[o] : (double)static_cast<const float*>(scores)[o];
        const int64_t id = ids[o];
        sc[i] = s;
        lo = s < lo ? s : lo;
        hi = s > hi ? s : hi;
        nrm[i] = (id >= first_row && id - first_row < n_rows) ? norm2[id - first_row] : 0.0;   // (id >= first_row first: no wrap)
        alive[i] = 1;
    }
    if (norm >= HR_NORM_MINMAX) {   // block-uniform
        for (int d = 32; d; d >>= 1) {
            const double o_lo = __shfl_xor(lo, d), o_hi = __shfl_xor(hi, d);
            lo = o_lo < lo ? o_lo : lo;
            hi = o_hi > hi ? o_hi : hi;
        }
        if (lane == 0) { w_lo[wave] = lo; w_hi[wave] = hi; }
        __syncthreads();
        lo = w_lo[0];
        hi = w_hi[0];
        for (int w = 1; w < 4; ++w) {
            lo = w_lo[w] < lo ? w_lo[w] : lo;
            hi = w_hi[w] > hi ? w_hi[w] : hi;
        }
    }
    if (norm >= 0)
        for (int i = tid; i < n; i += 256) sc[i] = fuse_normalise(norm, sc[i], lo, hi);   // the thread's own entries
    for (int i = tid; i < k_out; i += 256) {
        out_pos[(int64_t)q * k_out + i] = -1;
        out_val[(int64_t)q * k_out + i] = 0.0;
    }
    __syncthreads();
    const int full = dim / E;   // whole chunks of a row
    int n_sel = 0;
    for (; n_sel < limit; ++n_sel) {
        // step A: block argmax by (val desc, position asc) over the live candidates with val > -1e9
        double bv = 0.0;
        int bp = kFuseMax;   // = none
        for (int i = tid; i < n; i += 256) {
            if (!alive[i]) continue;
            const double v = n_sel ? __dsub_rn(__dmul_rn(lam, sc[i]), __dmul_rn(one_minus, msim[i])) : sc[i];
            if (v > -1e9 && (bp == kFuseMax || v > bv)) { bv = v; bp = i; }   // positions ascend per thread: > keeps the first
        }
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_down(bv, off);
            const int op = __shfl_down(bp, off);
            if (op != kFuseMax && (bp == kFuseMax || ov > bv || (ov == bv && op < bp))) { bv = ov; bp = op; }
        }
        if (lane == 0) { w_val[wave] = bv; w_pos[wave] = bp; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) {
                const double ov = w_val[w];
                const int op = w_pos[w];
                if (op != kFuseMax && (bp == kFuseMax || ov > bv || (ov == bv && op < bp))) { bv = ov; bp = op; }
            }
            s_best = bp;
            s_best_val = bv;
            if (bp != kFuseMax) alive[bp] = 0;
        }
        __syncthreads();
        const int best = s_best;   // the same for every thread: the loop exit below is block-uniform
        if (best == kFuseMax) break;
        if (tid == 0) {
            out_pos[(int64_t)q * k_out + n_sel] = best;
            out_val[(int64_t)q * k_out + n_sel] = s_best_val;
        }
        if (n_sel + 1 >= limit) continue;   // the last pick: nobody reads the similarities to it
        // step B: the new member's row into LDS, then thread = candidate
        const STORE* mrow = rows + ((int64_t)q * k_in + best) * stride;
        for (int k = tid; k < dim; k += 256) member[k] = (float)mrow[k];
        __syncthreads();
        const double nb = nrm[best];
        for (int c = tid; c < n; c += 256) {
            if (!alive[c]) continue;
            double sim = 0.0;
            const double d = __dmul_rn(nrm[c], nb);
            if (d > 0.0) {
                const STORE* crow = rows + ((int64_t)q * k_in + c) * stride;
                const chunk_t* cp = reinterpret_cast<const chunk_t*>(crow);
                double s = 0.0;
#pragma unroll 4
                for (int kc = 0; kc < full; ++kc) {
                    union { chunk_t v; STORE e[E]; } x;
                    x.v = cp[kc];
#pragma unroll
                    for (int j = 0; j < E; ++j) s = __dadd_rn(s, __dmul_rn((double)x.e[j], (double)member[kc * E + j]));
                }
                for (int k = full * E; k < dim; ++k) s = __dadd_rn(s, __dmul_rn((double)crow[k], (double)member[k]));
                sim = (double)(float)(s / sqrt(d));
            }
            msim[c] = (n_sel == 0 || sim > msim[c]) ? sim : msim[c];
        }
        __syncthreads();
    }
    if (tid == 0) out_n[q] = n_sel;
}

}  // namespace hbmrag
