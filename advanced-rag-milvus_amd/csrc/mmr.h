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

}  // namespace hbmrag
