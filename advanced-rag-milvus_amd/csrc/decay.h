// Decay ranker (the third ranker of a Milvus search, beside RRF and the weighted ranker): every entry of a ranked list
// is re-scored as  normalised relevance x decay(|field - origin|)  and the list is re-sorted.  include/hbmrag.h holds
// the contract; advanced_rag/decay.py restates it on the host, bit for bit.
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

// Canonical exponential: no table and no library call, every operation a separately rounded IEEE fp64 one, so that the
// host restatement (decay.canonical_exp) gives the same bits.  x = k ln2 + r with |r| <= ln2 / 2 (ln2 split in two so
// that k * hi is exact), a 13th-degree Taylor polynomial in r, then an exact scaling by 2^k: x >= -708 keeps k >= -1021
// and p in [0.70, 1.42], so the result is a normal number.
__device__ inline double canonical_exp(double x) {
    if (x != x) return 0.0;
    if (x >= 0.0) return 1.0;   // covers -0.0
    if (x < -708.0) return 0.0;
    const double k = rint(__dmul_rn(x, 0x1.71547652b82fep+0));   // ties to even
    const double r = __dsub_rn(__dsub_rn(x, __dmul_rn(k, 0x1.62e42fee00000p-1)), __dmul_rn(k, 0x1.a39ef35793c76p-33));
    double p = 1.0 / 6227020800.0;                 // c_i = 1 / i!: the divisions are folded, correctly rounded
    p = __dadd_rn(1.0 / 479001600.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 39916800.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 3628800.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 362880.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 40320.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 5040.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 720.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 120.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 24.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 6.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0 / 2.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0, __dmul_rn(r, p));
    p = __dadd_rn(1.0, __dmul_rn(r, p));
    return ldexp(p, (int)k);
}

// The decay factor of a field value v for one query's operands (the table of include/hbmrag.h).
__device__ inline double decay_factor(const hr_decay_query& p, double v) {
    if (v != v) return 0.0;   // the row has no value
    const double a = fabs(__dsub_rn(v, p.origin));
    const double u = __dsub_rn(a, p.offset);
    const double d = u > 0.0 ? u : 0.0;
    switch (p.func) {
    case HR_DECAY_GAUSS: return canonical_exp(__dmul_rn(p.coef, __dmul_rn(d, d)));
    case HR_DECAY_EXP: return canonical_exp(__dmul_rn(p.coef, d));
    case HR_DECAY_LINEAR: {
        const double g = __dsub_rn(1.0, __dmul_rn(d, p.coef));
        return g > 0.0 ? g : 0.0;
    }
    default: return 0.0;   // an unknown function code: defined, not refused (the operands live on the device)
    }
}

// One block (256 threads) per query; lists of up to kFuseMax entries.
//   n        = n_valid[q] clamped into [0, k_in], or without n_valid the position of the first id < 0 (k_in if none)
//   sc[i]    = the entry's score widened to double, then normalised in place (fuse_normalise; norm < 0 = identity);
//              lo / hi for the min-max codes are a block minimum / maximum over the valid prefix (order-free, exact)
//   fin[i]   = sc[i] * decay_factor(field value of ids[i]); an id outside [first_row, first_row + col_rows) has factor 0
//   order    = stable descending sort of fin by counting, as in rerank_linear_block: rank = #{larger} + #{equal, earlier}
// Every output word is written once by the thread its rank names; no atomic decides anything but the prefix length,
// which is a minimum.
__global__ __launch_bounds__(256) void decay_rerank_kernel(
    const int64_t* __restrict__ ids, const void* __restrict__ scores, int score_is_f64, const int32_t* __restrict__ n_valid,
    int k_in, const void* __restrict__ col, int col_kind, int64_t col_rows, int64_t first_row,
    const hr_decay_query* __restrict__ params, int norm, int k_out, int32_t* __restrict__ out_pos,
    int64_t* __restrict__ out_ids, double* __restrict__ out_scores, int32_t* __restrict__ out_n) {
    __shared__ double sc[kFuseMax];
    __shared__ double fin[kFuseMax];
    __shared__ double w_lo[4], w_hi[4];
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* my_ids = ids + (int64_t)q * k_in;
    if (tid == 0) {
        int n = k_in;
        if (n_valid) {
            n = n_valid[q];
            n = n < 0 ? 0 : (n > k_in ? k_in : n);
        }
        s_n = n;
    }
    __syncthreads();
    if (!n_valid) {   // the list ends at its first negative id
        int end = k_in;
        for (int i = tid; i < k_in; i += 256)
            if (my_ids[i] < 0) { end = i; break; }   // positions ascend per thread
        if (end < k_in) atomicMin(&s_n, end);
        __syncthreads();
    }
    const int n = s_n;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int i = tid; i < n; i += 256) {
        const int64_t o = (int64_t)q * k_in + i;
        const double s = score_is_f64 ? static_cast<const double*>(scores)[o] : (double)static_cast<const float*>(scores)[o];
        sc[i] = s;
        lo = s < lo ? s : lo;
        hi = s > hi ? s : hi;
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
    const hr_decay_query p = params[q];
    for (int i = tid; i < n; i += 256) {   // every thread touches its own entries only: no barrier since sc[] was written
        const int64_t id = my_ids[i];
        const int64_t r = id - first_row;
        double f = 0.0;
        if (id >= first_row && r < col_rows) {   // (id >= first_row first: r cannot have wrapped when it is read)
            const double v = col_kind == HR_COL_I64   ? (double)static_cast<const int64_t*>(col)[r]
                             : col_kind == HR_COL_F32 ? (double)static_cast<const float*>(col)[r]
                                                      : static_cast<const double*>(col)[r];
            f = decay_factor(p, v);
        }
        const double ns = norm < 0 ? sc[i] : fuse_normalise(norm, sc[i], lo, hi);
        fin[i] = __dmul_rn(ns, f);
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {
        const double v = fin[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (fin[j] > v) || (fin[j] == v && j < e);
        if (rank < k_out) {
            out_pos[(int64_t)q * k_out + rank] = e;
            out_ids[(int64_t)q * k_out + rank] = my_ids[e];
            out_scores[(int64_t)q * k_out + rank] = v;
        }
    }
    const int kept = n < k_out ? n : k_out;
    for (int i = kept + tid; i < k_out; i += 256) {
        out_pos[(int64_t)q * k_out + i] = -1;
        out_ids[(int64_t)q * k_out + i] = -1;
        out_scores[(int64_t)q * k_out + i] = 0.0;
    }
    if (tid == 0) out_n[q] = kept;
}

}  // namespace hbmrag
