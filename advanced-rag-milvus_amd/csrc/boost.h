// Boost ranker / function score (the fourth ranker of a search): every entry of a ranked list is re-scored by the
// filter expressions its row matches —  normalised relevance (x or +) the combined weight of the matching functions —
// and the list is re-sorted.  include/hbmrag.h holds the contract; advanced_rag/boost.py restates it on the host, bit
// for bit.
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

// The finaliser of splitmix64: the integer mix of the draw (the table of include/hbmrag.h), mod 2^64.
__device__ inline uint64_t boost_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

constexpr uint64_t kBoostGolden = 0x9E3779B97F4A7C15ull;

// One block (256 threads) per query; lists of up to kFuseMax entries.  The shape of decay_rerank_kernel:
//   n        = n_valid[q] clamped into [0, k_in], or without n_valid the position of the first id < 0 (k_in if none)
//   sc[i]    = the entry's score widened to double; lo / hi for the min-max codes are a block minimum / maximum over the
//              valid prefix (order-free, exact)
//   fin[i]   = n(sc[i]) combined with the factor of the functions that match ids[i], walked in ascending j; the query's
//              n_funcs operand structs are staged in LDS once, with h = mix(seed + G) of every function beside them
//   order    = stable sort of fin by counting, as in decay_rerank_kernel: rank = #{before} + #{equal, earlier}.  sc[i] is
//              overwritten with the sort key (fin, negated for the ascending direction: exact, and -0.0 still ties with
//              0.0), so the inner loop is one comparison pair whatever the direction; a NaN key compares false both ways,
//              so it is counted by no number — and a NaN entry counts every number and the NaNs before it: NaNs last, in
//              input order, in either direction
// Every output word is written once by the thread its rank names; no atomic decides anything but the prefix length,
// which is a minimum.
__global__ __launch_bounds__(256) void boost_rerank_kernel(
    const int64_t* __restrict__ ids, const void* __restrict__ scores, int score_is_f64, const int32_t* __restrict__ n_valid,
    int k_in, const hr_boost_func* __restrict__ funcs, int n_funcs, int64_t first_row, int function_mode, int boost_mode,
    int norm, int ascending, int k_out, int32_t* __restrict__ out_pos, int64_t* __restrict__ out_ids,
    double* __restrict__ out_scores, int32_t* __restrict__ out_matched, int32_t* __restrict__ out_n) {
    __shared__ double sc[kFuseMax];
    __shared__ double fin[kFuseMax];
    __shared__ int hit[kFuseMax];
    __shared__ double w_lo[4], w_hi[4];
    __shared__ uint64_t s_func[HR_MAX_BOOST_FUNCS * (sizeof(hr_boost_func) / 8)];
    __shared__ uint64_t s_h[HR_MAX_BOOST_FUNCS];
    __shared__ int s_n;
    constexpr int kWords = sizeof(hr_boost_func) / 8;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* my_ids = ids + (int64_t)q * k_in;
    if (tid < n_funcs * kWords)
        s_func[tid] = reinterpret_cast<const uint64_t*>(funcs + (int64_t)q * n_funcs)[tid];
    if (tid == 0) {
        int n = k_in;
        if (n_valid) {
            n = n_valid[q];
            n = n < 0 ? 0 : (n > k_in ? k_in : n);
        }
        s_n = n;
    }
    __syncthreads();
    const hr_boost_func* fn = reinterpret_cast<const hr_boost_func*>(s_func);
    if (tid < n_funcs) s_h[tid] = boost_mix(fn[tid].seed + kBoostGolden);
    if (!n_valid) {   // the list ends at its first negative id
        int end = k_in;
        for (int i = tid; i < k_in; i += 256)
            if (my_ids[i] < 0) { end = i; break; }   // positions ascend per thread
        if (end < k_in) atomicMin(&s_n, end);
    }
    __syncthreads();
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
    for (int i = tid; i < n; i += 256) {   // every thread touches its own entries only: no barrier since sc[] was written
        const int64_t id = my_ids[i];
        const int64_t r = id - first_row;   // read only behind id >= first_row: it cannot have wrapped then
        const bool at = id >= first_row;
        double f = 0.0;
        int matched = 0;
        for (int j = 0; j < n_funcs; ++j) {
            const hr_boost_func& p = fn[j];
            if (!(p.flags & HR_BOOST_ACTIVE)) continue;
            if (p.mask && !(at && r < p.mask_rows && ((p.mask[r >> 3] >> (r & 7)) & 1))) continue;
            double v = p.weight;
            if (p.flags & HR_BOOST_RANDOM) {
                const uint64_t key = (uint64_t)((p.key_col && at && r < p.key_rows) ? p.key_col[r] : id);
                const uint64_t z = boost_mix((s_h[j] ^ key) + kBoostGolden);
                v = __dmul_rn(p.weight, __dmul_rn((double)(z >> 11), 0x1.0p-53));   // u in [0, 1), exact
            }
            f = !matched ? v : (function_mode == HR_BOOST_SUM ? __dadd_rn(f, v) : __dmul_rn(f, v));
            matched |= 1 << j;
        }
        const double ns = norm < 0 ? sc[i] : fuse_normalise(norm, sc[i], lo, hi);
        const double fv = !matched ? ns : (boost_mode == HR_BOOST_SUM ? __dadd_rn(ns, f) : __dmul_rn(ns, f));
        fin[i] = fv;
        sc[i] = ascending ? -fv : fv;
        hit[i] = matched;
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {
        const double v = sc[e];
        int rank = 0;
        if (v != v) {
            for (int j = 0; j < n; ++j) rank += (sc[j] == sc[j]) || j < e;
        } else {
            for (int j = 0; j < n; ++j) rank += (sc[j] > v) || (sc[j] == v && j < e);
        }
        if (rank < k_out) {
            out_pos[(int64_t)q * k_out + rank] = e;
            out_ids[(int64_t)q * k_out + rank] = my_ids[e];
            out_scores[(int64_t)q * k_out + rank] = fin[e];
            out_matched[(int64_t)q * k_out + rank] = hit[e];
        }
    }
    const int kept = n < k_out ? n : k_out;
    for (int i = kept + tid; i < k_out; i += 256) {
        out_pos[(int64_t)q * k_out + i] = -1;
        out_ids[(int64_t)q * k_out + i] = -1;
        out_scores[(int64_t)q * k_out + i] = 0.0;
        out_matched[(int64_t)q * k_out + i] = 0;
    }
    if (tid == 0) out_n[q] = kept;
}

}  // namespace hbmrag
