// Multi-list fusion: up to HR_MAX_FUSE_LISTS ranked lists per query, reciprocal-rank or weighted-score (hr_fuse_lists_dev).
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

constexpr int kFuseListsMaxEntries = HR_MAX_FUSE_LISTS * HR_MAX_TOPK;   // 4096 entries per query at the cap
constexpr unsigned kFuseListsEmpty = 0xFFFFFFFFu;                       // a table slot nobody has claimed

// Sizes of one launch, derived from (n_lists, k_in) on the host and passed to the kernel: n = entries per query,
// n_sort = the power of two the sort runs over, n_slots = the power of two of the id table (>= 2 n: load <= 0.5).
struct FuseListsShape {
    int n_lists, k_in, n, n_sort, n_slots, slot_shift;   // slot_shift = 64 - log2(n_slots)
};
__host__ inline FuseListsShape fuse_lists_shape(int n_lists, int k_in) {
    FuseListsShape s{n_lists, k_in, n_lists * k_in, 64, 128, 64 - 7};
    while (s.n_sort < s.n) s.n_sort <<= 1;
    while (s.n_slots < 2 * s.n) { s.n_slots <<= 1; --s.slot_shift; }
    return s;
}
// Dynamic LDS of one block: ids [n] int64 | values / sort keys [n_sort] 8 B | table [n_slots] u32 | owner / sorted
// position [n_sort] u16 | list masks [n] u16 (rounded up to 8 bytes).  16 x 256: 32 + 32 + 32 + 8 + 8 = 112 KiB.
__host__ __device__ inline size_t fuse_lists_lds_bytes(const FuseListsShape& s) {
    return (size_t)s.n * 8 + (size_t)s.n_sort * 8 + (size_t)s.n_slots * 4 + (size_t)s.n_sort * 2 + (((size_t)s.n * 2 + 7) & ~(size_t)7);
}

struct FuseListsArgs {
    double w[HR_MAX_FUSE_LISTS];    // host weights (replaced per query by w_query)
    int32_t norm[HR_MAX_FUSE_LISTS];   // HR_NORM_* per list (weighted mode)
    int rrf_k;
};

// A double as an unsigned key of the same order (no NaN in a defined call, and a fused score is never -0.0).
__device__ inline uint64_t fuse_lists_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double fuse_lists_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// One 256-thread block per query.  Restates retrieval.rrf_rank_lists / score_fuse_lists for L lists:
//   1. every list's valid prefix (first id < 0) is found, ids and contributions c (1 / (rrf_k + rank), or the
//      normalised score) are staged in LDS; entry e = l * k_in + rank is also its first-seen position;
//   2. an open-addressing table keyed by the id keeps, per id, the SMALLEST position that shows it (integer atomicMin:
//      the slot an id lands in depends on thread order, the value it ends with does not); that entry owns the id;
//   3. the lists are folded in one at a time, a barrier between: the thread of entry e of list l does
//      sum[owner] = sum[owner] + c * w_l (0.0 + c * w_l for the owner itself), two separately rounded operations.  Ids
//      inside a list are unique, so no two threads of a step touch one sum, and the sums grow in list order;
//   4. owners are sorted by (score descending, position ascending) — a unique key, so the bitonic network's result
//      is the stable descending sort — and the first top_k are written.
// Duplicate ids inside a list break the precondition of 3: two threads then race on one sum and that query's values
// are unspecified, but every index stays a position < n taken from the table, and every loop is bounded.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void fuse_lists_kernel(
    const int64_t* __restrict__ ids, const float* __restrict__ scores, FuseListsShape sh, FuseListsArgs a,
    const double* __restrict__ w_query, int top_k, int64_t* __restrict__ out_ids, double* __restrict__ out_scores,
    int32_t* __restrict__ out_lists, int32_t* __restrict__ n_out) {
    extern __shared__ int64_t fl_lds[];
    __shared__ int s_len[HR_MAX_FUSE_LISTS];
    __shared__ double s_w[HR_MAX_FUSE_LISTS], s_lo[HR_MAX_FUSE_LISTS], s_hi[HR_MAX_FUSE_LISTS];
    __shared__ int s_n_ids;
    const int tid = threadIdx.x, q = blockIdx.x;
    const int L = sh.n_lists, k_in = sh.k_in, n = sh.n;
    int64_t* s_id = fl_lds;
    double* s_val = reinterpret_cast<double*>(s_id + n);
    uint64_t* s_key = reinterpret_cast<uint64_t*>(s_val);            // the same words, as sort keys, from step 4 on
    unsigned* s_tab = reinterpret_cast<unsigned*>(s_val + sh.n_sort);
    uint16_t* s_own = reinterpret_cast<uint16_t*>(s_tab + sh.n_slots);   // owner position; the sorted positions in step 4
    uint16_t* s_mask = s_own + sh.n_sort;
    const int64_t* qi = ids + (int64_t)q * n;
    const float* qs = WEIGHTED ? scores + (int64_t)q * n : nullptr;
    const unsigned slot_mask = (unsigned)sh.n_slots - 1;

    if (tid < L) {
        s_len[tid] = k_in;
        s_w[tid] = w_query ? w_query[(int64_t)q * L + tid] : a.w[tid];
    }
    if (tid == 0) s_n_ids = 0;
    for (int i = tid; i < sh.n_slots; i += 256) s_tab[i] = kFuseListsEmpty;
    __syncthreads();
    // 1. stage the ids; a list's length is the position of its first negative id
    for (int e = tid; e < n; e += 256) {
        const int64_t v = qi[e];
        s_id[e] = v;
        if (v < 0) atomicMin(&s_len[e / k_in], e % k_in);
    }
    __syncthreads();
    if constexpr (WEIGHTED) {
        for (int e = tid; e < n; e += 256)
            if (e % k_in < s_len[e / k_in]) s_val[e] = (double)qs[e];
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;
        for (int l = wave; l < L; l += 4) {   // one wave per list: the branch is wave-uniform
            if (a.norm[l] < HR_NORM_MINMAX) continue;
            double lo = HUGE_VAL, hi = -HUGE_VAL;
            for (int i = lane; i < s_len[l]; i += 64) {
                const double v = s_val[l * k_in + i];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            for (int d = 32; d; d >>= 1) {
                const double o_lo = __shfl_xor(lo, d), o_hi = __shfl_xor(hi, d);
                lo = o_lo < lo ? o_lo : lo;
                hi = o_hi > hi ? o_hi : hi;
            }
            if (lane == 0) { s_lo[l] = lo; s_hi[l] = hi; }
        }
        __syncthreads();
        for (int e = tid; e < n; e += 256) {
            const int l = e / k_in;
            if (e - l * k_in >= s_len[l]) continue;
            const bool mm = a.norm[l] >= HR_NORM_MINMAX;
            s_val[e] = fuse_normalise(a.norm[l], s_val[e], mm ? s_lo[l] : 0.0, mm ? s_hi[l] : 0.0);
        }
    } else {
        for (int e = tid; e < n; e += 256) {
            const int l = e / k_in, rank = e - l * k_in;
            if (rank < s_len[l]) s_val[e] = 1.0 / (double)(a.rrf_k + rank + 1);
        }
    }
    // 2. the table: id -> smallest position.  A slot, once claimed, keeps its id (only its position shrinks), and at most
    //    n <= n_slots / 2 ids are inserted, so a probe sequence always ends; it is bounded by n_slots all the same.
    auto slot_of = [&](int64_t id) { return (unsigned)(((uint64_t)id * 0x9E3779B97F4A7C15ull) >> sh.slot_shift); };
    for (int e = tid; e < n; e += 256) {
        if (e % k_in >= s_len[e / k_in]) continue;
        const int64_t me = s_id[e];
        unsigned s = slot_of(me);
        for (int probe = 0; probe < sh.n_slots; ++probe, s = (s + 1) & slot_mask) {
            const unsigned old = atomicCAS(&s_tab[s], kFuseListsEmpty, (unsigned)e);
            if (old == kFuseListsEmpty) break;
            if (old < (unsigned)n && s_id[old] == me) {
                atomicMin(&s_tab[s], (unsigned)e);
                break;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < sh.n_sort; e += 256) {
        unsigned own = 0xFFFFu;   // entries past a list's end, and the sort's padding, own nothing and belong to nobody
        if (e < n && e % k_in < s_len[e / k_in]) {
            const int64_t me = s_id[e];
            unsigned s = slot_of(me);
            for (int probe = 0; probe < sh.n_slots; ++probe, s = (s + 1) & slot_mask) {
                const unsigned v = s_tab[s];
                if (v >= (unsigned)n) break;   // an empty slot: cannot happen for an inserted id
                if (s_id[v] == me) { own = v; break; }
            }
            if (own == (unsigned)e) atomicAdd(&s_n_ids, 1);
        }
        s_own[e] = (uint16_t)own;
    }
    __syncthreads();
    // 3. fold the lists in, in list order (k_in <= 256: one entry per thread and step)
    for (int l = 0; l < L; ++l) {
        if (tid < s_len[l]) {
            const int e = l * k_in + tid;
            const int o = s_own[e];
            if (o < n) {
                const double c = __dmul_rn(s_val[e], s_w[l]);
                const bool first = o == e;
                s_val[o] = __dadd_rn(first ? 0.0 : s_val[o], c);
                s_mask[o] = (uint16_t)((first ? 0u : (unsigned)s_mask[o]) | (1u << l));
            }
        }
        __syncthreads();
    }
    // 4. sort keys: an owner's score as an ordered integer, 0 for everything else; position = the first-seen order
    for (int e = tid; e < sh.n_sort; e += 256) {
        const bool owner = s_own[e] == (unsigned)e && e < n;
        s_key[e] = owner ? fuse_lists_key(s_val[e]) : 0ull;
        s_own[e] = (uint16_t)e;
    }
    __syncthreads();
    for (int k = 2; k <= sh.n_sort; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (sh.n_sort >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i + j;
                const uint64_t ka = s_key[i], kb = s_key[p];
                const unsigned pa = s_own[i], pb = s_own[p];
                const bool a_first = ka > kb || (ka == kb && pa < pb);   // a belongs before b in the final order
                if (((i & k) == 0) != a_first) {
                    s_key[i] = kb; s_key[p] = ka;
                    s_own[i] = (uint16_t)pb; s_own[p] = (uint16_t)pa;
                }
            }
            __syncthreads();
        }
    }
    const int n_ids = s_n_ids;
    const int n_fused = n_ids < top_k ? n_ids : top_k;
    for (int r = tid; r < top_k; r += 256) {
        const int64_t o = (int64_t)q * top_k + r;
        if (r < n_fused) {
            const int p = s_own[r] < n ? s_own[r] : 0;
            out_ids[o] = s_id[p];
            out_scores[o] = fuse_lists_unkey(s_key[r]);
            out_lists[o] = (int32_t)s_mask[p];
        } else {
            out_ids[o] = -1;
            out_scores[o] = 0.0;
            out_lists[o] = 0;
        }
    }
    if (tid == 0) n_out[q] = n_fused;
}

}  // namespace hbmrag
