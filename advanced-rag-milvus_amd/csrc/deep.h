// Deep selection: the best W <= HR_MAX_DEEP_K rows of n candidates per query, n up to a whole shard, sorted, and the window
// [offset, offset + k) of that list written out.  The candidates come in the layout the refine kernels write (score fp32,
// row int32, row < 0 = invalid) and rank by the same unique 64-bit key as everywhere else (rank_key, common.h), so a deep
// list's head is the list select_topk_kernel returns.
//
//   deep_hist_kernel  x 8   many blocks per query (blockIdx.y = query): one 8-bit digit of the keys that still match the
//   deep_pick_kernel  x 8   query's (prefix, mask), histogrammed in LDS and added to the query's table in global memory
//                           with integer atomics (order-independent); one wave per query then takes the digit that holds
//                           the remaining-th largest key and advances the query's state.  No host round trip: the sixteen
//                           launches are enqueued as a fixed sequence, and a query that is resolved — every key that
//                           shares its prefix belongs to the list — makes the rest of its passes exit at once.
//   deep_gather_kernel      keys >= the threshold (and != 0) into the query's W slots through an atomic slot counter
//                           (one request per wave: the takers of a wave share it by their rank in the ballot)
//   deep_sort_kernel        one block per query: bitonic sort of the gathered keys in LDS, then the window and its padding
//
// Ties at the W-th score are ties of the upper 32 bits only: the lower four passes resolve them by the row bits exactly as
// block_kth_largest (select.h) does, and when every score is equal they decide alone.
//
// A ranking is a total order on unique keys, so "the next k rows after the last hit seen" and "the rows whose score lies
// in a range" are both one open key interval (lo, hi) per query (deep_key_interval below).  The windowed instantiations
// of the hist and gather kernels turn a key outside it into 0 where the key is formed; nothing else changes, and a
// query with fewer than W keys inside behaves as one with masked rows does: the zeros are counted as the smallest keys,
// the threshold may end at 0, and the gather, which never takes a 0, counts exactly the valid keys.
#pragma once
#include "common.h"

namespace hbmrag {

constexpr int kDeepPasses = 8;          // 64-bit keys, 8-bit digits
constexpr int kDeepHistThreads = 256;
constexpr int kDeepSortThreads = 1024;

struct DeepState {                       // per query, zeroed before the first pass
    unsigned long long prefix, mask;     // the digits chosen so far; after the last pass prefix is the W-th largest key
    int remaining;                       // rank of the wanted key among the keys that match (prefix, mask)
    int done;                            // prefix is a threshold already: keys >= prefix are exactly the list
    unsigned count;                      // gather: slots handed out
    unsigned pad_;
};

struct DeepArgs {
    const float* score;                  // [B][n]
    const int32_t* row;                  // [B][n], < 0 = invalid
    int64_t n;
    int W;                               // offset + k
    DeepState* state;                    // [B]
    unsigned* hist;                      // [B][kDeepPasses][256]
    unsigned long long* keys;            // [B][W]
    const unsigned long long* bounds;    // [B][2] or null: the windowed kernels keep bounds[q][0] < key < bounds[q][1]
};

__device__ inline uint64_t deep_key(const float* __restrict__ sc, const int32_t* __restrict__ rw, int64_t i) {
    const int32_t r = rw[i];
    return r < 0 ? 0ull : rank_key(sc[i], (uint32_t)r);
}

// WIN: a key outside the query's open interval (lo, hi) is an invalid candidate (0), like a masked row: every pass below
// treats it as the smallest key there is, and the gather never takes it.
template <bool WIN>
__device__ inline uint64_t deep_key(const float* __restrict__ sc, const int32_t* __restrict__ rw, int64_t i, uint64_t lo,
                                    uint64_t hi) {
    const uint64_t kk = deep_key(sc, rw, i);
    if constexpr (WIN) return (kk > lo && kk < hi) ? kk : 0ull;
    return kk;
}

// The open key interval of one query of the cursor forms (hr_search_*_deep_after), host side.  Scores are in the KEY
// domain (an L2 caller negates its distances and bounds first): kept are the keys of rows with above < score <= upto
// (-inf / +inf = that side open) that come strictly after the cursor (after_score, after_row) in the ranking: score
// worse, or score equal and row larger.  after_row is a position, any int64: below 0 every row of that score follows,
// beyond the 32-bit row space none does.  A zero BOUND is +0.0, so that both zeros fall on the side float comparison
// puts them; the cursor's score is taken bit for bit.
inline void deep_key_interval(bool has_after, float after_score, int64_t after_row, float above, float upto,
                              unsigned long long out[2]) {
    const auto canon = [](float x) { return x == 0.f ? 0.f : x; };
    unsigned long long lo = 0ull, hi = ~0ull;
    if (above != -__builtin_inff()) lo = ((unsigned long long)ord_f32(canon(above)) << 32) | 0xFFFFFFFFull;
    if (upto != __builtin_inff()) hi = ((unsigned long long)ord_f32(canon(upto)) + 1ull) << 32;
    if (has_after) {
        const unsigned long long s = (unsigned long long)ord_f32(after_score) << 32;
        const unsigned long long c = after_row < 0 ? s + (1ull << 32) : after_row > 0xFFFFFFFFll ? s : s | (0xFFFFFFFFull - (unsigned long long)after_row);
        if (c < hi) hi = c;
    }
    out[0] = lo;
    out[1] = hi;
}

template <bool WIN>
__global__ __launch_bounds__(kDeepHistThreads) void deep_hist_kernel(DeepArgs a, int pass) {
    __shared__ unsigned bins[256];
    const int q = blockIdx.y;
    const DeepState st = a.state[q];
    if (st.done) return;                 // uniform over the block
    bins[threadIdx.x] = 0;
    __syncthreads();
    const float* __restrict__ sc = a.score + (int64_t)q * a.n;
    const int32_t* __restrict__ rw = a.row + (int64_t)q * a.n;
    const int shift = 56 - 8 * pass;
    const int64_t stride = (int64_t)gridDim.x * kDeepHistThreads;
    const uint64_t lo = WIN ? a.bounds[2 * q] : 0ull, hi = WIN ? a.bounds[2 * q + 1] : 0ull;
    for (int64_t i = (int64_t)blockIdx.x * kDeepHistThreads + threadIdx.x; i < a.n; i += stride) {
        const uint64_t kk = deep_key<WIN>(sc, rw, i, lo, hi);
        const bool hit = (kk & st.mask) == st.prefix;
        const unsigned d = (unsigned)(kk >> shift) & 255u;
        // the upper digits of a shard's scores are nearly all equal: a wave whose hits share one digit adds once
        const unsigned long long hits = __ballot(hit);
        if (hits == 0) continue;
        const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, __builtin_ctzll(hits));
        if (__ballot(hit && d == d0) == hits) {
            if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(hits)) atomicAdd(&bins[d0], (unsigned)__builtin_popcountll(hits));
        } else if (hit) {
            atomicAdd(&bins[d], 1u);
        }
    }
    __syncthreads();
    const unsigned c = bins[threadIdx.x];
    if (c) atomicAdd(&a.hist[((int64_t)q * kDeepPasses + pass) * 256 + threadIdx.x], c);
}

// One wave per query: the digit of this pass (lane l owns bins 255-4l .. 252-4l, as radix_pass in select.h).
__global__ __launch_bounds__(64) void deep_pick_kernel(DeepArgs a, int pass) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const DeepState st = a.state[q];
    if (st.done) return;
    const int remaining = pass == 0 ? (int)(a.n < (int64_t)a.W ? a.n : (int64_t)a.W) : st.remaining;
    const unsigned* bins = a.hist + ((int64_t)q * kDeepPasses + pass) * 256;
    const int top = 255 - 4 * lane;
    const int c0 = (int)bins[top], c1 = (int)bins[top - 1], c2 = (int)bins[top - 2], c3 = (int)bins[top - 3];
    const int mine = c0 + c1 + c2 + c3;
    const int incl = (int)wave_scan_add((unsigned)mine);
    const int before = incl - mine;
    if (before < remaining && incl >= remaining) {  // exactly one lane: the matching keys number at least `remaining`
        int cum = before, d, cd;
        if (cum + c0 >= remaining) { d = top; cd = c0; }
        else if ((cum += c0) + c1 >= remaining) { d = top - 1; cd = c1; }
        else if ((cum += c1) + c2 >= remaining) { d = top - 2; cd = c2; }
        else { cum += c2; d = top - 3; cd = c3; }
        const int shift = 56 - 8 * pass;
        DeepState* o = a.state + q;
        o->prefix = st.prefix | ((unsigned long long)d << shift);
        o->mask = st.mask | (0xFFull << shift);
        o->remaining = remaining - cum;
        // every key that shares the new prefix is wanted: prefix (lower digits zero) is a threshold as it stands
        o->done = (cd == remaining - cum) || pass == kDeepPasses - 1;
    }
}

template <bool WIN>
__global__ __launch_bounds__(kDeepHistThreads) void deep_gather_kernel(DeepArgs a) {
    const int q = blockIdx.y;
    const uint64_t thr = a.state[q].prefix;
    const float* __restrict__ sc = a.score + (int64_t)q * a.n;
    const int32_t* __restrict__ rw = a.row + (int64_t)q * a.n;
    unsigned long long* out = a.keys + (int64_t)q * a.W;
    const int64_t stride = (int64_t)gridDim.x * kDeepHistThreads;
    const uint64_t lo = WIN ? a.bounds[2 * q] : 0ull, hi = WIN ? a.bounds[2 * q + 1] : 0ull;
    for (int64_t i = (int64_t)blockIdx.x * kDeepHistThreads + threadIdx.x; i < a.n; i += stride) {
        const uint64_t kk = deep_key<WIN>(sc, rw, i, lo, hi);
        const bool take = kk != 0 && kk >= thr;      // unique keys: exactly min(W, valid) of them
        const unsigned long long takers = __ballot(take);
        if (takers == 0) continue;
        // one slot request per wave: the first taker asks for all of them, every taker adds its rank among them
        const int lane = threadIdx.x & 63, leader = __builtin_ctzll(takers);
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&a.state[q].count, (unsigned)__builtin_popcountll(takers));
        base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
        if (take) {
            const unsigned slot = base + (unsigned)__builtin_popcountll(takers & ((1ull << lane) - 1ull));
            if (slot < (unsigned)a.W) out[slot] = kk;
        }
    }
}

// P = the power of two the host padded W to (dynamic LDS = P * 8 bytes).  Sorted descending, the padding keys (0) last.
// Consecutive lanes take consecutive 8-byte keys of a half (ds_read_b64 over 32 lanes covers the 64 banks once) for every
// distance j >= 32; the last five distances of a merge put lanes 16 bytes and less apart and pay a 2-way conflict.
__global__ __launch_bounds__(kDeepSortThreads) void deep_sort_kernel(DeepArgs a, int P, int k, int offset, int ascending,
                                                                      int64_t row_offset, int64_t* __restrict__ out_ids,
                                                                      float* __restrict__ out_scores) {
    extern __shared__ unsigned long long deep_keys[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const unsigned got = a.n > 0 ? a.state[q].count : 0u;
    const int found = (int)(got < (unsigned)a.W ? got : (unsigned)a.W);
    const unsigned long long* in = a.keys + (int64_t)q * a.W;
    for (int i = tid; i < P; i += kDeepSortThreads) deep_keys[i] = i < found ? in[i] : 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kDeepSortThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const unsigned long long x = deep_keys[i], y = deep_keys[i + j];
                const bool desc = (i & size) == 0;
                if (desc ? x < y : x > y) {
                    deep_keys[i] = y;
                    deep_keys[i + j] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += kDeepSortThreads) {
        const int src = offset + i;
        const int64_t o = (int64_t)q * k + i;
        if (src < found) {
            const uint64_t me = deep_keys[src];
            out_ids[o] = (int64_t)key_row(me) + row_offset;
            out_scores[o] = ascending ? -key_score(me) : key_score(me);
        } else {
            out_ids[o] = -1;
            out_scores[o] = 0.f;
        }
    }
}

}  // namespace hbmrag
