// Grouping search (Milvus' Collection.search(..., group_by_field=..., group_size=...)) on the device: the first entry —
// or the first group_size entries — of every group of a batch of ranked lists, and the row masks that take whole groups
// out of the next search or keep nothing but them.
//
// A group key is an int64 per row (advanced_rag/columns.py: an integer column as it is, or the ordinal of a string in
// a collection-wide dictionary).  No kernel here reads a score: descending, ascending (L2) and fp64 fused lists are
// all "a list in ranking order".
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

// The valid prefix of one list and its entries' keys, staged in LDS by a block of 256 threads (both select kernels):
//   n = *n_valid clamped into [0, k_in], or without n_valid the position of the first id < 0 (k_in if none)
//   key[i] / has_key[i] for i < n: the key of entry i, or the id itself and 0 for an id outside [first_row, first_row + key_rows)
// -> n.  The caller's next __syncthreads() makes key / has_key visible to the block.
__device__ inline int group_stage_list(const int64_t* __restrict__ my_ids, const int32_t* __restrict__ n_valid, int k_in,
                                       const int64_t* __restrict__ keys, int64_t key_rows, int64_t first_row, int64_t* key,
                                       int* has_key, int* s_n) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int n = k_in;
        if (n_valid) {
            n = *n_valid;
            n = n < 0 ? 0 : (n > k_in ? k_in : n);
        }
        *s_n = n;
    }
    __syncthreads();
    if (!n_valid) {   // the list ends at its first negative id: the smallest such position (a minimum: order-free)
        int end = k_in;
        for (int i = tid; i < k_in; i += 256)
            if (my_ids[i] < 0) { end = i; break; }   // positions ascend per thread
        if (end < k_in) atomicMin(s_n, end);
        __syncthreads();
    }
    const int n = *s_n;
    for (int i = tid; i < n; i += 256) {
        const int64_t id = my_ids[i];
        const int64_t r = id - first_row;
        const bool in = id >= first_row && r < key_rows;   // (id >= first_row first: r cannot have wrapped when it is read)
        key[i] = in ? keys[r] : id;
        has_key[i] = in;
    }
    return n;
}

// One block (256 threads) per query.  Restates "the first occurrence of every key, in list order, at most k_out":
//   n        = n_valid[q] clamped into [0, k_in], or without n_valid the position of the first id < 0 (k_in if none)
//   first[i] = entry i has no key (its id lies outside [first_row, first_row + key_rows)): a group of its own — or no
//              entry j < i with a key has the same key
//   out_pos  = the first k_out positions with first[i], ascending, -1 padded; out_keys their keys (the id itself for
//              an entry without a key); out_n their number
//   flag     = out_n == k_out (the list gave every group asked for) or n < k_in (the search behind the list ran out
//              of qualifying rows); 0 = the window ended before the k_out-th group
// "First of its group" is decided by position alone — every thread compares its entries with the entries before
// them in LDS — and the output slot of a first is the number of firsts before it (ballot + wave totals): nothing
// depends on the order threads run in.
__global__ __launch_bounds__(256) void group_select_kernel(
    const int64_t* __restrict__ ids, const int32_t* __restrict__ n_valid, int k_in, const int64_t* __restrict__ keys,
    int64_t key_rows, int64_t first_row, int k_out, int32_t* __restrict__ out_pos, int64_t* __restrict__ out_keys,
    int32_t* __restrict__ out_n, int32_t* __restrict__ flags) {
    __shared__ int64_t key[kFuseMax];
    __shared__ int has_key[kFuseMax];
    __shared__ int first[kFuseMax];
    __shared__ int w_count[4];
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = group_stage_list(ids + (int64_t)q * k_in, n_valid ? n_valid + q : nullptr, k_in, keys, key_rows, first_row, key,
                                   has_key, &s_n);
    for (int i = tid; i < k_out; i += 256) {
        out_pos[(int64_t)q * k_out + i] = -1;
        if (out_keys) out_keys[(int64_t)q * k_out + i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        int f = 1;
        if (has_key[i]) {
            const int64_t k = key[i];
            for (int j = 0; j < i; ++j)
                if (has_key[j] && key[j] == k) { f = 0; break; }
        }
        first[i] = f;
    }
    __syncthreads();
    // output slot of a first = firsts before it: 256 positions per trip, ballot within a wave, totals across the waves
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {   // n is block-uniform: every thread takes part in every barrier
        const int i = c0 + tid;
        const bool f = i < n && first[i];
        const unsigned long long m = __ballot(f);
        if (lane == 0) w_count[wave] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += w_count[w];
        const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
        if (f && slot < k_out) {
            out_pos[(int64_t)q * k_out + slot] = i;
            if (out_keys) out_keys[(int64_t)q * k_out + slot] = key[i];
        }
        base += w_count[0] + w_count[1] + w_count[2] + w_count[3];
        __syncthreads();   // w_count is rewritten by the next trip
    }
    if (tid == 0) {
        const int sel = base < k_out ? base : k_out;
        out_n[q] = sel;
        if (flags) flags[q] = (sel == k_out || n < k_in) ? 1 : 0;
    }
}

// One block (256 threads) per query.  group_select_kernel with up to group_size members per group — restates "walk the
// list, count the members of every key, keep the first k_out groups and the first group_size members of each":
//   rank[i]  = entries j < i of entry i's group (an entry without a key is a group of its own); leader = rank 0
//   ord      = a leader's ordinal: the leaders before it (ballot + wave totals, as above)
//   out_pos  [k_out][group_size]: slot ord * group_size + rank = i for every entry with ord < k_out and rank <
//              group_size, -1 padded; out_keys [k_out] the groups' keys, 0 padded; out_cnt [k_out] = min(members of
//              the group in the list, group_size), 0 padded; out_n = min(leaders, k_out)
//   flags    bit 0 = group_select_kernel's flag; bit 1 = every selected group has group_size members, or n < k_in
// Every output word is written once, by the thread that position arithmetic names: no atomic decides anything.
__global__ __launch_bounds__(256) void group_select_n_kernel(
    const int64_t* __restrict__ ids, const int32_t* __restrict__ n_valid, int k_in, const int64_t* __restrict__ keys,
    int64_t key_rows, int64_t first_row, int k_out, int group_size, int32_t* __restrict__ out_pos,
    int64_t* __restrict__ out_keys, int32_t* __restrict__ out_cnt, int32_t* __restrict__ out_n, int32_t* __restrict__ flags) {
    __shared__ int64_t key[kFuseMax];
    __shared__ int has_key[kFuseMax];
    __shared__ int rank[kFuseMax];      // entries of the same group before this one
    __shared__ int lead[kFuseMax];      // position of the group's leader; at a leader: minus the group's members in the list
    __shared__ int ord[kFuseMax];       // leaders only: the group's ordinal
    __shared__ int cnt[kFuseMax];       // by ordinal < k_out: members written
    __shared__ int w_count[4];
    __shared__ int s_n, s_short;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = group_stage_list(ids + (int64_t)q * k_in, n_valid ? n_valid + q : nullptr, k_in, keys, key_rows, first_row, key,
                                   has_key, &s_n);
    if (tid == 0) s_short = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        int before = 0, members = 1, leader = i;
        if (has_key[i]) {
            const int64_t k = key[i];
            members = 0;
            for (int j = 0; j < n; ++j) {      // every thread reads the same word: an LDS broadcast
                const bool same = has_key[j] && key[j] == k;
                if (same && !members) leader = j;
                members += same;
                before += same && j < i;
            }
        }
        rank[i] = before;
        lead[i] = before ? leader : -members;      // a leader keeps its group's size, negated: told apart by the sign
    }
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {   // n is block-uniform: every thread takes part in every barrier
        const int i = c0 + tid;
        const bool f = i < n && rank[i] == 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) w_count[wave] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += w_count[w];
        if (f) ord[i] = before + __popcll(m & ((1ull << lane) - 1ull));
        base += w_count[0] + w_count[1] + w_count[2] + w_count[3];
        __syncthreads();   // w_count is rewritten by the next trip
    }
    const int sel = base < k_out ? base : k_out;
    int32_t* my_pos = out_pos + (int64_t)q * k_out * group_size;
    for (int i = tid; i < n; i += 256) {
        const int r = rank[i];
        const int o = ord[r ? lead[i] : i];
        if (o >= k_out) continue;
        if (r < group_size) my_pos[o * group_size + r] = i;
        if (r == 0) {
            const int members = -lead[i];
            cnt[o] = members < group_size ? members : group_size;
            if (members < group_size) s_short = 1;      // (every writer stores the same value)
            if (out_keys) out_keys[(int64_t)q * k_out + o] = key[i];
        }
    }
    __syncthreads();
    for (int s = tid; s < k_out * group_size; s += 256) {      // the slots no entry owns
        const int o = s / group_size;
        if (o >= sel || s - o * group_size >= cnt[o]) my_pos[s] = -1;
    }
    for (int o = tid; o < k_out; o += 256) {
        out_cnt[(int64_t)q * k_out + o] = o < sel ? cnt[o] : 0;
        if (out_keys && o >= sel) out_keys[(int64_t)q * k_out + o] = 0;
    }
    if (tid == 0) {
        out_n[q] = sel;
        const int ran_out = n < k_in;
        if (flags) flags[q] = ((sel == k_out || ran_out) ? 1 : 0) | ((!s_short || ran_out) ? 2 : 0);
    }
}

// Bit r of mask_out = bit r of mask_in (all ones when mask_in is null) AND "keys[r] is not one of the n_drop keys"
// (kKeep = false: hr_mask_drop_groups_dev) or AND "keys[r] is one of them" (kKeep = true: hr_mask_keep_groups_dev; an
// empty set keeps no row).
// The 64-row grid of filter.h: one wave per 64 consecutive rows per trip, lane = row, so the key column is read with
// coalesced wave loads and the 64 verdicts leave as one 8-byte store by lane 0, which has read the same word of
// mask_in before — the buffers may alias.  Rows at and beyond n_rows are written 0.
// The key set (any order, duplicates allowed, at most kFuseMax keys) is staged in LDS in ascending order — every
// thread places its keys at their rank among all of them (equal keys keep their order: the ranks are a permutation) —
// and a row looks its key up by binary search.
template <bool kKeep>
__global__ __launch_bounds__(256) void mask_groups_kernel(
    const unsigned long long* mask_in, unsigned long long* mask_out, int64_t n_rows,
    const int64_t* __restrict__ keys, const int64_t* __restrict__ drop, int n_drop) {
    __shared__ int64_t raw[kFuseMax];
    __shared__ int64_t sorted[kFuseMax];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < n_drop; i += 256) raw[i] = drop[i];
    __syncthreads();
    for (int i = tid; i < n_drop; i += 256) {
        const int64_t k = raw[i];
        int rank = 0;
        for (int j = 0; j < n_drop; ++j) rank += (raw[j] < k || (raw[j] == k && j < i)) ? 1 : 0;
        sorted[rank] = k;
    }
    __syncthreads();
    const int64_t wave = (int64_t)blockIdx.x * 4 + (tid >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_words = (n_rows + 63) / 64;
    for (int64_t w = wave; w < n_words; w += n_waves) {
        const int64_t row = w * 64 + lane;
        bool keep = row < n_rows;
        if (keep && mask_in) keep = (mask_in[w] >> lane) & 1ull;
        if (keep && (kKeep || n_drop)) {
            bool found = false;
            if (n_drop) {
                const int64_t k = keys[row];
                int lo = 0, hi = n_drop;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sorted[mid] < k) lo = mid + 1; else hi = mid;
                }
                found = lo < n_drop && sorted[lo] == k;
            }
            keep = found == kKeep;
        }
        const unsigned long long km = __ballot(keep);
        if (lane == 0) mask_out[w] = km;
    }
}

}  // namespace hbmrag
