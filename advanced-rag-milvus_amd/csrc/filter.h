// Filter expressions on the device: `field OP value and field OP value ...` (the expressions
// HybridRetriever._build_filter_expression emits, reference src/advanced_rag/retrieval.py:565-632, over the scalar
// fields of the collection schema, indexing.py:191-225) evaluated over columns that live in HBM, straight into the
// packed row mask the scans and refines test (bit r%8 of byte r/8) — Milvus evaluates them server-side; nothing
// row-sized crosses PCIe here.
//
// Columns: int64 (chunk_index, token_count), float32 (entropy, redundancy, domain_density), and for string fields
// (doc_id, chunk_id, timestamp) an ORDER-PRESERVING 16-byte prefix key per row (two big-endian uint64 words of the
// zero-padded UTF-8 bytes; advanced_rag/columns.py).  A string term is decided by the key wherever the first 16 bytes
// of row and value differ; rows that tie are reported in a second bit mask ("undecided") and resolved by the host on
// the full strings — a handful of rows, if any.  Comparison rules are numpy's for the same column and literal types
// (advanced_rag/filters.py is the restatement the tests compare with): int64 column vs int -> int64; int64 column vs
// float -> float64; float32 column vs number -> float32.
#pragma once
#include "common.h"

namespace hbmrag {

constexpr int kFilterMaxTerms = 16;

struct FilterArgs {
    hr_filter_term t[kFilterMaxTerms];
    int n_terms;
    int64_t n_rows;
    const uint8_t* deleted;      // tombstones, 1 bit per row (1 = deleted), or null
    unsigned long long* mask;    // out: ceil(n_rows / 64) words
    unsigned long long* undecided;
    int32_t* counts;             // [0] += rows kept, [1] += rows undecided
};

template <typename T>
__device__ inline bool filter_cmp(T a, T b, int op) {
    switch (op) {
        case HR_OP_EQ: return a == b;
        case HR_OP_NE: return a != b;
        case HR_OP_LT: return a < b;
        case HR_OP_LE: return a <= b;
        case HR_OP_GT: return a > b;
        default: return a >= b;
    }
}

// One wave per 64 consecutive rows per trip: lane = row, so every column read is one coalesced wave load and the
// 64 verdicts leave as one 8-byte store (ballot).
__global__ __launch_bounds__(256) void filter_eval_kernel(FilterArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_words = (a.n_rows + 63) / 64;
    int kept = 0, und = 0;
    for (int64_t w = wave; w < n_words; w += n_waves) {
        const int64_t row = w * 64 + lane;
        const bool in = row < a.n_rows;
        bool fail = !in, maybe = false;
        if (in && a.deleted) fail = (a.deleted[row >> 3] >> (row & 7)) & 1;
        for (int i = 0; i < a.n_terms; ++i) {
            const hr_filter_term& t = a.t[i];
            bool pass = true, tie = false;
            if (in) {
                switch (t.kind) {
                    case HR_COL_I64: pass = filter_cmp<int64_t>(((const int64_t*)t.col)[row], t.ival, t.op); break;
                    case HR_COL_I64_VS_F64: pass = filter_cmp<double>((double)((const int64_t*)t.col)[row], t.dval, t.op); break;
                    case HR_COL_F32: pass = filter_cmp<float>(((const float*)t.col)[row], t.fval, t.op); break;
                    default: {  // HR_COL_STR16
                        const unsigned long long k0 = ((const unsigned long long*)t.col)[2 * row];
                        const unsigned long long k1 = ((const unsigned long long*)t.col)[2 * row + 1];
                        if (k0 == t.key[0] && k1 == t.key[1]) {
                            tie = true;  // the first 16 bytes agree: the host compares the full strings
                        } else {
                            const bool less = k0 < t.key[0] || (k0 == t.key[0] && k1 < t.key[1]);
                            pass = t.op == HR_OP_EQ ? false : t.op == HR_OP_NE ? true
                                 : (t.op == HR_OP_LT || t.op == HR_OP_LE) ? less : !less;
                        }
                    }
                }
            }
            if (tie) maybe = true;
            else if (!pass) fail = true;
        }
        const bool keep = !fail && !maybe, undecided = !fail && maybe;
        const unsigned long long km = __ballot(keep), um = __ballot(undecided);
        if (lane == 0) {
            a.mask[w] = km;
            a.undecided[w] = um;
            kept += __popcll(km);
            und += __popcll(um);
        }
    }
    if (lane == 0 && (kept | und)) {
        if (kept) atomicAdd(&a.counts[0], kept);
        if (und) atomicAdd(&a.counts[1], und);
    }
}

// ---- expressions beyond the conjunction: `in` lists, or, not, parentheses (hr_filter_eval_expr_dev) ------------------
// The expression arrives as leaves (a comparison as above, or a membership test against a sorted set) and a postfix
// program over them.  A string leaf cannot always decide a row, so a leaf's value is true, false or unknown and the
// operators are Kleene's; the value is held as a pair of bounds (lo = "certainly true", hi = "possibly true"), and the
// evaluation stack as two 32-bit fields of such bits, top of stack in bit 0: a push is a shift, and / or combine bits 0
// and 1 of both fields, not swaps and inverts bit 0 of the two.  No indexed array, so no scratch memory.
//
// The sets are staged in LDS once per block (each at a 16-byte aligned offset) and searched per lane by a binary search
// whose trip count depends on the set's size alone: the wave stays converged, only the LDS addresses differ.
constexpr int kFilterMaxProgram = 64;
constexpr int kFilterMaxDepth = 32;
constexpr int kFilterMaxSetBytes = 65536;

struct FilterExprArgs {
    hr_filter_term t[kFilterMaxTerms];
    const void* set[kFilterMaxTerms];     // device arrays, ascending; staged at set_off
    int32_t set_off[kFilterMaxTerms];     // byte offset inside the block's LDS
    int32_t n_set[kFilterMaxTerms];
    int8_t program[kFilterMaxProgram];    // >= 0: push that leaf; HR_FILTER_AND / _OR / _NOT
    int n_leaves, n_program;
    int64_t n_rows;
    const uint8_t* deleted;
    unsigned long long* mask;
    unsigned long long* undecided;
    int32_t* counts;
};

// Index of the last member <= v among n >= 1 ascending members (0 when there is none): the member to compare with.
template <typename T>
__device__ inline bool filter_set_has(const T* set, int n, T v) {
    int base = 0;
    for (int len = n; len > 1;) {
        const int half = len >> 1;
        if (set[base + half] <= v) base += half;
        len -= half;
    }
    return set[base] == v;
}

struct FilterKey {
    unsigned long long w0, w1;
    __device__ bool operator<=(const FilterKey& o) const { return w0 < o.w0 || (w0 == o.w0 && w1 <= o.w1); }
    __device__ bool operator==(const FilterKey& o) const { return w0 == o.w0 && w1 == o.w1; }
};

// A TEXT_MATCH leaf (kind HR_COL_TOKENS, op HR_OP_MATCH) reads a row's WORD SET, not one scalar: a CSR of ascending int32
// word ids per row (term.col = int64 indptr[tok_rows + 1], term.key[0] = the word array, term.key[1] = tok_rows, a row at or
// beyond tok_rows is empty).  A row passes iff at least term.ival of the leaf's set members are among its words.  A lane
// that walked its own row would read 4 bytes at a stride of the row length, so the leaf is wave-cooperative instead: the
// words of the wave's 64 rows are ONE contiguous span of the array, indptr[64w] .. indptr[min(64w + 64, tok_rows)], which
// the wave streams 64 entries at a time (lane = entry: coalesced).  Every entry is looked up in the LDS-staged set with
// the fixed-trip search above; a hit belongs to the row whose span holds the entry — the number of row ENDS <= the
// entry's offset, an upper bound, so that empty rows (equal ends) are stepped over — and bumps that row's counter in LDS
// (integer atomics: the sum does not depend on their order).  Lane r then reads counter r.  Ends and counters are per
// wave and rewritten by every leaf of every trip.  Only filter_expr_kernel<true> carries any of this: an expression
// without such a leaf launches <false>, the kernel it always ran.
struct FilterMatchScratch {
    long long end[4][64];   // per wave: offset, from the span's start, where the words of row r end
    int count[4][64];       // per wave: set members found in row r
};

__device__ inline bool filter_match(const hr_filter_term& t, const int32_t* set, int n, int64_t w, int lane,
                                    long long* end, int* count) {
    const int64_t* indptr = (const int64_t*)t.col;
    const int32_t* words = (const int32_t*)(uintptr_t)t.key[0];
    const int64_t tok_rows = (int64_t)t.key[1], r0 = w * 64;
    const int64_t begin = indptr[r0 < tok_rows ? r0 : tok_rows];
    const int64_t last = r0 + lane + 1;
    end[lane] = indptr[last < tok_rows ? last : tok_rows] - begin;   // one coalesced 8-byte load; non-decreasing over the lanes
    count[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t total = end[63];
    for (int64_t e0 = 0; e0 < total; e0 += 64) {    // wave-uniform trip count
        const int64_t e = e0 + lane;
        const bool live = e < total;
        const int32_t word = live ? words[begin + e] : 0;
        if (live && filter_set_has<int32_t>(set, n, word)) {
            int r = 0;                               // the rows whose words end at or before e: at most 63, as end[63] > e
            for (int step = 32; step; step >>= 1)
                if (end[r + step - 1] <= e) r += step;
            atomicAdd(&count[r], 1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool pass = (int64_t)count[lane] >= t.ival;
    __builtin_amdgcn_wave_barrier();                 // the next leaf rewrites ends and counters only after every lane has read
    return pass;
}

template <bool kHasMatch>
__global__ __launch_bounds__(256) void filter_expr_kernel(FilterExprArgs a) {
    extern __shared__ __align__(16) unsigned char filter_sets[];
    for (int i = 0; i < a.n_leaves; ++i) {
        int per_member;
        if constexpr (kHasMatch) {
            if (a.t[i].op != HR_OP_IN && a.t[i].op != HR_OP_MATCH) continue;
            per_member = (a.t[i].kind == HR_COL_F32 || a.t[i].kind == HR_COL_TOKENS) ? 1 : a.t[i].kind == HR_COL_I64 ? 2 : 4;
        } else {
            if (a.t[i].op != HR_OP_IN) continue;
            per_member = a.t[i].kind == HR_COL_F32 ? 1 : a.t[i].kind == HR_COL_I64 ? 2 : 4;
        }
        const int words = a.n_set[i] * per_member;
        const uint32_t* src = (const uint32_t*)a.set[i];
        uint32_t* dst = (uint32_t*)(filter_sets + a.set_off[i]);
        for (int j = threadIdx.x; j < words; j += 256) dst[j] = src[j];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int64_t n_words = (a.n_rows + 63) / 64;
    int kept = 0, und = 0;
    for (int64_t w = wave; w < n_words; w += n_waves) {
        const int64_t row = w * 64 + lane;
        const bool in = row < a.n_rows;
        bool dead = !in;
        if (in && a.deleted) dead = (a.deleted[row >> 3] >> (row & 7)) & 1;
        uint32_t lo = 0, hi = 0;
        for (int pc = 0; pc < a.n_program; ++pc) {
            const int code = a.program[pc];
            if (code == HR_FILTER_AND) {
                lo = (lo >> 1) & (lo | ~1u);
                hi = (hi >> 1) & (hi | ~1u);
            } else if (code == HR_FILTER_OR) {
                lo = (lo >> 1) | (lo & 1u);
                hi = (hi >> 1) | (hi & 1u);
            } else if (code == HR_FILTER_NOT) {
                const uint32_t was = lo;
                lo = (lo & ~1u) | (~hi & 1u);
                hi = (hi & ~1u) | (~was & 1u);
            } else {
                const hr_filter_term& t = a.t[code];
                bool pass = false, tie = false;
                if (kHasMatch && t.op == HR_OP_MATCH) {
                    if constexpr (kHasMatch) {
                        __shared__ FilterMatchScratch scratch;
                        const int n = a.n_set[code], wv = threadIdx.x >> 6;
                        if (n > 0)   // an empty set: no member is found in any row, and ival >= 1
                            pass = filter_match(t, (const int32_t*)(filter_sets + a.set_off[code]), n, w, lane, scratch.end[wv],
                                                scratch.count[wv]);
                    }
                } else if (t.op == HR_OP_IN) {
                    const int n = a.n_set[code];
                    const unsigned char* set = filter_sets + a.set_off[code];
                    if (n > 0) {   // a row beyond n_rows searches for 0: every read stays inside the set
                        if (t.kind == HR_COL_I64) {
                            pass = filter_set_has<int64_t>((const int64_t*)set, n, in ? ((const int64_t*)t.col)[row] : 0);
                        } else if (t.kind == HR_COL_F32) {
                            pass = filter_set_has<float>((const float*)set, n, in ? ((const float*)t.col)[row] : 0.0f);
                        } else {
                            FilterKey k{0, 0};
                            if (in) k = FilterKey{((const unsigned long long*)t.col)[2 * row], ((const unsigned long long*)t.col)[2 * row + 1]};
                            tie = filter_set_has<FilterKey>((const FilterKey*)set, n, k);   // equal prefix: the host decides
                        }
                    }
                } else if (in) {
                    switch (t.kind) {
                        case HR_COL_I64: pass = filter_cmp<int64_t>(((const int64_t*)t.col)[row], t.ival, t.op); break;
                        case HR_COL_I64_VS_F64: pass = filter_cmp<double>((double)((const int64_t*)t.col)[row], t.dval, t.op); break;
                        case HR_COL_F32: pass = filter_cmp<float>(((const float*)t.col)[row], t.fval, t.op); break;
                        default: {  // HR_COL_STR16
                            const unsigned long long k0 = ((const unsigned long long*)t.col)[2 * row];
                            const unsigned long long k1 = ((const unsigned long long*)t.col)[2 * row + 1];
                            if (k0 == t.key[0] && k1 == t.key[1]) {
                                tie = true;
                            } else {
                                const bool less = k0 < t.key[0] || (k0 == t.key[0] && k1 < t.key[1]);
                                pass = t.op == HR_OP_EQ ? false : t.op == HR_OP_NE ? true
                                     : (t.op == HR_OP_LT || t.op == HR_OP_LE) ? less : !less;
                            }
                        }
                    }
                }
                lo = (lo << 1) | (uint32_t)(pass && !tie);
                hi = (hi << 1) | (uint32_t)(pass || tie);
            }
        }
        const bool keep = !dead && (lo & 1u), undecided = !dead && (hi & 1u) && !(lo & 1u);
        const unsigned long long km = __ballot(keep), um = __ballot(undecided);
        if (lane == 0) {
            a.mask[w] = km;
            a.undecided[w] = um;
            kept += __popcll(km);
            und += __popcll(um);
        }
    }
    if (lane == 0 && (kept | und)) {
        if (kept) atomicAdd(&a.counts[0], kept);
        if (und) atomicAdd(&a.counts[1], und);
    }
}

}  // namespace hbmrag
