// Read path (Collection.query): a row mask becomes a page of row ids, and stored rows come back out of the tiles.
//
// Replaces Collection.query(expr, output_fields, limit, offset) of the Milvus server (pymilvus; the reference reads rows
// back only through search hits, indexing.py:527-547).  Two kernels, and the sparse rows' gather at the end of the file:
//   mask_rows_window_kernel  the third phase of compact.h's scan with a window: of the set bits of a packed row mask, in
//                            ascending row order, the ones numbered [offset, offset + limit) are written as 64-bit row ids.
//                            Phases 1 and 2 are compact.h's own (compact_block_sums_kernel<KeepCount>,
//                            compact_scan_sums_kernel); an ordered prefix decides every position, nothing races.
//   get_rows_kernel          compact_tiles_kernel turned round: the tiles are the source, a row-major matrix the
//                            destination.  Stored bits are moved (or widened exactly); nothing is re-quantised.
#pragma once
#include <type_traits>
#include "common.h"
#include "compact.h"

namespace hbmrag {

// d_mask == NULL (every row passes) and n_rows == 0: the page is an arithmetic sequence, no scan.
__global__ void mask_rows_all_kernel(int64_t n_rows, int64_t first_row, int64_t offset, int64_t limit,
                                     int64_t* __restrict__ rows, int64_t* __restrict__ counts) {
    const int64_t n_out = n_rows > offset ? (n_rows - offset < limit ? n_rows - offset : limit) : 0;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        counts[0] = n_rows;
        counts[1] = n_out;
    }
    if (i < n_out) rows[i] = first_row + offset + i;
}

// Phase 3 with a window.  A block takes 1024 mask words; block_off[b] is the number of set bits before the block (phase
// 2), *total the number of all.  A block whose bits [block_off, block_off + block_total) miss [offset, offset + limit)
// returns at once, before the scan's first barrier (the test is block-uniform).  Writes are bounded by the window:
// rows[dst - offset] for offset <= dst < offset + limit, and dst < *total <= n_rows always holds.
__global__ void __launch_bounds__(kCompactBlock) mask_rows_window_kernel(const unsigned long long* __restrict__ mask, int64_t n_rows,
                                                                        int64_t n_words, const unsigned long long* __restrict__ block_off,
                                                                        const unsigned long long* __restrict__ total, int64_t first_row,
                                                                        int64_t offset, int64_t limit, int64_t* __restrict__ rows,
                                                                        int64_t* __restrict__ counts) {
    __shared__ unsigned long long wave_tot[kCompactBlock / 64];
    __shared__ unsigned long long word_base[kCompactBlock];
    const int64_t n_set = (int64_t)*total;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = n_set;
        counts[1] = n_set > offset ? (n_set - offset < limit ? n_set - offset : limit) : 0;
    }
    const int64_t lo = (int64_t)block_off[blockIdx.x];
    const int64_t hi = blockIdx.x + 1 < gridDim.x ? (int64_t)block_off[blockIdx.x + 1] : n_set;
    // offset + limit cannot wrap: the entry point keeps both below 2^62
    if (limit == 0 || hi <= offset || lo >= offset + limit || hi == lo) return;
    const int64_t w_mine = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const unsigned v = w_mine < n_words ? (unsigned)__popcll(compact_keep_word(mask, w_mine, n_rows)) : 0u;
    unsigned long long block_total;
    word_base[threadIdx.x] = (unsigned long long)lo + compact_block_scan(v, wave_tot, &block_total);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < 64; ++i) {
        const int64_t w = (int64_t)blockIdx.x * kCompactBlock + wave * 64 + i;
        if (w >= n_words) break;  // wave-uniform
        const unsigned long long m = compact_keep_word(mask, w, n_rows);
        if ((m >> lane) & 1ull) {
            const int64_t dst = (int64_t)word_base[wave * 64 + i] + __popcll(m & ((1ull << lane) - 1ull));
            if (dst >= offset && dst - offset < limit) rows[dst - offset] = first_row + w * 64 + lane;
        }
    }
}

// Stored rows out of the tiles.  A wave takes 16 consecutive OUTPUT rows and walks the KT tiles of their source rows (KT
// is a multiple of 4).  Lane l holds output row ob*16 + (l & 15) and k-chunk kt*4 + (l >> 4) — the lane map of
// compact_tiles_kernel with source and destination swapped: it reads its row id once, then per tile one guarded 16-byte
// load from chunk_index(src, kchunk, KT); four tiles' loads are issued before the first store.  An id outside the shard
// reads nothing and gives a row of zeros; *missing counts such ids (one order-independent atomic per wave).  Padding is
// never shown: only elements below dim are stored.
//   SRC_HALF  the shard stores fp16 (8 elements per chunk), else fp32 (4)
//   OUT_HALF  raw fp16 bits out (only with SRC_HALF), else fp32 (fp16 widened exactly)
//   VEC       out + row * out_stride is 16-byte aligned for every row: whole chunks leave as 16-byte stores, the four
//             lanes of a row writing 64 (fp16 -> fp32: 128) contiguous bytes per tile; else element by element
constexpr int kGetRowsWaves = 4;  // waves (blocks of 16 output rows) per block
template <bool SRC_HALF, bool OUT_HALF, bool VEC>
__global__ void __launch_bounds__(kGetRowsWaves * 64) get_rows_kernel(const chunk_t* __restrict__ tiles, int64_t n_rows, int64_t row_offset,
                                                                     int KT, int64_t dim, const int64_t* __restrict__ ids, int64_t n,
                                                                     void* __restrict__ out_, int64_t out_stride, int32_t* __restrict__ missing) {
    static_assert(SRC_HALF || !OUT_HALF, "fp16 output needs an fp16 shard");
    using out_t = typename std::conditional<OUT_HALF, _Float16, float>::type;
    using src_vec_t = typename std::conditional<SRC_HALF, half8_t, f32x4_t>::type;
    constexpr int E = SRC_HALF ? 8 : 4;  // elements per chunk
    const int lane = threadIdx.x & 63;
    const int64_t ob = (int64_t)blockIdx.x * kGetRowsWaves + (threadIdx.x >> 6);
    if (ob * kRowsPerBlock >= n) return;  // wave-uniform
    const int64_t orow = ob * kRowsPerBlock + (lane & 15);
    const bool wanted = orow < n;
    const int64_t src = wanted ? ids[orow] - row_offset : 0;
    const bool live = wanted && src >= 0 && src < n_rows;
    const int c = lane >> 4;
    if (missing) {
        const int n_miss = __popcll(__ballot(wanted && !live && c == 0));
        if (lane == 0 && n_miss) atomicAdd(missing, n_miss);
    }
    if (!wanted) return;
    // chunk_index(src, kt*4 + c, KT) = ((src >> 4) * KT + kt) * 64 + (src & 15) + 16 * c
    const chunk_t* sp = tiles + (live ? (src >> 4) * KT * kTileChunks + (src & 15) + 16 * c : 0);
    out_t* op = (out_t*)out_ + orow * out_stride;
    const chunk_t zero = chunk_t{0u, 0u, 0u, 0u};
    for (int kt = 0; kt < KT; kt += 4) {
        chunk_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = live ? sp[(int64_t)(kt + u) * kTileChunks] : zero;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e0 = ((int64_t)(kt + u) * 4 + c) * E;  // first element of this lane's chunk
            if (e0 >= dim) continue;
            if (VEC && e0 + E <= dim) {
                if (SRC_HALF == OUT_HALF) {  // the bits as they are
                    *(chunk_t*)(op + e0) = v[u];
                } else {  // fp16 -> fp32 is exact
                    const half8_t x = __builtin_bit_cast(half8_t, v[u]);
                    *(f32x4_t*)(op + e0) = f32x4_t{(float)x[0], (float)x[1], (float)x[2], (float)x[3]};
                    *(f32x4_t*)(op + e0 + 4) = f32x4_t{(float)x[4], (float)x[5], (float)x[6], (float)x[7]};
                }
            } else {  // the ragged last chunk, or rows that are not 16-byte aligned: element by element, never past dim
                const src_vec_t x = __builtin_bit_cast(src_vec_t, v[u]);
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if (e0 + j < dim) op[e0 + j] = (out_t)x[j];
            }
        }
    }
}

// ---- stored sparse rows out of the CSR (hr_get_sparse_rows_dev) ----
// compact.h's CSR gather with an id list in place of the row map.  The lengths of the requested rows are summed by the
// three-phase scan (compact_block_sums_kernel<RequestedLength>, compact_scan_sums_kernel, get_sparse_indptr_kernel), so
// every output position is an ordered prefix over the request.  An id outside the shard has length 0.
struct RequestedLength {
    const int64_t* indptr;
    const int64_t* ids;
    int64_t n_rows, row_offset;
    // n_rows > 0 whenever indptr is read; the subtraction cannot wrap for any id the test below lets through
    __device__ bool holds(int64_t id) const { return id >= row_offset && id - row_offset < n_rows; }
    __device__ unsigned operator()(int64_t i) const {
        const int64_t id = ids[i];
        if (!holds(id)) return 0u;
        const int64_t s = id - row_offset;
        return (unsigned)(indptr[s + 1] - indptr[s]);
    }
};

// n == 0: the indptr's one entry and both counts.
__global__ void get_sparse_empty_kernel(int64_t* __restrict__ out_indptr, int64_t* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_indptr[0] = 0;
        counts[0] = 0;
        counts[1] = 0;
    }
}

// Phase 3: out_indptr[i] = entries of the requested rows before i, out_indptr[n] = counts[0] = all of them (*total, phase
// 2).  counts[1], zeroed by the caller, counts the ids outside the shard: one order-independent atomic per wave.
__global__ void __launch_bounds__(kCompactBlock) get_sparse_indptr_kernel(RequestedLength len, int64_t n,
                                                                         const unsigned long long* __restrict__ block_off,
                                                                         const unsigned long long* __restrict__ total,
                                                                         int64_t* __restrict__ out_indptr, int64_t* __restrict__ counts) {
    __shared__ unsigned long long wave_tot[kCompactBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const bool wanted = i < n;
    const bool live = wanted && len.holds(len.ids[i]);
    const unsigned v = live ? len(i) : 0u;
    unsigned long long block_total;
    const unsigned long long before = block_off[blockIdx.x] + compact_block_scan(v, wave_tot, &block_total);
    if (wanted) out_indptr[i] = (int64_t)before;
    if (i == 0) {
        out_indptr[n] = (int64_t)*total;
        counts[0] = (int64_t)*total;
    }
    const int n_miss = __popcll(__ballot(wanted && !live));
    if ((threadIdx.x & 63) == 0 && n_miss) atomicAdd((unsigned long long*)&counts[1], (unsigned long long)n_miss);
}

// The entries: a wave per requested row, lanes over its entries (compact_csr_kernel's walk).  Entry e of output row i
// goes to out_indptr[i] + e, and only when that is below cap: nothing at or past cap is touched.
constexpr int kGetSparseWaves = 4;  // waves (requested rows) per block
__global__ void __launch_bounds__(kGetSparseWaves * 64) get_sparse_rows_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                                              const float* __restrict__ val, int64_t n_rows, int64_t row_offset,
                                                                              const int64_t* __restrict__ ids, int64_t n,
                                                                              const int64_t* __restrict__ out_indptr, int32_t* __restrict__ out_idx,
                                                                              float* __restrict__ out_val, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kGetSparseWaves + (threadIdx.x >> 6);
    if (i >= n) return;  // wave-uniform
    const int64_t id = ids[i];
    if (id < row_offset || id - row_offset >= n_rows) return;  // wave-uniform: an empty row
    const int64_t s = id - row_offset;
    const int64_t e0 = indptr[s], d0 = out_indptr[i];
    int64_t len = indptr[s + 1] - e0;
    if (d0 >= cap) return;
    if (cap - d0 < len) len = cap - d0;  // the row that cap cuts
    for (int64_t e = lane; e < len; e += 64) {
        out_idx[d0 + e] = idx[e0 + e];
        out_val[d0 + e] = val[e0 + e];
    }
}

}  // namespace hbmrag
