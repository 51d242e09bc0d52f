// Compaction kernels (hr_compact): drop rows from the shard store for good.
//
// Replaces Collection.compact() of the Milvus server behind the reference's delete path (indexing.py:692-696
// delete_by_filter -> Collection.delete(expr)): the keep mask becomes a row map (src_of[new row] = old row), and the
// dense tiles, the per-row values and the sparse CSR are GATHERED through it into new buffers.  Stored bits are copied;
// nothing is re-quantised.  Everything here is out of place: no kernel writes a buffer the handle still serves from.
//
// Scans are three-phase (block sums, one block over the block sums, block-local scan + write), 1024 elements per block;
// inside a wave they are wave_scan_add.  A wave's 64 values sum below 2^32 (64 mask bits per word; a sparse row holds
// fewer than 2^24 entries), everything above a wave is 64-bit.
#pragma once
#include "common.h"

namespace hbmrag {

constexpr int kCompactBlock = 1024;  // elements (threads) per scan block

// Bits of mask word w that name rows below n.
__device__ inline unsigned long long compact_keep_word(const unsigned long long* __restrict__ mask, int64_t w, int64_t n) {
    unsigned long long m = mask[w];
    const int64_t left = n - w * 64;
    if (left < 64) m &= (1ull << left) - 1ull;
    return m;
}

// Exclusive prefix of v over the block's 1024 threads (every thread calls it); *block_total receives the block's sum.
__device__ inline unsigned long long compact_block_scan(unsigned v, unsigned long long* wave_tot /* LDS [16] */,
                                                        unsigned long long* block_total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned incl = wave_scan_add(v);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kCompactBlock / 64; ++w) {
        const unsigned long long t = wave_tot[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();  // wave_tot may be reused by the caller's next scan
    *block_total = total;
    return before + (incl - v);
}

// What the two scans sum: kept rows per mask word / entries per surviving sparse row.
struct KeepCount {
    const unsigned long long* mask;
    int64_t n_rows;
    __device__ unsigned operator()(int64_t w) const { return (unsigned)__popcll(compact_keep_word(mask, w, n_rows)); }
};
struct RowLength {
    const int64_t* indptr;
    const uint32_t* src_of;
    __device__ unsigned operator()(int64_t r) const {
        const int64_t s = src_of[r];
        return (unsigned)(indptr[s + 1] - indptr[s]);
    }
};

// Phase 1: block_sum[b] = sum of f over the block's elements.
template <typename F>
__global__ void __launch_bounds__(kCompactBlock) compact_block_sums_kernel(F f, int64_t n, unsigned long long* __restrict__ block_sum) {
    __shared__ unsigned long long wave_tot[kCompactBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const unsigned v = i < n ? f(i) : 0u;
    unsigned long long total;
    (void)compact_block_scan(v, wave_tot, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// Phase 2 (one block): block_sum[0 .. nb) -> its exclusive prefix, in place; *total = the sum of all.  Every thread sums
// a contiguous run of entries, thread 0 chains the 1024 run totals through LDS, every thread rewrites its run.
__global__ void __launch_bounds__(kCompactBlock) compact_scan_sums_kernel(unsigned long long* __restrict__ block_sum, int64_t nb,
                                                                         unsigned long long* __restrict__ total) {
    __shared__ unsigned long long run_tot[kCompactBlock];
    const int64_t per = (nb + kCompactBlock - 1) / kCompactBlock;
    const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (int64_t b = b0; b < b1; ++b) s += block_sum[b];
    run_tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int t = 0; t < kCompactBlock; ++t) {
            const unsigned long long x = run_tot[t];
            run_tot[t] = acc;
            acc += x;
        }
        *total = acc;
    }
    __syncthreads();
    unsigned long long acc = run_tot[threadIdx.x];
    for (int64_t b = b0; b < b1; ++b) {
        const unsigned long long x = block_sum[b];
        block_sum[b] = acc;
        acc += x;
    }
}

// Phase 3 of the row map: src_of[new row] = old row.  A block takes 1024 mask words; after the block-local scan every
// wave walks 64 of them, lane l owning bit l, so that the kept rows of a word are written side by side.
// n_kept bounds the writes (it is the scan's total).
__global__ void __launch_bounds__(kCompactBlock) compact_row_map_kernel(const unsigned long long* __restrict__ mask, int64_t n_rows,
                                                                       int64_t n_words, const unsigned long long* __restrict__ block_off,
                                                                       int64_t n_kept, uint32_t* __restrict__ src_of) {
    __shared__ unsigned long long wave_tot[kCompactBlock / 64];
    __shared__ unsigned long long word_base[kCompactBlock];
    const int64_t w_mine = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const unsigned v = w_mine < n_words ? (unsigned)__popcll(compact_keep_word(mask, w_mine, n_rows)) : 0u;
    unsigned long long total;
    word_base[threadIdx.x] = block_off[blockIdx.x] + compact_block_scan(v, wave_tot, &total);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < 64; ++i) {
        const int64_t w = (int64_t)blockIdx.x * kCompactBlock + wave * 64 + i;
        if (w >= n_words) break;  // wave-uniform
        const unsigned long long m = compact_keep_word(mask, w, n_rows);
        if ((m >> lane) & 1ull) {
            const int64_t dst = (int64_t)word_base[wave * 64 + i] + __popcll(m & ((1ull << lane) - 1ull));
            if (dst < n_kept) src_of[dst] = (uint32_t)(w * 64 + lane);
        }
    }
}

// Dense tiles, destination-driven: a wave owns one destination row block and walks its KT tiles (KT is a multiple of
// 4).  Lane l holds destination row rb*16 + (l & 15) and k-chunk kt*4 + (l >> 4): it reads its source row once, then
// per tile one 16-byte load from chunk_index(src, kchunk, KT) and one 16-byte store — the wave's stores are the
// destination tile's contiguous 1 KiB.  Four tiles' loads are issued before the first store, and a compute unit holds
// many such waves, which is what covers the HBM latency of the scattered reads.  The lanes of the ragged last row block
// store zeros.  The chunks are moved, never looked into: one kernel for both store types.
constexpr int kCompactWaves = 4;  // waves (row blocks) per block
__global__ void __launch_bounds__(kCompactWaves * 64) compact_tiles_kernel(const chunk_t* __restrict__ src_tiles,
                                                                          const uint32_t* __restrict__ src_of, int64_t n_kept,
                                                                          int KT, int64_t n_dst_blocks, chunk_t* __restrict__ dst_tiles) {
    const int lane = threadIdx.x & 63;
    const int64_t rb = (int64_t)blockIdx.x * kCompactWaves + (threadIdx.x >> 6);
    if (rb >= n_dst_blocks) return;  // wave-uniform
    const int64_t row = rb * kRowsPerBlock + (lane & 15);
    const bool live = row < n_kept;
    const int64_t src = live ? (int64_t)src_of[row] : 0;
    const int c = lane >> 4;
    // chunk_index(src, kt*4 + c, KT) = ((src >> 4) * KT + kt) * 64 + (src & 15) + 16 * c
    const chunk_t* sp = src_tiles + (src >> 4) * KT * kTileChunks + (src & 15) + 16 * c;
    chunk_t* dp = dst_tiles + rb * KT * kTileChunks + lane;
    const chunk_t zero = chunk_t{0u, 0u, 0u, 0u};
    for (int kt = 0; kt < KT; kt += 4) {
        chunk_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = live ? sp[(int64_t)(kt + u) * kTileChunks] : zero;
#pragma unroll
        for (int u = 0; u < 4; ++u) dp[(int64_t)(kt + u) * kTileChunks] = v[u];
    }
}

// Per-row values of the survivors: the fp32 per-row array (1/|x|, 1, or the L2 row term), norm2, and the maximum row norm
// in the representation row_norms_kernel leaves it in (uint bits of (float)sqrt(norm2), an order-independent atomicMax).
__global__ void compact_row_values_kernel(const float* __restrict__ scale, const double* __restrict__ norm2,
                                          const uint32_t* __restrict__ src_of, int64_t n_kept, float* __restrict__ new_scale,
                                          double* __restrict__ new_norm2, unsigned int* __restrict__ max_norm_bits) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float nrm = 0.f;
    if (r < n_kept) {
        const int64_t s = src_of[r];
        const double n2 = norm2[s];
        new_scale[r] = scale[s];
        new_norm2[r] = n2;
        nrm = (float)sqrt(n2);
    }
    nrm = wave_max_dpp(nrm);
    if ((threadIdx.x & 63) == 0) atomicMax(max_norm_bits, __float_as_uint(nrm));
}

// Phase 3 of the CSR scan: new_indptr[r] = entries of the survivors before r; new_indptr[n_kept] = all of them.
__global__ void __launch_bounds__(kCompactBlock) compact_indptr_kernel(RowLength len, int64_t n_kept,
                                                                      const unsigned long long* __restrict__ block_off,
                                                                      int64_t* __restrict__ new_indptr) {
    __shared__ unsigned long long wave_tot[kCompactBlock / 64];
    const int64_t r = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
    const unsigned v = r < n_kept ? len(r) : 0u;
    unsigned long long total;
    const unsigned long long before = block_off[blockIdx.x] + compact_block_scan(v, wave_tot, &total);
    if (r < n_kept) {
        new_indptr[r] = (int64_t)before;
        if (r == n_kept - 1) new_indptr[n_kept] = (int64_t)(before + v);
    }
}

// CSR entries: a wave per surviving row, lanes over its entries.  stats[0] = uint bits of max |value| copied, stats[1]
// != 0 when some copied value is negative (order-independent atomics, one per wave).
__global__ void compact_csr_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                   const uint32_t* __restrict__ src_of, int64_t n_kept, const int64_t* __restrict__ new_indptr,
                                   int32_t* __restrict__ new_idx, float* __restrict__ new_val, unsigned int* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= n_kept) return;  // wave-uniform
    const int64_t s = src_of[r];
    const int64_t e0 = indptr[s], len = indptr[s + 1] - e0, d0 = new_indptr[r];
    float mx = 0.f;
    unsigned neg = 0;
    for (int64_t e = lane; e < len; e += 64) {
        const float v = val[e0 + e];
        new_idx[d0 + e] = idx[e0 + e];
        new_val[d0 + e] = v;
        mx = fmaxf(mx, fabsf(v));
        neg |= v < 0.f;
    }
    mx = wave_max_dpp(mx);
    const bool any_neg = __ballot(neg != 0) != 0ull;
    if (lane == 0) {
        if (mx > 0.f) atomicMax(&stats[0], __float_as_uint(mx));
        if (any_neg) atomicOr(&stats[1], 1u);
    }
}

}  // namespace hbmrag
