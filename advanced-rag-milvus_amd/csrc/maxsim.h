// Late-interaction rerank (ColBERT-style MaxSim; Milvus 2.6 embedding lists with MAX_SIM): every entry of a ranked list is
// re-scored as  S = sum over query tokens t of  max over the row's stored tokens u of  <q_t, d_u>  and the list is
// re-sorted.  include/hbmrag.h holds the contract; advanced_rag/maxsim.py restates it on the host, bit for bit.
// The first-stage search (maxsim_scan_kernel, at the end of this file) scores every row of the store with the same
// arithmetic: the pieces both kernels need are device functions, written once.
//
// The similarity is DEFINED as the k-ascending fp32 fma chain.  v_mfma_f32_16x16x4_f32 is exactly that chain (one
// rounding per product, no wider accumulation), instruction i adding k = 4i .. 4i + 3 in ascending order, so the matrix
// core produces the canonical bits directly: a tile is 16 query tokens (A rows) x 16 document tokens (B columns), the
// fp16 operands widened in registers (exact), dim / 4 instructions per tile and accumulator.
#pragma once
#include "common.h"
#include "fuse.h"

namespace hbmrag {

constexpr int kMaxSimWaves = 4;        // 256 threads
constexpr int kMaxSimBatch = 16;       // candidates whose per-token maxima a wave collects before it sums them
constexpr int kMaxSimMStride = 65;     // floats per collected candidate: 64 tokens + 1, so that 16 lanes read 16 banks
constexpr int kMaxSimChunks = 8;       // 16-byte chunks of a 16-token tile per lane: 16 * (256 / 8) / 64

// Bytes of one LDS token row: the fp16 elements plus one 16-byte slot, so that the 16 rows a ds_read_b128 touches start
// in different slots of the 256-byte bank row (dim / 8 + 1 slots per row: odd whenever dim is a multiple of 16).
__host__ __device__ inline int maxsim_row_bytes(int dim) { return dim * 2 + 16; }

// Dynamic LDS of one block, in the order the kernel carves it.
__host__ __device__ inline size_t maxsim_lds_bytes(int tq_stride, int dim, int k_in) {
    const size_t rb = (size_t)maxsim_row_bytes(dim), q_rows = (size_t)((tq_stride + 15) & ~15);
    return q_rows * rb                                      // query tokens, rows padded to whole 16-token tiles
           + (size_t)kMaxSimWaves * 16 * rb                 // one document tile per wave
           + (size_t)k_in * 8 + (size_t)k_in * 8            // S per entry (fp64), first token of the entry's row (int64)
           + (size_t)kMaxSimWaves * kMaxSimBatch * kMaxSimMStride * 4   // collected maxima
           + (size_t)k_in * 4                               // tokens of the entry's row
           + (size_t)kMaxSimWaves * kMaxSimBatch * 4 + 16;  // the entries the collected maxima belong to; the prefix length
}

// Element 4 * hi + g (hi compile-time, g = lane >> 4) of the 8 fp16 values of one 16-byte chunk, widened exactly.
template <int HI>
__device__ __forceinline__ float maxsim_pick(const chunk_t& v, int g) {
    const unsigned w = (g >> 1) ? (HI ? v.w : v.y) : (HI ? v.z : v.x);
    const unsigned short b = (unsigned short)(w >> ((g & 1) * 16));
    return (float)__builtin_bit_cast(_Float16, b);
}

// Orders one wave's LDS writes before its later reads (and the reverse): the document tile and the collected maxima are
// private to a wave, so no block barrier is needed inside the candidate loop, whose trip count differs between waves.
__device__ __forceinline__ void maxsim_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- what the rerank and the scan share: one arithmetic, written once ------------------------------------------------------
// The query's tokens into LDS: rows [0, Tq) from the operand, zeros up to the tile edge (all 256 threads).
__device__ __forceinline__ void maxsim_load_query(unsigned char* s_q, const chunk_t* __restrict__ qtok, int q, int tq_stride,
                                                  int Tq, int nT, int cpr, int rb, int tid) {
    for (int c = tid; c < nT * 16 * cpr; c += 256) {
        const int row = c / cpr, cc = c - row * cpr;
        chunk_t v = {0u, 0u, 0u, 0u};
        if (row < Tq) v = qtok[((int64_t)q * tq_stride + row) * cpr + cc];
        *(chunk_t*)(s_q + (size_t)row * rb + cc * 16) = v;
    }
}

// Where lane's chunk i of a 16-token tile goes in the wave's LDS tile.
__device__ __forceinline__ void maxsim_tile_offsets(int (&loff)[kMaxSimChunks], int cpr, int rb, int lane) {
#pragma unroll
    for (int i = 0; i < kMaxSimChunks; ++i) {
        const int c = lane + 64 * i, row = c / cpr;
        loff[i] = row * rb + (c - row * cpr) * 16;
    }
}

// Tokens [u, u + 16) of a row that starts at token `beg` and has T tokens: the valid ones from the store, zeros for the
// rows the tile does not have.  Registers only: the loads are in flight while the previous tile is multiplied.
__device__ __forceinline__ void maxsim_fetch_tile(chunk_t (&pf)[kMaxSimChunks], const chunk_t* __restrict__ tok, int64_t beg,
                                                  int T, int u, int cpr, int lane) {
    const chunk_t* src = tok + (beg + u) * cpr;
    const int left = T - u, lim = (left < 16 ? left : 16) * cpr;
#pragma unroll
    for (int i = 0; i < kMaxSimChunks; ++i) {
        const int x = lane + 64 * i;
        chunk_t v = {0u, 0u, 0u, 0u};
        if (x < lim) v = src[x];
        pf[i] = v;
    }
}

__device__ __forceinline__ void maxsim_store_tile(unsigned char* s_doc, const int (&loff)[kMaxSimChunks],
                                                  const chunk_t (&pf)[kMaxSimChunks], int tile_chunks, int lane) {
#pragma unroll
    for (int i = 0; i < kMaxSimChunks; ++i)
        if (lane + 64 * i < tile_chunks) *(chunk_t*)(s_doc + loff[i]) = pf[i];
}

// a[rt] = the 16 x 16 similarities of query tile rt (rt < nT) and the wave's document tile: the canonical chain.  Returned
// by value: with the accumulators passed by reference maxsim_rerank_kernel allocates 132 registers instead of 128 and
// loses a wave of occupancy (make asm).
struct MaxSimTile { f32x4_t a[4]; };
__device__ __forceinline__ MaxSimTile maxsim_tile_product(const unsigned char* s_q, const unsigned char* s_doc, int nT, int cpr,
                                                          int rb, int g, int col) {
    MaxSimTile tile;
    f32x4_t (&acc)[4] = tile.a;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const unsigned char* dp = s_doc + col * rb;
    const unsigned char* qp = s_q + col * rb;
    for (int j = 0; j < cpr; ++j) {
        const chunk_t dv = *(const chunk_t*)(dp + j * 16);
        const float b0 = maxsim_pick<0>(dv, g), b1 = maxsim_pick<1>(dv, g);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (rt < nT) {
                const chunk_t qv = *(const chunk_t*)(qp + (size_t)rt * 16 * rb + j * 16);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(maxsim_pick<0>(qv, g), b0, acc[rt], 0, 0, 0);   // k = 8j + g
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(maxsim_pick<1>(qv, g), b1, acc[rt], 0, 0, 0);   // k = 8j + 4 + g
            }
        }
    }
    return tile;
}

// m = max(m, acc) for the columns this tile has (`have`); `first`: the row's first tile starts the maximum at -inf.
__device__ __forceinline__ void maxsim_fold_tile(f32x4_t (&m)[4], const f32x4_t (&acc)[4], bool first, bool have) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float old = first ? -INFINITY : m[rt][r];
            m[rt][r] = have ? fmaxf(old, acc[rt][r]) : old;
        }
}

// The row's last tile is folded: the maximum over the 16 columns, m_t for t = 16 rt + 4 g + reg, into dst[t].
__device__ __forceinline__ void maxsim_column_max(const f32x4_t (&m)[4], int nT, float* dst, int g, int col) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        if (rt < nT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = m[rt][r];
                for (int d = 1; d < 16; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
                if (col == 0) dst[rt * 16 + g * 4 + r] = v;
            }
        }
    }
}

// S = 0.0; S += (double)m_t, t ascending: one rounded fp64 add each.
__device__ __forceinline__ double maxsim_sum_tokens(const float* m, int Tq) {
    double S = 0.0;
    for (int t = 0; t < Tq; ++t) S = __dadd_rn(S, (double)m[t]);
    return S;
}

// One block (256 threads, four waves) per query.
//   n       = the valid prefix, as decay_rerank_kernel finds it
//   Tq      = qn[q] clamped into [0, tq_stride]; the query's tokens sit in LDS once, zero rows up to a whole tile
//   entry i = row ids[i] - first_row; outside [0, tok_rows), or a row without tokens: S = 0.0.  The CSR bounds are
//             clamped into [0, indptr[tok_rows]] so that no operand on the device can send a load out of the token store.
//   waves take the non-empty entries in turn (entry = wave, wave + 4, ...).  A 16-token tile of the row is one contiguous
//   piece of the store: it is fetched with 16-byte loads into registers WHILE the previous tile is multiplied, then
//   written to the wave's LDS tile and read back as the strided view the instruction needs (lane group g = lane >> 4
//   supplies k = 4i + g at instruction i: elements g and 4 + g of every 8-element chunk).
//   m[rt][reg] = running maximum of D[t = 16 rt + 4 g + reg][u = lane & 15] over the row's tiles; the columns a short
//   last tile does not have never enter it.  At the row's end the maximum over the 16 columns is taken across lanes.
//   S       = fp64 sum of the maxima in ascending t, by one lane per entry, sixteen entries at a time
//   order   = stable descending sort of S by counting, as decay_rerank_kernel does
__global__ __launch_bounds__(256) void maxsim_rerank_kernel(
    const int64_t* __restrict__ ids, const int32_t* __restrict__ n_valid, int k_in, const chunk_t* __restrict__ qtok,
    const int32_t* __restrict__ qn, int tq_stride, int dim, const int64_t* __restrict__ indptr,
    const chunk_t* __restrict__ tok, int64_t tok_rows, int64_t first_row, int k_out, int32_t* __restrict__ out_pos,
    int64_t* __restrict__ out_ids, double* __restrict__ out_scores, int32_t* __restrict__ out_n) {
    extern __shared__ __align__(16) unsigned char ms_lds[];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, col = lane & 15;
    const int rb = maxsim_row_bytes(dim), cpr = dim >> 3, q_rows = (tq_stride + 15) & ~15;
    unsigned char* s_q = ms_lds;
    unsigned char* s_doc = s_q + (size_t)q_rows * rb + (size_t)wave * 16 * rb;
    double* s_fin = (double*)(s_q + (size_t)q_rows * rb + (size_t)kMaxSimWaves * 16 * rb);
    int64_t* s_beg = (int64_t*)(s_fin + k_in);
    float* s_m = (float*)(s_beg + k_in) + wave * kMaxSimBatch * kMaxSimMStride;
    int* s_T = (int*)((float*)(s_beg + k_in) + kMaxSimWaves * kMaxSimBatch * kMaxSimMStride);
    int* s_cid = s_T + k_in + wave * kMaxSimBatch;
    int* s_n = s_T + k_in + kMaxSimWaves * kMaxSimBatch;
    const int64_t* my_ids = ids + (int64_t)q * k_in;

    if (tid == 0) {
        int n = k_in;
        if (n_valid) {
            n = n_valid[q];
            n = n < 0 ? 0 : (n > k_in ? k_in : n);
        }
        *s_n = n;
    }
    __syncthreads();
    if (!n_valid) {   // the list ends at its first negative id
        int end = k_in;
        for (int i = tid; i < k_in; i += 256)
            if (my_ids[i] < 0) { end = i; break; }   // positions ascend per thread
        if (end < k_in) atomicMin(s_n, end);
        __syncthreads();
    }
    const int n = *s_n;
    int Tq = qn[q];
    Tq = Tq < 0 ? 0 : (Tq > tq_stride ? tq_stride : Tq);
    const int nT = (Tq + 15) >> 4;

    maxsim_load_query(s_q, qtok, q, tq_stride, Tq, nT, cpr, rb, tid);
    const int64_t total = tok_rows > 0 ? indptr[tok_rows] : 0;
    for (int i = tid; i < n; i += 256) {
        const int64_t id = my_ids[i];
        const int64_t r = id - first_row;
        int64_t b = 0, e = 0;
        if (id >= first_row && r < tok_rows) {   // (id >= first_row first: r cannot have wrapped when it is read)
            b = indptr[r];
            e = indptr[r + 1];
            b = b < 0 ? 0 : (b > total ? total : b);
            e = e < b ? b : (e > total ? total : e);
        }
        const int64_t T = e - b;
        s_beg[i] = b;
        s_T[i] = T > (int64_t)0x40000000 ? 0x40000000 : (int)T;
        s_fin[i] = 0.0;
    }
    __syncthreads();

    if (nT > 0) {   // block-uniform
        int loff[kMaxSimChunks];
        maxsim_tile_offsets(loff, cpr, rb, lane);
        const int tile_chunks = 16 * cpr;
        chunk_t pf[kMaxSimChunks];
        auto next_entry = [&](int c) {
            while (c < n && s_T[c] == 0) c += kMaxSimWaves;
            return c;
        };
        auto fetch = [&](int c, int u) { maxsim_fetch_tile(pf, tok, s_beg[c], s_T[c], u, cpr, lane); };
        auto flush = [&](int cnt) {   // lane l sums entry l of the collected batch
            maxsim_wave_sync();
            if (lane < cnt) s_fin[s_cid[lane]] = maxsim_sum_tokens(s_m + lane * kMaxSimMStride, Tq);
            maxsim_wave_sync();
        };

        int ci = next_entry(wave), u0 = 0, slot = 0;
        if (ci < n) fetch(ci, 0);
        f32x4_t m[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) m[rt] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        while (ci < n) {   // wave-uniform
            const int T = s_T[ci];
            maxsim_store_tile(s_doc, loff, pf, tile_chunks, lane);
            maxsim_wave_sync();
            int nci = ci, nu0 = u0 + 16;
            if (nu0 >= T) {
                nci = next_entry(ci + kMaxSimWaves);
                nu0 = 0;
            }
            if (nci < n) fetch(nci, nu0);   // in flight while this tile is multiplied

            const MaxSimTile tile = maxsim_tile_product(s_q, s_doc, nT, cpr, rb, g, col);
            maxsim_fold_tile(m, tile.a, u0 == 0, u0 + col < T);   // a column the last tile does not have loses every maximum
            if (u0 + 16 >= T) {   // the row's last tile: the maximum over the 16 columns, then collect
                maxsim_column_max(m, nT, s_m + slot * kMaxSimMStride, g, col);
                if (lane == 0) s_cid[slot] = ci;
                if (++slot == kMaxSimBatch) {
                    flush(slot);
                    slot = 0;
                }
            }
            maxsim_wave_sync();   // every lane has read the tile before the next one is written
            ci = nci;
            u0 = nu0;
        }
        if (slot) flush(slot);
    }
    __syncthreads();

    for (int e = tid; e < n; e += 256) {
        const double v = s_fin[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (s_fin[j] > v) || (s_fin[j] == v && j < e);
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

// ---- first-stage search: every row of the store instead of a list of ids (hr_maxsim_scan_dev) --------------------------------
constexpr int kMaxSimScanLanes = 64;   // rows of one wave's piece of a range at most: a lane per row

// Dynamic LDS of one scan block, in the order the kernel carves it.
__host__ __device__ inline size_t maxsim_scan_lds_bytes(int tq_stride, int dim) {
    const size_t rb = (size_t)maxsim_row_bytes(dim), q_rows = (size_t)((tq_stride + 15) & ~15);
    return q_rows * rb                                                  // query tokens, rows padded to whole 16-token tiles
           + (size_t)kMaxSimWaves * 16 * rb                             // one document tile per wave
           + (size_t)kMaxSimWaves * kMaxSimBatch * kMaxSimMStride * 4   // collected maxima
           + (size_t)kMaxSimWaves * kMaxSimBatch * 4;                   // the lanes (rows of the piece) they belong to
}

// Grid (blocks per query, queries), 256 threads.  Query blockIdx.y's tokens sit in LDS for the block's whole life.  The
// rows are cut into ranges of 4 * rpw consecutive rows (rpw <= 64); block x walks ranges x, x + gridDim.x, ... and wave w
// of it takes rows [range * 4 rpw + w * rpw, + rpw) of each: a lane per row reads the mask bit and the clamped CSR bounds,
// writes the (0.0f, -1) cell of a row that is no hit at once, and the wave then walks the remaining rows in ascending
// order with the rerank's loop: "the next entry" is the next set bit of the ballot.  The rows of a piece are consecutive in
// the token store, so a wave's tiles are one forward stream; a masked-out or empty row costs its 17 bytes of mask and CSR.
// The score is written by the lane that sums it (sixteen rows at a time), rounded once: (float)S.  No block barrier
// after the query load; no atomic anywhere.
__global__ __launch_bounds__(256) void maxsim_scan_kernel(
    const chunk_t* __restrict__ qtok, const int32_t* __restrict__ qn, int tq_stride, int dim,
    const int64_t* __restrict__ indptr, const chunk_t* __restrict__ tok, int64_t tok_rows, int64_t n_rows,
    const uint8_t* __restrict__ rowmask, int rpw, float* __restrict__ scores, int32_t* __restrict__ rows) {
    extern __shared__ __align__(16) unsigned char ms_lds[];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, col = lane & 15;
    const int rb = maxsim_row_bytes(dim), cpr = dim >> 3, q_rows = (tq_stride + 15) & ~15;
    unsigned char* s_q = ms_lds;
    unsigned char* s_doc = s_q + (size_t)q_rows * rb + (size_t)wave * 16 * rb;
    float* s_m = (float*)(s_q + (size_t)q_rows * rb + (size_t)kMaxSimWaves * 16 * rb) + wave * kMaxSimBatch * kMaxSimMStride;
    int* s_cid = (int*)((float*)(s_q + (size_t)q_rows * rb + (size_t)kMaxSimWaves * 16 * rb) +
                        kMaxSimWaves * kMaxSimBatch * kMaxSimMStride) + wave * kMaxSimBatch;
    int Tq = qn[q];
    Tq = Tq < 0 ? 0 : (Tq > tq_stride ? tq_stride : Tq);
    const int nT = (Tq + 15) >> 4;
    maxsim_load_query(s_q, qtok, q, tq_stride, Tq, nT, cpr, rb, tid);
    __syncthreads();

    const int64_t total = tok_rows > 0 ? indptr[tok_rows] : 0;
    float* my_scores = scores + (int64_t)q * n_rows;
    int32_t* my_rows = rows + (int64_t)q * n_rows;
    int loff[kMaxSimChunks];
    maxsim_tile_offsets(loff, cpr, rb, lane);
    const int tile_chunks = 16 * cpr;
    const int64_t range_rows = (int64_t)kMaxSimWaves * rpw, n_ranges = (n_rows + range_rows - 1) / range_rows;
    chunk_t pf[kMaxSimChunks];
    f32x4_t m[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) m[rt] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};

    for (int64_t range = blockIdx.x; range < n_ranges; range += gridDim.x) {
        const int64_t base = range * range_rows + (int64_t)wave * rpw, i = base + lane;
        const bool mine = lane < rpw && i < n_rows;
        int64_t beg = 0;
        int T = 0;
        if (mine && i < tok_rows && (!rowmask || ((rowmask[i >> 3] >> (i & 7)) & 1))) {
            int64_t b = indptr[i], e = indptr[i + 1];
            b = b < 0 ? 0 : (b > total ? total : b);
            e = e < b ? b : (e > total ? total : e);
            beg = b;
            T = e - b > (int64_t)0x40000000 ? 0x40000000 : (int)(e - b);
        }
        const bool hit = T > 0;
        if (mine && !(hit && nT > 0)) {   // no hit, or a query without tokens: nothing to multiply
            my_scores[i] = 0.f;
            my_rows[i] = hit ? (int32_t)i : -1;
        }
        unsigned long long todo = nT > 0 ? __ballot(hit) : 0ull;   // wave-uniform
        if (!todo) continue;
        auto flush = [&](int cnt) {   // lane l sums row l of the collected batch and writes its cell
            maxsim_wave_sync();
            if (lane < cnt) {
                const int64_t r = base + s_cid[lane];
                my_scores[r] = (float)maxsim_sum_tokens(s_m + lane * kMaxSimMStride, Tq);
                my_rows[r] = (int32_t)r;
            }
            maxsim_wave_sync();
        };
        int cur = __builtin_ctzll(todo), u0 = 0, slot = 0;
        int cT = __shfl(T, cur);
        maxsim_fetch_tile(pf, tok, __shfl(beg, cur), cT, 0, cpr, lane);
        while (todo) {   // wave-uniform
            maxsim_store_tile(s_doc, loff, pf, tile_chunks, lane);
            maxsim_wave_sync();
            const bool last = u0 + 16 >= cT;
            const unsigned long long rest = last ? todo & (todo - 1) : todo;
            const int ncur = rest ? __builtin_ctzll(rest) : cur, nu0 = last ? 0 : u0 + 16;
            const int64_t nbeg = __shfl(beg, ncur);
            const int nTr = __shfl(T, ncur);
            if (rest) maxsim_fetch_tile(pf, tok, nbeg, nTr, nu0, cpr, lane);   // in flight while this tile is multiplied

            const MaxSimTile tile = maxsim_tile_product(s_q, s_doc, nT, cpr, rb, g, col);
            maxsim_fold_tile(m, tile.a, u0 == 0, u0 + col < cT);
            if (last) {
                maxsim_column_max(m, nT, s_m + slot * kMaxSimMStride, g, col);
                if (lane == 0) s_cid[slot] = cur;
                if (++slot == kMaxSimBatch) {
                    flush(slot);
                    slot = 0;
                }
            }
            maxsim_wave_sync();   // every lane has read the tile before the next one is written
            todo = rest;
            cur = ncur;
            cT = nTr;
            u0 = nu0;
        }
        if (slot) flush(slot);
    }
}

}  // namespace hbmrag
