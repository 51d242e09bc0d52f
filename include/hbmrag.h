/*
 * hbmrag.h — C ABI of libhbmrag.so: the MI355X (gfx950) in-HBM shard store and
 * hybrid-search kernels that replace the Milvus server behind
 * advanced-rag-milvus's search hot path.
 *
 * The reference has no FFI of its own: its boundary is the duck-typed
 * index-manager protocol that HybridRetriever consumes
 * (reference src/advanced_rag/retrieval.py:341-419, :634-648) and that
 * MilvusIndexManager implements by RPC to a Milvus server
 * (reference src/advanced_rag/indexing.py:264-437 index_chunks,
 * :439-551 search).  Every entry point below names the reference call it
 * stands in for.  The Python host package (advanced-rag-milvus_amd/advanced_rag)
 * binds these with ctypes; INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this line;
 *   - every function returns an hr_status (0 = ok) and never throws or aborts;
 *     hr_last_error() gives the message for the last failure on that handle
 *     (or, with NULL, the last failure of a call that had no handle);
 *   - the caller owns every host buffer it passes in; the library owns all
 *     device memory it allocates; `*_dev` entry points take DEVICE pointers
 *     owned by the caller (e.g. torch tensors) and are asynchronous on the
 *     given hipStream_t (passed as void*);
 *   - results are written into caller-allocated arrays of size B*k, padded
 *     with id -1 / score 0 when fewer than k rows qualify;
 *   - row ids are int64 "global row numbers": local row + the shard's row
 *     offset (hr_set_row_offset), so per-shard lists can be merged across GPUs;
 *   - search calls are thread-safe against each other: a host-form call takes a
 *     private workspace + stream from a pool; `*_dev` calls on the same stream
 *     share one workspace and are serialised while they enqueue (their kernels
 *     then run in stream order); add/finalize take an exclusive lock.
 *
 * Result semantics (what the oracle in oracle/ restates bit-for-bit)
 *   dense  : score32 = (float) S, S computed in fp64 by a k-ordered sequential
 *            sum of exact products x[k]*q[k];  COSINE divides by
 *            sqrt(sum x^2 * sum q^2) (0 when either norm is 0).  Rows are
 *            ranked by (score32 desc, row id asc).  Milvus' HNSW(ef=64) is
 *            approximate; this is the exact FLAT answer of the same metric.
 *   dense, HR_METRIC_L2 : score32 = (float) D, D = k-ordered sequential fp64 sum of
 *            d_k * d_k with d_k = (double)x[k] - (double)q[k], every subtraction,
 *            product and sum a separately rounded IEEE fp64 operation (no FMA),
 *            k = 0 .. dim-1: Milvus' L2 "distance", squared, no root.  Rows are
 *            ranked by (score32 ASCENDING, row id asc); lists are written smallest
 *            distance first, padded with id -1 / score 0.  A row equal to the query
 *            is a valid hit at distance exactly +0.  A zero query is legal
 *            (D = |x|^2).  Row norms must stay inside the fp32 range squared
 *            (|x|^2 / 2 is kept per row as a float).
 *   dense, range search (hr_search_dense_range*): the best k rows among the rows whose
 *            canonical score lies in the range; ranking, padding and scores are those of
 *            the plain search.  The test is made on the fp32 score the list carries,
 *            widened to double and compared with the bounds as doubles (Milvus' rules):
 *              COSINE, IP : radius < (double)score32 <= range_filter
 *              L2         : range_filter <= (double)D32 < radius
 *            so a row equal to the query is a hit at range_filter = 0.  Either bound may
 *            be absent: an absent radius is -inf (COSINE, IP) / +inf (L2), an absent
 *            range_filter the opposite.  Both absent: the plain search bit for bit, ids,
 *            scores and flags.  Fewer than k rows in range: the list is shorter and padded
 *            as usual.  No row in range: all padding, and proven.  Bounds are per query.
 *            A NaN bound and an empty interval (radius >= range_filter; L2: range_filter
 *            >= radius) are refused with HR_EINVAL naming the query, nothing is launched.
 *   sparse : score32 = (float) sum over the row's stored entries, in stored
 *            (index) order, of value*query_value in fp64; only rows with
 *            score32 > 0 qualify; same ranking rule.
 *   fuse   : reciprocal-rank fusion exactly as reference
 *            retrieval.py:421-491 (float64, k=60 by default, stable order).
 */
#ifndef HBMRAG_H
#define HBMRAG_H

#include <stdint.h>
#include <stddef.h>

#if defined(HR_BUILD)
#define HR_API __attribute__((visibility("default")))
#else
#define HR_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hr_index hr_index; /* opaque shard handle (one per GPU / process) */

typedef enum hr_status {
    HR_OK = 0,
    HR_EINVAL = 1, /* bad argument / shape; Python maps to ValueError            */
    HR_ESTATE = 2, /* call not valid in this state (e.g. search before finalize) */
    HR_EHIP = 3,   /* HIP runtime failure (message holds hipGetErrorString)      */
    HR_ENOMEM = 4, /* host or device allocation failed                           */
    HR_ELIMIT = 5  /* argument exceeds a compiled-in limit (see HR_MAX_*)        */
} hr_status;

enum { HR_F32 = 0, HR_F16 = 1 };               /* storage dtype of the dense shard */
enum { HR_METRIC_IP = 0, HR_METRIC_COSINE = 1, HR_METRIC_L2 = 2 }; /* dense metric_type (Milvus: IP, COSINE, L2) */
enum { HR_METHOD_SEMANTIC = 1, HR_METHOD_SPARSE = 2, HR_METHOD_DOMAIN = 4 };

#define HR_MAX_TOPK 256  /* reference clamps top_k to 100 and over-retrieves 2x (constants.py:47, retrieval.py:351) */
#define HR_MAX_DIM 4096  /* dense dimension limit; fp32 rows longer than 2496 (and fp16 ones longer than 4992, beyond
                          this limit) leave no room for the LDS-resident query tile, and every batch of such a shard
                          takes the k-chunked pass */
#define HR_MAX_QUERY_NNZ 4096

/* ---- lifecycle -------------------------------------------------------------
 * Replaces MilvusIndexManager._connect/_initialize_collections/_create_collection
 * (reference indexing.py:134-262): one handle holds the "semantic_index"
 * (dense) and "sparse_index" collections of one shard on one GPU.
 * dim = 0 or sparse_dim = 0 disables that collection. */
HR_API int hr_create(int device, int64_t dim, int dtype, int metric, int64_t sparse_dim, hr_index** out);
HR_API void hr_destroy(hr_index* h);
HR_API const char* hr_last_error(const hr_index* h);
/* Library/ABI version: major*10000 + minor*100 + patch. */
HR_API int hr_version(void);

/* Global id of local row 0 (multi-GPU row sharding; default 0). */
HR_API int hr_set_row_offset(hr_index* h, int64_t first_row);
/* Optional: pre-size the dense store so appends never reallocate. */
HR_API int hr_reserve(hr_index* h, int64_t n_rows);

/* ---- ingest ----------------------------------------------------------------
 * Replaces Collection.insert on semantic_index / sparse_index
 * (reference indexing.py:370-427).  Rows are appended; row numbers are
 * assigned in call order.  hr_add_dense takes row-major fp32 rows and stores
 * them in the shard's dtype (fp16: round-to-nearest-even, as numpy astype).
 * hr_add_dense_raw takes rows already in the shard's dtype (fp16 bits as
 * uint16).  The `_dev` forms take device pointers.
 * Every element must be finite AS STORED: a batch that holds a NaN or an
 * infinity, or on an fp16 shard an fp32 value that rounds to one (|x| >= 65520),
 * is refused with HR_EINVAL by all three forms (Milvus rejects such vectors at
 * insert).  hr_last_error names the lowest offending row as an index into the
 * call's batch.  The check runs on the device beside the conversion.  A refused
 * call appends nothing: hr_num_rows, the finalized state, the row norms and the
 * bounds of the exactness proofs derived from them are what they were. */
HR_API int hr_add_dense(hr_index* h, const float* rows, int64_t n);
HR_API int hr_add_dense_raw(hr_index* h, const void* rows, int64_t n);
HR_API int hr_add_dense_raw_dev(hr_index* h, const void* d_rows, int64_t n, void* stream);
/* CSR batch: indptr[n+1], indices sorted ascending within a row, < sparse_dim
 * (the {"indices","values"} payload of reference indexing.py:647-654, batched
 * the way indexing.py:379-404 builds its scipy CSR). */
HR_API int hr_add_sparse(hr_index* h, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n);
/* Replaces Collection.flush/load (reference indexing.py:430-431, :259):
 * computes row norms, builds the doc-range-partitioned postings, sizes the
 * search workspaces.  May be called again after further adds. */
HR_API int hr_finalize(hr_index* h);

/* Remove rows for good (Milvus compacts its segments after Collection.delete, reference indexing.py:692-696, and
 * offers Collection.compact()).  keep: 1 bit per LOCAL row (bit r%8 of byte r/8, the rowmask convention), 1 = the row stays.
 * on_device = 0: host buffer of ceil(n/8) bytes; 1: device buffer of 8*ceil(n/64) bytes (what hr_filter_eval_dev
 * writes), n = max(hr_num_rows, hr_num_sparse_rows).  Surviving rows keep their order; new local row = number of
 * kept rows before it.  The dense and the sparse collection of the handle are compacted with the same mask (each
 * over the rows it has).  *kept_dense / *kept_sparse (may be NULL) receive the new row counts.
 *   Result: afterwards the handle cannot be told apart from one built from the surviving rows alone — the same create
 *     arguments and hr_set_row_offset, hr_add_dense_raw / hr_add_sparse of the survivors in order, hr_finalize: identical
 *     search results and exactness flags through every entry point and a byte-identical hr_save file (tiles, the per-row
 *     fp32 array, norm2, the CSR, and the header's max_row_norm, max_sparse_abs, n_rows, n_sparse, nnz); the "some weight
 *     is negative" state and the postings' dense-run bookkeeping are recomputed from the survivors.  Stored bits are
 *     gathered; no row is re-quantised.
 *   Capacity: the dense store gets what hr_reserve gives an empty handle for that many rows, the CSR buffers hold
 *     exactly the surviving rows, the postings are rebuilt from the first range; hr_device_bytes drops accordingly and
 *     later appends grow by the usual rule.
 *   All-or-nothing: the operation is OUT OF PLACE — every new buffer is allocated and filled beside the old store, so
 *     the old and the new store are in HBM at once — and only then moved into the handle.  A failure before that
 *     (HR_ENOMEM when the new store does not fit beside the old one) leaves the handle exactly as it was.  If only the
 *     posting rebuild fails after that, the handle is in the state a failed hr_finalize leaves (CSR complete, not
 *     finalized) and the next hr_finalize completes it.
 *   Exclusive like hr_finalize, and it waits for the device first: `*_dev` searches enqueued earlier finish on the old
 *     store.  The caller issues no search while it runs and forgets every row number and row mask it holds.
 *   HR_ESTATE on a handle that is not finalized (pending rows must be flushed first); HR_EINVAL for a NULL handle or
 *     mask.  A mask that keeps every row returns HR_OK and changes nothing, capacity included.  A mask that keeps no row
 *     leaves a finalized empty handle that answers searches with padded lists and accepts appends. */
HR_API int hr_compact(hr_index* h, const uint8_t* keep, int on_device, int64_t* kept_dense, int64_t* kept_sparse);

/* Shard snapshot (checkpoint / resume; the reference relies on Milvus'
 * persistence, indexing.py:185-188, :430-431).  One file: header (with the file's
 * total size), dense tiles + norms exactly as they sit in HBM, and the sparse CSR
 * (read back from the device); the range-major postings are rebuilt on load.
 * hr_save writes `path`.tmp and renames it over `path` once complete.  hr_load
 * does not trust the file: sizes are checked against the header and the CSR goes
 * through hr_add_sparse's checks; it creates a finalized handle on `device`. */
HR_API int hr_save(hr_index* h, const char* path);
HR_API int hr_load(const char* path, int device, hr_index** out);
/* What a handle (e.g. one returned by hr_load) holds: dimension, storage dtype, metric, sparse dimension.
 * Any out pointer may be NULL. */
HR_API int hr_get_info(const hr_index* h, int64_t* dim, int32_t* dtype, int32_t* metric, int64_t* sparse_dim);

HR_API int64_t hr_num_rows(const hr_index* h);        /* dense rows (Collection.num_entities, indexing.py:687) */
HR_API int64_t hr_num_sparse_rows(const hr_index* h);
HR_API int64_t hr_device_bytes(const hr_index* h);    /* HBM held by the shard */

/* ---- search (host buffers, synchronous) --------------------------------------
 * Replace Collection.search on "semantic_index" / "sparse_index"
 * (reference indexing.py:503-525) for a batch of B queries.
 * Query values must be finite: the host forms (the _dmask forms included) refuse a NaN or an infinity with HR_EINVAL.
 *   q        [B*dim] fp32 query vectors
 *   rowmask  optional bitmask over local rows, 1 bit per row (bit r%8 of byte
 *            r/8), 1 = row passes the filter expression; NULL = all rows
 *   out_ids  [B*k] int64, out_scores [B*k] fp32, best first. */
HR_API int hr_search_dense(hr_index* h, const float* q, int B, int k, const uint8_t* rowmask,
                    int64_t* out_ids, float* out_scores);
/* Range search (Collection.search with params {"radius": r, "range_filter": f}; semantics above).  radius and
 * range_filter are HOST arrays of B doubles, NULL = that side unbounded for every query (+-inf in an entry = unbounded
 * for that query).  rowmask as in hr_search_dense, or with mask_on_device != 0 a device pointer as in
 * hr_search_dense_dmask.  Escalates by itself like hr_search_dense: the lists are exact whatever the bounds.  A refused
 * call (NaN, empty interval) launches nothing and leaves the output buffers untouched. */
HR_API int hr_search_dense_range(hr_index* h, const float* q, int B, int k, const uint8_t* rowmask, int mask_on_device,
                                 const double* radius, const double* range_filter, int64_t* out_ids, float* out_scores);
/* Sparse queries as CSR (q_indptr[B+1]); drop_ratio = Milvus
 * drop_ratio_search (reference retrieval.py:97-101): the
 * floor(drop_ratio*nnz) smallest-|value| entries of each query are ignored. */
HR_API int hr_search_sparse(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val,
                     int B, int k, float drop_ratio, const uint8_t* rowmask,
                     int64_t* out_ids, float* out_scores);

/* The same two searches with the row mask already in HBM (hr_filter_eval_dev's output, or a caller's cached mask):
 * host buffers in and out, escalation included, no mask upload. */
HR_API int hr_search_dense_dmask(hr_index* h, const float* q, int B, int k, const uint8_t* d_rowmask,
                          int64_t* out_ids, float* out_scores);
HR_API int hr_search_sparse_dmask(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val,
                           int B, int k, float drop_ratio, const uint8_t* d_rowmask,
                           int64_t* out_ids, float* out_scores);

/* ---- deep search: top_k + offset up to HR_MAX_DEEP_K rows per query, exact ---------------------------------------
 * R = the collection's ranking of one query: the rows that pass the mask (sparse: with a positive score), by canonical
 * score descending (L2: distance ascending), then row ascending.  The deep list is R[offset : offset + k]: global ids
 * and canonical fp32 scores, padded with -1 / 0 when R is shorter.  1 <= k, 0 <= offset (HR_EINVAL otherwise),
 * W = offset + k <= HR_MAX_DEEP_K (HR_ELIMIT beyond).  With offset = 0 the first HR_MAX_TOPK entries are, bit for
 * bit, the list hr_search_dense / hr_search_sparse return.
 *   How: no scan and no proof.  Every row of the shard is refined in the canonical fp64 arithmetic (the last rung of
 *     the host forms' escalation ladder) and a grid-wide radix select + one LDS sort per query take the window, so the
 *     list is exact by construction and a call costs a full read of the shard per query whatever W is.
 *   Host arrays in and out, synchronous.  rowmask / mask_on_device as in hr_search_dense_range; the finite-value checks
 *     (and drop_ratio) are those of hr_search_dense / hr_search_sparse.
 *   Memory: the candidate arrays (8 bytes per row and query, + 4 bytes per candidate group) belong to the call and are
 *     freed before it returns; queries run in passes that keep them under 512 MiB.  When one query's arrays cannot be
 *     allocated the call fails with HR_ENOMEM, writes nothing and leaves the handle as it was.  hr_device_bytes is
 *     unchanged by a call. */
#define HR_MAX_DEEP_K 16384  /* Milvus' cap on offset + limit */
HR_API int hr_search_dense_deep(hr_index* h, const float* q, int B, int k, int offset, const uint8_t* rowmask,
                                int mask_on_device, int64_t* out_ids, float* out_scores);
HR_API int hr_search_sparse_deep(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B,
                                 int k, int offset, float drop_ratio, const uint8_t* rowmask, int mask_on_device,
                                 int64_t* out_ids, float* out_scores);
/* The selection of the deep search on the caller's device arrays (no handle): d_scores / d_rows [B][n], a candidate with
 * row < 0 is invalid, the valid (score, row) pairs of one query are unique.  Writes [B][k] ids (row + row_offset) and
 * scores: entries offset .. offset + k - 1 of the candidates ordered by (score desc, row asc), then -1 / 0.
 * ascending != 0: the scores are negated distances and are written out negated (the order is the same).
 * d_scratch: hr_deep_topk_scratch_bytes(n, B, k + offset) bytes, 8-byte aligned, owned by the call until the stream has
 * run it.  Asynchronous on `stream`; the result is a function of the inputs alone (integer atomics, then a sort).
 * HR_EINVAL: k < 1, offset < 0, n < 0, B < 1, a NULL buffer; HR_ELIMIT: k + offset > HR_MAX_DEEP_K, n >= 2^31, B > 65535.
 * n == 0 writes only padding.  A refused call launches nothing. */
HR_API size_t hr_deep_topk_scratch_bytes(int64_t n, int B, int window);
HR_API int hr_deep_topk_dev(const float* d_scores, const int32_t* d_rows, int64_t n, int B, int k, int offset, int ascending,
                            int64_t row_offset, int64_t* d_out_ids, float* d_out_scores, void* d_scratch, void* stream);

/* ---- search iterator: the next k entries of a ranking after a cursor, at any depth ---------------------------------
 * hr_search_dense_deep_after / hr_search_sparse_deep_after are the two deep host forms with `offset` replaced by
 * per-query operands, each [B] on the host, any of them NULL = no query has one:
 *   after_score, after_id, has_after   the cursor of query b where has_after[b] != 0 (all three arrays given);
 *   radius, range_filter (dense)       the bounds of a range search, NULL / -+inf = that side unbounded.
 * R is the ranking defined above hr_search_dense_deep, cut to the rows in range by the rules of hr_search_dense_range
 * decided on the fp32 score the hit carries (COSINE, IP: radius < score <= range_filter; L2: range_filter <= distance <
 * radius).  The result is the first k <= HR_MAX_DEEP_K entries of R that come strictly AFTER (after_score, after_id):
 * score worse, or score equal and id larger.  Ids are the handle's (row + row_offset); under L2 cursor and hits are
 * distances.  after_id may be ANY int64: below the row offset, beyond the last row, the id of a masked or deleted row.
 * It is a position in the order, not a row that has to exist, so several shards share one cursor and a delete between
 * two pages is harmless.  Feeding the last hit of a page back gives the next page: R is walked to its end, past
 * HR_MAX_DEEP_K rows, with nothing kept on the device between the calls; every call costs one full refine of the shard.
 *   The library turns cursor and bounds into one open interval of ranking keys per query.  +0.0 and -0.0 are different
 *   keys but equal floats: a zero BOUND puts both zeros on the side float comparison puts them; the cursor's score is
 *   taken bit for bit (it is a score the library returned).
 *   HR_EINVAL: a non-finite after_score where has_after is set, a NaN bound, an empty interval (hr_search_dense_range's
 *   rule), and what the deep forms refuse; HR_ELIMIT: k > HR_MAX_DEEP_K.  A refused call launches and writes nothing.
 *   Memory, HR_ENOMEM and the profiling spans are those of the deep forms (+ 16 bytes per query). */
HR_API int hr_search_dense_deep_after(hr_index* h, const float* q, int B, int k, const float* after_score,
                                      const int64_t* after_id, const uint8_t* has_after, const float* radius,
                                      const float* range_filter, const uint8_t* rowmask, int mask_on_device,
                                      int64_t* out_ids, float* out_scores);
HR_API int hr_search_sparse_deep_after(hr_index* h, const int64_t* q_indptr, const int32_t* q_idx, const float* q_val, int B,
                                       int k, const float* after_score, const int64_t* after_id, const uint8_t* has_after,
                                       float drop_ratio, const uint8_t* rowmask, int mask_on_device, int64_t* out_ids,
                                       float* out_scores);
/* hr_deep_topk_dev with a per-query open key interval instead of an offset: d_bounds [B][2] on the device, kept are the
 * candidates with d_bounds[b][0] < rank_key(score, row) < d_bounds[b][1], where rank_key = (ord(score) << 32) |
 * (0xFFFFFFFF - row) and ord maps an fp32 to a uint32 of the same order (sign bit set: all bits flipped, else the sign bit
 * set).  The first k of them in ranking order are written, then -1 / 0: a query whose interval holds nothing writes only
 * padding.  d_bounds NULL = no interval (hr_deep_topk_dev at offset 0).  Scratch: hr_deep_topk_scratch_bytes(n, B, k).
 * Refusals as hr_deep_topk_dev. */
HR_API int hr_deep_topk_window_dev(const float* d_scores, const int32_t* d_rows, int64_t n, int B, int k, int ascending,
                                   int64_t row_offset, const unsigned long long* d_bounds, int64_t* d_out_ids,
                                   float* d_out_scores, void* d_scratch, void* stream);

/* Reciprocal-rank fusion of up to three ranked id lists of ONE query
 * (reference HybridRetriever._fuse_results, retrieval.py:421-491), executed
 * by the device kernel.  ids < 0 end a list.  out arrays hold na+nb+nc
 * entries; *n_out receives the number of fused ids. */
HR_API int hr_fuse_rrf(hr_index* h, const int64_t* ids_a, int na, const int64_t* ids_b, int nb,
                const int64_t* ids_c, int nc, double wa, double wb, double wc, int rrf_k,
                int64_t* out_ids, double* out_scores, int32_t* out_methods, int32_t* n_out);

/* ---- weighted score fusion (the second ranker of a hybrid search, beside RRF) ---------------------------------------
 * Every list's scores are normalised into [0, 1] and an id's fused score is the weighted sum of its normalised scores.
 * For an entry with fp32 score x let s = (double)x.  Every operation is a separately rounded IEEE fp64 operation, no
 * FMA.  The normalisation n is chosen per list:
 *   HR_NORM_COSINE       (1.0 + s) * 0.5                      COSINE lists
 *   HR_NORM_ATAN         0.5 + catan(s) / PI                  IP lists, dense or sparse
 *   HR_NORM_ATAN_DIST    1.0 - (2.0 * catan(s)) / PI          L2 lists (distances, ascending)
 *   HR_NORM_MINMAX       (s - lo) / (hi - lo)                 any descending list; 1.0 when hi == lo
 *   HR_NORM_MINMAX_DIST  (hi - s) / (hi - lo)                 L2 lists; 1.0 when hi == lo
 * lo / hi = the smallest / largest score of the list's valid prefix for that query; PI = 0x400921FB54442D18.  Codes
 * 0-2 follow the activation functions of Milvus' WeightedRanker, but THIS TABLE is the contract, not Milvus (which also
 * rounds to float32; fp64 is kept here, as in the RRF path).  catan is a canonical arctangent without tables or library
 * calls, so that host and device agree bit for bit:
 *   a = |x|; inv = a > 1.0; if inv: a = 1.0 / a
 *   3 times: a = a / (1.0 + sqrt(1.0 + a * a))
 *   t = a * a; c_i = (-1)^i * (1.0 / (2 i + 1)), i = 0..11; p = c_11; for i = 10 .. 0: p = c_i + t * p
 *   r = 8.0 * (a * p); if inv: r = 0x3FF921FB54442D18 - r; result = copysign(r, x)
 * Fusion is hr_fuse_rrf's with n in place of 1 / (k + rank): lists are visited a (semantic) -> b (sparse) -> c (domain),
 * an id keeps the slot of the first list that shows it, score[id] = 0.0, then += n * w_list (multiply, then add) for
 * every list that holds the id; method bits as in RRF; the final order is the stable descending sort of the fused
 * scores (ties keep first-seen order).  Weights are any doubles.  Scores must be finite.
 * HR_EINVAL: a NULL score pointer of a used list, a norm code outside 0..4; HR_ELIMIT: a list longer than HR_MAX_TOPK.
 * A refused call launches nothing and leaves the outputs alone. */
enum { HR_NORM_COSINE = 0, HR_NORM_ATAN = 1, HR_NORM_ATAN_DIST = 2, HR_NORM_MINMAX = 3, HR_NORM_MINMAX_DIST = 4 };
/* One query, host arrays (the form beside hr_fuse_rrf): out arrays hold na+nb+nc entries, *n_out the fused ids. */
HR_API int hr_fuse_scores(hr_index* h, const int64_t* ids_a, const float* sc_a, int na, int norm_a,
                   const int64_t* ids_b, const float* sc_b, int nb, int norm_b,
                   const int64_t* ids_c, const float* sc_c, int nc, int norm_c, double wa, double wb, double wc,
                   int64_t* out_ids, double* out_scores, int32_t* out_methods, int32_t* n_out);
/* A batch, device arrays (the form beside hr_fuse_rrf_dev): ids / scores [B][ka], [B][kb], [B][kc] (k = 0 / NULL for
 * none; the valid prefix of a list ends at its first id < 0); d_w_query (optional) = [B][3] doubles that replace
 * wa, wb, wc per query; outputs [B][top_k] ids / fp64 scores / method bitmasks (-1 / 0.0 / 0 padded) and d_n_out[B]. */
HR_API int hr_fuse_scores_dev(const int64_t* d_ids_a, const float* d_sc_a, int ka, int norm_a,
                       const int64_t* d_ids_b, const float* d_sc_b, int kb, int norm_b,
                       const int64_t* d_ids_c, const float* d_sc_c, int kc, int norm_c, int B,
                       double wa, double wb, double wc, const double* d_w_query, int top_k, int64_t* d_out_ids,
                       double* d_out_scores, int32_t* d_out_methods, int32_t* d_n_out, void* stream);

/* ---- multi-list fusion: up to HR_MAX_FUSE_LISTS ranked lists per query (RAG-fusion, pymilvus hybrid_search(reqs)) ----
 * The contract of the two fusions above with "three lists" replaced by "L lists"; retrieval.rrf_rank_lists and
 * retrieval.score_fuse_lists restate it.  For one query, list l = 0 .. n_lists-1 is a ranked run of non-negative ids
 * (unique inside the list) whose valid prefix ends at its first id < 0.  Lists are visited in index order, entries in
 * rank order; an id keeps the slot of its first appearance.  score[id] = 0.0, then, for every list that holds the id
 * in ASCENDING list order, score += c * w_list: one separately rounded fp64 multiply, one separately rounded fp64 add,
 * no FMA.  HR_FUSE_RRF: c = 1.0 / (double)(rrf_k + rank), rank from 1.  HR_FUSE_WEIGHTED: c = n(score) by the HR_NORM_*
 * table above, lo / hi over the list's valid prefix.  Output: the stable descending sort of the fused scores (ties keep
 * first-seen order), cut to top_k, and per id the bit mask of the lists that hold it (bit l = list l; for L <= 3 these
 * are the HR_METHOD_* bits and all outputs equal hr_fuse_rrf_dev / hr_fuse_scores_dev bit for bit).  The result is a
 * function of the inputs alone: no floating-point atomic and no thread order decides anything.
 *   d_ids [B][n_lists][k_in] int64, d_scores [B][n_lists][k_in] fp32 (NULL allowed for HR_FUSE_RRF: never read);
 *   norms: HOST array of n_lists HR_NORM_* codes (read for HR_FUSE_WEIGHTED only; NULL allowed for RRF);
 *   weights: HOST array of n_lists doubles; d_w_query (optional) DEVICE [B][n_lists] doubles that replace them per query;
 *   outputs [B][top_k]: ids (-1 padded), fp64 fused scores (0.0 padded), list masks (0 padded); d_n_out[B].
 * 1 <= n_lists <= HR_MAX_FUSE_LISTS, 1 <= k_in <= HR_MAX_TOPK, 1 <= top_k <= 3 * HR_MAX_TOPK: HR_ELIMIT beyond the
 * upper limits.  HR_EINVAL: a value below a lower limit or a negative B, a mode outside 0..1, a NULL required buffer,
 * NULL weights with NULL d_w_query, NULL scores or norms in weighted mode, a norm outside 0..4 in weighted mode, a
 * misaligned buffer (8 bytes: ids, fp64 arrays; 4 bytes: the rest), a non-finite host weight.  B == 0: HR_OK, nothing is
 * launched.  A refused call launches and writes nothing.  Asynchronous on `stream`; allocates nothing, needs no handle.
 * Scores and weights must be finite.  Whatever the ids are (duplicates inside a list included) the kernel stays inside
 * its buffers and terminates; only the values of such a query are unspecified. */
#define HR_MAX_FUSE_LISTS 16
enum { HR_FUSE_RRF = 0, HR_FUSE_WEIGHTED = 1 };
HR_API int hr_fuse_lists_dev(const int64_t* d_ids, const float* d_scores, int n_lists, int k_in, int B, int mode,
                             int rrf_k, const int32_t* norms, const double* weights, const double* d_w_query,
                             int top_k, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_lists,
                             int32_t* d_n_out, void* stream);

/* ---- search (device buffers, asynchronous on `stream`) -------------------------
 * Same results as the host forms.  d_flags[B] (optional) receives 1 when the
 * candidate-generation bound proves the list exact, 0 when the caller must
 * re-run that query through the host form (which escalates by itself).
 * The device forms do not look at the query values on the host: finite values are
 * the caller's to check (pack_sparse_queries does it for the sparse CSR).
 * Sparse weights may be signed (documents and queries): where products can be negative
 * the bound widens by 2^-11 * sum|w_q| * max|doc w| and such lists are proven less
 * often; a query whose sum|w_q| * max|doc w| leaves the fp32 range is never proven. */
/* The sparse form takes queries already reduced (drop_ratio applied) and
 * sorted by index, as CSR; max_q_nnz = the longest query (sets the scan's
 * rounding bound). */
HR_API int hr_search_dense_dev(hr_index* h, const float* d_q, int B, int k, const uint8_t* d_rowmask,
                        int64_t* d_ids, float* d_scores, int32_t* d_flags, void* stream);
HR_API int hr_search_sparse_dev(hr_index* h, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                         const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                         const uint8_t* d_rowmask, int64_t* d_ids, float* d_scores,
                         int32_t* d_flags, void* stream);
/* Range search, device form: d_radius / d_range_filter are DEVICE arrays of B doubles (NULL = unbounded for every
 * query).  The bound values are not looked at on the host: NaN and empty intervals are the caller's to check, like
 * query values.  d_flags[q] = 0 where the proof fails: always possible for rows within the scan's error of a bound. */
HR_API int hr_search_dense_range_dev(hr_index* h, const float* d_q, int B, int k, const uint8_t* d_rowmask,
                                     const double* d_radius, const double* d_range_filter,
                                     int64_t* d_ids, float* d_scores, int32_t* d_flags, void* stream);
/* Both modalities of one query batch in ONE call: the dense scan runs alone on
 * `stream`; the sparse chain then runs on a library-owned side stream so that
 * it overlaps the dense path's latency-bound tail (candidate select, refine,
 * top-k); `stream` waits for both before the call's work is considered done.
 * Results are identical to calling the two *_dev forms one after the other.
 * d_ids/d_scores/d_flags: dense lists first, then sparse ([2][B][k], [2][B]). */
HR_API int hr_search_hybrid_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                         const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                         const uint8_t* d_rowmask, int64_t* d_ids, float* d_scores, int32_t* d_flags,
                         void* stream);
/* Two-phase form of the same search, for keeping several query batches in
 * flight: phase 1 (`scan`) = query prep + the two bandwidth-bound shard scans,
 * leaving the per-group maxima in workspace `slot` (0 <= slot < HR_MAX_SLOTS);
 * phase 2 (`finish`) = candidate select + canonical refine + top-k for both
 * modalities from that slot.  A caller alternates slots and puts the scans of
 * batch i+1 on one stream while the finish of batch i (plus exchange, merge,
 * fuse, rerank) runs on another — scans never overlap each other, the
 * latency-bound tail hides behind them.  The caller orders the phases of one
 * slot with events; `finish` takes the same query buffers as `scan`. */
#define HR_MAX_SLOTS 4
/* Optional phase 0: the query preparation of `slot` alone (unit-normalised fragment-order queries, canonical |q|^2,
 * fixed-stride sparse queries and their fixed-point scale) on a stream of the caller's choice, so that the stream
 * that carries the scans carries nothing else.  The next hr_hybrid_scan_dev on the same slot then enqueues the two
 * scans only; the caller orders prep -> scan with an event.  Without this call `scan` prepares the queries itself. */
HR_API int hr_hybrid_prep_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                       const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k, int slot, void* stream);
HR_API int hr_hybrid_scan_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                       const float* d_q_val, int B, int64_t q_nnz_total, int max_q_nnz, int k,
                       const uint8_t* d_rowmask, int slot, void* stream);
HR_API int hr_hybrid_finish_dev(hr_index* h, const float* d_q, const int64_t* d_q_indptr, const int32_t* d_q_idx,
                         const float* d_q_val, int B, int max_q_nnz, int k, const uint8_t* d_rowmask, int slot,
                         int64_t* d_ids, float* d_scores, int32_t* d_flags, void* stream);
/* Batched RRF: lists are [B][ka], [B][kb], [B][kc] (kc = 0 / NULL for none);
 * outputs [B][top_k] ids / fp64 scores / method bitmasks and d_n_out[B]. */
HR_API int hr_fuse_rrf_dev(const int64_t* d_ids_a, int ka, const int64_t* d_ids_b, int kb,
                    const int64_t* d_ids_c, int kc, int B, double wa, double wb, double wc,
                    int rrf_k, int top_k, int64_t* d_out_ids, double* d_out_scores,
                    int32_t* d_out_methods, int32_t* d_n_out, void* stream);
/* Cross-shard merge after the RCCL all-gather: n_lists per-shard lists of
 * k_in (score, id) pairs per query, each sorted by score descending as the
 * search entry points write them (ids < 0 pad the tail); list l starts
 * l*score_stride floats / l*id_stride int64s after the base pointers and is
 * laid out [B][k_in] (so the lists can sit inside the ranks' slots of one
 * all-gather buffer); output the best k_out by (score desc, id asc).  (No
 * reference analogue: Milvus merges its num_shards=4 segments server-side,
 * indexing.py:234-239.) */
HR_API int hr_merge_topk_dev(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t score_stride,
                      int64_t id_stride, int B, int k_in, int k_out, int64_t* d_out_ids,
                      float* d_out_scores, void* stream);
/* The same merge for lists sorted by score ASCENDING (the per-shard lists of an HR_METRIC_L2 collection): output the
 * best k_out by (score asc, id asc). */
HR_API int hr_merge_topk_asc_dev(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t score_stride,
                          int64_t id_stride, int B, int k_in, int k_out, int64_t* d_out_ids,
                          float* d_out_scores, void* stream);
/* LearnedRanker.score + HybridRetriever.rerank's stable sort and cut
 * (reference ranker.py:109-125, retrieval.py:544-563) for a batch:
 *   new = base_w*score + method_bonus*popcount(methods) + recency_w*recency
 * Inputs are the outputs of hr_fuse_rrf_dev ([B][k_in], d_n[B] valid entries);
 * d_recency may be NULL (= 0).  Outputs [B][k_out]: ids, new scores, and the
 * fused score each kept entry had before (original_retrieval_score). */
HR_API int hr_rerank_linear_dev(const int64_t* d_ids, const double* d_scores, const int32_t* d_methods,
                         const int32_t* d_n, const double* d_recency, int B, int k_in, double base_w,
                         double method_bonus, double recency_w, int k_out, int64_t* d_out_ids,
                         double* d_out_scores, double* d_out_orig, void* stream);

/* HybridRetriever._mmr_diversify (reference retrieval.py:493-516) for a batch of fused lists: greedy MMR on the token
 * Jaccard similarity of the rows' contents, value = lambda * score - (1 - lambda) * max similarity to the selected
 * (float64, every operation rounded on its own); the first candidate in fused order with the largest value wins, only
 * values > -1e9 can be selected, and the selection stops at min(k_out, d_n[q]) or when no candidate qualifies.
 * d_ids / d_scores [B][k_in], d_n[B] valid entries: the outputs of hr_fuse_rrf_dev / hr_post_lists_dev.
 * Token sets: row r = d_tok[d_tok_indptr[r - first_row] .. d_tok_indptr[r - first_row + 1]), int32, ascending, unique;
 * an id outside [first_row, first_row + tok_rows) has the empty set.  d_tok_indptr / d_tok are NULL iff tok_rows == 0.
 * Rows may be of any length.  k_out <= k_in <= 3 * HR_MAX_TOPK (HR_ELIMIT beyond).
 * d_lambda[B]: mmr_lambda per query.
 * Out: d_out_pos [B][k_out] positions into the query's fused list in selection order (-1 padded), d_out_n[B]. */
HR_API int hr_mmr_select_dev(const int64_t* d_ids, const double* d_scores, const int32_t* d_n, int B, int k_in,
                      const int64_t* d_tok_indptr, const int32_t* d_tok, int64_t tok_rows, int64_t first_row,
                      const double* d_lambda, int k_out, int32_t* d_out_pos, int32_t* d_out_n, void* stream);

/* ---- vector MMR: the same greedy selection on the cosine of the STORED embeddings ---------------------------------------
 * What RAG stacks call max_marginal_relevance_search, without fetching fetch_k vectors per query to the host.  For query
 * q take its list of n valid entries in list order (n = d_n[q] clamped into [0, k_in]): global row ids id_i and scores
 * s_i (fp32 widened to double, or fp64 when score_is_f64 != 0).  Every operation below is a separately rounded IEEE fp64
 * operation, no FMA; division and square root are correctly rounded.
 *   relevance    rel_i = n(s_i): n is the identity (HR_NORM_NONE) or one of the five HR_NORM_* codes, exactly as
 *                hr_decay_rerank_dev applies them; lo / hi are taken over the list's valid prefix (by comparisons that a
 *                NaN score never wins), the arithmetic is the table of the weighted fusion.
 *   similarity   sim(i, j) = (double) c32(i, j), where c32 is the canonical COSINE score the library reports for the
 *                stored row id_i when the query is the stored row id_j widened exactly to fp32:
 *                  S = the k-ordered sequential fp64 sum of the exact products x_i[k] * x_j[k]
 *                  d = N_i * N_j, N = the row's canonical fp64 sum of squares (the store's norm2)
 *                  c = d > 0 ? S / sqrt(d) : 0;   c32 = (float) c
 *                ALWAYS cosine, whatever the collection's metric (IP and L2 shards keep norm2 too).  Symmetric bit for
 *                bit: products and the norm product commute.  An id outside [row_offset, row_offset + hr_num_rows) has
 *                the zero vector: its similarity to everyone is 0.  A duplicate id gets what the formula gives (1.0 or
 *                one ulp below).
 *   selection    the rule of hr_mmr_select_dev with one difference.  First pick: val_i = rel_i.  Afterwards
 *                val_i = lambda * rel_i - (1 - lambda) * m_i (two products and one subtraction, 1 - lambda computed
 *                once), m_i = the maximum of sim(i, s) over the selected s.  THE DIFFERENCE: m_i starts from the
 *                similarity to the first selected member, not from 0 — cosine can be negative, and an anti-parallel
 *                candidate is rewarded.  Every step takes the live candidate with the largest val > -1e9, among equals
 *                the first in list order; NaN is never selected; the selection stops at min(k_out, n) or when nobody
 *                qualifies.
 * d_ids / d_scores [B][k_in]; d_lambda[B]: lambda per query, so that requests with different lambdas share one launch.
 * Out: d_out_pos [B][k_out] list positions in pick order (-1 padded); d_out_val [B][k_out] val at the time of each pick
 * (0.0 padded); d_out_n[B] the picks per query.
 * d_scratch: hr_mmr_vec_scratch_bytes(h, B, k_in) bytes, 16-byte aligned: the candidates' rows, gathered once per call
 * (B * k_in rows of dim elements rounded up to 16 bytes, in the shard's element type).  Its contents are scratch.
 * 1 <= k_out <= k_in <= 3 * HR_MAX_TOPK (HR_ELIMIT for a k_in beyond; HR_EINVAL for the other orderings).  B == 0: HR_OK,
 * nothing is launched.  HR_ESTATE before hr_finalize and on a handle without a dense collection.  HR_EINVAL: a NULL
 * handle or buffer, a misaligned one (8 bytes: d_ids, d_lambda, d_out_val, fp64 scores; 4 bytes: fp32 scores, d_n,
 * d_out_pos, d_out_n; 16 bytes: d_scratch), a norm outside -1..4, negative B.  A refused call launches and writes
 * nothing.  Asynchronous on `stream`; allocates nothing; takes the handle's shared lock while it enqueues, like
 * hr_get_dense_rows_dev (the caller keeps writers away until `stream` has passed).  The result is a function of the
 * inputs alone: positions decide ties, no atomic decides anything. */
HR_API size_t hr_mmr_vec_scratch_bytes(const hr_index* h, int B, int k_in);
HR_API int hr_mmr_select_vec_dev(hr_index* h, const int64_t* d_ids, const void* d_scores, int score_is_f64, int norm,
                          const int32_t* d_n, int B, int k_in, const double* d_lambda, int k_out, void* d_scratch,
                          int32_t* d_out_pos, double* d_out_val, int32_t* d_out_n, void* stream);

/* ---- grouping search: Collection.search(..., group_by_field=F) ---------------------------------------------------
 * Milvus' grouping search returns the best entity of each of the k best groups.  A group key is an int64 per row
 * (d_keys[r - first_row], key_rows entries): an integer field as it is, or the ordinal of a string field's value in a
 * collection-wide dictionary (advanced_rag/columns.py).  Neither entry point reads a score, so descending, ascending
 * (HR_METRIC_L2) and fp64 fused lists are served alike.
 *
 * hr_group_select_dev: the first entry of every group of B ranked lists, in list order (one block per query).
 *   d_ids [B][k_in]; the valid prefix of list q is d_n[q] entries (clamped into [0, k_in]), or with d_n == NULL the
 *   entries before the first id < 0.  k_out <= k_in <= 3 * HR_MAX_TOPK (HR_ELIMIT beyond: fused lists fit, as in
 *   hr_mmr_select_dev).  An id outside [first_row, first_row + key_rows) has no key and is a group of its own (two
 *   equal such ids are two groups).  d_keys may be NULL when key_rows == 0 (it is not read then).
 *   Out: d_out_pos [B][k_out] positions into the query's list, ascending, -1 padded; d_out_keys (may be NULL)
 *   [B][k_out] the keys of the selected entries (the id itself for an entry without a key; 0 padded) — such an id is
 *   NOT a key: a caller whose lists can hold ids outside the key column must not hand d_out_keys on to
 *   hr_mask_drop_groups_dev as they are, or every row whose key equals that id is dropped; d_out_n[B];
 *   d_flags[B] (may be NULL) = 1 iff d_out_n[q] == k_out or the list held fewer than k_in valid entries (the search
 *   behind it ran out of qualifying rows), else 0: the window ended before the k_out-th group, and every distinct key
 *   of the window is among the selected.  The result is a function of the inputs alone (positions decide, no race).
 * hr_mask_drop_groups_dev: bit r of d_mask_out = bit r of d_mask_in AND "d_keys[r] is not among the n_drop keys at
 *   d_drop" for the n_rows rows of a packed row mask (bit r%8 of byte r/8; both buffers hold 8 * ceil(n_rows / 64)
 *   bytes, 8-byte aligned; bits at and beyond n_rows are written 0).  d_mask_in == NULL = all rows pass; the two
 *   buffers may be the same.  d_drop is a DEVICE pointer: any order, duplicates allowed, 0 <= n_drop <=
 *   3 * HR_MAX_TOPK (HR_ELIMIT beyond).
 * Together they continue a grouping search exactly: while a window of the ranking ends before the k-th group, the
 * groups it showed are dropped from the mask and the search is repeated — the dropped rows could never be selected
 * again.  Bad arguments: HR_EINVAL.  B == 0 / n_rows == 0: HR_OK, nothing is launched.  Asynchronous on `stream`.
 *
 * group_size > 1 (the best group_size entities of each of the k best groups):
 * hr_group_select_n_dev: hr_group_select_dev with up to group_size members per group.  Inputs and conventions are
 *   the same (valid prefix by d_n or the first id < 0; an id outside the key column is a group of its own with one
 *   member; d_keys may be NULL when key_rows == 0).  1 <= group_size, k_out <= k_in <= 3 * HR_MAX_TOPK and
 *   k_out * group_size <= 3 * HR_MAX_TOPK (HR_ELIMIT beyond).
 *   Out: d_out_pos [B][k_out * group_size]: slot o * group_size + m = the list position of the m-th member, in list
 *   order, of the o-th group, in order of first appearance; -1 padded.  d_out_keys [B][k_out] (may be NULL) the keys
 *   of the selected groups, 0 padded; d_out_cnt [B][k_out] the members written per group, 0 padded; d_out_n [B] the
 *   groups selected; d_flags [B] (may be NULL): bit 0 = hr_group_select_dev's flag (d_out_n[q] == k_out, or fewer than
 *   k_in valid entries), bit 1 = every selected group has group_size members, or the list held fewer than k_in valid
 *   entries.  An entry's rank in its group is the number of earlier entries with its key, a group's ordinal the number
 *   of group leaders before its leader: positions decide, no atomic or thread order does.  With group_size == 1,
 *   d_out_pos, d_out_keys, d_out_n and bit 0 of d_flags equal hr_group_select_dev's outputs.
 * hr_mask_keep_groups_dev: the complement sense of hr_mask_drop_groups_dev — bit r of d_mask_out = bit r of d_mask_in
 *   AND "d_keys[r] IS among the n_keep keys at d_keep" — with the same buffer rules (8 * ceil(n_rows / 64) bytes, bits
 *   at and beyond n_rows written 0, NULL input = all rows, the buffers may be the same, d_keep a device array in any
 *   order with duplicates, 0 <= n_keep <= 3 * HR_MAX_TOPK).  n_keep == 0 writes an all-zero mask.
 * Together they make the members exact: a group whose window showed group_size members, or whose window was not full,
 * is closed — a window is a prefix of the masked ranking.  The open groups are filled by searching under "base mask AND
 * key among the open groups": restricting a ranking to some groups keeps its order, and a full list of at least
 * |open| * group_size rows closes at least one group. */
HR_API int hr_group_select_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in,
                        const int64_t* d_keys, int64_t key_rows, int64_t first_row, int k_out,
                        int32_t* d_out_pos, int64_t* d_out_keys, int32_t* d_out_n, int32_t* d_flags, void* stream);
HR_API int hr_mask_drop_groups_dev(const uint8_t* d_mask_in, uint8_t* d_mask_out, int64_t n_rows,
                            const int64_t* d_keys, const int64_t* d_drop, int n_drop, void* stream);
HR_API int hr_group_select_n_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in,
                          const int64_t* d_keys, int64_t key_rows, int64_t first_row, int k_out, int group_size,
                          int32_t* d_out_pos, int64_t* d_out_keys, int32_t* d_out_cnt, int32_t* d_out_n,
                          int32_t* d_flags, void* stream);
HR_API int hr_mask_keep_groups_dev(const uint8_t* d_mask_in, uint8_t* d_mask_out, int64_t n_rows,
                            const int64_t* d_keys, const int64_t* d_keep, int n_keep, void* stream);

/* ---- decay ranker (the third ranker of a search, beside RRF and the weighted ranker) -------------------------------
 * Re-ranks B ranked lists by  final = n(score) * decay(|field - origin|):  relevance damped by the distance of a
 * numeric field (a timestamp, a chunk index, ...) from an origin.  The forms follow the decay functions of Milvus /
 * Elasticsearch, but THIS TABLE is the contract, not Milvus.  Every operation is a separately rounded IEEE fp64
 * operation, no FMA; division is correctly rounded.  For a list entry with score s (fp32 widened, or fp64) and field
 * value v widened to double ((double)v for int64: exact below 2^53):
 *   t = v - origin;  a = |t|;  u = a - offset;  d = u > 0 ? u : 0
 *   f = HR_DECAY_GAUSS : cexp(coef * (d * d))          coef = ln(decay) / (scale * scale)
 *       HR_DECAY_EXP   : cexp(coef * d)                coef = ln(decay) / scale
 *       HR_DECAY_LINEAR: g = 1.0 - d * coef; g > 0 ? g : 0.0      coef = (1 - decay) / scale
 *   v is NaN (the row has no value), or the id lies outside [first_row, first_row + col_rows):  f = 0.0
 *   final = n(s) * f
 * coef is computed by the caller (scale > 0, offset >= 0, 0 < decay < 1, so coef < 0 for gauss / exp and > 0 for
 * linear) and travels as an operand: the device needs no logarithm.  An infinite d gives f = 0.  A `func` outside 0..2
 * cannot be seen on the host, because the operands live on the device: it is DEFINED to give f = 0 for that query.
 * n is the identity (HR_NORM_NONE, valid only in this entry point) or one of the five HR_NORM_* codes, exactly as in
 * weighted score fusion; lo / hi are taken over the list's valid prefix.  Scores must be finite.
 * The output order is the stable descending sort of `final` (ties keep input order, so a list whose rows all lack the
 * field keeps its order with all-zero scores), cut to k_out.
 * cexp is a canonical exponential without tables or library calls, so that host and device agree bit for bit:
 *   x is NaN -> 0.0;  x >= 0 -> 1.0 (covers -0.0);  x < -708.0 -> 0.0
 *   k = rint(x * 0x1.71547652b82fep+0)                    (ties to even)
 *   r = (x - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33
 *   c_i = 1.0 / i!  (i = 0..13, each the correctly rounded double);  p = c_13;  for i = 12 .. 0: p = c_i + r * p
 *   result = ldexp(p, (int)k)                              (exact: k >= -1021, the result is normal)
 * d_ids / d_scores [B][k_in] (d_scores fp64 when score_is_f64 != 0, else fp32); the valid prefix of list q is d_n[q]
 * entries (clamped into [0, k_in]), or with d_n == NULL the entries before the first id < 0, as in hr_group_select_dev.
 * d_col: the field's column, col_rows values of kind HR_COL_I64, HR_COL_F32 or HR_COL_F64 (the last valid only here;
 * the filter entry points keep refusing it), row r at d_col[r - first_row]; it may be NULL iff col_rows == 0.
 * d_params: DEVICE array of B operand sets, so that queries with different curves share one launch.
 * Out, [B][k_out]: d_out_pos positions into the query's list (-1 padded), d_out_ids (-1 padded), d_out_scores the
 * final scores (0.0 padded); d_out_n[B] the entries written.
 * 1 <= k_out <= k_in <= 3 * HR_MAX_TOPK (HR_ELIMIT for a k_in beyond; HR_EINVAL for the other orderings).  HR_EINVAL:
 * a NULL required buffer, a norm outside -1..4, a col_kind outside the three, negative B / col_rows / first_row.  A
 * refused call launches nothing and leaves the outputs alone.  B == 0: HR_OK, nothing is launched.  Asynchronous on
 * `stream`.  The result is a function of the inputs alone: ranks come from comparisons, no atomic decides anything. */
enum { HR_DECAY_GAUSS = 0, HR_DECAY_EXP = 1, HR_DECAY_LINEAR = 2 };
enum { HR_COL_F64 = 5 };       /* valid only in hr_decay_rerank_dev */
enum { HR_NORM_NONE = -1 };    /* valid only in hr_decay_rerank_dev and hr_mmr_select_vec_dev */
typedef struct hr_decay_query { double origin, offset, coef; int32_t func, reserved; } hr_decay_query;
HR_API int hr_decay_rerank_dev(const int64_t* d_ids, const void* d_scores, int score_is_f64, const int32_t* d_n,
                        int B, int k_in, const void* d_col, int col_kind, int64_t col_rows, int64_t first_row,
                        const hr_decay_query* d_params /* device, [B] */, int norm, int k_out,
                        int32_t* d_out_pos, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_n, void* stream);

/* ---- boost ranker / function score (the ranker that re-scores by FILTER MATCHES) -----------------------------------
 * Re-ranks B ranked lists by  final = n(score) (x or +) f,  f the combined value of the functions whose row mask holds
 * the entry's row.  The forms follow the boost ranker and function score of Milvus 2.6, but THIS TABLE is the contract,
 * not Milvus.  Every operation is a separately rounded IEEE fp64 operation, no FMA.  Lists, valid prefix (d_n, or the
 * first id < 0), score widening, norm (-1..4) and lo / hi are exactly as in hr_decay_rerank_dev.
 * For an entry with id i, r = i - first_row, and the functions j = 0 .. n_funcs - 1 of its query:
 *   match   function j matches iff it is HR_BOOST_ACTIVE and (mask == NULL, or 0 <= r < mask_rows and bit r of mask is
 *           set: bit r % 8 of byte r / 8, as every rowmask).  A function without HR_BOOST_ACTIVE matches nothing: it is
 *           the padding that lets queries with fewer functions share a launch.
 *   draw    (HR_BOOST_RANDOM)  key = (uint64)(key_col && 0 <= r < key_rows ? key_col[r] : i);  G = 0x9E3779B97F4A7C15;
 *           fin(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (mod
 *           2^64);  h = fin(seed + G);  z = fin((h ^ key) + G);  u = (double)(z >> 11) * 2^-53  (exact, in [0, 1))
 *   value   v_j = HR_BOOST_RANDOM ? weight * u : weight                          (one rounded fp64 multiply)
 *   factor  over the matching functions IN ASCENDING j: the first gives f = v_j, each later one f = f * v_j
 *           (function_mode HR_BOOST_MULTIPLY) or f = f + v_j (HR_BOOST_SUM), each separately rounded
 *   final   no function matches: n(s), bit for bit; otherwise n(s) * f (boost_mode HR_BOOST_MULTIPLY) or n(s) + f
 *           (HR_BOOST_SUM)
 *   order   stable sort of final, descending when ascending == 0 and ascending otherwise; ties (-0.0 == 0.0 is one)
 *           keep input order; a NaN final ranks after every number in either direction, NaNs keep input order; cut to
 *           k_out
 * Known answers of the draw, (seed, key) -> u:  (0, 0) -> 0.6524484863740322;  (126, 0) -> 0.4642177690240783;
 * (126, 1) -> 0.9170314847966232;  (126, -1) -> 0.1269855469743124;  (2^64 - 1, 2^62) -> 0.2569625771059303;
 * (1, 126) -> 0.3342356104450862.
 * d_funcs: DEVICE array [B][n_funcs] of operand structs, so that queries with different masks, weights and seeds share
 * one launch; their contents cannot be seen on the host and are never refused: whatever they hold gives what the table
 * says (a negative mask_rows or key_rows is an empty range).
 * Out, [B][k_out]: d_out_pos, d_out_ids, d_out_scores and d_out_n[B] as hr_decay_rerank_dev writes and pads them;
 * d_out_matched[q][rank] = bit j set iff function j matched the entry, 0 in the padding.
 * 1 <= k_out <= k_in <= 3 * HR_MAX_TOPK (HR_ELIMIT for a k_in beyond; HR_EINVAL for the other orderings); 1 <= n_funcs
 * <= HR_MAX_BOOST_FUNCS (HR_ELIMIT beyond, HR_EINVAL below).  HR_EINVAL: a NULL required buffer, a mode outside 0..1, a
 * norm outside -1..4, negative B / first_row.  A refused call launches nothing and leaves the outputs alone.  B == 0:
 * HR_OK, nothing is launched.  Asynchronous on `stream`.  The result is a function of the inputs alone. */
#define HR_MAX_BOOST_FUNCS 8
enum { HR_BOOST_ACTIVE = 1, HR_BOOST_RANDOM = 2 };          /* hr_boost_func::flags */
enum { HR_BOOST_MULTIPLY = 0, HR_BOOST_SUM = 1 };           /* function_mode and boost_mode */
typedef struct hr_boost_func {
    const uint8_t* mask;      /* device, packed as every rowmask; NULL = every entry matches */
    const int64_t* key_col;   /* device; only read with HR_BOOST_RANDOM; NULL = the draw is keyed by the id */
    int64_t mask_rows, key_rows;
    double weight;
    uint64_t seed;
    int32_t flags, reserved;
} hr_boost_func;              /* 56 bytes */
HR_API int hr_boost_rerank_dev(const int64_t* d_ids, const void* d_scores, int score_is_f64, const int32_t* d_n,
                        int B, int k_in, const hr_boost_func* d_funcs /* device, [B][n_funcs] */, int n_funcs,
                        int64_t first_row, int function_mode, int boost_mode, int norm, int ascending, int k_out,
                        int32_t* d_out_pos, int64_t* d_out_ids, double* d_out_scores, int32_t* d_out_matched,
                        int32_t* d_out_n, void* stream);

/* ---- late-interaction rerank (ColBERT-style MaxSim; the embedding lists with MAX_SIM of Milvus 2.6) ----------------
 * Re-ranks B ranked lists by how well every query token is matched by the entry's best stored token.  THIS TABLE is the
 * contract.  Operands: row r of the token store has T_r >= 0 vectors of `dim` fp16 elements (CSR: d_indptr[tok_rows + 1]
 * non-decreasing from 0, d_tok [d_indptr[tok_rows]][dim], row r at d_indptr[r - first_row]); query q has Tq = d_qn[q]
 * vectors (clamped into [0, tq_stride]) at d_qtok[q][0 .. Tq).  dim is a multiple of 8 in 8 .. HR_MAX_TOKEN_DIM; every
 * element is finite.  For an entry with id i:
 *   token similarity  s(t, u): acc = 0.0f; for k = 0 .. dim - 1: acc = fmaf(q[t][k], d[u][k], acc), both operands
 *                     widened exactly (an fp16 x fp16 product is exact in fp32, so this is also "fp32 product, then one
 *                     rounded fp32 add"); 256 * 65504^2 < fp32 max: no overflow, no NaN
 *   per query token   m_t = the largest s(t, u) over u < T_r (fp32 compare); m_t = 0.0f when T_r == 0 or i lies outside
 *                     [first_row, first_row + tok_rows)
 *   score             S = 0.0 (fp64, plus zero); for t = 0 .. Tq - 1: S = S + (double)m_t, one rounded fp64 add each.
 *                     S is never -0.0, whatever sign a zero m_t carries.
 *   order             the stable descending sort of S (ties keep list order), cut to k_out
 * A query with 0 tokens scores every entry 0.0 and so keeps list order (defined, not refused: the operand lives on the
 * device).  CSR bounds read on the device are clamped into [0, d_indptr[tok_rows]], so a damaged CSR cannot send a load
 * outside d_tok.  Lists and valid prefix (d_n, or with d_n == NULL the entries before the first id < 0) and the outputs
 * (d_out_pos, d_out_ids -1 padded, d_out_scores 0.0 padded, d_out_n) are exactly as in hr_decay_rerank_dev.
 * 1 <= k_out <= k_in <= 3 * HR_MAX_TOPK; HR_ELIMIT for a k_in beyond, for tq_stride > HR_MAX_QUERY_TOKENS and for a dim
 * beyond HR_MAX_TOKEN_DIM; HR_EINVAL for the other orderings, a NULL required buffer (d_indptr / d_tok may be NULL iff
 * tok_rows == 0), a dim below 8 or not a multiple of 8, d_qtok / d_tok not 16-byte aligned, tq_stride < 1, negative B /
 * tok_rows / first_row.  A refused call launches nothing and leaves the outputs alone.  B == 0: HR_OK, nothing is
 * launched.  Asynchronous on `stream`; allocates nothing; not tied to an hr_index.  The result is a function of the
 * inputs alone: no atomic decides anything but the prefix length, which is a minimum. */
#define HR_MAX_QUERY_TOKENS 64
#define HR_MAX_TOKEN_DIM 256
HR_API int hr_maxsim_rerank_dev(const int64_t* d_ids, const int32_t* d_n, int B, int k_in,
                        const void* d_qtok /* fp16 [B][tq_stride][dim] */, const int32_t* d_qn /* [B] */, int tq_stride,
                        int dim, const int64_t* d_indptr /* [tok_rows + 1] */, const void* d_tok /* fp16 [..][dim] */,
                        int64_t tok_rows, int64_t first_row, int k_out, int32_t* d_out_pos, int64_t* d_out_ids,
                        double* d_out_scores, int32_t* d_out_n, void* stream);

/* ---- MaxSim as a first-stage search: every row of the token store is scored, not a list of ids (1.22.0) --------------
 * Milvus 2.6 searches an embedding list with MAX_SIM as the METRIC of the request; a rerank can only reorder what another
 * first stage found.  hr_maxsim_scan_dev writes, for B queries and the n_rows local rows of a shard, the candidate arrays
 * hr_deep_topk_dev / hr_deep_topk_window_dev select from (row_offset = the global id of local row 0):
 *   S of (query q, row i)   the value the table above defines, unchanged: the k-ascending fp32 fma chain per token pair,
 *                           m_t the fp32 maximum over the row's tokens, S the fp64 sum of the m_t in ascending t from +0.0
 *   a hit                   i < tok_rows, T_i > 0 (after the CSR bounds were clamped into [0, d_indptr[tok_rows]], as the
 *                           rerank clamps them) and bit i of d_rowmask set (packed as every rowmask: bit i & 7 of byte
 *                           i >> 3; NULL = every row passes): d_rows[q][i] = i, d_scores[q][i] = (float)S, S rounded ONCE
 *                           to fp32, nearest even — the fp32 score every other search returns.  S is never -0.0, so the
 *                           score is not; (float) is monotone, so score_a < score_b implies S_a < S_b
 *   no hit                  d_rows[q][i] = -1, d_scores[q][i] = 0.0f: a row without vectors, beyond the token store, or
 *                           masked out.  Such a row costs its mask bit and two CSR bounds: no token traffic and no matrix
 *                           work, so a selective filter makes the scan proportionally cheaper
 * Every cell of d_scores / d_rows [B][n_rows] is written by exactly one lane.  The ranking of a search is then the hits
 * by (score descending, row ascending) — hr_deep_topk_dev's rank_key — so it is exact by construction, has no proof and
 * no escalation, and the depth limit of the deep search (offset + k <= HR_MAX_DEEP_K).  Two rows whose S differ by less
 * than an fp32 ulp tie and are ordered by row: the fp64 order of a window is what hr_maxsim_rerank_dev gives on the hits.
 * Query tokens: Tq = d_qn[q] clamped into [0, tq_stride] at d_qtok[q][0 .. Tq); with Tq = 0 every row with tokens that
 * passes the mask scores +0.0f and stays a hit (defined, not refused: the operand lives on the device).
 * HR_ELIMIT: tq_stride > HR_MAX_QUERY_TOKENS, dim > HR_MAX_TOKEN_DIM, n_rows >= 2^31, B > 65535.  HR_EINVAL: a dim below 8
 * or not a multiple of 8, tq_stride < 1, negative B / tok_rows / n_rows, a NULL required buffer (d_indptr / d_tok may be
 * NULL iff tok_rows == 0; d_rowmask may always be NULL), d_qtok / d_tok not 16-byte aligned.  A refused call launches
 * nothing and leaves the outputs alone.  B == 0 or n_rows == 0: HR_OK, nothing is launched.  tok_rows may be smaller or
 * larger than n_rows.  Asynchronous on `stream`; allocates nothing; not tied to an hr_index.  No atomic takes part: the
 * result is a function of the inputs alone (and not of HR_DEBUG_MAXSIM_SCAN_BLOCKS).
 *   How: the grid is (blocks per query, B), sized so that one query still fills the chip.  A block keeps its query's
 *   tokens in LDS and walks ranges of consecutive rows; a wave takes a run of consecutive rows of each range (one forward
 *   stream through d_tok) with the rerank's loop, on v_mfma_f32_16x16x4_f32, which IS the canonical chain.  A document
 *   tile is multiplied for one query only: B queries read the store B times. */
HR_API int hr_maxsim_scan_dev(const void* d_qtok /* fp16 [B][tq_stride][dim] */, const int32_t* d_qn /* [B] */, int B,
                              int tq_stride, int dim, const int64_t* d_indptr /* [tok_rows + 1] */,
                              const void* d_tok /* fp16 [..][dim] */, int64_t tok_rows, int64_t n_rows,
                              const uint8_t* d_rowmask /* packed, bit i = local row i passes; NULL = all */,
                              float* d_scores /* [B][n_rows] */, int32_t* d_rows /* [B][n_rows] */, void* stream);

/* Everything after the per-shard lists of a query batch in ONE launch (one block per query): [hr_merge_topk_dev of
 * every modality's exchanged lists] -> hr_fuse_rrf_dev (or hr_fuse_scores_dev: `fusion`) -> [hr_rerank_linear_dev]; results are bit-identical to the
 * separate calls (reference retrieval.py:421-491 fusion, :518-563 rerank, after the server-side shard merge of
 * indexing.py:234-239).  Modality m = 0 semantic, 1 sparse, 2 domain; k_in[m] = 0 leaves a modality out.
 *   n_lists = 1: ids[m] are [B][k_in[m]] lists fused as they are (k_fuse[m] must equal k_in[m]; scores/merged_* unused by RRF);
 *   n_lists > 1: ids[m] / scores[m] point at list 0 of modality m inside the gathered buffer, list l lies l*id_stride
 *                int64s / l*score_stride floats further; the merged [B][k_fuse[m]] lists are written to merged_*[m]
 *                and fused.
 * fused_* are [B][top_k] (+ fused_n[B]); with rerank != 0 the learned-ranker outputs rr_* are [B][k_out].
 * B blocks are launched: agg_flags (if asked for) is filled by strided loops over all n_flag_rows. */
typedef struct hr_post_args {
    const int64_t* ids[3];
    const float* scores[3];
    int32_t k_in[3];
    int32_t k_fuse[3];
    int32_t n_lists;
    int32_t rrf_k;
    int64_t id_stride, score_stride;
    int64_t* merged_ids[3];
    float* merged_scores[3];
    double w[3];
    int64_t* fused_ids;
    double* fused_scores;
    int32_t* fused_methods;
    int32_t* fused_n;
    int32_t top_k;
    int32_t rerank;
    double base_w, method_bonus, recency_w;
    const double* recency;
    int32_t k_out;
    int32_t asc_mask;          /* bit m = 1: the lists of modality m are sorted by score ASCENDING (the distances of an
                                * HR_METRIC_L2 collection) and merged by (score asc, id asc); 0 = every list descending */
    int64_t* rr_ids;
    double* rr_scores;
    double* rr_orig;
    /* optional (n_lists > 1): the per-list "proven exact" flags that travelled with the lists — list l's flags are
     * n_flag_rows int32 ([modality][B]) starting l*flag_stride int32s after `flags`; agg_flags[n_flag_rows] receives
     * their minimum over the lists (a list is proven iff every shard proved its part) */
    const int32_t* flags;
    int64_t flag_stride;
    int32_t n_flag_rows;
    int32_t reserved2;
    int32_t* agg_flags;
    /* optional: fusion weights per query, [B][3] doubles (semantic, sparse, domain) — the reference lets a
     * weight_adapter choose them per request (retrieval.py:251-262); NULL = `w` for every query of the batch */
    const double* w_query;
    /* fusion: 0 = reciprocal-rank fusion (rrf_k), 1 = weighted score fusion (hr_fuse_scores_dev) with norm[m] = the
     * HR_NORM_* code of modality m.  Weighted fusion reads the scores beside the fused ids: scores[m] ([B][k_in[m]],
     * required then) when n_lists = 1, merged_scores[m] after the merge when n_lists > 1.  Zeros = RRF: the launch and
     * its operands are what they were before these fields existed.  HR_EINVAL: fusion outside 0..1, a norm code of a
     * used modality outside 0..4, a NULL scores[m] of a used modality. */
    int32_t fusion;
    int32_t norm[3];
} hr_post_args;
HR_API int hr_post_lists_dev(const hr_post_args* args, int B, void* stream);

/* ---- filter expressions -> row mask, on the device ------------------------------------------------------------
 * Replaces the server-side evaluation of the `expr` argument of Collection.search (reference indexing.py:503-525; the
 * expressions come from HybridRetriever._build_filter_expression, retrieval.py:565-632: a conjunction of
 * `field OP literal` terms over the scalar fields of the schema, indexing.py:191-225).  Columns are device arrays of
 * n_rows entries: int64, float32, or — for string fields — two uint64 per row holding the big-endian words of the
 * first 16 UTF-8 bytes, zero padded (an order-preserving prefix key).  d_mask receives the packed predicate (bit r%8 of
 * byte r/8, what every search entry point takes as rowmask); rows a string term cannot decide from the key alone
 * (first 16 bytes equal to the literal's) are left 0 in d_mask and set in d_undecided for the caller to resolve on the
 * full strings.  Both buffers hold 8 * ceil(n_rows / 64) bytes.  d_counts[2] (zeroed by the call) receives the
 * number of rows kept / undecided.  d_deleted (optional) = tombstones, 1 bit per row, 1 = never passes. */
enum { HR_COL_I64 = 0, HR_COL_I64_VS_F64 = 1, HR_COL_F32 = 2, HR_COL_STR16 = 3 };
enum { HR_OP_EQ = 0, HR_OP_NE = 1, HR_OP_LT = 2, HR_OP_LE = 3, HR_OP_GT = 4, HR_OP_GE = 5 };
#define HR_MAX_FILTER_TERMS 16
typedef struct hr_filter_term {
    int32_t kind;        /* HR_COL_* */
    int32_t op;          /* HR_OP_*  */
    const void* col;     /* device column */
    int64_t ival;        /* literal for HR_COL_I64 */
    double dval;         /* literal for HR_COL_I64_VS_F64 */
    float fval;          /* literal for HR_COL_F32 (already rounded to float32) */
    uint32_t reserved;
    uint64_t key[2];     /* literal's prefix key for HR_COL_STR16 */
} hr_filter_term;
HR_API int hr_filter_eval_dev(const hr_filter_term* terms, int n_terms, int64_t n_rows, const uint8_t* d_deleted,
                       uint8_t* d_mask, uint8_t* d_undecided, int32_t* d_counts, void* stream);

/* The same mask for the rest of the filter language: `field in [..]`, `or`, `not`, parentheses (advanced_rag/filters.py
 * has the grammar).  The expression is a set of LEAVES and a postfix PROGRAM over them, both HOST arrays copied into
 * the launch: at most HR_MAX_FILTER_TERMS leaves and HR_MAX_FILTER_PROGRAM codes.  A code >= 0 pushes the value of that
 * leaf; HR_FILTER_AND / HR_FILTER_OR pop two values and push one, HR_FILTER_NOT replaces the top.  The program is checked
 * before anything is enqueued: every leaf index in range, no pop from an empty stack, depth never above 32 and exactly 1
 * at the end (HR_EINVAL otherwise; HR_ELIMIT for too many leaves, codes or set bytes).  A refused call launches nothing
 * and leaves the outputs alone.
 *
 * A leaf is a comparison (term as in hr_filter_eval_dev) or, with term.op == HR_OP_IN, a membership test of the column
 * (term.kind HR_COL_I64, HR_COL_F32 or HR_COL_STR16; never HR_COL_I64_VS_F64) against `set`: a DEVICE array of n_set
 * members, strictly ascending (int64; float32 without NaN, membership is float32 ==, so -0.0 and 0.0 are one member
 * and a NaN row is a member of nothing; two-word prefix keys in unsigned lexicographic order), naturally aligned, NULL
 * iff n_set == 0 (no row is a member).  All sets of one call, each rounded up to 16 bytes, hold at most
 * HR_MAX_FILTER_SET_BYTES: 8192 int64, 16384 float32 or 4096 keys.  They are read while the kernel runs: keep them
 * alive until `stream` has passed the call.
 *
 * Values are three-valued, because a string leaf cannot always decide: a string comparison is unknown for a row whose
 * key equals the literal's (today's tie), a string membership leaf is unknown iff the row's key equals a member key and
 * false otherwise (literals that share their first 16 bytes are ONE member key), a numeric leaf is never unknown.  The
 * operators are Kleene's: `and` is false if a side is false, else unknown if a side is unknown; `or` mirrors it;
 * not unknown = unknown.  d_mask bit = row not deleted and the expression true; d_undecided bit = row not deleted and
 * the expression unknown — for the caller to settle by evaluating the WHOLE expression on the full strings of those
 * rows.  A decided bit is right whatever the full strings say; an undecided row may turn out either way (also where
 * Kleene cannot see that it is decided, `a or not a`).  For a conjunction of comparison leaves all four outputs equal
 * hr_filter_eval_dev's.  d_mask, d_undecided, d_counts, their alignment, the bits at and beyond n_rows, n_rows == 0 and
 * d_deleted are as in hr_filter_eval_dev.
 *
 * A KEYWORD leaf (TEXT_MATCH(content, "words"[, minimum_should_match=m]) of the filter language) has term.kind ==
 * HR_COL_TOKENS and term.op == HR_OP_MATCH; the two constants are valid only together and only here
 * (hr_filter_eval_dev refuses kind 4, and (HR_COL_I64, op 7) stays a bad term).  It reads the rows' WORD SETS, a CSR in
 * device memory, and is true for a row iff at least m of the leaf's set members are among the row's words:
 *   term.col     device int64 indptr[tok_rows + 1], non-decreasing, 8-byte aligned, never NULL; the words of row r are
 *                entries indptr[r] .. indptr[r + 1] of the word array
 *   term.key[0]  device address of the int32 word array, 4-byte aligned; 0 allowed only when tok_rows == 0
 *   term.key[1]  tok_rows >= 0; a row r >= tok_rows (n_rows may be larger or smaller) has the empty set
 *   term.ival    m >= 1
 *   set, n_set   the query's word ids: strictly ascending int32, 4-byte aligned, NULL iff n_set == 0 (no row passes)
 * Within a row the word ids are ascending and unique; the kernel may rely on that (a repeated id would be counted
 * twice).  The ids share the HR_MAX_FILTER_SET_BYTES budget with the `in` sets at 4 bytes each, rounded up to 16 per
 * set: 16384 ids alone.  m > n_set is allowed and matches no row.  The leaf is never unknown: ids are exact, nothing is
 * hashed or truncated.  HR_EINVAL "bad filter term i": either constant with the wrong partner, m < 1, tok_rows < 0, a
 * NULL or misaligned indptr, a misaligned word array or a NULL one with tok_rows > 0, a set pointer that disagrees
 * with n_set or is misaligned; HR_ELIMIT past the set budget; as every refusal, before anything is enqueued or written.
 * The word CSR is read once per leaf, 4 * entries + 8 * rows bytes, whatever n_set is. */
enum { HR_OP_IN = 6 };                          /* membership leaf; valid only in hr_filter_eval_expr_dev */
enum { HR_COL_TOKENS = 4, HR_OP_MATCH = 7 };    /* keyword leaf: only together, only in hr_filter_eval_expr_dev */
enum { HR_FILTER_AND = -1, HR_FILTER_OR = -2, HR_FILTER_NOT = -3 };   /* program codes; code >= 0 pushes leaf `code` */
#define HR_MAX_FILTER_PROGRAM 64
#define HR_MAX_FILTER_SET_BYTES 65536           /* all sets of one expression together: 8192 int64, 16384 float32, or 4096 string keys */
typedef struct hr_filter_leaf {
    hr_filter_term term;     /* comparison leaf: as in hr_filter_eval_dev.  op == HR_OP_IN: kind HR_COL_I64 / HR_COL_F32 / HR_COL_STR16 and col as there, literal fields unused */
    const void* set;         /* HR_OP_IN: DEVICE array of n_set members, strictly ascending (int64; float32 without NaN; two-word keys in unsigned lexicographic order); NULL iff n_set == 0 */
    int32_t n_set, reserved; /* HR_OP_MATCH: set = the query's word ids, strictly ascending int32 (see the keyword leaf above) */
} hr_filter_leaf;
HR_API int hr_filter_eval_expr_dev(const hr_filter_leaf* leaves, int n_leaves, const int32_t* program, int n_program,
                                   int64_t n_rows, const uint8_t* d_deleted, uint8_t* d_mask, uint8_t* d_undecided,
                                   int32_t* d_counts, void* stream);

/* ---- read path: Collection.query(expr, output_fields, limit, offset) ---------------------------------------------------
 * pymilvus reads rows back without a query vector: the rows that pass an expression, paged, with their fields and
 * vectors.  The expression becomes a packed row mask (hr_filter_eval_dev / hr_filter_eval_expr_dev); these entry points
 * turn the mask into a page of row ids and fetch stored rows out of the tiles.
 *
 * hr_mask_rows_dev: d_mask is the packed row mask every search entry point takes (bit r%8 of byte r/8, 8 * ceil(n_rows /
 *   64) bytes, 8-byte aligned); bits at and beyond n_rows may hold anything and are ignored; NULL = every row passes.
 *   d_counts[0] = the number of set bits below n_rows, whatever the page ("count(*)"); d_counts[1] = the number of ids
 *   written, max(0, min(limit, d_counts[0] - offset)); d_rows[i] = first_row + the (offset + i)-th set bit in ascending
 *   row order for i < d_counts[1] — entries at and beyond d_counts[1] are not written.  n_rows == 0 and limit == 0 still
 *   write the counts (d_rows may be NULL when limit == 0).  d_scratch: hr_mask_rows_scratch_bytes(n_rows) bytes of
 *   device memory, 8-byte aligned, not read or written when d_mask is NULL.  HR_EINVAL: a negative n_rows, offset or
 *   limit (or one of 2^62 and more), NULL outputs.  Asynchronous on `stream`; allocates nothing and never waits for the
 *   device.  The result is a function of the inputs alone: a three-phase ordered prefix (the scan of hr_compact) decides
 *   every position, no atomic does.
 *
 * hr_get_dense_rows_dev: output row i = the stored elements 0 .. dim-1 of the row with GLOBAL id d_rows[i] (local row +
 *   hr_set_row_offset), as they sit in HBM: nothing is re-quantised and the padding of the last tile is never shown.  Ids
 *   may come in any order and may repeat.  out_dtype = HR_F32: every element widened exactly (fp16 shards too); HR_F16:
 *   the raw bits, valid only on an fp16 shard (HR_EINVAL on an fp32 one).  out_stride, in elements, >= dim; elements
 *   between dim and the stride are left alone, and nothing is written after element dim-1 of the last row.  An id
 *   outside [row_offset, row_offset + hr_num_rows) reads nothing: its output row is zeros, and *d_missing (may be NULL),
 *   which the call zeroes, counts such ids.  HR_ESTATE before hr_finalize and on a handle without a dense collection.
 *   The call takes the shared lock while it enqueues, like the `*_dev` searches; the caller keeps appends and
 *   compaction away until `stream` has passed (hr_compact waits for the device by itself).
 * hr_get_dense_rows: the host form, fp32, out [n][dim], synchronous.  It refuses an id outside the shard with HR_EINVAL,
 *   naming the first one, and writes nothing.
 *
 * hr_get_sparse_rows_dev: the stored sparse rows with GLOBAL ids d_rows[0 .. n) (local row + hr_set_row_offset; any
 *   order, repeats allowed), as one CSR: d_out_indptr[0] = 0, d_out_indptr[i+1] - d_out_indptr[i] = the stored length of
 *   row d_rows[i], its entries at d_out_idx / d_out_val [d_out_indptr[i], d_out_indptr[i+1]) — the indices ascending as
 *   hr_add_sparse stored them, the values the stored bits.  An id outside [row_offset, row_offset + hr_num_sparse_rows)
 *   is an empty row and is counted in d_counts[1].  d_counts[0] = the entries of all requested rows = d_out_indptr[n] =
 *   what `cap` must be for nothing to be cut.  `cap` is the capacity of the two entry buffers, in entries: an entry whose
 *   output position is at or beyond cap is not written and nothing past cap is touched, while d_out_indptr and d_counts
 *   are always complete — the caller compares d_counts[0] with cap and calls again if it was too small.  cap == 0 (the
 *   entry buffers may then be NULL) is the count pass: sizes only.  n == 0 writes d_out_indptr[0] = 0 and both counts and
 *   launches nothing that reads the store (d_rows may be NULL).  d_scratch: hr_get_sparse_rows_scratch_bytes(n) bytes of
 *   device memory, 8-byte aligned.  The result is a function of the inputs alone: the three-phase ordered prefix of
 *   hr_compact over the request's row lengths decides every position, no atomic does (the missing count is an
 *   order-independent sum).  Asynchronous on `stream`; allocates nothing and never waits for the device.  The call takes
 *   the shared lock while it enqueues, like the `*_dev` searches; the caller keeps appends and compaction away until
 *   `stream` has passed.  HR_ESTATE before hr_finalize (rows added since are staged on the host) and on a handle without
 *   a sparse collection; HR_EINVAL: a NULL handle, a negative n or cap, NULL d_out_indptr / d_counts / d_scratch (or
 *   d_rows with n > 0), NULL entry buffers with cap > 0, d_rows / d_out_indptr / d_counts / d_scratch not 8-byte or an
 *   entry buffer not 4-byte aligned; HR_ELIMIT: n too large for one grid.  A refused call launches nothing.
 * hr_get_sparse_rows: the host form, synchronous: out_indptr [n+1] and *nnz_total (= out_indptr[n]) are always written;
 *   the entries only when *nnz_total <= cap — otherwise the call still returns HR_OK, and the caller sizes its buffers from
 *   *nnz_total and calls again (cap == 0 with NULL entry buffers is the sizing call).  It refuses an id outside the shard
 *   with HR_EINVAL, naming the first one, and writes nothing. */
HR_API size_t hr_mask_rows_scratch_bytes(int64_t n_rows);
HR_API int hr_mask_rows_dev(const uint8_t* d_mask, int64_t n_rows, int64_t first_row, int64_t offset, int64_t limit,
                     int64_t* d_rows, int64_t* d_counts, void* d_scratch, void* stream);
HR_API int hr_get_dense_rows_dev(hr_index* h, const int64_t* d_rows, int64_t n, int out_dtype, void* d_out,
                          int64_t out_stride, int32_t* d_missing, void* stream);
HR_API int hr_get_dense_rows(hr_index* h, const int64_t* rows, int64_t n, float* out);
HR_API size_t hr_get_sparse_rows_scratch_bytes(int64_t n);
HR_API int hr_get_sparse_rows_dev(hr_index* h, const int64_t* d_rows, int64_t n, int64_t* d_out_indptr, int32_t* d_out_idx,
                           float* d_out_val, int64_t cap, int64_t* d_counts, void* d_scratch, void* stream);
HR_API int hr_get_sparse_rows(hr_index* h, const int64_t* rows, int64_t n, int64_t* out_indptr, int32_t* out_idx,
                       float* out_val, int64_t cap, int64_t* nnz_total);

/* ---- BM25 document payloads (ingest) ----------------------------------------------------------------------------
 * The `encode_sparse` hook of the ingest path (reference indexing.py:629-654, called per chunk from index_chunks
 * :379-404) for the BM25 encoder of this build (advanced_rag/bm25.py), a batch at a time on the device: d_text = the
 * documents' UTF-8 bytes back to back, d_off[n_docs + 1] their byte offsets.  Per document: lower-cased `\b\w+\b` tokens
 * (ASCII classes), slot = crc32(token) mod sparse_dim, weight = (float)(tf (k1 + 1) / (tf + k1 (1 - b + b dl / avgdl))) in
 * double — bit for bit what BM25SparseEncoder.encode_document returns.  Out: d_idx / d_val [n_docs][cap] (slots ascending),
 * d_nnz[n_docs], d_flags[n_docs]: 0 = encoded, 1 = the document holds a byte >= 0x80 (Unicode case mapping and
 * categories are the host's), 2 = longer than 65 535 bytes or more than `cap` distinct slots — flagged documents have
 * nnz = 0 and are encoded by the caller on the host.  sparse_dim <= 65 536.  Asynchronous on `stream`. */
HR_API int hr_bm25_encode_dev(const uint8_t* d_text, const int64_t* d_off, int n_docs, int sparse_dim, double k1, double b,
                       double avgdl, int cap, int32_t* d_idx, float* d_val, int32_t* d_nnz, int32_t* d_flags, void* stream);

/* The hash tokenizer in front of the sentence encoder (advanced_rag/encoders.py::HashTokenizer; reference hook
 * embedding_generator.encode_semantic, indexing.py:610-620 / :580-587) for a batch of single texts: tokens of the
 * lower-cased text = `\w+|[^\w\s]`, id = 1000 + crc32(token) mod (vocab - 1000), row = CLS(101) ids[: max_len - 2] SEP(102),
 * zero padded to max_len.  d_ids [n][max_len] int64, d_lens[n] (CLS and SEP included), d_flags[n]: 1 = the text holds a
 * byte >= 0x80 (tokenise on the host).  Asynchronous on `stream`. */
HR_API int hr_hash_tokenize_dev(const uint8_t* d_text, const int64_t* d_off, int n, int max_len, int vocab, int64_t* d_ids,
                         int32_t* d_lens, int32_t* d_flags, void* stream);

/* ---- encoder / cross-encoder forward: fused elementwise pieces -----------------
 * The GEMMs and the attention of the PyTorch-ROCm encoder forwards stay with
 * hipBLASLt / SDPA; this is the residual add + LayerNorm every post-LN BERT
 * layer runs twice (the model class the reference's CrossEncoderReranker names,
 * retrieval.py:651-662):  out = LayerNorm(x (+ residual)) * gamma + beta, fp16
 * rows of `hidden` values (multiple of 8, <= 1024), fp32 statistics, one pass.
 * All pointers are device pointers (16-byte aligned); residual may be NULL;
 * out may alias x or residual. */
HR_API int hr_add_layernorm_f16_dev(const void* d_x, const void* d_residual, const void* d_gamma, const void* d_beta,
                             void* d_out, int64_t rows, int hidden, float eps, void* stream);

/* The embedding layer of the same models in one pass: d_out[s][t] = LayerNorm(word[ids[s][t]] + pos[t] + seg[types[s][t]])
 * (fp16 tables and output, hidden as above; ids / types int64, clamped into [0, n_word) / [0, n_seg); d_pos holds at least
 * T rows; the two adds are rounded to fp16 one after the other, as the unfused fp16 module rounds them). */
HR_API int hr_embed_layernorm_f16_dev(const int64_t* d_ids, const int64_t* d_types, const void* d_word, const void* d_pos,
                               const void* d_seg, const void* d_gamma, const void* d_beta, void* d_out, int64_t n_seq, int T,
                               int hidden, float eps, int64_t n_word, int64_t n_seg, void* stream);

/* Self-attention for head dimensions 32 and 64, from the fused QKV projection's output to the layout the output
 * projection reads (the PyTorch SDPA call plus the permute / transpose copies around it, in one kernel):
 *   d_qkv [n_seq][T][3][heads][head_dim] fp16, d_lengths[n_seq] valid tokens per sequence (padding at the tail; NULL = T),
 *   d_out [n_seq][T][heads * head_dim] fp16 = softmax(scale * Q K^T, keys < length) V per head, fp32 accumulation.
 * T <= 1024 at head_dim 32, <= 512 at 64 (K and V of a (sequence, head) are staged in LDS); HR_ELIMIT beyond.
 * A length above T counts as T; a length of 0 or below leaves the sequence without a key, and ALL its output rows are
 * zeros (not NaN).  Rows at or beyond a sequence's length are computed like any other (their values depend on the
 * padding's contents); the rows below it depend on nothing at or beyond it. */
HR_API int hr_attention_f16_dev(const void* d_qkv, const int32_t* d_lengths, void* d_out, int64_t n_seq, int T, int heads,
                         int head_dim, float scale, void* stream);
/* The same kernel with its operands by pointer and stride (in halves, multiples of 8): query rows at
 * d_q + seq * q_seq_stride + token * q_token_stride + head * head_dim, key / value rows at d_k / d_v + seq * kv_seq_stride +
 * token * kv_token_stride + head * head_dim; the first n_queries (<= T) tokens of a sequence are its queries;
 * d_out [n_seq][n_queries][heads * head_dim].  The cross-encoder's last layer, whose head reads token 0 only, calls it with
 * n_queries = 1 over a [n_seq][T][2][heads][head_dim] key / value buffer (advanced_rag/encoders.py). */
HR_API int hr_attention_rows_f16_dev(const void* d_q, int64_t q_seq_stride, int64_t q_token_stride, const void* d_k, const void* d_v,
                              int64_t kv_seq_stride, int64_t kv_token_stride, const int32_t* d_lengths, void* d_out,
                              int64_t n_seq, int T, int n_queries, int heads, int head_dim, float scale, void* stream);

/* ---- encoder / cross-encoder layer: the linear maps as hand-written MFMA kernels (round 4) ---------------------------
 * The forward passes behind the reference's plugin hooks (`CrossEncoderReranker.model.predict`, retrieval.py:651-685;
 * `embedding_generator.encode_semantic`, indexing.py:610-620) are post-LN BERT layers.  These two entry points are the
 * GEMM-shaped part of a layer (csrc/encoder_layer.h): weights travel as PACKED streams of 1 KiB pieces — one
 * v_mfma_f32_16x16x32_f16 A fragment (16 output features x 32 inputs) in register-image order: lane l = 16 g + r of the
 * piece holds 8 consecutive halves of row 16 t + r —
 *   natural k order:      inputs 32 s + 8 g + j,                                    j = 0..7
 *   accumulator k order:  inputs 32 s + (j < 4 ? 4 g + j : 16 + 4 g + j - 4)        (the operand comes out of an MFMA)
 * built once per model by advanced_rag/encoder_kernels.py.  fp16 activations, fp32 accumulation, fp32 biases / LayerNorm
 * parameters.  All pointers are device pointers, 16-byte aligned.
 *
 * FRAGMENT ORDER ("FR") is the activation layout between the launches of a layer: X_fr[tile = row / 16][s][lane = 16 g + c][j]
 * = X[16 tile + c][32 s + 16 (j >> 2) + 4 g + (j & 3)], 1 KiB per (16-row tile, k-step); buffers hold ceil(rows / 16) tiles.
 * It is the accumulator layout of two neighbouring output tiles AND the B operand of the next product in accumulator k
 * order, so rows move with 16-byte accesses contiguous over the wave.  Row-major stays available per operand.
 * The PAD ROWS of the last tile (rows .. 16 ceil(rows / 16) - 1) may hold anything, NaN bit patterns included: the kernels
 * read them as part of whole tiles, use them for no stored row, and never write them.
 *
 * hr_linear_rows_f16_dev:  d_out[r][0..N) (row-major, row stride out_stride halves) = x[r][0..K) W^T + bias.  d_x: row-major
 *   [rows][K] (x_fr = 0: d_w_packed pieces [N/16][K/32] in natural k order) or FR (x_fr = 1: accumulator k order).
 *   The rows of W (and d_bias) are packed in STORE ORDER: packed row 32 so + 16 u + r = output feature
 *   32 so + 8 (r >> 2) + 4 u + (r & 3), which makes a lane's eight results of a stage eight consecutive features of its row.
 *   N a multiple of 32 (<= 4096); K = 384 (HR_ELIMIT otherwise: callers keep their GEMM).
 * hr_attention_fr_f16_dev: hr_attention_f16_dev with its output in FR ([rows = n_seq * T][heads * head_dim]).
 * hr_encoder_tail_f16_dev: out = LN2(x1 + W_down gelu(W_up x1 + b_up) + b_down), x1 = LN1(x + W_out attn + b_out)
 *   for rows of `hidden` halves: everything of a layer after the attention in ONE launch; the [rows][intermediate] FFN
 *   intermediate never leaves the compute unit.  d_attn_fr: FR.  d_x / d_out: FR or row-major per x_fr / out_fr.
 *   d_wstream: stages of hidden/16 pieces, ALL in accumulator k order —
 *     W_out, two output tiles per stage: hidden/32 stages;  then, with up(c) = output tiles 2c, 2c+1 of W_up [all k-steps]
 *     and down(c) = k-step c of every output tile of W_down:
 *     up(0) | up(1) down(0) | up(2) down(1) | ... | up(I/32-1) down(I/32-2) | down(I/32-1).
 *   d_tables (fp32): b_out[H] ln1_gamma[H] ln1_beta[H] b_down[H] ln2_gamma[H] ln2_beta[H] b_up[I].
 *   gelu_erf: 0 = tanh form, 1 = exact erf form.  (hidden, intermediate) = (384, 1536) (HR_ELIMIT otherwise). */
HR_API int hr_linear_rows_f16_dev(const void* d_x, int x_fr, const void* d_w_packed, const float* d_bias, void* d_out, int64_t rows,
                           int K, int N, int64_t out_stride, void* stream);
HR_API int hr_attention_fr_f16_dev(const void* d_qkv, const int32_t* d_lengths, void* d_out_fr, int64_t n_seq, int T, int heads,
                            int head_dim, float scale, void* stream);
HR_API int hr_encoder_tail_f16_dev(const void* d_attn_fr, const void* d_x, int x_fr, void* d_out, int out_fr, const void* d_wstream,
                            const float* d_tables, int64_t rows, int hidden, int intermediate, float eps, int gelu_erf,
                            void* stream);

/* ---- streams with a compute-unit mask -------------------------------------------
 * A HIP stream whose kernels may only occupy the compute units named by `cu_mask` (bit i of word i/32 = CU i;
 * n_words 32-bit words; on gfx950 consecutive bits alternate over the 8 XCDs) — the way to keep a latency-bound
 * finishing chain and the bandwidth-bound scans off each other's compute units.  priority: 0 = default, negative =
 * higher.  The stream is an ordinary hipStream_t for every other purpose (torch.cuda.ExternalStream wraps it).
 * hr_set_scan_cus tells the scans how many compute units their stream may use (their persistent grids are sized to
 * it; 0 = all of the device's). */
HR_API int hr_stream_create(int device, int priority, const uint32_t* cu_mask, int n_words, void** out_stream);
HR_API int hr_stream_destroy(int device, void* stream);
HR_API int hr_set_scan_cus(hr_index* h, int n_cus);

/* ---- test / diagnosis hooks ---------------------------------------------------------
 * HR_DEBUG_FINISH_MODE (process-wide, handle may be NULL): 0 = choose the finishing path by batch size (default),
 *   1 = always the multi-launch chain, 2 = the fused finishing kernel whenever the candidate set fits LDS — lets the
 *   parity tests drive both paths at any batch size.
 * HR_DEBUG_FAIL_NEXT_BUILD: value != 0 makes the next hr_finalize fail after the sparse rows have reached the device
 *   CSR and before the postings are rebuilt (what an allocation failure at that point leaves behind); the
 *   finalize after that must complete the build.
 * HR_DEBUG_DENSE_KERNELS (process-wide): bit mask that takes dense scan kernels out of the selection so that the
 *   others serve the shapes they would have served — 1 = no register-resident 256-query pass, 2 = no tiled-contraction
 *   pass, 4 = no k-chunked large-batch pass, 8 = prefer the tiled contraction where both 256-query passes apply, 16 = the 4 x 64-query register form
 *   (dense_scan_q64_kernel) instead of the 8 x 32-query one for the 256-query pass at D = 768.
 * HR_DEBUG_SPARSE_RPB (process-wide): doc ranges one sparse-scan block walks (0 = by shard size).
 * HR_DEBUG_GROUP_ROWS (process-wide): rows per candidate group (16 or 64; 0 = by shard size) of handles created
 *   afterwards.
 * HR_DEBUG_NO_TRIM (process-wide): 1 = refine every one of the C candidate groups of a query (round 3's behaviour) instead
 *   of only those whose maximum is within twice the scan's error bound of the k-th largest group maximum (A/B, tests).
 * HR_DEBUG_NO_RANGE_CLAMP (process-wide): 1 = the scans of a range search get +inf ceilings, i.e. they do not drop the
 *   rows above range_filter.  Results through the host form do not change (exactness never rests on the clamp); the
 *   device form's flags show what the clamp proves (tests, tests/probes/range_probe.py).
 * HR_DEBUG_MAXSIM_SCAN_BLOCKS (process-wide): blocks per query of hr_maxsim_scan_dev, 1 .. 65535 (0 = by batch and store
 *   size).  The range size follows it, so a small value makes every block walk several ranges of 256 rows on a store of
 *   a few thousand rows (tests); the result does not depend on it.
 * The library reads no environment variables. */
enum { HR_DEBUG_FINISH_MODE = 1, HR_DEBUG_FAIL_NEXT_BUILD = 2, HR_DEBUG_DENSE_KERNELS = 3, HR_DEBUG_SPARSE_RPB = 4,
       HR_DEBUG_GROUP_ROWS = 5, HR_DEBUG_NO_TRIM = 6, HR_DEBUG_NO_RANGE_CLAMP = 7, HR_DEBUG_MAXSIM_SCAN_BLOCKS = 8 };
HR_API int hr_debug_option(hr_index* h, int key, int value);

/* ---- measurement hooks -------------------------------------------------------
 * hr_set_profiling(1) brackets every dense-scan and sparse-scan launch with
 * HIP events on the stream it is launched on; (2) brackets all ten phases:
 * [0] query prep, [1] dense scan, [2] group select, [3] refine, [4] top-k,
 * [5] sparse scan, [6] sparse select, [7] sparse refine, [8] sparse top-k,
 * [9] the fused finishing kernel (select + refine + top-k of a batch in one launch).
 * hr_last_kernel_ms drains the recorded spans: out_ms[p] = mean ms per launch
 * of phase p since the previous call, out_ms[HR_N_PHASES + p] = launches
 * averaged.  n must be >= 2*HR_N_PHASES. */
#define HR_N_PHASES 10
HR_API int hr_set_profiling(hr_index* h, int enabled);
HR_API int hr_last_kernel_ms(hr_index* h, float* out_ms, int n);
/* The last hr_compact that changed the handle: out_ms[0] = compact_tiles_kernel between two HIP events (0 unless
 * hr_set_profiling was on and dense rows survived), out_ms[1] = the whole call, out_ms[2] = the posting rebuild inside
 * it (host wall time, ms).  n must be >= 3. */
HR_API int hr_last_compact_ms(hr_index* h, float* out_ms, int n);
/* Algorithmic bytes one dense scan launch reads (rows*dim*sizeof(elem) + 4*rows: the rows and one float per row —
 * the scale of a COSINE / IP shard, the row term |x|^2 / 2 of an L2 shard, which takes the scale's place). */
HR_API int64_t hr_dense_scan_bytes(const hr_index* h);

#ifdef __cplusplus
}
#endif
#endif /* HBMRAG_H */
