// Which dense scan kernel serves a pass of a search, as a pure function of the shard's shape and the batch: no HIP, no
// handle, so a stand-alone host program can print it (tests/test_scan_plan.py holds it to a table recorded from the
// selection as it stood before it lived here; bench.py derives its kernel label from the same inputs).
#pragma once
#include <stdint.h>

#include "../../include/hbmrag.h"

namespace hbmrag {

enum ScanKind {
    SCAN_NONE = 0,  // the query tile does not fit LDS and the k-chunked pass is switched off: HR_ELIMIT
    SCAN_LDS,       // dense_scan_kernel: up to 64 queries, the whole query tile in LDS
    SCAN_BIGQ,      // dense_scan_bigq_kernel: 128 queries per pass, the query tile streamed through LDS in k-chunks
    SCAN_QREG,      // dense_scan_qreg_kernel: 256 queries per pass, queries in registers (fp16, KT = 24)
    SCAN_Q64,       // dense_scan_q64_kernel: the same with 4 waves x 64 queries (opt-in)
    SCAN_GEMM,      // dense_scan_gemm_kernel: 256 queries per pass as a tiled contraction (fp16, KT >= 8)
};

struct ScanPlan {
    int kind;     // ScanKind of this pass
    int G;        // query groups of 16 this pass prepares and scans
    int chunk_q;  // queries per full pass of the search (16 x the groups a pass owns in the fragment buffer)
    int NRB;      // row blocks per candidate group: 1 (16-row groups) or 4 (64-row groups)
    bool l2;      // the squared-Euclidean epilogue
    bool range;   // the range-search epilogue (per-query ceilings)
};

// HR_DEBUG_DENSE_KERNELS bit mask (tests drive every scan kernel at every shape): 1 = no register-resident 256-query
// pass, 2 = no tiled-contraction pass, 4 = no k-chunked large-batch pass, 8 = prefer the tiled contraction to the
// register-resident pass where both apply, 16 = the 4 x 64-query form of the register-resident pass
enum { SCAN_NO_QREG = 1, SCAN_NO_GEMM = 2, SCAN_NO_BIGQ = 4, SCAN_PREFER_GEMM = 8, SCAN_Q64_FORM = 16 };

constexpr int kScanTileKiB = 156;  // LDS the LDS-resident pass's query tile may take: G * KT KiB

// Rows (docs) per candidate group.  Small shards (a rank of a multi-GPU corpus) use 16-row
// groups: 4x less refine traffic per query, and the 4x larger table of group maxima is
// still small.  Big shards use 64-row groups, where selecting among 4x more maxima would
// cost more than the refine saves (measured at 10M x 768: 3.88 ms/step vs 4.08).
inline int scan_group_rows(int64_t n_rows, int group_rows_override) {
    if (group_rows_override) return group_rows_override;
    return n_rows > 3000000 ? 64 : 16;
}

// The pass that scans a chunk of nq queries of a batch of B (nq = min(chunk_q, what is left of B); the first pass of
// a batch: nq = min(B, its own chunk_q), so scan_plan(..., B, B) yields chunk_q).  KT = 1 KiB tiles per row.
// range = a pass of a range search: the two generic kernels only (the inline-asm forms have no ceiling), so 256 ranged
// queries are two 128-query passes, as for L2.
inline ScanPlan scan_plan(int KT, int dtype, int metric, int64_t n_rows, int group_rows_override, int mask, int B,
                          int nq, bool range = false) {
    ScanPlan p{};
    p.l2 = metric == HR_METRIC_L2;
    p.range = range;
    p.NRB = scan_group_rows(n_rows, group_rows_override) == 16 ? 1 : 4;
    const int g_fit = kScanTileKiB / (KT > 1 ? KT : 1);
    const int g_small = g_fit < 1 ? 1 : g_fit > 4 ? 4 : g_fit;  // groups of the LDS-resident tile
    // fp32 rows longer than 2496 (KT > 156) do not fit even one group of 16 queries: every batch of such a shard takes
    // the k-chunked pass, whose LDS does not grow with KT
    const bool fits = g_small * KT <= kScanTileKiB;
    // batches beyond what fits LDS whole go through the k-chunked large-batch pass, 128 or 256 queries at a time
    const bool big = (B > 16 * g_small || !fits) && KT % 4 == 0 && !(mask & SCAN_NO_BIGQ);
    if (!big) {
        p.kind = fits ? SCAN_LDS : SCAN_NONE;
        p.G = (nq + 15) / 16;
        p.chunk_q = 16 * g_small;
        return p;
    }
    // 256 queries per pass: fp16 COSINE / IP without a range only (the inline-asm forms have no L2 and no range epilogue);
    // which form
    const bool f16 = dtype == HR_F16;
    const bool gemm = f16 && KT >= 8 && !(mask & SCAN_NO_GEMM);
    const bool qreg = f16 && KT == 24 && !(mask & SCAN_NO_QREG) && !((mask & SCAN_PREFER_GEMM) && gemm);
    const int kind256 = (B <= 128 || p.l2 || range) ? SCAN_NONE
                        : qreg             ? ((mask & SCAN_Q64_FORM) ? SCAN_Q64 : SCAN_QREG)
                        : gemm             ? SCAN_GEMM
                                           : SCAN_NONE;
    // a trailing chunk of <= 128 queries takes the 128-query pass
    p.kind = (kind256 != SCAN_NONE && nq > 128) ? kind256 : SCAN_BIGQ;
    p.G = p.kind == SCAN_BIGQ ? 8 : 16;
    p.chunk_q = kind256 != SCAN_NONE ? 256 : 128;
    return p;
}

}  // namespace hbmrag
