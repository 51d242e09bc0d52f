// Prints the dense scan plan (csrc/scan_plan.h) of every search on its input: tests/test_scan_plan.py compiles this for
// the host, feeds it the searches of tests/golden/scan_plan_table.txt and compares.
//   in:  KT dtype metric n_rows group_rows_override mask B
//   out: KT dtype metric n_rows group_rows_override mask B | chunk_q NRB l2 G_total | nq:kernel:G ...   (or: | none)
#include <cstdio>
#include <cstring>

#include "../advanced-rag-milvus_amd/csrc/scan_plan.h"

int main() {
    static const char* const names[] = {"none", "lds", "bigq", "qreg", "q64", "gemm"};
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int KT, dtype, metric, override, mask, B;
        long long n_rows;
        if (sscanf(line, "%d %d %d %lld %d %d %d", &KT, &dtype, &metric, &n_rows, &override, &mask, &B) != 7) return 2;
        printf("%d %d %d %lld %d %d %d |", KT, dtype, metric, n_rows, override, mask, B);
        auto plan = [&](int nq) { return hbmrag::scan_plan(KT, dtype, metric, n_rows, override, mask, B, nq); };
        const hbmrag::ScanPlan first = plan(B);
        if (first.kind == hbmrag::SCAN_NONE) {
            printf(" none\n");
            continue;
        }
        const int chunk_q = first.chunk_q, n_chunks = (B + chunk_q - 1) / chunk_q;
        printf(" %d %d %d %d |", chunk_q, first.NRB, (int)first.l2,
               (n_chunks - 1) * (chunk_q / 16) + plan(B - (n_chunks - 1) * chunk_q).G);
        for (int c0 = 0; c0 < B; c0 += chunk_q) {
            const int nq = B - c0 < chunk_q ? B - c0 : chunk_q;
            const hbmrag::ScanPlan p = plan(nq);
            if (p.chunk_q != chunk_q || p.NRB != first.NRB || p.l2 != first.l2) return 3;  // per-search fields
            printf(" %d:%s:%d", nq, names[p.kind], p.G);
        }
        printf("\n");
    }
    return 0;
}
