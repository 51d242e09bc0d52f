"""Writes scan_plan_table.txt: which dense scan serves every pass of a search, for a table of shard shapes and batches.

The expectation is NOT computed by csrc/scan_plan.h.  `parent_selection` below is the selection as dense_search_enqueue
and its launch helpers (csrc/hbmrag.hip) made it before the plan had a header of its own: the boolean expressions were
ported verbatim, once, from that revision (max_groups_for_dim, scan_tile_fits, qreg_supported, gemm_supported, big,
prefer_gemm, use_qreg, big256, groups_of, pass256 and the if-ladder in front of the launches).  Do not "simplify" it to
match the header; tests/test_scan_plan.py compares the header against this file's output.

    python tests/golden/gen_scan_plan_table.py > tests/golden/scan_plan_table.txt

The table is the full cross product (KT x dtype x metric x B x mask x group line = 11520 searches), written compactly:
every distinct outcome once under a two-digit code, then one line of codes per (KT, dtype, metric).
"""
HR_F32, HR_F16 = 0, 1
HR_METRIC_IP, HR_METRIC_COSINE, HR_METRIC_L2 = 0, 1, 2
kScanTileKiB = 156


def parent_selection(KT, dtype, metric, n_rows, group_rows_override, g_dense_kernels, B):
    # group_rows_for
    group_rows = group_rows_override if group_rows_override else (64 if n_rows > 3000000 else 16)
    NRB = 1 if group_rows == 16 else 4
    # max_groups_for_dim, scan_tile_fits
    Gsmall = max(1, min(4, kScanTileKiB // max(KT, 1)))
    scan_tile_fits = Gsmall * KT <= kScanTileKiB
    # qreg_supported, gemm_supported
    qreg_supported = (not (g_dense_kernels & 1)) and dtype == HR_F16 and KT == 24
    gemm_supported = (not (g_dense_kernels & 2)) and dtype == HR_F16 and KT >= 8
    # dense_search_enqueue
    big = (B > 16 * Gsmall or not scan_tile_fits) and KT % 4 == 0 and not (g_dense_kernels & 4)
    if not big and not scan_tile_fits:
        return None  # HR_ELIMIT
    prefer_gemm = (g_dense_kernels & 8) != 0
    use_qreg = qreg_supported and not (prefer_gemm and gemm_supported)
    l2 = metric == HR_METRIC_L2
    big256 = big and B > 128 and not l2 and (use_qreg or gemm_supported)
    Gmax = 16 if big256 else 8 if big else Gsmall
    chunk_q = 16 * Gmax
    n_chunks = (B + chunk_q - 1) // chunk_q

    def groups_of(nq):
        return (16 if (big256 and nq > 128) else 8) if big else (nq + 15) // 16

    G_total = (n_chunks - 1) * Gmax + groups_of(B - (n_chunks - 1) * chunk_q)
    passes = []
    for c0 in range(0, B, chunk_q):
        nq = min(chunk_q, B - c0)
        pass256 = big256 and nq > 128
        G = groups_of(nq)
        if pass256:
            kernel = "q64" if (use_qreg and (g_dense_kernels & 16)) else "qreg" if use_qreg else "gemm"
        elif big:
            kernel = "bigq"
        else:
            kernel = "lds"
        passes.append((nq, kernel, G))
    return chunk_q, NRB, int(l2), G_total, passes


KTS = (4, 8, 24, 32, 156, 160)
BS = (1, 16, 17, 64, 65, 128, 129, 256, 257, 300)
MASKS = (0, 1, 2, 3, 4, 8, 16, 1 | 16)
GROUPS = ((3000000, 0), (3000001, 0), (1000, 64), (3000001, 16))   # (n_rows, override): by shard size, and pinned


def outcome(r):
    return "none" if r is None else "%d %d %d | %s" % (r[0], r[2], r[3], " ".join("%d:%s:%d" % p for p in r[4]))


if __name__ == "__main__":
    codes, rows = {}, []
    for KT in KTS:
        for dtype in (HR_F16, HR_F32):
            for metric in (HR_METRIC_IP, HR_METRIC_COSINE, HR_METRIC_L2):
                cells = []
                for B in BS:
                    cell = []
                    for mask in MASKS:
                        rs = [parent_selection(KT, dtype, metric, n, o, mask, B) for n, o in GROUPS]
                        # the group size decides NRB and nothing else
                        assert len({outcome(r) for r in rs}) == 1
                        cell.append("%02d" % codes.setdefault(outcome(rs[0]), len(codes)))
                    cells.append(",".join(cell))
                rows.append("%d %d %d : %s" % (KT, dtype, metric, " ".join(cells)))
    print("# groups: n_rows group_rows_override -> NRB")
    for n, o in GROUPS:
        print("%d %d -> %d" % (n, o, parent_selection(24, HR_F16, HR_METRIC_IP, n, o, 0, 1)[1]))
    print("# outcomes: code = chunk_q l2 G_total | nq:kernel:G per pass   (none: HR_ELIMIT)")
    for o, c in codes.items():
        print("%02d = %s" % (c, o))
    print("# plans: KT dtype metric : per B in %s the codes for the masks %s, the same for every group line above"
          % (",".join(map(str, BS)), ",".join(map(str, MASKS))))
    for r in rows:
        print(r)
