"""The persistent-grid walk of the five dense scans, on a few compute units.

The scans' grids are sized to hr_set_scan_cus; at the default (every CU of the device) a wave takes a second super-group
of 64 rows only beyond ~131 k rows and a block of a 256-query pass beyond 16 k, so the grid-stride step, the prefetch
cursor crossing a group boundary, the "past my last group" re-read, the lockstep rounds with idle waves of the 128-query
pass, the reuse of the LDS-DMA ring across super-groups and a ragged last trip after full ones run in a few large
tests only.  Here a 6 437-row shard (101 super-groups, the last one ragged) is searched with set_scan_cus(1), (3) and
(0) on the same handle: at one CU every wave or block makes 3 to 101 trips, at three the trip counts differ between
waves.  The corpora are planted (tests/planted_rows.py): the best row of every query sits at a chosen position — every
super-group, every in-group offset, rows 0 and n - 1, both ends of the ragged group — and beats every other allowed row
by more than 100 x the scans' error bound (tests/test_planted_rows.py), so that

  1. k = 1, device form: ids[b, 0] == pos[b], the score bits are the oracle's, and EVERY flag is 1: an unproven list
     means a wrong group maximum or a wrong cut;
  2. k = 40: the host form equals the oracle bit for bit, the device form wherever its flag is 1, on both edges of
     every group of 16 query slots (hence of every pass);
  3. ids, score bits and flags of the device form at 1 and 3 CUs equal those at the default grid bit for bit, for the
     whole batch: a group's maximum must not depend on which wave computed it or on which trip;
  4. masked corpora: no decoy (a copy of the planted row under a cleared mask bit at p +- 1, p + 8, p + 16, p + 64)
     appears in any list; ranged corpora: no list holds a decoy of its own query (a row above that query's ceiling
     beside p and at p + 16; to the other queries it is an ordinary row).

Which kernel serves which pass is asserted with the selection restated in tests/golden/gen_scan_plan_table.py, which
tests/test_scan_plan.py holds to csrc/scan_plan.h."""
import functools
import os
import runpy

import numpy as np
import pytest

import oracle
import planted_rows as pr
import range_yardstick as ry
from advanced_rag import _native as nat
from l2_yardstick import bits

pytestmark = pytest.mark.gpu

assert (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE, nat.HR_METRIC_L2) == (pr.IP, pr.COSINE, pr.L2)
HR_DTYPE = {np.float16: nat.HR_F16, np.float32: nat.HR_F32}
METRIC_NAME = {pr.IP: "IP", pr.COSINE: "COSINE", pr.L2: "L2"}
CUS = (0, 1, 3)                   # the default grid first: what the small grids are compared with
K = 40

_SELECTION = runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_scan_plan_table.py"))


def passes(d, np_dtype, metric, B, kernels_mask=0):
    """[(queries, kernel, query groups)] of a search, by the recorded selection (n_rows and the group size do not enter)."""
    f16 = np_dtype == np.float16
    KT = ry.padded_dim(d, f16) // (32 if f16 else 16)
    sel = _SELECTION["parent_selection"](KT, 1 if f16 else 0, metric, 1000, 16, kernels_mask, B)
    assert sel is not None
    return list(sel[4])


@pytest.fixture
def options():
    def set_(key, value):
        nat.debug_option(key, value)
    yield set_
    for key in (nat.HR_DEBUG_DENSE_KERNELS, nat.HR_DEBUG_SPARSE_RPB, nat.HR_DEBUG_GROUP_ROWS, nat.HR_DEBUG_FINISH_MODE):
        nat.debug_option(key, 0)


def _shard(X, metric):
    """Two add_dense calls with a finalize between them."""
    h = nat.ShardHandle(X.shape[1], HR_DTYPE[X.dtype.type], metric)
    cut = X.shape[0] // 3
    h.add_dense(X[:cut])
    h.finalize()
    h.add_dense(X[cut:])
    h.finalize()
    assert h.num_rows == X.shape[0]
    return h


def _picks(B):
    """Both edges of every group of 16 query slots (every pass starts on one) and the last query; where that gives fewer
    than 16 queries (B < 128), further slots from inside the groups (7, 8, then 3, 12, ...) until there are 16, or all B."""
    if B <= 40:
        return list(range(B))
    picks = {q for g in range(0, B, 16) for q in (g, min(g + 15, B - 1))} | {B - 1}
    for inner in (7, 8, 3, 12, 5, 10, 1, 14):
        if len(picks) >= 16:
            break
        picks |= {g + inner for g in range(0, B, 16) if g + inner < B}
    assert len(picks) >= 16
    return sorted(picks)


@functools.lru_cache(maxsize=12)     # the twelve corpora of the d = 768 cases (2 metrics x 2 variants x 3 batches), ~10 MB each
def _expect(name, np_dtype, metric, B, variant):
    """-> (planted corpus, picks, (ids, scores) at k = 1 for the whole batch, (ids, scores) at k = K for the picks).
    The oracle's k-ordered fp64 chain costs 60 ms per query at 6 437 x 768, so every row is scored for the picks only, once,
    and ranked by the oracle's top-k; at k = 1 the id is the planted row (test_planted_rows.py: it wins by 100 error bounds
    in fp64) and the score is the oracle's canonical score of that one row.  Shared between the cases; read-only."""
    s = pr.SHARDS[name]
    p = pr.planted(s.n, s.d, np_dtype, metric, B, variant)

    def scores(X, qs):
        if metric == pr.L2:
            return ry.l2_dist_batch(X, p.Q[qs])
        return np.stack([oracle.dense_scores(X, p.Q[b], metric) for b in qs])

    def topk(S_b, b, k):
        if variant == "range":
            return ry.topk_in_range(S_b, metric, k, p.radius[b], p.range_filter[b], p.keep)
        if metric == pr.L2:                                     # l2_yardstick.l2_search on the rows already scored
            i, v = oracle.topk(-S_b, k, p.mask)
            v = -v
            v[i < 0] = 0.0
            return i, v
        return oracle.topk(S_b, k, p.mask)

    picks = _picks(B)
    S = scores(p.X, picks)
    got = [topk(S[j], b, K) for j, b in enumerate(picks)]
    wantk = (np.stack([g[0] for g in got]), np.stack([g[1] for g in got]))
    own = np.array([scores(p.X[r:r + 1], [b])[0, 0] for b, r in enumerate(p.pos)], np.float32)
    want1 = (p.pos.reshape(B, 1).copy(), own.reshape(B, 1))
    # the two agree where both exist: the planted row heads the full list of every pick, with that score
    assert np.array_equal(wantk[0][:, 0], p.pos[picks]) and np.array_equal(bits(wantk[1][:, 0]), bits(own[picks]))
    return p, picks, want1, wantk


class _Device:
    """The device buffers of one (corpus, batch): queries, mask and bounds go up once."""

    def __init__(self, p):
        import torch
        self.torch = torch
        self.B = p.Q.shape[0]
        self.q = torch.from_numpy(np.array(p.Q)).cuda()
        self.mask = torch.from_numpy(pr.device_mask(p.mask, p.X.shape[0])).cuda() if p.mask is not None else None
        self.ranged = p.range_filter is not None
        if self.ranged:
            self.radius = torch.from_numpy(np.array(p.radius, dtype=np.float64)).cuda()
            self.rfilter = torch.from_numpy(np.array(p.range_filter, dtype=np.float64)).cuda()

    def search(self, h, k):
        torch, B = self.torch, self.B
        ids = torch.full((B, k), -5, dtype=torch.int64, device="cuda")
        sc = torch.full((B, k), -5.0, dtype=torch.float32, device="cuda")
        fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream()
        m = self.mask.data_ptr() if self.mask is not None else 0
        if self.ranged:
            h.search_dense_range_dev(self.q.data_ptr(), B, k, self.radius.data_ptr(), self.rfilter.data_ptr(), ids.data_ptr(),
                                     sc.data_ptr(), fl.data_ptr(), m, st.cuda_stream)
        else:
            h.search_dense_dev(self.q.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), m, st.cuda_stream)
        st.synchronize()
        return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def _host(h, p, k):
    if p.range_filter is not None:
        return h.search_dense_range(p.Q, k, p.radius, p.range_filter, p.mask)
    return h.search_dense(p.Q, k, p.mask)


def _walk(h, name, np_dtype, metric, B, variant, what):
    """Assertions 1-4 of the module docstring for one batch on one handle."""
    p, picks, want1, wantk = _expect(name, np_dtype, metric, B, variant)
    dev = _Device(p)
    seen = {}
    for cus in CUS:
        h.set_scan_cus(cus)
        tag = f"{what} B={B} cus={cus}"
        ids1, sc1, fl1 = dev.search(h, 1)
        assert np.array_equal(ids1[:, 0], p.pos), f"{tag} k=1: queries {np.flatnonzero(ids1[:, 0] != p.pos)[:8]} miss their planted row"
        assert np.array_equal(bits(sc1), bits(want1[1])), f"{tag} k=1: score bits"
        assert np.array_equal(fl1, np.ones(B, np.int32)), f"{tag} k=1: lists of queries {np.flatnonzero(fl1 != 1)[:8]} not proven"
        idsk, sck, flk = dev.search(h, K)
        assert set(np.unique(flk).tolist()) <= {0, 1}, f"{tag} k={K}: flags {np.unique(flk)}"
        for j, b in enumerate(picks):
            if flk[b] == 1:
                assert np.array_equal(idsk[b], wantk[0][j]), f"{tag} k={K}: proven list of query {b} differs"
                assert np.array_equal(bits(sck[b]), bits(wantk[1][j])), f"{tag} k={K}: proven scores of query {b} differ"
        hid, hsc = _host(h, p, K)
        wrong = [picks[j] for j in np.flatnonzero((hid[picks] != wantk[0]).any(axis=1))]
        assert not wrong, f"{tag} host: ids of queries {wrong[:8]}"
        assert np.array_equal(bits(hsc[picks]), bits(wantk[1])), f"{tag} host: score bits"
        for lst, form in ((ids1, "device k=1"), (idsk, f"device k={K}"), (hid, "host")):
            owner = np.where(lst >= 0, p.decoy_of[np.clip(lst, 0, None)], -1)
            # a masked decoy may appear in no list; a range decoy lies above the ceiling of the query it was written for
            bad = (owner >= 0) if variant == "mask" else (owner == np.arange(B)[:, None])
            assert not bad.any(), f"{tag} {form}: a decoy in the lists of queries {np.flatnonzero(bad.any(axis=1))[:8]}"
        seen[cus] = (ids1, sc1, fl1, idsk, sck, flk)
    h.set_scan_cus(0)
    for cus in CUS[1:]:
        parts = ("k=1 ids", "k=1 scores", "k=1 flags", f"k={K} ids", f"k={K} scores", f"k={K} flags")
        for a, b_, part in zip(seen[cus], seen[0], parts):
            same = np.array_equal(bits(a), bits(b_)) if a.dtype == np.float32 else np.array_equal(a, b_)
            assert same, f"{what} B={B}: {part} at {cus} CUs differ from the default grid's"


# ---- d = 128: the LDS scan at G = 1, 3, 4 and the 128-query pass with a 2-query tail, fp16 and fp32, three metrics -------
@pytest.mark.parametrize("variant", ["plain", "mask"])
@pytest.mark.parametrize("group_rows", [16, 64])
@pytest.mark.parametrize("metric", [pr.COSINE, pr.IP, pr.L2], ids=lambda m: METRIC_NAME[m])
@pytest.mark.parametrize("np_dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_lds_scan_and_128_query_pass_walk(gpu, options, np_dtype, metric, group_rows, variant):
    s = pr.SHARDS["d128"]
    options(nat.HR_DEBUG_GROUP_ROWS, group_rows)
    options(nat.HR_DEBUG_DENSE_KERNELS, 0)                     # bit 4 off: B = 130 takes the 128-query pass, at L2 as well
    assert [passes(s.d, np_dtype, metric, B) for B in s.batches] == [
        [(1, "lds", 1)], [(33, "lds", 3)], [(64, "lds", 4)], [(128, "bigq", 8), (2, "bigq", 8)]]
    h = None
    try:
        for B in s.batches:
            X = pr.planted(s.n, s.d, np_dtype, metric, B, variant).X
            h = _shard(X, metric)
            _walk(h, "d128", np_dtype, metric, B, variant, f"d128 {np.dtype(np_dtype).name} {METRIC_NAME[metric]} g{group_rows} {variant}")
            h.close()
            h = None
    finally:
        if h is not None:
            h.close()


@pytest.mark.parametrize("group_rows", [16, 64])
@pytest.mark.parametrize("metric", [pr.COSINE, pr.IP, pr.L2], ids=lambda m: METRIC_NAME[m])
@pytest.mark.parametrize("np_dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_range_epilogue_walks_on_both_generic_kernels(gpu, options, np_dtype, metric, group_rows):
    """RANGE = true on the LDS scan (B = 64) and the 128-query pass (B = 130): the planted row lies in the range, rows
    above the ceiling sit in its 16-row block and in the next one."""
    s = pr.SHARDS["d128_range"]
    options(nat.HR_DEBUG_GROUP_ROWS, group_rows)
    assert [passes(s.d, np_dtype, metric, B) for B in s.batches] == [[(64, "lds", 4)], [(128, "bigq", 8), (2, "bigq", 8)]]
    h = None
    try:
        for B in s.batches:
            X = pr.planted(s.n, s.d, np_dtype, metric, B, "range").X
            h = _shard(X, metric)
            _walk(h, "d128_range", np_dtype, metric, B, "range", f"range {np.dtype(np_dtype).name} {METRIC_NAME[metric]} g{group_rows}")
            h.close()
            h = None
    finally:
        if h is not None:
            h.close()


# ---- d = 768, fp16: the one-block-per-CU LDS scan and every 256-query pass ---------------------------------------------
KERNELS_768 = {0: "qreg", 16: "q64", 8: "gemm", 1 | 2: "bigq"}


@pytest.mark.parametrize("variant", ["plain", "mask"])
@pytest.mark.parametrize("group_rows", [16, 64])
@pytest.mark.parametrize("metric", [pr.COSINE, pr.IP], ids=lambda m: METRIC_NAME[m])
@pytest.mark.parametrize("kernels_mask", sorted(KERNELS_768), ids=lambda m: KERNELS_768[m])
def test_256_query_passes_walk(gpu, options, kernels_mask, metric, group_rows, variant):
    """B = 256 and 300 under HR_DEBUG_DENSE_KERNELS 0 (register-resident pass), 16 (its 4 x 64-query form), 8 (tiled
    contraction), 1|2 (two 128-query passes); the <= 128 tail of B = 300 takes the 128-query pass.  With the default
    selection also B = 64: a 96 KiB query tile, the 512-thread, one-block-per-CU form of the LDS scan."""
    s = pr.SHARDS["d768"]
    options(nat.HR_DEBUG_GROUP_ROWS, group_rows)
    options(nat.HR_DEBUG_DENSE_KERNELS, kernels_mask)
    kern = KERNELS_768[kernels_mask]
    assert passes(s.d, np.float16, metric, 64, kernels_mask) == [(64, "lds", 4)]
    if kern == "bigq":
        assert passes(s.d, np.float16, metric, 256, kernels_mask) == [(128, "bigq", 8)] * 2
        assert passes(s.d, np.float16, metric, 300, kernels_mask) == [(128, "bigq", 8)] * 2 + [(44, "bigq", 8)]
    else:
        assert passes(s.d, np.float16, metric, 256, kernels_mask) == [(256, kern, 16)]
        assert passes(s.d, np.float16, metric, 300, kernels_mask) == [(256, kern, 16), (44, "bigq", 8)]
    h = None
    try:
        for B in s.batches:
            if B == 64 and kernels_mask != 0:
                continue                                       # the LDS scan does not depend on the 256-query selection
            X = pr.planted(s.n, s.d, np.float16, metric, B, variant).X
            h = _shard(X, metric)
            _walk(h, "d768", np.float16, metric, B, variant, f"d768 {kern} {METRIC_NAME[metric]} g{group_rows} {variant}")
            h.close()
            h = None
    finally:
        if h is not None:
            h.close()


def test_tiled_contraction_walks_at_32_tiles_per_row(gpu, options):
    """d = 1024 (KT = 32): no register-resident form, B = 256 takes the tiled contraction; 26 row tiles, the last one with
    a single group of four row blocks."""
    s = pr.SHARDS["d1024"]
    options(nat.HR_DEBUG_GROUP_ROWS, 16)
    assert passes(s.d, np.float16, pr.COSINE, 256) == [(256, "gemm", 16)]
    h = _shard(pr.planted(s.n, s.d, np.float16, pr.COSINE, 256, "plain").X, pr.COSINE)
    try:
        _walk(h, "d1024", np.float16, pr.COSINE, 256, "plain", "d1024 gemm")
    finally:
        h.close()


@pytest.mark.parametrize("metric", [pr.IP, pr.L2], ids=lambda m: METRIC_NAME[m])
def test_k_chunked_pass_walks_rows_too_long_for_the_tile(gpu, options, metric):
    """d = 3000, fp32 (KT = 188 > 156): no query tile fits LDS, every batch — one query too — takes the 128-query pass."""
    s = pr.SHARDS["d3000"]
    assert [passes(s.d, np.float32, metric, B) for B in s.batches] == [[(1, "bigq", 8)], [(20, "bigq", 8)]]
    h = None
    try:
        for B in s.batches:
            h = _shard(pr.planted(s.n, s.d, np.float32, metric, B, "plain").X, metric)
            _walk(h, "d3000", np.float32, metric, B, "plain", f"d3000 {METRIC_NAME[metric]}")
            h.close()
            h = None
    finally:
        if h is not None:
            h.close()


# ---- hr_set_scan_cus itself --------------------------------------------------------------------------------------------
def test_set_scan_cus_contract(gpu, options):
    """A negative value is refused (HR_EINVAL -> ValueError) and leaves the setting alone; a value above the device's CU
    count behaves as 0; the setting applies to the next search without a new finalize.  The setting has no read-back, and
    results do not depend on it (that is the point of this file), so it is observed the way the pipelined engine relies
    on it: the scan of a 256-query batch over 101 super-groups runs as ONE block at one CU and as 101 blocks by default —
    one block streams the shard through a single CU's LDS, more than ten times slower; the assertion asks for three, on
    the FASTEST of five launches each (a launch delayed by a neighbour on a shared device does not decide it)."""
    import torch
    s = pr.SHARDS["d768"]
    p, _, want1, _ = _expect("d768", np.float16, pr.COSINE, 256, "plain")
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    h = _shard(p.X, pr.COSINE)
    dev = _Device(p)
    try:
        h.set_profiling(1)

        def scan_ms():
            best = np.inf
            for _ in range(5):
                h.kernel_ms()
                ids, sc, _ = dev.search(h, 1)
                assert np.array_equal(ids, want1[0]) and np.array_equal(bits(sc), bits(want1[1]))
                ms, launches = h.kernel_ms()["dense_scan"]
                assert launches == 1
                best = min(best, ms)
            return best

        scan_ms()                                              # first launches
        default = scan_ms()
        h.set_scan_cus(1)                                      # no finalize in between: the next search is a one-block scan
        one = scan_ms()
        assert one > 3 * default, (one, default)
        for bad in (-1, -2 ** 31):
            with pytest.raises(ValueError, match="n_cus"):
                h.set_scan_cus(bad)
        still_one = scan_ms()                                  # the refused calls left the setting at 1
        assert still_one > 3 * default, (still_one, default)
        for beyond in (cu_count + 1, 2 ** 31 - 1):
            h.set_scan_cus(beyond)                             # as 0: every CU
            assert 3 * scan_ms() < one
        h.set_scan_cus(1)
        h.set_scan_cus(0)
        assert 3 * scan_ms() < one
        h.set_scan_cus(cu_count)                               # exactly the device's count: the default grid as well
        assert 3 * scan_ms() < one
    finally:
        h.close()


# ---- the sparse side: the automatic ranges-per-block depend on scan_cus -------------------------------------------------
def test_sparse_scan_on_one_cu_matches_the_oracle_and_the_default_grid(gpu, options):
    """6 001 documents, V = 3 000, 70 queries.  The shard is ONE doc range (a range is 16 384 documents), so this does not
    make a block walk several real ranges: what set_scan_cus(1) changes is the automatic ranges-per-block, 1 by default
    and 5 (70 / 12) at one CU, i.e. a block whose walk is cut short at the shard's last range.  Host and device form at
    set_scan_cus(1) against the oracle and, bit for bit, against set_scan_cus(0).  (Several real ranges per block:
    HR_DEBUG_SPARSE_RPB in test_gpu_kernel_variants.py.)"""
    import torch
    from advanced_rag.engine import pack_sparse_queries
    rng = np.random.default_rng(6001)
    V, nd, B = 3000, 6001, 70
    idx = [np.sort(rng.choice(V, size=rng.integers(1, 60), replace=False)).astype(np.int32) for _ in range(nd)]
    val = [np.abs(rng.standard_normal(len(i))).astype(np.float32) + 0.01 for i in idx]
    indptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    idx, val = np.concatenate(idx), np.concatenate(val)
    qs = [(np.sort(rng.choice(V, size=12, replace=False)).astype(np.int32), np.abs(rng.standard_normal(12)).astype(np.float32))
          for _ in range(B)]
    keep = np.packbits(rng.random(nd) < 0.5, bitorder="little")
    ptr, qi, qv, mx = pack_sparse_queries(qs, 0.0)
    d_ptr, d_qi, d_qv = (torch.from_numpy(a).cuda() for a in (ptr, qi, qv))
    d_keep = torch.from_numpy(pr.device_mask(keep, nd)).cuda()
    h = nat.ShardHandle(0, sparse_dim=V)
    h.add_sparse(indptr, idx, val)
    h.finalize()
    try:
        for mask, d_mask in ((None, 0), (keep, d_keep.data_ptr())):
            want = oracle.sparse_search(indptr, idx, val, qs, K, 0.0, mask)
            seen = {}
            for cus in (0, 1):
                h.set_scan_cus(cus)
                ids, sc = h.search_sparse(qs, K, 0.0, mask)
                assert np.array_equal(ids, want[0]) and np.array_equal(bits(sc), bits(want[1])), f"host, cus={cus}"
                d_ids = torch.full((B, K), -5, dtype=torch.int64, device="cuda")
                d_sc = torch.full((B, K), -5.0, dtype=torch.float32, device="cuda")
                d_fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
                st = torch.cuda.current_stream()
                h.search_sparse_dev(d_ptr.data_ptr(), d_qi.data_ptr(), d_qv.data_ptr(), B, len(qi), mx, K, d_ids.data_ptr(),
                                    d_sc.data_ptr(), d_fl.data_ptr(), d_mask, st.cuda_stream)
                st.synchronize()
                ids, sc, fl = d_ids.cpu().numpy(), d_sc.cpu().numpy(), d_fl.cpu().numpy()
                assert set(np.unique(fl).tolist()) <= {0, 1}
                proven = fl == 1
                assert np.array_equal(ids[proven], want[0][proven]) and np.array_equal(bits(sc[proven]), bits(want[1][proven])), f"device, cus={cus}"
                print(f"sparse, cus={cus}, mask={'yes' if mask is not None else 'no'}: {int(proven.sum())} of {B} device lists proven")
                assert proven.any(), f"device, cus={cus}: no list proven, the comparison with the oracle checked nothing"
                seen[cus] = (ids, sc, fl)
            assert np.array_equal(seen[1][0], seen[0][0]) and np.array_equal(bits(seen[1][1]), bits(seen[0][1]))
            assert np.array_equal(seen[1][2], seen[0][2])
    finally:
        h.close()
