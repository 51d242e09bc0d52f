"""The candidate scans' exactness proofs on adversarial inputs.

Every list the library returns rests on one claim: the scan's error bound proves that no row outside the refined
candidate groups can enter the top k, and the select kernel then sets the list's flag to 1.  The host forms only widen
the candidate set when a flag is 0, the engine and the multi-rank merge trust the flags as they are.  These tests hold
that claim to the oracle where it is easiest to get wrong: signed sparse weights (a posting's fp16 rounding error scales
with |w·d|, not with the score), fixed-point scales outside the fp32 range, fp16 collisions and near-ties at the cut,
fp16 subnormals, and the whole dense dimension envelope.

Each case runs three ways: the host form (ids and score bits equal to the oracle's), the device form (every list with
flag 1 equal to the oracle bit for bit; flag 0 where a case is built so that the bound cannot decide it), and, where it
is cheap, under the finishing / trim / group-size debug options."""
import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.engine import EngineConfig, HybridSearchEngine, pack_sparse_queries

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HR_MAX_QUERY_NNZ = 4096   # include/hbmrag.h

# (key, value) settings each sparse case is repeated under: the default path, the multi-launch chain, the fused finishing
# kernel, no candidate trim, and both candidate-group sizes (HR_DEBUG_GROUP_ROWS applies to handles created afterwards)
VARIANTS = [(), ((nat.HR_DEBUG_FINISH_MODE, 1),), ((nat.HR_DEBUG_FINISH_MODE, 2),), ((nat.HR_DEBUG_NO_TRIM, 1),),
            ((nat.HR_DEBUG_GROUP_ROWS, 16),), ((nat.HR_DEBUG_GROUP_ROWS, 64), (nat.HR_DEBUG_FINISH_MODE, 2))]
DEBUG_KEYS = (nat.HR_DEBUG_DENSE_KERNELS, nat.HR_DEBUG_SPARSE_RPB, nat.HR_DEBUG_GROUP_ROWS, nat.HR_DEBUG_FINISH_MODE,
              nat.HR_DEBUG_NO_TRIM)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def options():
    def set_(settings):
        for key in DEBUG_KEYS:
            nat.debug_option(key, 0)
        for key, value in settings:
            nat.debug_option(key, value)
    yield set_
    for key in DEBUG_KEYS:
        nat.debug_option(key, 0)


def csr(rows):
    """rows: list of dicts {term: weight} -> (indptr int64, idx int32, val float32)."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    idx, val = [], []
    for r, row in enumerate(rows):
        for t in sorted(row):
            idx.append(t)
            val.append(row[t])
        indptr[r + 1] = len(idx)
    return indptr, np.asarray(idx, np.int32), np.asarray(val, np.float32)


def sparse_shard(V, indptr, idx, val):
    h = nat.ShardHandle(0, sparse_dim=V)
    h.add_sparse(indptr, idx, val)
    h.finalize()
    return h


def sparse_dev(h, queries, k, drop=0.0):
    """Device form (queries reduced and packed on the host): ids, scores, flags as numpy."""
    ptr, qi, qv, mx = pack_sparse_queries(queries, drop, h.sparse_dim)
    B = len(queries)
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(ptr).to(dev)
    ti = torch.from_numpy(qi if qi.size else np.zeros(1, np.int32)).to(dev)
    tv = torch.from_numpy(qv if qv.size else np.zeros(1, np.float32)).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    sc = torch.empty((B, k), dtype=torch.float32, device=dev)
    fl = torch.full((B,), 7, dtype=torch.int32, device=dev)
    h.search_sparse_dev(tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), B, int(ptr[-1]), max(mx, 1), k, ids.data_ptr(),
                        sc.data_ptr(), fl.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def check_sparse(h, indptr, idx, val, queries, k, drop=0.0, unproven=()):
    """Host form == oracle; device form sound (flag 1 => == oracle); flag 0 on the queries listed in `unproven`.
    Returns the device flags."""
    oids, osc = oracle.sparse_search(indptr, idx, val, queries, k, drop)
    ids, sc = h.search_sparse(queries, k, drop)
    assert np.array_equal(ids, oids), (ids[:, :8], oids[:, :8])
    assert np.array_equal(bits(sc), bits(osc))
    dids, dsc, fl = sparse_dev(h, queries, k, drop)
    assert set(np.unique(fl)) <= {0, 1}, fl
    for b in range(len(queries)):
        if fl[b]:
            assert np.array_equal(dids[b], oids[b]) and np.array_equal(bits(dsc[b]), bits(osc[b])), \
                f"query {b}: list flagged proven exact differs from the oracle: {dids[b][:8]} vs {oids[b][:8]}"
    for b in unproven:
        assert fl[b] == 0, f"query {b}: the scan bound cannot decide this list, yet it was flagged proven"
    return fl


def run_variants(options, build, body):
    """build() -> (h, indptr, idx, val) under each debug setting; body(h, indptr, idx, val)."""
    for v in VARIANTS:
        options(v)
        h, indptr, idx, val = build()
        try:
            body(h, indptr, idx, val)
        except AssertionError as e:
            raise AssertionError(f"debug options {v}: {e}") from e
        finally:
            h.close()


# ------------------------------------------------------------------------------------------------------ sparse
def s1_rows(n=40000):
    """Term 3 at 0.1 everywhere but rows 20000..20063; row 5 at 0.2; row 20000 = {1: 1000.24, 2: 1000.0}, whose score
    against {1: +1, 2: -1, 3: +1} is 0.24 in fp32 but ~0 after fp16 rounding of the postings (1000.24 -> 1000)."""
    rows = [{3: 0.1} for _ in range(n)]
    for r in range(20000, 20064):
        rows[r] = {}
    rows[20000] = {1: 1000.24, 2: 1000.0}
    rows[5] = {3: 0.2}
    return rows


S1_QUERY = (np.array([1, 2, 3], np.int32), np.array([1.0, -1.0, 1.0], np.float32))


@pytest.mark.parametrize("k", [1, 5, 20])
def test_s1_signed_cancellation_hides_the_best_row(gpu, options, k):
    def build():
        indptr, idx, val = csr(s1_rows())
        return sparse_shard(64, indptr, idx, val), indptr, idx, val

    def body(h, indptr, idx, val):
        oids, _ = oracle.sparse_search(indptr, idx, val, [S1_QUERY], k)
        assert oids[0, 0] == 20000
        check_sparse(h, indptr, idx, val, [S1_QUERY], k, unproven=(0,))
    run_variants(options, build, body)


def signed_family(rng, n, V, nnz, doc_sign, q_sign, B=6, q_nnz=12):
    idx = np.sort(np.argpartition(rng.random((n, V)), nnz - 1, axis=1)[:, :nnz], axis=1).astype(np.int32).reshape(-1)
    mag = np.abs(rng.standard_normal(n * nnz)).astype(np.float32) + 0.01
    val = (mag * doc_sign(rng, n * nnz)).astype(np.float32)
    indptr = np.arange(n + 1, dtype=np.int64) * nnz
    qs = []
    for _ in range(B):
        qi = np.sort(rng.choice(V, size=q_nnz, replace=False)).astype(np.int32)
        qv = (np.abs(rng.standard_normal(q_nnz)) + 0.05) * q_sign(rng, q_nnz)
        qs.append((qi, qv.astype(np.float32)))
    return indptr, idx, val, qs


POS = lambda rng, m: np.ones(m)  # noqa: E731
NEG = lambda rng, m: -np.ones(m)  # noqa: E731
MIX = lambda rng, m: np.where(rng.random(m) < 0.5, -1.0, 1.0)  # noqa: E731
SOME_NEG = lambda rng, m: np.where(rng.random(m) < 0.25, -1.0, 1.0)  # noqa: E731


@pytest.mark.parametrize("family", ["signed_docs_signed_queries", "positive_docs_some_negative_terms",
                                    "negative_docs_positive_queries", "all_negative_query"])
def test_s2_random_signed_families(gpu, options, family):
    doc_sign, q_sign = {"signed_docs_signed_queries": (MIX, MIX), "positive_docs_some_negative_terms": (POS, SOME_NEG),
                        "negative_docs_positive_queries": (NEG, POS), "all_negative_query": (POS, NEG)}[family]
    rng = np.random.default_rng(len(family))
    indptr, idx, val, qs = signed_family(rng, 30000, 400, 8, doc_sign, q_sign)
    # plus the hidden-row construction of S1, appended: one query of the batch depends on it
    extra = [{1: 1000.24, 2: 1000.0}] + [{} for _ in range(63)]
    e_ptr, e_idx, e_val = csr(extra)
    indptr = np.concatenate([indptr, e_ptr[1:] + indptr[-1]])
    idx, val = np.concatenate([idx, e_idx]), np.concatenate([val, e_val])
    qs.append(S1_QUERY)

    def body(h, indptr_, idx_, val_):
        for k in (1, 10, 40):
            check_sparse(h, indptr_, idx_, val_, qs, k)
    run_variants(options, lambda: (sparse_shard(400, indptr, idx, val), indptr, idx, val), body)
    if family == "all_negative_query":
        oids, _ = oracle.sparse_search(indptr, idx, val, qs[:-1], 10)
        assert (oids == -1).all()


def test_s3_fewer_than_k_positive_rows_with_signed_weights(gpu, options):
    """Three rows score above 0 in the scan's eyes, a fourth (the S1 row) only in fp32: k = 10 must not be proven
    by the 'nothing outside can qualify' shortcut."""
    n = 20000
    rows = [{3: -0.5} for _ in range(n)]
    for r in (7, 9000, 15000):
        rows[r] = {3: 0.3}
    for r in range(12000, 12064):
        rows[r] = {}
    rows[12000] = {1: 1000.24, 2: 1000.0}
    indptr, idx, val = csr(rows)

    def body(h, indptr_, idx_, val_):
        for k in (5, 10, 40):
            oids, _ = oracle.sparse_search(indptr_, idx_, val_, [S1_QUERY], k)
            assert set(oids[0][oids[0] >= 0]) == {7, 9000, 15000, 12000}
            check_sparse(h, indptr_, idx_, val_, [S1_QUERY, (np.array([3], np.int32), np.array([1.0], np.float32))], k,
                         unproven=(0,))
    run_variants(options, lambda: (sparse_shard(64, indptr, idx, val), indptr, idx, val), body)


def test_s4_unsigned_fp16_collisions_at_the_cut(gpu, options):
    """200 rows in 200 groups whose weights differ in fp32 but all round to 1000.0 in fp16: the cut falls among them, the
    device cannot prove the list, the host form escalates to the exact answer."""
    rng = np.random.default_rng(4)
    n = 40000
    rows = [{5: float(rng.uniform(0.1, 1.0))} for _ in range(n)]
    w = 1000.0 + rng.uniform(-0.24, 0.24, 200)
    for i in range(200):
        rows[64 * i + 3] = {5: float(w[i])}
    indptr, idx, val = csr(rows)
    assert np.all(val.astype(np.float16)[indptr[[64 * i + 3 for i in range(200)]]] == np.float16(1000.0))
    q = [(np.array([5], np.int32), np.array([1.0], np.float32))]

    def body(h, indptr_, idx_, val_):
        for k in (5, 40):
            check_sparse(h, indptr_, idx_, val_, q, k, unproven=(0,))
    run_variants(options, lambda: (sparse_shard(16, indptr, idx, val), indptr, idx, val), body)


@pytest.mark.parametrize("case", ["docs_60000", "docs_1e-9", "docs_signed_1e-9", "query_1e-6_to_1e6", "max_query_nnz"])
def test_s5_magnitude_extremes(gpu, options, case):
    rng = np.random.default_rng(5)
    V, n = 500, 20000
    if case == "max_query_nnz":
        V, n = HR_MAX_QUERY_NNZ + 100, 3000
    indptr, idx, val, qs = signed_family(rng, n, V, 10, POS if case in ("docs_1e-9", "query_1e-6_to_1e6") else MIX,
                                         SOME_NEG if case != "query_1e-6_to_1e6" else POS)
    if case == "docs_60000":
        val = np.where(rng.random(val.size) < 0.5, np.sign(val) * 60000.0, val).astype(np.float32)
    elif case in ("docs_1e-9", "docs_signed_1e-9"):
        val = (np.sign(val) * rng.uniform(1e-9, 3e-9, val.size)).astype(np.float32)
        assert np.all(np.abs(val.astype(np.float16)) == 0)  # below fp16: stored as the smallest subnormal
    elif case == "query_1e-6_to_1e6":
        qs = [(qi, (10.0 ** rng.uniform(-6, 6, qi.size)).astype(np.float32)) for qi, _ in qs]
    else:
        # rows that hold every query term at the largest weight the shard accepts: the fixed-point sums reach the top of
        # their int32 headroom
        qi = np.arange(HR_MAX_QUERY_NNZ, dtype=np.int32)
        full = [{int(t): 60000.0 for t in qi} for _ in range(3)]
        f_ptr, f_idx, f_val = csr(full)
        indptr = np.concatenate([indptr, f_ptr[1:] + indptr[-1]])
        idx, val = np.concatenate([idx, f_idx]), np.concatenate([val, f_val])
        qs = [(qi, np.full(qi.size, 60000.0, np.float32)), (qi, np.abs(rng.standard_normal(qi.size)).astype(np.float32)),
              (qi, (rng.standard_normal(qi.size) * 100).astype(np.float32))]

    def body(h, indptr_, idx_, val_):
        for k in (1, 40):
            check_sparse(h, indptr_, idx_, val_, qs, k)
    run_variants(options, lambda: (sparse_shard(V, indptr, idx, val), indptr, idx, val), body)


@pytest.mark.parametrize("direction", ["overflow", "underflow"])
def test_s6_fixed_point_scale_out_of_range(gpu, options, direction):
    """sum|w_q| * max|doc w| beyond the fp32 range (scale 0) or below 2^30 / FLT_MAX (scale inf): the scan learns
    nothing, so no list may be proven; the host form still returns the oracle's list."""
    rng = np.random.default_rng(6)
    n, V = 20000, 64
    rows = [{int(t): float(rng.uniform(0.5, 1.0)) for t in rng.choice(8, 2, replace=False)} for _ in range(n)]
    rows[n - 1] = {40: 60000.0}                     # max |doc w| of the shard, on a term no query holds
    indptr, idx, val = csr(rows)
    qw = 1e34 if direction == "overflow" else 1e-35
    qs = [(np.array([0, 1, 2], np.int32), np.array([qw, 2 * qw, 0.5 * qw], np.float32)),
          (np.array([3, 5], np.int32), np.array([qw, qw], np.float32))]
    if direction == "underflow":
        rows[n - 1] = {40: 1.0}
        indptr, idx, val = csr(rows)

    def body(h, indptr_, idx_, val_):
        for k in (1, 40):
            check_sparse(h, indptr_, idx_, val_, qs, k, unproven=(0, 1))
    run_variants(options, lambda: (sparse_shard(V, indptr, idx, val), indptr, idx, val), body)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_s7_non_finite_query_values_are_refused(gpu, bad):
    indptr, idx, val = csr([{1: 1.0}, {2: 2.0}])
    h = sparse_shard(8, indptr, idx, val)
    q = [(np.array([1, 2], np.int32), np.array([1.0, bad], np.float32))]
    with pytest.raises(ValueError):
        h.search_sparse(q, 2)
    with pytest.raises(ValueError):
        h.search_sparse(q, 2, 0.5)              # refused before drop_ratio is applied
    with pytest.raises(ValueError):
        pack_sparse_queries(q, 0.0, 8)
    h.close()
    X = np.ones((40, 16), np.float32)
    for dtype in (nat.HR_F16, nat.HR_F32):
        for metric in (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE):
            hd = nat.ShardHandle(16, dtype, metric)
            hd.add_dense(X)
            hd.finalize()
            Q = np.ones((3, 16), np.float32)
            Q[1, 7] = bad
            with pytest.raises(ValueError):
                hd.search_dense(Q, 5)
            d_mask = torch.full((8,), 255, dtype=torch.uint8, device="cuda")
            with pytest.raises(ValueError):
                hd.search_dense(Q, 5, d_rowmask=d_mask.data_ptr())
            hd.close()


def test_s8_drop_ratio_with_signed_values_of_equal_magnitude(gpu, options):
    qi = np.array([10, 3, 7, 1, 12, 5, 9, 0], np.int32)
    qv = np.array([0.5, -0.5, 0.25, -0.25, 1.0, -1.0, 0.25, 2.0], np.float32)
    rng = np.random.default_rng(8)
    rows = [{int(t): float(rng.uniform(0.1, 1.0)) for t in rng.choice(16, 3, replace=False)} for _ in range(5000)]
    indptr, idx, val = csr(rows)
    for drop in (0.125, 0.25, 0.5, 0.75):
        ptr, pi, pv, _ = pack_sparse_queries([(qi, qv)], drop, 16)
        oi, ov = oracle.drop_query(qi, qv, drop)
        order = np.argsort(oi, kind="stable")
        assert np.array_equal(pi, oi[order]) and np.array_equal(bits(pv), bits(ov[order])), drop

    def body(h, indptr_, idx_, val_):
        for drop in (0.125, 0.25, 0.5, 0.75):
            check_sparse(h, indptr_, idx_, val_, [(qi, qv), (qi[::-1].copy(), qv[::-1].copy())], 10, drop)
    run_variants(options, lambda: (sparse_shard(16, indptr, idx, val), indptr, idx, val), body)


def test_s9_hybrid_engine_and_snapshot_of_a_signed_shard(gpu, tmp_path):
    rng = np.random.default_rng(9)
    n, d, V = 40000, 64, 64
    rows = s1_rows(n)
    for r in range(0, n, 7):
        if not (20000 <= r < 20064):
            rows[r] = {3: 0.1, int(rng.integers(4, 64)): float(rng.uniform(-1, 1))}
    indptr, idx, val = csr(rows)
    X = rng.standard_normal((n, d)).astype(np.float16)
    SQ = [S1_QUERY, (np.array([3, 9, 20], np.int32), np.array([1.0, -0.5, 0.7], np.float32)),
          (np.array([3, 40], np.int32), np.array([0.3, 1.0], np.float32))]
    Q = rng.standard_normal((len(SQ), d)).astype(np.float32)
    h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    h.add_dense(X)
    h.add_sparse(indptr, idx, val)
    h.finalize()
    cfg = EngineConfig(top_k=20)
    eng = HybridSearchEngine(h, cfg)
    out = eng.search(torch.from_numpy(Q).cuda(), eng.upload_sparse(pack_sparse_queries(SQ, 0.0, V)))
    torch.cuda.synchronize()
    kp = 2 * cfg.top_k
    osi, oss = oracle.sparse_search(indptr, idx, val, SQ, kp)
    flags = out["flags"].cpu().numpy()
    si = out["ids"][1].cpu().numpy()
    for b in range(len(SQ)):
        if flags[1, b]:
            assert np.array_equal(si[b], osi[b]), b
    assert flags[1, 0] == 0
    eng.resolve_inexact(out, Q, SQ, 0.0)
    torch.cuda.synchronize()
    assert np.array_equal(out["ids"][1].cpu().numpy(), osi)
    # snapshot round trip: the loaded shard must know that it holds negative weights
    path = str(tmp_path / "signed.snap")
    h.save(path)
    h.close()
    h2 = nat.ShardHandle.load(path, d, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    check_sparse(h2, indptr, idx, val, SQ, 5, unproven=(0,))
    h2.close()


# ------------------------------------------------------------------------------------------------------- dense
def dense_dev(h, Q, k):
    B = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    h.search_dense_dev(q.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), 0,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def check_dense(h, X, Q, k, metric, pick=None, unproven=()):
    """Host form == oracle on the queries `pick` (all by default), device form sound on them."""
    pick = list(range(Q.shape[0])) if pick is None else sorted(set(pick))
    oids, osc = oracle.dense_search(X, Q[pick], k, metric)
    ids, sc = h.search_dense(Q, k)
    assert np.array_equal(ids[pick], oids), (ids[pick][:, :6], oids[:, :6])
    assert np.array_equal(bits(sc[pick]), bits(osc))
    dids, dsc, fl = dense_dev(h, Q, k)
    assert set(np.unique(fl)) <= {0, 1}, fl
    for j, b in enumerate(pick):
        if fl[b]:
            assert np.array_equal(dids[b], oids[j]) and np.array_equal(bits(dsc[b]), bits(osc[j])), \
                f"query {b}: list flagged proven exact differs from the oracle"
    for b in unproven:
        assert fl[b] == 0, f"query {b}: flagged proven although the bound cannot decide it"
    return fl


D1_DIMS = [8, 100, 1000, 1536, 2048, 2560, 2592, 3000, 4096]


def d1_batches(h_dim, dtype):
    """B values that cross the routing boundaries of the dense scan: 1, 16 * Gsmall (the largest batch one LDS-resident
    pass serves), one more, 129 and 256 (the 256-query passes)."""
    tile = 16 if dtype == nat.HR_F32 else 32
    KT = -(-(-(-h_dim // tile)) // 4) * 4
    g_small = max(1, min(4, 156 // KT))
    return sorted({1, 16 * g_small, 16 * g_small + 1, 129, 256})


@pytest.mark.parametrize("dtype", [nat.HR_F32, nat.HR_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", [nat.HR_METRIC_IP, nat.HR_METRIC_COSINE], ids=["ip", "cosine"])
def test_d1_dimension_envelope(gpu, dtype, metric):
    rng = np.random.default_rng(dtype * 2 + metric)
    n = 3000
    for i, d in enumerate(D1_DIMS):
        X = rng.standard_normal((n, d)).astype(np.float32)
        if dtype == nat.HR_F16:
            X = X.astype(np.float16)
        X[n // 2] = X[11]                              # an exact duplicate: ties broken by row id
        h = nat.ShardHandle(d, dtype, metric)
        h.add_dense(X)
        h.finalize()
        for j, B in enumerate(d1_batches(d, dtype)):
            k = (1, 40, 256)[(i + j) % 3]
            Q = rng.standard_normal((B, d)).astype(np.float32)
            Q[0] = X[11]
            try:
                check_dense(h, X, Q, k, metric, pick=[0, B // 2, B - 1])
            except AssertionError as e:
                raise AssertionError(f"d={d} B={B} k={k}: {e}") from e
        h.close()


@pytest.mark.parametrize("d", [2048, 4096])
def test_d1_kernel_masks_at_large_dimensions(gpu, options, d):
    rng = np.random.default_rng(d)
    n = 2500
    X = rng.standard_normal((n, d)).astype(np.float16)
    h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_COSINE)
    h.add_dense(X)
    h.finalize()
    for mask in (1, 2, 4, 8, 16):
        options(((nat.HR_DEBUG_DENSE_KERNELS, mask),))
        for B in (1, 129, 256):
            Q = rng.standard_normal((B, d)).astype(np.float32)
            try:
                check_dense(h, X, Q, 40, nat.HR_METRIC_COSINE, pick=[0, B - 1])
            except AssertionError as e:
                raise AssertionError(f"mask={mask} B={B}: {e}") from e
    h.close()


@pytest.mark.parametrize("dtype", [nat.HR_F32, nat.HR_F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", [nat.HR_METRIC_IP, nat.HR_METRIC_COSINE], ids=["ip", "cosine"])
def test_d2_fp16_subnormal_components(gpu, dtype, metric):
    rng = np.random.default_rng(22)
    d, n = 2048, 4000
    # queries: one large component, the other ~1500 around 1e-5 (fp16 subnormals after normalisation)
    Q = np.zeros((4, d), np.float32)
    Q[:, 0] = 1.0
    Q[:, 1:1501] = (rng.uniform(0.5, 1.5, (4, 1500)) * 1e-5).astype(np.float32)
    Q[1:, 1:1501] *= np.where(rng.random((3, 1500)) < 0.5, -1, 1)
    # rows: mass on exactly those dimensions, none on the large one
    X = np.zeros((n, d), np.float32)
    X[:, 1:1501] = rng.standard_normal((n, 1500)).astype(np.float32)
    X[:100, 0] = 1e-3 * rng.standard_normal(100)
    if dtype == nat.HR_F16:
        X = X.astype(np.float16)
    h = nat.ShardHandle(d, dtype, metric)
    h.add_dense(X)
    h.finalize()
    for k in (1, 40):
        check_dense(h, X, Q, k, metric)
    h.close()
    if metric == nat.HR_METRIC_COSINE:
        # rows made only of fp16 subnormals
        Xs = (rng.standard_normal((n, 256)) * 3e-6).astype(np.float16)
        Xs = Xs if dtype == nat.HR_F16 else Xs.astype(np.float32)
        assert np.all(np.abs(Xs.astype(np.float32)) < 6.2e-5)
        hs = nat.ShardHandle(256, dtype, metric)
        hs.add_dense(Xs)
        hs.finalize()
        Qs = rng.standard_normal((5, 256)).astype(np.float32)
        for k in (1, 40):
            check_dense(hs, Xs, Qs, k, metric)
        hs.close()


@pytest.mark.parametrize("dtype", [nat.HR_F32, nat.HR_F16], ids=["fp32", "fp16"])
def test_d3_near_ties_at_the_cut(gpu, dtype):
    rng = np.random.default_rng(33)
    d, n = 64, 30000
    X = rng.standard_normal((n, d)).astype(np.float32) * 0.3
    proto = rng.standard_normal(d).astype(np.float32)
    # 300 rows, each in a group of its own, whose scores against `proto` differ by far less than the scan's bound
    near = np.arange(300) * 64 + 5
    step = np.float32(2.0 ** -8) if dtype == nat.HR_F16 else np.float32(1e-6)
    for i, r in enumerate(near):
        X[r] = proto
        X[r, i % d] += step * (1 + i // d)
    # and rows whose fp64 scores differ but whose fp32 scores are equal: ties broken by row id
    tie = np.arange(300) * 64 + 40
    for i, r in enumerate(tie):
        X[r] = proto
        X[r, 3] += np.float32(1e-12) * i
    if dtype == nat.HR_F16:
        X = X.astype(np.float16)
    for metric in (nat.HR_METRIC_COSINE, nat.HR_METRIC_IP):
        h = nat.ShardHandle(d, dtype, metric)
        h.add_dense(X)
        h.finalize()
        Q = np.stack([proto, proto * 3, rng.standard_normal(d).astype(np.float32)])
        for k in (1, 40, 256):
            fl = check_dense(h, X, Q, k, metric)
            if k == 40 and metric == nat.HR_METRIC_COSINE:
                # the cut falls among hundreds of groups whose cosines differ (second order in the perturbation) far less
                # than the bound
                assert fl[0] == 0 and fl[1] == 0, fl
        h.close()


def test_d4_append_raises_the_inner_product_bound(gpu):
    rng = np.random.default_rng(44)
    d, n = 64, 20000
    for dtype in (nat.HR_F16, nat.HR_F32):
        X = rng.standard_normal((n, d)).astype(np.float32)
        X = X.astype(np.float16) if dtype == nat.HR_F16 else X
        h = nat.ShardHandle(d, dtype, nat.HR_METRIC_IP)
        h.add_dense(X)
        h.finalize()
        Q = rng.standard_normal((4, d)).astype(np.float32)
        check_dense(h, X, Q, 40, nat.HR_METRIC_IP)
        big = np.full((1, d), 60000.0, np.float32)
        big[0, ::2] = -60000.0
        big = big.astype(np.float16) if dtype == nat.HR_F16 else big
        h.add_dense(big)
        h.finalize()
        X2 = np.concatenate([X, big])
        Q2 = np.concatenate([Q, big.astype(np.float32) / 60000.0, -big.astype(np.float32) / 60000.0])
        for k in (1, 40):
            check_dense(h, X2, Q2, k, nat.HR_METRIC_IP)
        h.close()
