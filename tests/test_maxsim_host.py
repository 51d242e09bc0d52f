"""Late interaction without a GPU: the numpy restatement against an exactly rounded scalar one, the spec object, the
token-vector column, save / load, and search(ranker=MaxSimRanker) / retrieve(late_interaction=True) on the manager over
oracle-backed stand-ins for the shard handles (the setup of test_sparse_query_host.py)."""
import asyncio
import struct
from fractions import Fraction

import numpy as np
import pytest

import test_sparse_query_host as sq
from advanced_rag import HybridRetriever, RetrievalConfig
from advanced_rag import _native as nat
from advanced_rag import maxsim as M
from advanced_rag.columns import PayloadColumns, TokenVectorColumn
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.maxsim import MaxSimRanker
from advanced_rag.pipeline import PipelineConfig
from advanced_rag.retrieval import rrf_rank_lists

TD = 16      # token dim of the stand-in managers


# ---- the restatement against exact arithmetic ---------------------------------------------------------------------------
def _round_f32(x: Fraction) -> float:
    """x rounded to the nearest float32, ties to even, by exact rational arithmetic (no overflow occurs in these tests)."""
    if x == 0:
        return 0.0
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                    # 2^e <= a < 2^(e+1)
    q = max(e, -126) - 23                         # the spacing of float32 at a (subnormals: 2^-149)
    scaled = a / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return sign * float(Fraction(n) * Fraction(2) ** q)


def _exact_chain(q, d) -> float:
    """acc = fmaf(q[k], d[k], acc) for k ascending, every fma rounded once from the exact value."""
    acc = 0.0
    for a, b in zip(q, d):
        acc = _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(acc))
        assert struct.unpack("f", struct.pack("f", acc))[0] == acc
    return acc


def _scalar_score(q, doc) -> float:
    S = 0.0
    for t in range(len(q)):
        m = max((_exact_chain(q[t], doc[u]) for u in range(len(doc))), default=0.0)
        S = S + float(m)
    return S


def _cases():
    rng = np.random.default_rng(11)
    yield rng.standard_normal((3, 8)).astype(np.float16), rng.standard_normal((5, 8)).astype(np.float16)
    yield (rng.standard_normal((4, 24)) * 37).astype(np.float16), (rng.standard_normal((17, 24)) * 0.01).astype(np.float16)
    sub = lambda shape: (rng.integers(0, 1024, shape) | (rng.integers(0, 2, shape) << 15)).astype(np.uint16).view(np.float16)
    yield sub((2, 16)), np.where(rng.random((6, 16)) < 0.5, sub((6, 16)), rng.standard_normal((6, 16)).astype(np.float16))
    yield rng.choice([-60000.0, 60000.0, 3.0], (2, 32)).astype(np.float16), rng.choice([-60000.0, 59999.0], (3, 32)).astype(np.float16)
    yield -np.abs(rng.standard_normal((2, 8))).astype(np.float16), np.abs(rng.standard_normal((4, 8))).astype(np.float16)


def test_restatement_equals_exactly_rounded_fma_chains():
    for q, d in _cases():
        sims = M.token_similarities(q, d)
        assert sims.dtype == np.float32
        for t in range(len(q)):
            for u in range(len(d)):
                assert float(sims[t, u]) == _exact_chain(q[t], d[u])
        assert M.maxsim_scores(q, [d, d[:1], None, d[:0]]) == [_scalar_score(q, d), _scalar_score(q, d[:1]), 0.0, 0.0]


def test_scores_are_never_minus_zero_and_the_sort_is_stable():
    q = np.array([[-1.0] + [0.0] * 7], dtype=np.float16)
    zero_doc = np.zeros((2, 8), dtype=np.float16)                      # every product is -0.0 or +0.0
    s = M.maxsim_scores(q, [zero_doc, None])
    assert s == [0.0, 0.0] and not np.signbit(s).any()
    d = np.eye(8, dtype=np.float16)[:3]
    pos, ids, fin = M.maxsim_rerank([7, 8, 7, 9, 8], np.ones((1, 8), np.float16), [d[:1], d * 2, d[:1], None, d * 2], 4)
    assert pos == [1, 4, 0, 2] and ids == [8, 8, 7, 7] and fin == [2.0, 2.0, 1.0, 1.0]


def test_csr_form_equals_the_list_form():
    rng = np.random.default_rng(5)
    T = [0, 1, 15, 16, 17, 0, 33, 100, 0]
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    vals = rng.standard_normal((int(indptr[-1]), 24)).astype(np.float16)
    q = rng.standard_normal((17, 24)).astype(np.float16)
    rows = [3, 0, 8, 7, -1, 9, 2, 2, 5]
    docs = [vals[indptr[r]:indptr[r + 1]] if 0 <= r < len(T) else None for r in rows]
    assert M.maxsim_scores_csr(q, indptr, vals, rows).tolist() == M.maxsim_scores(q, docs)
    ids = [r + 100 for r in rows]
    assert M.maxsim_rerank_csr(ids, q, indptr, vals, 100, 6) == M.maxsim_rerank(ids, q, docs, 6)
    assert M.maxsim_scores_csr(q, np.zeros(1, np.int64), vals[:0], [0, 1]).tolist() == [0.0, 0.0]


def test_ranker_validation():
    ok = MaxSimRanker(np.ones((3, 8), np.float32), candidates=40)
    assert ok.query_tokens.dtype == np.float16 and ok.window(10) == 40 and ok.window(50) == 50
    assert MaxSimRanker(np.ones((64, 256))).window(7) == 7
    third = np.float32(1.0) / np.float32(3.0)
    assert MaxSimRanker(np.full((1, 8), third)).query_tokens[0, 0] == np.float16(third)      # numpy's astype: nearest even
    for bad in (np.ones(8), np.ones((2, 3, 8)), np.ones((0, 8)), np.ones((65, 8)), np.ones((2, 12)), np.ones((2, 264)),
                np.ones((2, 4)), np.full((2, 8), np.nan), np.full((2, 8), np.inf), np.full((2, 8), 65520.0, np.float32),
                [["a"] * 8]):
        with pytest.raises(ValueError):
            MaxSimRanker(bad)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="candidates"):
            MaxSimRanker(np.ones((1, 8)), candidates=bad)
    assert MaxSimRanker(np.full((1, 8), 65519.0, np.float32)).query_tokens[0, 0] == np.float16(65504)   # rounds to the largest finite


def test_configs_carry_the_option():
    assert RetrievalConfig().late_interaction is False and PipelineConfig().late_interaction is False
    assert PipelineConfig(late_interaction=True).late_interaction is True
    retr = HybridRetriever(object(), RetrievalConfig(late_interaction=True))
    assert all(p.late_interaction for p in retr.profiles.values())
    assert nat.HR_MAX_QUERY_TOKENS == 64 and "hr_maxsim_rerank_dev" in nat.EXPORTED_SYMBOLS


# ---- the column -------------------------------------------------------------------------------------------------------------
def test_token_vector_column():
    rng = np.random.default_rng(1)
    col = TokenVectorColumn(8)
    v1 = rng.standard_normal((5, 8)).astype(np.float16)
    col.extend(np.array([0, 2, 2, 5]), v1)
    col.pad_to(5)                                                       # two rows appended without vectors
    v2 = rng.standard_normal((1500, 8)).astype(np.float16)              # grows the buffers
    col.extend(np.array([0, 1, 1500]), v2)
    assert len(col) == 7 and col.indptr().tolist() == [0, 2, 2, 5, 5, 5, 6, 1505]
    assert np.array_equal(col.row(0), v1[:2]) and col.row(1).shape == (0, 8) and np.array_equal(col.row(6), v2[1:])
    assert col.values().dtype == np.float16 and col.values().shape == (1505, 8)
    ip, vals = col.gather([2, 9, 0, 5, -1])
    assert ip.tolist() == [0, 3, 3, 5, 6, 6] and np.array_equal(vals, np.concatenate([v1[2:5], v1[:2], v2[:1]]))
    with pytest.raises(IndexError):
        col.row(7)
    col.compact(np.array([1, 0, 1, 0, 0, 1, 0], bool))
    assert col.indptr().tolist() == [0, 2, 5, 6] and np.array_equal(col.values(), np.concatenate([v1, v2[:1]]))
    with pytest.raises(ValueError):
        col.compact(np.ones(2, bool))
    cols = PayloadColumns()
    assert cols.token_vectors() is None                                # off: nothing is kept
    cols.enable_token_vectors(8)
    cols["id"].extend(["a", "b", "c"])
    assert cols.token_vectors().indptr().tolist() == [0, 0, 0, 0]      # rows without vectors: T_r = 0


# ---- the manager over stand-ins -------------------------------------------------------------------------------------------
class _Shard(sq._OracleShard):
    def compact(self, keep=None, d_keep=0):
        keep = np.asarray(keep, dtype=bool)
        rows = np.nonzero(keep[:self.num_sparse_rows])[0]
        take = np.concatenate([np.arange(self.ptr[r], self.ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        lens = (self.ptr[1:] - self.ptr[:-1])[rows]
        self.ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.idx, self.val, self.X = self.idx[take], self.val[take], self.X[keep]
        return int(keep.sum()), int(keep.sum())


def _token_rows(n, seed=3):
    """Token vectors for n rows: 0..40 vectors each, every seventh row none."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 41, n)
    T[::7] = 0
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    return indptr, rng.standard_normal((int(indptr[-1]), TD)).astype(np.float32)


def _manager(shards, token_dim=TD):
    X, csr = sq._corpus()
    n = sq.N
    mgr = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False,
                             token_dim=token_dim)
    mgr.attach_shards([_Shard(sq.V) for _ in range(shards)])
    indptr, vals = _token_rows(n)
    for lo in range(0, n, 60):                     # several appends; the middle one carries no token vectors
        hi = min(n, lo + 60)
        tv = {} if lo == 60 or token_dim is None else \
            {"token_vectors": (indptr[lo:hi + 1] - indptr[lo], vals[indptr[lo]:indptr[hi]])}
        mgr.add_rows(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]), ids=[f"c{r}" for r in range(lo, hi)],
                     contents=[f"topic{r % 5} word{r % 7}" for r in range(lo, hi)], **tv)
    return mgr, X, csr, indptr, vals.astype(np.float16)


@pytest.fixture(scope="module", params=[1, 3])
def host(request):
    mgr, X, csr, indptr, vals = _manager(request.param)
    assert mgr._filters_on_device() is None
    yield mgr, X, csr, indptr, vals
    asyncio.run(mgr.close())


def _row_tokens(indptr, vals, r):
    return None if 60 <= r < 120 else vals[indptr[r]:indptr[r + 1]]


def _query_tokens(seed, tq):
    return np.random.default_rng(seed).standard_normal((tq, TD)).astype(np.float32)


def test_the_store_holds_what_was_appended(host):
    mgr, _, _, indptr, vals = host
    col = mgr._cols.token_vectors()
    assert len(col) == sq.N and col.dim == TD
    for r in (0, 1, 7, 59, 60, 100, 119, 120, 156):
        want = _row_tokens(indptr, vals, r)
        assert np.array_equal(col.row(r), want if want is not None else np.zeros((0, TD), np.float16))


def _check_search(mgr, indptr, vals, query, coll, ranker, top_k, **kw):
    W = ranker.window(top_k)
    before = mgr.stats["maxsim_host_reranks"]
    plain = asyncio.run(mgr.search(query, coll, W, **kw))
    got = asyncio.run(mgr.search(query, coll, top_k, ranker=ranker, **kw))
    rows = [h["_row"] for h in plain]
    pos, _, fin = M.maxsim_rerank(rows, ranker.query_tokens, [_row_tokens(indptr, vals, r) for r in rows], W)
    assert [h["id"] for h in got] == [plain[p]["id"] for p in pos[:top_k]]
    assert [h["score"] for h in got] == fin[:top_k]
    assert [h["raw_score"] for h in got] == [plain[p]["score"] for p in pos[:top_k]]
    assert mgr.stats["maxsim_host_reranks"] == before + 1
    return got, plain


def test_search_with_the_ranker_equals_the_restatement_over_the_plain_search(host):
    mgr, X, csr, indptr, vals = host
    q = X[5] + 0.25 * X[40]
    got, plain = _check_search(mgr, indptr, vals, q, "semantic_index", MaxSimRanker(_query_tokens(1, 9), candidates=40), 10)
    assert [h["id"] for h in got] != [h["id"] for h in plain[:10]]                        # the rerank says something
    for tq, cand in ((1, None), (17, 25), (64, 12)):
        _check_search(mgr, indptr, vals, q, "semantic_index", MaxSimRanker(_query_tokens(tq, tq), candidates=cand), 10)
    _check_search(mgr, indptr, vals, q, "semantic_index", MaxSimRanker(_query_tokens(2, 5), candidates=30), 7,
                  filters="chunk_index >= 3")
    a, b = csr[0][12], csr[0][13]
    sparse_q = {"indices": csr[1][a:b].tolist(), "values": csr[2][a:b].tolist()}
    got, _ = _check_search(mgr, indptr, vals, sparse_q, "sparse_index", MaxSimRanker(_query_tokens(3, 6), candidates=20), 5)
    assert len(got) == 5
    r = MaxSimRanker(_query_tokens(4, 8), candidates=15)
    by_id = asyncio.run(mgr.search_by_ids(["c7"], "semantic_index", 6, ranker=r))[0]      # search_by_ids passes the ranker through
    direct = asyncio.run(mgr.search(mgr.collections["semantic_index"].handle.get_dense_rows([7])[0], "semantic_index", 6, ranker=r))
    assert [(h["id"], h["score"]) for h in by_id] == [(h["id"], h["score"]) for h in direct] and len(by_id) == 6


def test_list_hook_equals_the_restatement(host):
    mgr, _, _, indptr, vals = host
    qt = _query_tokens(9, 12)
    rows = [3, 70, None, 150, 3, 500, 14]
    docs = [_row_tokens(indptr, vals, r) if r is not None and r < sq.N else None for r in rows]
    pos, _, fin = M.maxsim_rerank(list(range(len(rows))), qt.astype(np.float16), docs, 4)
    for got in (mgr.maxsim_rerank_lists(rows, qt, 4), asyncio.run(mgr.maxsim_rerank_lists_async(rows, qt, 4))):
        assert got[0].tolist() == pos and got[1].tolist() == fin
    assert len(mgr.maxsim_rerank_lists([], qt, 4)[0]) == 0


def test_refusals(host):
    mgr, X, _, _, _ = host
    q, r = X[0], MaxSimRanker(_query_tokens(1, 4))
    run = lambda **kw: asyncio.run(mgr.search(q, "semantic_index", kw.pop("top_k", 5), **kw))
    with pytest.raises(ValueError, match="group_by_field"):
        run(ranker=r, group_by_field="doc_id")
    with pytest.raises(ValueError, match="offset"):
        run(ranker=r, offset=3)
    with pytest.raises(ValueError, match="deep window"):
        run(ranker=r, top_k=nat.HR_MAX_TOPK + 1)
    with pytest.raises(ValueError, match="deep window"):
        run(ranker=MaxSimRanker(_query_tokens(1, 4), candidates=nat.HR_MAX_TOPK + 1))
    with pytest.raises(ValueError, match="dim"):
        run(ranker=MaxSimRanker(np.ones((3, TD + 8))))
    with pytest.raises(ValueError, match="MaxSimRanker"):
        run(ranker="maxsim")
    with pytest.raises(ValueError, match="not found"):
        asyncio.run(mgr.search(q, "nope", 5, ranker=r))
    with pytest.raises(ValueError, match="group_by_field"):
        asyncio.run(mgr.search_by_ids(["c1"], "semantic_index", 5, ranker=r, group_by_field="doc_id"))
    with pytest.raises(ValueError):
        mgr.maxsim_rerank_lists([1, 2], np.ones((65, TD)), 2)
    import types
    coll = mgr.collections["semantic_index"]
    real, coll.handle = coll.handle, types.SimpleNamespace(round=None)                    # the torchrun form's mark
    try:
        with pytest.raises(NotImplementedError):
            run(ranker=r)
    finally:
        coll.handle = real
    # a malformed token CSR is refused whole, before any shard is touched
    n0 = mgr.num_rows
    good = np.ones((3, TD), np.float32)
    for tv in ((np.array([0, 2, 1, 3]), good), (np.array([1, 2, 3, 3]), good), (np.array([0, 1, 3]), good),
               (np.array([0, 1, 2, 4]), good), (np.array([0, 1, 2, 3]), np.ones((3, TD + 8))),
               (np.array([0, 1, 2, 3]), np.full((3, TD), np.nan)), (np.array([0, 1, 2, 3]), np.full((3, TD), 1e6)),
               (np.array([0.0, 1.0, 2.0, 3.0]), good), "nope"):
        with pytest.raises(ValueError):
            mgr.add_rows(X[:3], None, ids=["x", "y", "z"], token_vectors=tv)
    assert mgr.num_rows == n0 and mgr._main.num_rows == n0 and len(mgr._cols.token_vectors()) == n0
    assert len(run(ranker=None)) == 5                                                    # the default: the call it was


def test_a_manager_without_token_dim_refuses_and_is_unchanged():
    mgr, X, csr, _, _ = _manager(1, token_dim=None)
    try:
        assert mgr.token_dim is None and mgr._cols.token_vectors() is None and mgr._dev_tokvec is None
        with pytest.raises(ValueError, match="token_dim"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=MaxSimRanker(_query_tokens(1, 4))))
        with pytest.raises(ValueError, match="token_dim"):
            mgr.add_rows(X[:1], None, ids=["x"], token_vectors=(np.array([0, 1]), np.ones((1, TD))))
        with pytest.raises(ValueError, match="token_dim"):
            mgr.save_token_vectors("unused.npz")
        with pytest.raises(ValueError, match="token_dim"):
            mgr.maxsim_rerank_lists([1], _query_tokens(1, 4), 1)
        calls = []
        real = mgr._main.search_dense
        mgr._main.search_dense = lambda *a, **k: calls.append(1) or real(*a, **k)
        hits = asyncio.run(mgr.search(X[0], "semantic_index", 5))
        assert len(hits) == 5 and calls == [1] and mgr.stats["maxsim_host_reranks"] == 0   # the calls it made
        with pytest.raises(ValueError, match="token_dim"):
            MilvusIndexManager(connect=False, token_dim=12)
    finally:
        asyncio.run(mgr.close())


def test_save_and_load_round_trip(tmp_path):
    mgr, X, _, indptr, vals = _manager(1)
    other, _, _, _, _ = _manager(1)
    path = str(tmp_path / "tokens.npz")
    try:
        mgr.save_token_vectors(path)
        with np.load(path) as z:
            assert sorted(z.files) == ["indptr", "token_dim", "values"] and int(z["token_dim"]) == TD
            assert z["values"].dtype == np.float16
        other._cols.enable_token_vectors(TD, reset=True)               # a collection of the same rows, no vectors yet
        r = MaxSimRanker(_query_tokens(5, 7), candidates=30)
        want = asyncio.run(mgr.search(X[3], "semantic_index", 8, ranker=r))
        empty = asyncio.run(other.search(X[3], "semantic_index", 8, ranker=r))
        assert all(h["score"] == 0.0 for h in empty)
        other.load_token_vectors(path)
        got = asyncio.run(other.search(X[3], "semantic_index", 8, ranker=r))
        assert [(h["id"], h["score"]) for h in got] == [(h["id"], h["score"]) for h in want]
        other.add_rows(X[:2], None, ids=["p", "q"])
        with pytest.raises(ValueError, match="rows"):
            other.load_token_vectors(path)                              # another row count
        wide = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False,
                                  token_dim=TD + 8)
        with pytest.raises(ValueError, match="dim"):
            wide.load_token_vectors(path)
    finally:
        asyncio.run(mgr.close())
        asyncio.run(other.close())


def test_compact_keeps_every_survivors_vectors():
    mgr, X, _, indptr, vals = _manager(3)
    try:
        r = MaxSimRanker(_query_tokens(6, 10), candidates=50)
        before = asyncio.run(mgr.search(X[9], "semantic_index", 50, ranker=r))
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 3"))
        alive = [h for h in asyncio.run(mgr.search(X[9], "semantic_index", 50, ranker=r))]
        out = mgr.compact()
        assert out["rows_after"] < out["rows_before"] == sq.N
        col = mgr._cols.token_vectors()
        assert len(col) == out["rows_after"]
        for new in range(0, len(col), 5):
            old = int(mgr._cols["id"][new][1:])
            want = _row_tokens(indptr, vals, old)
            assert np.array_equal(col.row(new), want if want is not None else np.zeros((0, TD), np.float16))
        after = asyncio.run(mgr.search(X[9], "semantic_index", 50, ranker=r))
        assert [(h["id"], h["score"]) for h in after] == [(h["id"], h["score"]) for h in alive]
        assert {h["id"] for h in after} <= {h["id"] for h in before} | {h["id"] for h in alive}
    finally:
        asyncio.run(mgr.close())


# ---- index_chunks and retrieve() ------------------------------------------------------------------------------------------
class _Gen:
    """Deterministic stub: semantic / sparse queries from the corpus, token vectors from a hash of the text."""

    def __init__(self, X, csr, fail_tokens=False):
        self.X, self.csr, self.fail_tokens, self.token_calls = X, csr, fail_tokens, 0

    def _n(self, text):
        return int(text.rsplit("q", 1)[1])

    def encode_semantic(self, text):
        return self.X[self._n(text)] + 0.5 * self.X[self._n(text) + 1]

    def encode_sparse(self, text):
        r = self._n(text) + 1
        a, b = self.csr[0][r], self.csr[0][r + 1]
        return {"indices": self.csr[1][a:b].tolist(), "values": self.csr[2][a:b].astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)

    def encode_token_vectors(self, texts):
        self.token_calls += 1
        if self.fail_tokens:
            raise RuntimeError("token encoder down")
        lens = [1 + len(t) % 5 for t in texts]
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rng = np.random.default_rng(sum(map(len, texts)))
        return indptr, rng.standard_normal((int(indptr[-1]), TD)).astype(np.float32)


def test_retrieve_with_late_interaction_equals_the_restatement_over_the_fused_list(host):
    mgr, X, csr, indptr, vals = host
    mgr.embedding_generator = _Gen(X, csr)
    top_k = 6
    old, RetrievalConstants.TIMEOUT_SECONDS = RetrievalConstants.TIMEOUT_SECONDS, 60.0
    try:
        for qn in (10, 30):
            initialize_caches()
            text = f"plain statement q{qn}"
            gen = mgr.embedding_generator
            sem = asyncio.run(mgr.search(gen.encode_semantic(text), "semantic_index", 2 * top_k))
            spa = asyncio.run(mgr.search(gen.encode_sparse(text), "sparse_index", 2 * top_k, None,
                                         {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
            ranked = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa]], (0.7, 0.3))
            row_of = {h["id"]: h["_row"] for h in sem + spa}
            rows = [row_of[i] for i, _, _ in ranked]
            qt = gen.encode_token_vectors([text])[1].astype(np.float16)
            pos, _, fin = M.maxsim_rerank(rows, qt, [_row_tokens(indptr, vals, r) for r in rows], len(rows))
            want = [(ranked[p][0], f, ranked[p][1]) for p, f in zip(pos, fin)][:top_k]
            assert [w[0] for w in want] != [i for i, _, _ in ranked][:top_k]                # the rerank reorders the fused list
            got = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k, late_interaction=True)).retrieve(text, profile_hint="default"))
            assert [(h["id"], h["score"], h["fused_score"]) for h in got] == want
            plain = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k)).retrieve(text, profile_hint="default"))
            assert all("fused_score" not in h for h in plain) and [h["id"] for h in plain] == [i for i, _, _ in ranked][:top_k]
        mgr.embedding_generator = type("NoHook", (), {"encode_semantic": gen.encode_semantic, "encode_sparse": gen.encode_sparse})()
        with pytest.raises(ValueError, match="encode_token_vectors"):
            asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k, late_interaction=True)).retrieve("plain statement q10", profile_hint="default"))
    finally:
        RetrievalConstants.TIMEOUT_SECONDS = old
        mgr.embedding_generator = None


def test_index_chunks_calls_the_token_hook_once_and_keeps_rows_aligned():
    from advanced_rag.chunking import Chunk, ChunkMetadata

    def chunks(lo, hi):
        out = []
        for r in range(lo, hi):
            meta = ChunkMetadata(chunk_id=f"k{r}", doc_id=f"d{r // 3}", chunk_index=r % 3, token_count=5, char_start=0, char_end=9,
                                     entropy=0.5, redundancy=0.1, domain_density=0.2, coherence_score=0.9, source="t",
                                     timestamp="2024-01-01T00:00:00", version="1")
            out.append(Chunk(text=f"text {'x' * (r % 4)} q{r}", metadata=meta))
        return out

    X, csr = sq._corpus()
    mgr = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False, token_dim=TD)
    mgr.attach_shards([_Shard(sq.V)])
    try:
        gen = mgr.embedding_generator = _Gen(X, csr)
        first = chunks(0, 6)
        s = asyncio.run(mgr.index_chunks(first))
        assert s["indexed_semantic"] == 6 and gen.token_calls == 1 and not s["errors"]
        ip, v = gen.encode_token_vectors([c.text for c in first])
        col = mgr._cols.token_vectors()
        assert col.indptr().tolist() == ip.tolist() and np.array_equal(col.values(), v.astype(np.float16))
        gen.fail_tokens = True
        s = asyncio.run(mgr.index_chunks(chunks(6, 9)))
        assert s["indexed_semantic"] == 3 and any("token_vectors_error" in e for e in s["errors"])
        col = mgr._cols.token_vectors()
        assert len(col) == 9 == mgr.num_rows and col.indptr().tolist()[6:] == [int(ip[-1])] * 4      # T_r = 0, rows aligned
    finally:
        mgr.embedding_generator = None
        asyncio.run(mgr.close())
