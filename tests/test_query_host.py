"""Collection.query without a GPU: the manager over oracle-backed stand-ins for the shard handles (as
tests/test_group_host.py builds them) against the restatement
np.flatnonzero(filters.evaluate(...) & ~deleted)[offset:offset + limit] — paging, count(*), tombstones and compaction,
a synthetic collection, field selection, the limit / offset rules, and ShardSet.get_dense_rows over two shards."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag import filters
from advanced_rag.constants import QUERY_MAX_WINDOW
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.shards import CollectiveShardSet, ShardSet


class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given (local row numbers), with the handle's search
    signatures, compact() and get_dense_rows()."""

    def __init__(self):
        self.X = None
        self.device, self.sparse_dim = 0, 0

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = 0
    device_bytes = property(lambda self: 0 if self.X is None else self.X.nbytes)
    dim = property(lambda self: self.X.shape[1])

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def compact(self, keep=None, d_keep=0):
        self.X = self.X[np.asarray(keep, dtype=bool)]
        return self.X.shape[0], 0

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def get_dense_rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        if len(rows) and (rows.min() < 0 or rows.max() >= self.num_rows):
            raise ValueError("row outside the shard")
        return self.X[rows].astype(np.float32)

    def finalize(self):
        pass

    def close(self):
        pass


N, DIM = 203, 12
FIELDS = ["doc_id", "content", "chunk_index", "token_count", "entropy", "redundancy", "domain_density", "metadata_json",
          "timestamp"]
EXPRS = ['chunk_index >= 3 and entropy < 0.5', 'doc_id in ["doc3", "doc7", "doc19", "nope"]',
         '(chunk_index == 1 or token_count > 150) and not doc_id == "doc7"', 'chunk_id == "c77"', 'token_count < 0']


def _payload(n):
    return dict(ids=[f"c{r}" for r in range(n)], contents=[f"text of row {r}" for r in range(n)],
                doc_id=[f"doc{r // 10}" for r in range(n)], chunk_index=[r % 10 for r in range(n)],
                token_count=[r for r in range(n)], entropy=[(r % 8) / 8.0 for r in range(n)],
                redundancy=[(r % 4) / 4.0 for r in range(n)], domain_density=[(r % 16) / 16.0 for r in range(n)],
                timestamp=[f"2024-01-{1 + r % 28:02d}" for r in range(n)], metadata_json=[f"{{'r': {r}}}" for r in range(n)])


def _columns(p):
    """The payload as filters.evaluate takes it, built from the test's own lists."""
    cols = {k: np.asarray(p[k], dtype=np.int64) for k in ("chunk_index", "token_count")}
    cols.update({k: np.asarray(p[k], dtype=np.float32) for k in ("entropy", "redundancy", "domain_density")})
    cols.update(id=np.asarray(p["ids"]), chunk_id=np.asarray(p["ids"]), doc_id=np.asarray(p["doc_id"]), timestamp=np.asarray(p["timestamp"]))
    return cols


def _manager(shards=2):
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N, DIM)).astype(np.float32)
    p = _payload(N)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard() for _ in range(shards)])
    for lo in range(0, N, 80):     # several appends: the pieces interleave over the shards
        hi = min(N, lo + 80)
        mgr.add_rows(X[lo:hi], None, ids=p["ids"][lo:hi], contents=p["contents"][lo:hi],
                     **{k: v[lo:hi] for k, v in p.items() if k not in ("ids", "contents")})
    assert isinstance(mgr._main, ShardSet) and mgr._filters_on_device() is None
    return mgr, X, p


@pytest.fixture(scope="module")
def host():
    mgr, X, p = _manager()
    yield mgr, X, p
    asyncio.run(mgr.close())


def _want_rows(p, expr, deleted=None, offset=0, limit=None):
    keep = filters.evaluate(expr, _columns(p), N) if expr else np.ones(N, bool)
    if deleted is not None:
        keep = keep & ~deleted
    rows = np.flatnonzero(keep)
    return rows[offset:] if limit is None else rows[offset:offset + limit]


def _q(mgr, *a, **kw):
    return asyncio.run(mgr.query("semantic_index", *a, **kw))


@pytest.mark.parametrize("expr", EXPRS)
def test_query_equals_the_restatement(host, expr):
    mgr, X, p = host
    want = _want_rows(p, expr)
    got = _q(mgr, expr)
    assert [h["id"] for h in got] == [p["ids"][r] for r in want]
    assert all(list(h) == ["id"] for h in got)                           # the primary key alone by default
    assert _q(mgr, expr, ["count(*)"]) == [{"count(*)": len(want)}]
    for offset, limit in ((0, 5), (3, 4), (len(want), 5), (len(want) + 3, 1), (max(len(want) - 1, 0), 10)):
        page = _q(mgr, expr, limit=limit, offset=offset)
        assert [h["id"] for h in page] == [p["ids"][r] for r in _want_rows(p, expr, None, offset, limit)], (offset, limit)
    assert [h["id"] for h in _q(mgr, expr, offset=2)] == [p["ids"][r] for r in want[2:]]      # limit=None: all after offset
    # the synchronous form on the collection view, named as in pymilvus
    assert mgr.collections["semantic_index"].query(expr, ["doc_id"], 5, 1) == _q(mgr, expr, ["doc_id"], 5, 1)


def test_pages_of_seven_concatenate(host):
    mgr, X, p = host
    for expr in (None, "", EXPRS[0]):
        want = [p["ids"][r] for r in _want_rows(p, expr)]
        got, offset = [], 0
        while True:
            page = _q(mgr, expr, limit=7, offset=offset)
            got += [h["id"] for h in page]
            offset += 7
            if len(page) < 7:
                break
        assert got == want


def test_fields_and_embedding(host):
    mgr, X, p = host
    expr = EXPRS[2]
    want = _want_rows(p, expr)
    got = _q(mgr, expr, FIELDS + ["embedding", "chunk_id", "id"])
    assert len(got) == len(want)
    names = {"content": "contents"}
    for h, r in zip(got, want):
        assert set(h) == {"id", "chunk_id", "embedding", *FIELDS}
        assert h["id"] == h["chunk_id"] == p["ids"][r]
        for f in FIELDS:
            w = p[names.get(f, f)][r]
            assert h[f] == (float(np.float32(w)) if isinstance(w, float) else w), f
        assert h["embedding"].dtype == np.float32 and np.array_equal(h["embedding"], X[r])
    assert list(_q(mgr, expr, ["token_count"], limit=1)[0]) == ["id", "token_count"]
    for bad in (["nope"], ["score"], ["count(*)", "doc_id"], "doc_id", [3]):
        with pytest.raises(ValueError):
            _q(mgr, expr, bad)
    with pytest.raises(ValueError):
        asyncio.run(mgr.query("no_such_collection", expr))


def test_limit_and_offset_rules(host):
    mgr, X, p = host
    with pytest.raises(ValueError):
        _q(mgr, None)                                   # every row: a limit is required
    with pytest.raises(ValueError):
        _q(mgr, "")
    assert len(_q(mgr, None, limit=N + 5)) == N
    assert _q(mgr, "", ["count(*)"]) == [{"count(*)": N}]
    assert QUERY_MAX_WINDOW == 16384
    for offset, limit in ((-1, 5), (0, -1), (0, 0), (QUERY_MAX_WINDOW, 1), (1, QUERY_MAX_WINDOW), (0, QUERY_MAX_WINDOW + 1),
                          (0, 2.5), (None, 3)):
        with pytest.raises(ValueError):
            _q(mgr, EXPRS[0], limit=limit, offset=offset)
    assert len(_q(mgr, None, limit=QUERY_MAX_WINDOW)) == N
    assert _q(mgr, None, limit=1, offset=QUERY_MAX_WINDOW - 1) == []
    assert _q(mgr, EXPRS[0], limit=5, offset=N) == []
    with pytest.raises(ValueError):
        _q(mgr, "chunk_index >>> 3", limit=5)           # the grammar's own refusal
    before = dict(mgr.stats)
    _q(mgr, EXPRS[0], limit=5)
    assert mgr.stats["queries"] == before["queries"] + 1 and mgr.stats["query_device"] == before["query_device"] == 0


def test_tombstones_then_compact():
    mgr, X, p = _manager()
    try:
        expr = EXPRS[0]
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 4 or token_count >= 190"))
        deleted = filters.evaluate("chunk_index == 4 or token_count >= 190", _columns(p), N)
        for e in (expr, None):
            want = _want_rows(p, e, deleted)
            assert [h["id"] for h in _q(mgr, e, limit=N)] == [p["ids"][r] for r in want]
            assert _q(mgr, e, ["count(*)"]) == [{"count(*)": len(want)}]
        before = _q(mgr, expr, ["doc_id", "embedding"])
        mgr.compact()
        after = _q(mgr, expr, ["doc_id", "embedding"])
        assert [(h["id"], h["doc_id"]) for h in after] == [(h["id"], h["doc_id"]) for h in before]
        assert all(np.array_equal(a["embedding"], b["embedding"]) for a, b in zip(after, before))
        assert _q(mgr, None, ["count(*)"]) == [{"count(*)": int((~deleted).sum())}] and mgr.num_rows == int((~deleted).sum())
        # rows are renumbered: the page is by the new ascending row order, which is the old order of the survivors
        want = _want_rows(p, expr, deleted)
        assert [h["id"] for h in _q(mgr, expr, limit=4, offset=2)] == [p["ids"][r] for r in want[2:6]]
    finally:
        asyncio.run(mgr.close())


def test_synthetic_collection():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((95, DIM)).astype(np.float32)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard()])
    mgr.add_rows_synthetic(X)
    try:
        got = _q(mgr, "chunk_index == 3", ["doc_id", "chunk_index", "content", "entropy", "timestamp", "embedding"])
        rows = list(range(3, 95, 10))
        assert [h["id"] for h in got] == [mgr.synthetic_id(r) for r in rows]
        for h, r in zip(got, rows):
            assert (h["doc_id"], h["chunk_index"], h["content"], h["entropy"], h["timestamp"]) == (f"doc{r // 10}", 3, "", 0.0, "")
            assert np.array_equal(h["embedding"], X[r])
        assert _q(mgr, None, ["count(*)"]) == [{"count(*)": 95}]
        assert [h["id"] for h in _q(mgr, None, limit=3, offset=90)] == [mgr.synthetic_id(r) for r in (90, 91, 92)]
        for field in ("token_count", "metadata_json"):           # what a hit of such a collection does not show either
            with pytest.raises(ValueError):
                _q(mgr, None, [field], limit=3)
        with pytest.raises(ValueError):
            _q(mgr, 'doc_id == "doc3"', limit=3)
    finally:
        asyncio.run(mgr.close())


def test_shard_set_returns_vectors_in_request_order(host):
    mgr, X, p = host
    s = mgr._main
    assert s.n_shards == 2 and all(len(r) for r in s.rows_of)
    rng = np.random.default_rng(2)
    for rows in (np.arange(N), np.arange(N)[::-1], rng.permutation(N), np.array([5, 5, 200, 0, 5, 200]), np.zeros(0, np.int64)):
        got = s.get_dense_rows(rows)
        assert got.dtype == np.float32 and got.shape == (len(rows), DIM) and np.array_equal(got, X[rows])
    for bad in ([N], [-1], [0, N + 7]):
        with pytest.raises(ValueError):
            s.get_dense_rows(bad)
    with pytest.raises(NotImplementedError):
        CollectiveShardSet.get_dense_rows(object(), [0])
