"""query(..., output_fields=["embedding"]) on sparse_index and search_by_ids without a GPU: the manager over oracle-backed
stand-ins for the shard handles (one shard, and three whose rows interleave) against numpy slicing of the CSR the test
ingested — the payload's shape and dtypes, rows without entries, rows without a sparse row, request order through
ShardSet.get_sparse_rows, and search_by_ids against search() with the stored vector."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.shards import CollectiveShardSet, ShardSet


class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given (local row numbers), with the handle's search
    signatures, get_dense_rows() and get_sparse_rows()."""

    def __init__(self, sparse_dim):
        self.X = None
        self.ptr, self.idx, self.val = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
        self.device, self.sparse_dim = 0, sparse_dim

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = property(lambda self: len(self.ptr) - 1)
    dim = property(lambda self: self.X.shape[1])

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def add_sparse(self, ptr, idx, val):
        self.idx = np.concatenate([self.idx, idx[ptr[0]:ptr[-1]]])
        self.val = np.concatenate([self.val, val[ptr[0]:ptr[-1]]])
        self.ptr = np.concatenate([self.ptr, ptr[1:] - ptr[0] + self.ptr[-1]])

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def search_sparse(self, queries, k, drop, mask=None):
        return oracle.sparse_search(self.ptr, self.idx, self.val, queries, k, drop, mask)

    def get_dense_rows(self, rows):
        return self.X[np.asarray(rows, dtype=np.int64)].astype(np.float32)

    def get_sparse_rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        if len(rows) and (rows.min() < 0 or rows.max() >= self.num_sparse_rows):
            raise ValueError("row outside the shard")
        lens = self.ptr[rows + 1] - self.ptr[rows]
        ptr = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lens, out=ptr[1:])
        take = np.concatenate([np.arange(self.ptr[r], self.ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        return ptr, self.idx[take], self.val[take]

    def finalize(self):
        pass

    def close(self):
        pass


N, N_BARE, DIM, V = 157, 11, 12, 90          # the last N_BARE rows are appended without sparse payloads
ODD_IDS = {3: 'say "hi"', 4: "back\\slash", 5: "a, b", 6: 'mixed \\" , "', 7: "shared-prefix-0123456789-A", 8: "shared-prefix-0123456789-B"}
EMPTY_ROWS = (0, 9, 77, N - 1)


def _ids(n):
    return [ODD_IDS.get(r, f"c{r}") for r in range(n)]


def _corpus():
    rng = np.random.default_rng(23)
    X = rng.standard_normal((N + N_BARE, DIM)).astype(np.float32)
    lens = rng.integers(1, 9, N)
    lens[list(EMPTY_ROWS)] = 0
    ptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(V, n, replace=False)) for n in lens]).astype(np.int32)
    val = (rng.random(idx.shape[0]) + 0.5).astype(np.float32)
    return X, (ptr, idx, val)


def _manager(shards):
    X, csr = _corpus()
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard(V) for _ in range(shards)])
    ids = _ids(N + N_BARE)
    for lo in range(0, N, 60):                     # several appends: the pieces interleave over the shards
        hi = min(N, lo + 60)
        mgr.add_rows(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]), ids=ids[lo:hi], doc_id=[f"doc{r // 5}" for r in range(lo, hi)],
                     chunk_index=[r % 5 for r in range(lo, hi)])
    mgr.add_rows(X[N:], None, ids=ids[N:], doc_id=[f"doc{r // 5}" for r in range(N, N + N_BARE)],
                 chunk_index=[r % 5 for r in range(N, N + N_BARE)])
    assert isinstance(mgr._main, ShardSet) and mgr._main.n_shards == shards and mgr._filters_on_device() is None
    assert mgr._main.num_rows == N + N_BARE and mgr._main.num_sparse_rows == N
    return mgr, X, csr


@pytest.fixture(scope="module", params=[1, 3])
def host(request):
    mgr, X, csr = _manager(request.param)
    yield mgr, X, csr
    asyncio.run(mgr.close())


def _row(csr, r):
    """Stored payload of global row r: its slice of the ingested CSR; nothing beyond the sparse rows."""
    if r >= N:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    return csr[1][csr[0][r]:csr[0][r + 1]], csr[2][csr[0][r]:csr[0][r + 1]]


def _q(mgr, *a, **kw):
    return asyncio.run(mgr.query("sparse_index", *a, **kw))


def test_query_returns_the_stored_payloads(host):
    mgr, X, csr = host
    ids = _ids(N + N_BARE)
    got = _q(mgr, None, ["embedding", "chunk_index"], limit=N + N_BARE)
    assert [h["id"] for h in got] == ids
    for r, h in enumerate(got):
        assert list(h) == ["id", "chunk_index", "embedding"] and h["chunk_index"] == r % 5
        e = h["embedding"]
        assert list(e) == ["indices", "values"]
        assert isinstance(e["indices"], np.ndarray) and e["indices"].dtype == np.int32 and e["indices"].ndim == 1
        assert isinstance(e["values"], np.ndarray) and e["values"].dtype == np.float32 and e["values"].ndim == 1
        wi, wv = _row(csr, r)
        assert np.array_equal(e["indices"], wi) and np.array_equal(e["values"].view(np.uint32), wv.view(np.uint32)), r
        # what search() makes of it is the payload itself
        pi, pv = mgr._as_sparse_payload(e)
        assert pi.dtype == np.int32 and pv.dtype == np.float32 and np.array_equal(pi, wi) and np.array_equal(pv, wv)
    for r in EMPTY_ROWS + (N, N + N_BARE - 1):          # no entries / no sparse row at all: two empty arrays
        assert got[r]["embedding"]["indices"].shape == got[r]["embedding"]["values"].shape == (0,)
    # an expression, and paging
    page = _q(mgr, 'doc_id in ["doc3", "doc1", "doc15"]', ["embedding"], limit=7, offset=2)
    rows = [r for r in range(N) if r // 5 in (1, 3, 15)][2:9]
    assert [h["id"] for h in page] == [ids[r] for r in rows]
    assert all(np.array_equal(h["embedding"]["indices"], _row(csr, r)[0]) for h, r in zip(page, rows))
    assert _q(mgr, "chunk_index == 2", ["count(*)"]) == [{"count(*)": len([r for r in range(N + N_BARE) if r % 5 == 2])}]
    assert mgr.collections["sparse_index"].query("chunk_index == 1", ["embedding"], 3)[1]["embedding"]["indices"].dtype == np.int32


def test_shard_set_returns_rows_in_request_order(host):
    mgr, X, csr = host
    s = mgr._main
    rng = np.random.default_rng(2)
    total = N + N_BARE
    for rows in (np.arange(total), np.arange(total)[::-1], rng.permutation(total), np.array([5, 5, 150, 0, 5, N, 150, N + 3]),
                 np.array(EMPTY_ROWS), np.zeros(0, np.int64)):
        ptr, idx, val = s.get_sparse_rows(rows)
        assert (ptr.dtype, idx.dtype, val.dtype) == (np.int64, np.int32, np.float32) and ptr.shape == (len(rows) + 1,)
        assert ptr[0] == 0 and ptr[-1] == len(idx) == len(val)
        for i, r in enumerate(rows):
            wi, wv = _row(csr, int(r))
            assert np.array_equal(idx[ptr[i]:ptr[i + 1]], wi) and np.array_equal(val[ptr[i]:ptr[i + 1]], wv), (i, r)
    for bad in ([total], [-1], [0, total + 7]):
        with pytest.raises(ValueError):
            s.get_sparse_rows(bad)
    with pytest.raises(NotImplementedError):
        CollectiveShardSet.get_sparse_rows(object(), [0])


def _search(mgr, query, collection, **kw):
    return asyncio.run(mgr.search(query, collection, **kw))


def _by_ids(mgr, ids, collection, **kw):
    return asyncio.run(mgr.search_by_ids(ids, collection, **kw))


def test_search_by_ids_equals_search_with_the_stored_vector(host):
    mgr, X, csr = host
    ids = _ids(N + N_BARE)
    rows = [40, 3, 4, 5, 6, 7, 8, 0, 40, 120]          # odd ids, a shared 16-byte prefix, an empty sparse row, a duplicate
    req = [ids[r] for r in rows]
    before = mgr.stats["search_by_ids"]
    for kw in ({}, {"top_k": 7, "filters": "chunk_index >= 2"}, {"top_k": 4, "group_by_field": "doc_id"}):
        got = _by_ids(mgr, req, "semantic_index", **kw)
        assert len(got) == len(rows)
        for r, hits in zip(rows, got):
            assert hits == _search(mgr, X[r], "semantic_index", **kw), (r, kw)
            if not kw:
                assert hits[0]["id"] == ids[r] and hits[0]["_row"] == r          # not excluded: its own best hit under COSINE
        got = _by_ids(mgr, req, "sparse_index", **kw)
        for r, hits in zip(rows, got):
            wi, wv = _row(csr, r)
            assert hits == _search(mgr, {"indices": wi, "values": wv}, "sparse_index", **kw), (r, kw)
    assert mgr.stats["search_by_ids"] == before + 6
    assert got[0] == got[8]                                                     # the duplicate id: two equal lists
    sync = mgr.collections["semantic_index"].search_by_ids(req[:3], 5, "chunk_index != 1")
    assert sync == _by_ids(mgr, req[:3], "semantic_index", top_k=5, filters="chunk_index != 1")
    # the filter that drops the entity itself
    hits = _by_ids(mgr, [ids[40]], "semantic_index", top_k=5, filters='id not in ["c40"]')[0]
    assert len(hits) == 5 and all(h["id"] != "c40" for h in hits)


def test_search_by_ids_refusals():
    mgr, X, csr = _manager(2)
    try:
        for bad in ([], (), "c1", None, 7, {"c1"}, [3], ["c1", None], ["c1", b"c2"], ["nope"], ["c1", "c1 "], ['say "hi'], ["c999"]):
            with pytest.raises(ValueError):
                _by_ids(mgr, bad, "semantic_index")
        with pytest.raises(ValueError) as ei:
            _by_ids(mgr, ["c1", "no such id", "c2"], "sparse_index")
        assert "no such id" in str(ei.value)
        with pytest.raises(ValueError):
            _by_ids(mgr, ["c1"], "no_such_collection")
        with pytest.raises(ValueError):
            _by_ids(mgr, ["c1"], "semantic_index", group_size=2)             # search()'s own refusal surfaces
        # a tombstoned id is not found; the others still are
        asyncio.run(mgr.delete_by_filter("semantic_index", 'id == "c20"'))
        with pytest.raises(ValueError) as ei:
            _by_ids(mgr, ["c21", "c20"], "semantic_index")
        assert "c20" in str(ei.value)
        assert _by_ids(mgr, ["c21"], "semantic_index", top_k=3)[0][0]["id"] == "c21"
        # one id on two live rows (a re-ingest without a delete): the lowest row's vector
        mgr.add_rows(X[50:51] * -1.0, None, ids=["c10"], doc_id=["again"], chunk_index=[0])
        assert _by_ids(mgr, ["c10"], "semantic_index", top_k=3) == [_search(mgr, X[10], "semantic_index", top_k=3)]
    finally:
        asyncio.run(mgr.close())
