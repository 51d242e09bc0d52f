"""query(..., output_fields=["embedding"]) on sparse_index and search_by_ids on the GPU: a one-shard manager (the page of
rows from the device mask, the payloads through hr_get_sparse_rows_dev) and a devices=[0, 0] manager (host view of the
mask, ShardSet.get_sparse_rows) against the payloads this file ingested, and search_by_ids against search() with the
stored vector.  The corpus has no ties: random dense rows, and sparse rows of unit norm, so that every entity is its own
best hit in both collections."""
import asyncio

import numpy as np
import pytest

from advanced_rag import MilvusIndexManager

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V = 613, 32, 400
ODD = {11: 'say "hi"', 12: "back\\slash", 13: "a, b", 14: 'all \\" , " of them', 15: "shared-prefix-0123456789-A",
       16: "shared-prefix-0123456789-B"}
EMPTY_ROWS = (0, 77, 300, N - 1)
PROBE_ROWS = [5, 11, 14, 16, 401]


def _corpus():
    rng = np.random.default_rng(61)
    X = rng.standard_normal((N, D)).astype(np.float32)
    lens = rng.integers(3, 30, N)
    lens[list(EMPTY_ROWS)] = 0
    lens[200] = 150
    ptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(V, n, replace=False)) for n in lens]).astype(np.int32)
    val = (rng.random(idx.shape[0]) + 0.25).astype(np.float32)
    for r in range(N):                                   # unit norm: IP(x, x) = 1 > IP(x, y)
        if lens[r]:
            val[ptr[r]:ptr[r + 1]] /= np.float32(np.sqrt(np.sum(val[ptr[r]:ptr[r + 1]].astype(np.float64) ** 2)))
    ids = [ODD.get(r, f"chunk-{r:04d}") for r in range(N)]
    return X, (ptr, idx, val), ids


def _manager(corpus, n=N, **kw):
    X, csr, ids = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, **kw)
    for lo in range(0, n, 250):
        hi = min(n, lo + 250)
        mgr.add_rows(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]), ids=ids[lo:hi], contents=[f"text {r}" for r in range(lo, hi)],
                     doc_id=[f"doc-{r // 6:03d}" for r in range(lo, hi)], chunk_index=[r % 6 for r in range(lo, hi)],
                     token_count=list(range(lo, hi)))
    mgr.finalize()
    return mgr


@pytest.fixture(scope="module")
def world(gpu):
    corpus = _corpus()
    one, two = _manager(corpus), _manager(corpus, devices=[0, 0])
    assert one._main.n_shards == 1 and two._main.n_shards == 2
    yield one, two, corpus
    for m in (one, two):
        asyncio.run(m.close())


def _payload(csr, r):
    return csr[1][csr[0][r]:csr[0][r + 1]], csr[2][csr[0][r]:csr[0][r + 1]]


def _assert_payloads(got, rows, corpus):
    X, csr, ids = corpus
    assert [h["id"] for h in got] == [ids[r] for r in rows]
    for h, r in zip(got, rows):
        e = h["embedding"]
        assert list(e) == ["indices", "values"] and e["indices"].dtype == np.int32 and e["values"].dtype == np.float32
        wi, wv = _payload(csr, r)
        assert np.array_equal(e["indices"], wi) and np.array_equal(e["values"].view(np.uint32), wv.view(np.uint32)), r


def _q(m, *a, **kw):
    return asyncio.run(m.query("sparse_index", *a, **kw))


def test_query_returns_the_ingested_payloads(world):
    one, two, corpus = world
    docs = ["doc-050", "doc-000", "doc-033", "doc-012", "doc-102", "doc-nope"]
    expr = "doc_id in [" + ", ".join(f'"{d}"' for d in docs) + "]"
    rows = [r for r in range(N) if f"doc-{r // 6:03d}" in docs]
    assert 0 in rows and 77 in rows and 200 in rows and N - 1 in rows        # empty rows and the long one among them
    for m in (one, two):
        before = dict(m.stats)
        got = _q(m, expr, ["embedding", "chunk_index"])
        assert m.stats["queries"] == before["queries"] + 1
        assert m.stats["query_device"] == before["query_device"] + (1 if m is one else 0)
        _assert_payloads(got, rows, corpus)
        assert all(list(h) == ["id", "chunk_index", "embedding"] and h["chunk_index"] == r % 6 for h, r in zip(got, rows))
        for r in (0, 77, N - 1):
            e = got[rows.index(r)]["embedding"]
            assert e["indices"].shape == e["values"].shape == (0,)
        pages, offset = [], 0
        while True:                                                          # pages concatenate
            page = _q(m, expr, ["embedding"], limit=7, offset=offset)
            pages += page
            offset += 7
            if len(page) < 7:
                break
        _assert_payloads(pages, rows, corpus)
        _assert_payloads(_q(m, None, ["embedding"], limit=N), list(range(N)), corpus)
        # a read-back payload is a query as it stands
        hits = asyncio.run(m.search(got[rows.index(200)]["embedding"], "sparse_index", top_k=3))
        assert hits[0]["_row"] == 200


def test_query_after_delete_and_compact(gpu):
    corpus = _corpus()
    X, csr, ids = corpus
    for kw in ({}, {"devices": [0, 0]}):
        m = _manager(corpus, **kw)
        try:
            asyncio.run(m.delete_by_filter("sparse_index", "chunk_index == 2 or token_count < 40"))
            survivors = [r for r in range(N) if r % 6 != 2 and r >= 40]
            _assert_payloads(_q(m, None, ["embedding"], limit=N), survivors, corpus)
            assert m.compact()["rows_after"] == len(survivors)
            _assert_payloads(_q(m, None, ["embedding"], limit=N), survivors, corpus)
            _assert_payloads(_q(m, "chunk_index >= 4", ["embedding"], limit=50, offset=3),
                             [r for r in survivors if r % 6 >= 4][3:53], corpus)
            # by id after the renumbering
            hits = asyncio.run(m.search_by_ids([ids[401]], "sparse_index", top_k=3))[0]
            assert hits[0]["id"] == ids[401] and hits[0]["_row"] == survivors.index(401)
        finally:
            asyncio.run(m.close())


def test_rows_without_a_sparse_row_read_back_empty(gpu):
    corpus = _corpus()
    X, csr, ids = corpus
    n, bare = 120, 9
    for kw in ({}, {"devices": [0, 0]}):
        m = _manager(corpus, n=n, **kw)
        try:
            m.add_rows(X[n:n + bare], None, ids=ids[n:n + bare], doc_id=["bare"] * bare, chunk_index=[0] * bare)
            m.finalize()
            assert m._main.num_rows == n + bare and m._main.num_sparse_rows == n
            got = _q(m, 'doc_id == "bare" or chunk_index == 5', ["embedding"])
            rows = [r for r in range(n + bare) if r >= n or r % 6 == 5]
            assert [h["id"] for h in got] == [ids[r] for r in rows]
            for h, r in zip(got, rows):
                wi, wv = _payload(csr, r) if r < n else (np.zeros(0, np.int32), np.zeros(0, np.float32))
                assert np.array_equal(h["embedding"]["indices"], wi) and np.array_equal(h["embedding"]["values"], wv)
                assert h["embedding"]["indices"].dtype == np.int32 and h["embedding"]["values"].dtype == np.float32
        finally:
            asyncio.run(m.close())


def _search(m, *a, **kw):
    return asyncio.run(m.search(*a, **kw))


def _by_ids(m, *a, **kw):
    return asyncio.run(m.search_by_ids(*a, **kw))


def _stored(X):
    return X.astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("kw", [{}, {"top_k": 9, "filters": "chunk_index >= 2 and token_count < 500"},
                                {"top_k": 6, "group_by_field": "doc_id"}], ids=["plain", "filter", "grouped"])
def test_search_by_ids_equals_search_with_the_stored_vector(world, kw):
    one, two, corpus = world
    X, csr, ids = corpus
    req = [ids[r] for r in PROBE_ROWS]
    for m in (one, two):
        before = m.stats["search_by_ids"]
        got = _by_ids(m, req, "semantic_index", **kw)
        assert len(got) == len(req) and m.stats["search_by_ids"] == before + 1
        for r, hits in zip(PROBE_ROWS, got):
            assert hits == _search(m, _stored(X[r]), "semantic_index", **kw), r
            if not kw:
                assert len(hits) == 20 and hits[0]["id"] == ids[r] and hits[0]["_row"] == r
        got = _by_ids(m, req, "sparse_index", **kw)
        for r, hits in zip(PROBE_ROWS, got):
            wi, wv = _payload(csr, r)
            assert hits == _search(m, {"indices": wi, "values": wv}, "sparse_index", **kw), r
            if not kw:
                assert hits[0]["id"] == ids[r] and hits[0]["_row"] == r
    assert _by_ids(one, req, "semantic_index", **kw) == _by_ids(two, req, "semantic_index", **kw)
    assert _by_ids(one, req, "sparse_index", **kw) == _by_ids(two, req, "sparse_index", **kw)


def test_odd_ids_duplicates_and_the_synchronous_form(world):
    one, two, corpus = world
    X, csr, ids = corpus
    for m in (one, two):
        odd = [ids[r] for r in sorted(ODD)]
        got = _by_ids(m, odd, "semantic_index", top_k=4)
        assert [hits[0]["id"] for hits in got] == odd                          # quotes, backslashes, ", " and shared prefixes
        assert [hits[0]["_row"] for hits in got] == sorted(ODD)
        dup = _by_ids(m, [ids[15], ids[40], ids[15]], "sparse_index", top_k=5)
        assert dup[0] == dup[2] and dup[0][0]["_row"] == 15 and dup[1][0]["_row"] == 40
        empty = _by_ids(m, [ids[77]], "sparse_index", top_k=5)[0]              # no entries: what search() gives for the empty payload
        assert empty == _search(m, {"indices": np.zeros(0, np.int32), "values": np.zeros(0, np.float32)}, "sparse_index", top_k=5)
        sync = m.collections["semantic_index"].search_by_ids([ids[5], ids[12]], 6, "chunk_index != 3")
        assert sync == _by_ids(m, [ids[5], ids[12]], "semantic_index", top_k=6, filters="chunk_index != 3")
    assert one._filters_on_device().stats["undecided_rows"] > 0                # the shared 16-byte prefix went through the host


def test_range_filter_drops_the_entity(world):
    one, two, corpus = world
    X, csr, ids = corpus
    params = {"metric_type": "COSINE", "params": {"radius": -1.0, "range_filter": 0.99}}
    for m in (one, two):
        plain = _by_ids(m, [ids[5]], "semantic_index", top_k=6)[0]
        ranged = _by_ids(m, [ids[5]], "semantic_index", top_k=5, search_params=params)[0]
        assert plain[0]["id"] == ids[5] and ranged == plain[1:]
        assert ranged == _search(m, _stored(X[5]), "semantic_index", top_k=5, search_params=params)


def test_l2_distance_to_itself_is_zero(gpu):
    corpus = _corpus()
    X, csr, ids = corpus
    for kw in ({}, {"devices": [0, 0]}):
        m = _manager(corpus, n=250, semantic_metric="L2", **kw)
        try:
            for r, hits in zip((3, 12, 249), _by_ids(m, [ids[3], ids[12], ids[249]], "semantic_index", top_k=4)):
                assert hits[0]["id"] == ids[r] and hits[0]["score"] == 0.0
                assert hits == _search(m, _stored(X[r]), "semantic_index", top_k=4)
        finally:
            asyncio.run(m.close())


def test_refusals(gpu):
    corpus = _corpus()
    X, csr, ids = corpus
    for kw in ({}, {"devices": [0, 0]}):
        m = _manager(corpus, n=250, **kw)
        try:
            for bad in ([], "chunk-0001", None, [3], ["chunk-0001", None], ["nope"], ['say "hi'], ["chunk-0001 "]):
                with pytest.raises(ValueError):
                    _by_ids(m, bad, "semantic_index")
            with pytest.raises(ValueError) as ei:
                _by_ids(m, ["chunk-0001", "no such id"], "sparse_index")
            assert "no such id" in str(ei.value)
            with pytest.raises(ValueError):
                _by_ids(m, ["chunk-0001"], "no_such_collection")
            with pytest.raises(ValueError):
                _by_ids(m, [f"id-{i}" for i in range(4097)], "semantic_index")         # the filter language's list cap
            with pytest.raises(ValueError):
                _by_ids(m, ["chunk-0001"], "semantic_index", group_size=2)            # search()'s own refusal
            with pytest.raises(ValueError):
                _by_ids(m, ["chunk-0001"], "sparse_index", search_params={"metric_type": "IP", "params": {"radius": 0.1}})
            asyncio.run(m.delete_by_filter("semantic_index", 'id == "chunk-0020"'))
            with pytest.raises(ValueError) as ei:
                _by_ids(m, ["chunk-0021", "chunk-0020"], "semantic_index")
            assert "chunk-0020" in str(ei.value)
            assert _by_ids(m, ["chunk-0021"], "semantic_index", top_k=3)[0][0]["id"] == "chunk-0021"
        finally:
            asyncio.run(m.close())


def test_a_stored_row_longer_than_a_query_may_be_is_refused(gpu):
    """search() refuses a sparse query of more than HR_MAX_QUERY_NNZ entries (HR_ELIMIT); a stored row may be longer, and
    search_by_ids lets that refusal through as it is."""
    max_query_nnz = 4096                                  # HR_MAX_QUERY_NNZ of include/hbmrag.h
    rng = np.random.default_rng(3)
    v, n = max_query_nnz + 200, 40
    lens = np.full(n, 5)
    lens[7] = max_query_nnz + 1
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(v, k, replace=False)) for k in lens]).astype(np.int32)
    val = (rng.random(idx.shape[0]) + 0.25).astype(np.float32)
    m = MilvusIndexManager(semantic_dim=D, sparse_dim=v, enable_domain=False)
    try:
        m.add_rows(rng.standard_normal((n, D)).astype(np.float32), (ptr, idx, val), ids=[f"c{r}" for r in range(n)])
        m.finalize()
        got = asyncio.run(m.query("sparse_index", 'id == "c7"', ["embedding"]))[0]["embedding"]       # reading it back is fine
        assert np.array_equal(got["indices"], idx[ptr[7]:ptr[8]])
        with pytest.raises(Exception) as direct:
            _search(m, got, "sparse_index", top_k=3)
        assert "HR_MAX_QUERY_NNZ" in str(direct.value)
        with pytest.raises(type(direct.value)) as by_id:
            _by_ids(m, ["c7"], "sparse_index", top_k=3)
        assert str(by_id.value) == str(direct.value)
        assert "c8" in [h["id"] for h in _by_ids(m, ["c8"], "sparse_index", top_k=3)[0]]      # the other rows still answer
    finally:
        asyncio.run(m.close())
