"""Search iterator end to end: MilvusIndexManager.search_iterator pages against the oracle's ranking mapped through the
payload, hit dict for hit dict — one shard with the mask in HBM, two shards behind one cursor, the sparse collection,
filters, range bounds, deletes and appends between pages, compaction, and one walk past 16 384 rows."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag import MilvusIndexManager, SearchIterator
from advanced_rag import _native as nat

import range_yardstick as ry
from l2_yardstick import l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V = 3000, 32, 64
CODE = {"IP": nat.HR_METRIC_IP, "COSINE": nat.HR_METRIC_COSINE, "L2": nat.HR_METRIC_L2}


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(41)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X[rng.permutation(N)[:200]] = X[7]                            # a long run of equal scores in every ranking
    val = (rng.integers(1, 16, (N, 4)) / 4).astype(np.float32)
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, (N, 4))).astype(np.int32)
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    Q = rng.standard_normal((4, D)).astype(np.float32)
    sq = {"indices": list(range(0, V, 2)), "values": [1.0] * (V // 2)}
    return X, csr, Q, sq


def _payload(lo, hi):
    return dict(ids=[f"c{r}" for r in range(lo, hi)], contents=[f"text {r}" for r in range(lo, hi)],
                doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 7 for r in range(lo, hi)])


def _manager(corpus, metric="COSINE", **kw):
    X, csr, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, semantic_metric=metric, **kw)
    mgr.add_rows(X, csr, **_payload(0, N))
    mgr.finalize()
    return mgr


def _want(mgr, X, q, metric, mask=None):
    """The complete ranking as hit dicts."""
    X = X.astype(np.float16)                                      # what the shard stores
    packed = None if mask is None else np.packbits(mask, bitorder="little")
    n = X.shape[0]
    ids, sc = l2_search(X, q[None, :], n, packed) if metric == "L2" else oracle.dense_search(X, q[None, :], n, CODE[metric], packed)
    return mgr._format_hits(ids[0], sc[0])


def _walk(it):
    pages = []
    while True:
        page = it.next_blocking()
        if not page:
            return pages
        pages.append(page)


def _flat(pages):
    return [h for p in pages for h in p]


@pytest.mark.parametrize("metric", ["COSINE", "L2", "IP"])
def test_pages_are_slices_of_the_ranking(gpu, corpus, metric):
    X, csr, Q, _ = corpus
    mgr = _manager(corpus, metric)
    try:
        q = Q[0]
        want = _want(mgr, X, q, metric)
        assert len(want) == N
        fetched = 0
        for batch, limit in ((100, 250), (256, None), (257, None), (1000, None), (1000, 250), (16384, None)):
            it = mgr.search_iterator(q, "semantic_index", batch_size=batch, limit=limit)
            assert isinstance(it, SearchIterator) and it.returned == 0
            pages = _walk(it)
            n = N if limit is None else limit
            assert [len(p) for p in pages] == [batch] * (n // batch) + ([n % batch] if n % batch else [])
            assert _flat(pages) == want[:n] and it.returned == n and it.next_blocking() == []
            # a full last page is followed by one empty fetch unless `limit` ended the walk
            fetched += len(pages) + (1 if limit is None and n % batch == 0 else 0)
            assert mgr.stats["iterator_pages"] == fetched
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=1000)) == want[:1000]      # search() and the pages agree
        assert mgr.stats["deep_searches"] == 1
        # a filter expression (evaluated on the device, the mask never leaves HBM)
        chunk = np.arange(N) % 7
        pages = _walk(mgr.search_iterator(q, "semantic_index", batch_size=700, filters="chunk_index >= 2"))
        assert _flat(pages) == _want(mgr, X, q, metric, chunk >= 2) and len(pages) == 4
    finally:
        asyncio.run(mgr.close())


def test_sparse_collection_async_for_and_the_collection_form(gpu, corpus):
    X, (indptr, idx, val), Q, sq = corpus
    mgr = _manager(corpus)
    try:
        ids, sc = oracle.sparse_search(indptr, idx, val, [(sq["indices"], sq["values"])], N)
        want = mgr._format_hits(ids[0], sc[0])
        assert 2000 < len(want) <= N
        assert _flat(_walk(mgr.search_iterator(sq, "sparse_index", batch_size=900))) == want
        with pytest.raises(ValueError, match="sparse"):
            mgr.search_iterator(sq, "sparse_index", search_params={"metric_type": "IP", "params": {"radius": 1.0}})

        async def collect(it):
            return [page async for page in it]
        it = mgr.search_iterator(Q[1], "semantic_index", batch_size=1200, limit=2500)
        pages = asyncio.run(collect(it))
        assert [len(p) for p in pages] == [1200, 1200, 100] and _flat(pages) == _want(mgr, X, Q[1], "COSINE")[:2500]
        assert asyncio.run(it.next()) == [] and it.returned == 2500
        it = mgr.collections["semantic_index"].search_iterator(Q[1], batch_size=1500, filters="chunk_index >= 2")
        assert _flat(_walk(it)) == _want(mgr, X, Q[1], "COSINE", np.arange(N) % 7 >= 2)
        it = mgr.search_iterator(Q[1], "semantic_index", batch_size=50)
        first = it.next_blocking()
        it.close()
        pages = mgr.stats["iterator_pages"]
        assert len(first) == 50 and it.next_blocking() == [] and asyncio.run(it.next()) == [] and it.returned == 50
        assert mgr.stats["iterator_pages"] == pages
    finally:
        asyncio.run(mgr.close())


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_radius_against_the_range_yardstick(gpu, corpus, metric):
    X, csr, Q, _ = corpus
    mgr = _manager(corpus, metric)
    try:
        q = Q[2]
        code = {"COSINE": ry.COSINE, "L2": ry.L2}[metric]
        s = ry.scores(X.astype(np.float16), q, code)
        mid = float(np.sort(s)[N // 2])                           # a bound that sits on a score: half the rows pass radius
        for params in ({"radius": mid}, {"radius": mid, "range_filter": float(np.sort(s)[N // 4 if metric == "L2" else 3 * N // 4])}):
            ids, sc = ry.topk_in_range(s, code, N, params.get("radius"), params.get("range_filter"))
            want = mgr._format_hits(ids, sc)
            assert 500 < len(want) < N
            pages = _walk(mgr.search_iterator(q, "semantic_index", batch_size=400, search_params={"metric_type": metric, "params": params}))
            assert _flat(pages) == want
            head = asyncio.run(mgr.search(q, "semantic_index", top_k=200, search_params={"metric_type": metric, "params": params}))
            assert head == want[:200]                             # what search() returns for the same rows
    finally:
        asyncio.run(mgr.close())


def test_two_shards_share_one_cursor(gpu, corpus):
    X, csr, Q, sq = corpus
    one, two = _manager(corpus), _manager(corpus, devices=[0, 0])
    try:
        assert two._main.n_shards == 2
        for batch, expr in ((256, None), (1000, None), (700, "chunk_index >= 2")):
            a = _walk(one.search_iterator(Q[3], "semantic_index", batch_size=batch, filters=expr))
            b = _walk(two.search_iterator(Q[3], "semantic_index", batch_size=batch, filters=expr))
            assert a == b and len(_flat(a)) == (N if expr is None else int((np.arange(N) % 7 >= 2).sum()))
        params = {"metric_type": "COSINE", "params": {"radius": 0.0}}
        a = _walk(one.search_iterator(Q[3], "semantic_index", batch_size=300, search_params=params))
        assert a == _walk(two.search_iterator(Q[3], "semantic_index", batch_size=300, search_params=params)) and len(a) > 2
        a = _walk(one.search_iterator(sq, "sparse_index", batch_size=800))
        assert a == _walk(two.search_iterator(sq, "sparse_index", batch_size=800)) and len(_flat(a)) > 2000
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_mutations_between_pages(gpu, corpus, devices):
    X, csr, Q, _ = corpus
    mgr = _manager(corpus, **({"devices": devices} if devices else {}))
    try:
        q = Q[0]
        want = _want(mgr, X, q, "COSINE")
        it = mgr.search_iterator(q, "semantic_index", batch_size=500)
        first = it.next_blocking()
        assert first == want[:500]
        # a delete between pages: one row already returned, one not yet
        gone = [want[20]["_row"], want[700]["_row"]]
        asyncio.run(mgr.delete_by_filter("semantic_index", 'chunk_id in [' + ', '.join(f'"c{r}"' for r in gone) + ']'))
        second = it.next_blocking()
        assert second == [h for h in want[500:] if h["_row"] != gone[1]][:500]
        # an append between pages: a copy of the best row (its place is before the cursor) and of the worst (after it)
        extra = np.stack([X[want[0]["_row"]], X[want[-1]["_row"]]])
        sparse = (np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32), np.array([1.0, 1.0], np.float32))
        mgr.add_rows(extra, sparse, **_payload(N, N + 2))
        mgr.finalize()
        alive = np.ones(N + 2, bool)
        alive[gone] = False
        now = _want(mgr, np.concatenate([X, extra]), q, "COSINE", alive)
        rest = _flat(_walk(it))
        seen = first + second + rest
        assert len({h["_row"] for h in seen}) == len(seen)        # no hit twice
        assert N + 1 in [h["_row"] for h in rest] and N not in [h["_row"] for h in seen]
        cut = next(i for i, h in enumerate(now) if h["_row"] == second[-1]["_row"])
        assert rest == now[cut + 1:]
        # compact() renumbers the rows: the iterator refuses, a new one walks the new numbering
        it = mgr.search_iterator(q, "semantic_index", batch_size=400)
        assert it.next_blocking() == now[:400]
        mgr.compact()
        with pytest.raises(RuntimeError, match=r"compact\(\)"):
            it.next_blocking()
        with pytest.raises(RuntimeError, match=r"compact\(\)"):
            asyncio.run(it.next())
        fresh = _flat(_walk(mgr.search_iterator(q, "semantic_index", batch_size=2000)))
        assert [(h["id"], h["score"]) for h in fresh] == [(h["id"], h["score"]) for h in now]
    finally:
        asyncio.run(mgr.close())


def test_creation_refusals(gpu, corpus):
    X, csr, Q, sq = corpus
    mgr = _manager(corpus)
    try:
        for kw, word in ((dict(batch_size=0), "batch_size"), (dict(batch_size=16385), "batch_size"), (dict(batch_size=True), "batch_size"),
                         (dict(batch_size=100.0), "batch_size"), (dict(limit=0), "limit"), (dict(limit=2.5), "limit"),
                         (dict(limit=True), "limit"), (dict(search_params={"metric_type": "L2"}), "metric_type"),
                         (dict(search_params={"params": {"radius": 0.9, "range_filter": 0.1}}), "empty range"),
                         (dict(search_params={"params": {"range_filter": float("nan")}}), "NaN")):
            with pytest.raises(ValueError, match=word):
                mgr.search_iterator(Q[0], "semantic_index", **kw)
            with pytest.raises(ValueError, match=word):
                mgr.collections["semantic_index"].search_iterator(Q[0], **kw)
        with pytest.raises(ValueError, match="not found"):
            mgr.search_iterator(Q[0], "no_such_index")
        assert mgr.stats["iterator_pages"] == 0                   # nothing was launched for any of them
    finally:
        asyncio.run(mgr.close())


def test_one_walk_past_the_deep_cap(gpu):
    rng = np.random.default_rng(77)
    n = 20_011
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[rng.permutation(n)[:300]] = X[5]
    q = rng.standard_normal(D).astype(np.float32)
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False)
    try:
        mgr.add_rows_synthetic(X)
        mgr.finalize()
        ids, sc = oracle.dense_search(X.astype(np.float16), q[None, :], n, nat.HR_METRIC_COSINE)
        pages = _walk(mgr.search_iterator(q, "semantic_index", batch_size=16384))
        assert [len(p) for p in pages] == [16384, n - 16384]
        assert _flat(pages) == mgr._format_hits(ids[0], sc[0])
    finally:
        asyncio.run(mgr.close())
