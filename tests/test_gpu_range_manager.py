"""Range search end to end: MilvusIndexManager.search(search_params={"params": {"radius": r, "range_filter": f}}) against
the numpy yardstick (tests/range_yardstick.py), hit dict for hit dict — through the batching front, the blocking paths (mask
in HBM, query in HBM, host mask over two shards), the domain collection, retrieve(), and the refusals."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest

import range_yardstick as ry
from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.batching import SearchCoalescer
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.shards import CollectiveShardSet

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, DD, V = 1500, 32, 8, 64
CODE = {"IP": ry.IP, "COSINE": ry.COSINE, "L2": ry.L2}


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(23)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Xdom = rng.standard_normal((N, DD)).astype(np.float32)
    val = np.abs(rng.standard_normal((N, 4))).astype(np.float32) + 0.1
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, (N, 4))).astype(np.int32)
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"text {r}" for r in range(N)],
                   doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 7 for r in range(N)])
    Q = rng.standard_normal((40, D)).astype(np.float32)
    sq = {"indices": list(range(0, V, 2)), "values": [1.0] * (V // 2)}
    return X, Xdom, csr, payload, Q, sq


def _manager(corpus, metric="COSINE", domain=False, **kw):
    X, Xdom, csr, payload, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, domain_dim=DD, enable_domain=domain, semantic_metric=metric, **kw)
    mgr.add_rows(X, csr, **payload)
    if domain:
        mgr._domain.add(Xdom)
    mgr.finalize()
    return mgr


def _between(s, metric, i):
    """A bound between the rows ranked i and i + 1 (best first) of one query's scores."""
    o = np.sort(s.astype(np.float64))
    o = o if metric == ry.L2 else o[::-1]
    return 0.5 * (o[i] + o[i + 1])


def _params(metric, radius=None, range_filter=None):
    p = {"ef": 64}
    if radius is not None:
        p["radius"] = radius
    if range_filter is not None:
        p["range_filter"] = range_filter
    return {"metric_type": metric, "params": p}


def _want(mgr, Xs, q, metric, top_k, radius, range_filter, mask=None):
    ids, sc = ry.range_search(Xs, q[None, :], top_k, CODE[metric], radius, range_filter, mask=mask)
    return mgr._format_hits(ids[0], sc[0])


@pytest.mark.parametrize("metric", ["COSINE", "L2", "IP"])
def test_search_with_radius_range_filter_and_both(gpu, corpus, metric):
    X, Xdom, csr, payload, Q, _ = corpus
    Xs = X.astype(np.float16)                                     # what the shard stores
    mgr = _manager(corpus, metric)
    try:
        q = Q[0]
        s = ry.scores(Xs, q, CODE[metric])
        worse, better = _between(s, CODE[metric], 12), _between(s, CODE[metric], 2)
        chunk = np.arange(N) % 7
        for expr, mask in ((None, None), ("chunk_index >= 2", chunk >= 2)):
            for top_k, r, f in ((8, worse, None), (8, None, better), (20, worse, better), (4, worse, better)):
                want = _want(mgr, Xs, q, metric, top_k, r, f, mask)
                assert 0 < len(want) <= top_k
                p = _params(metric, r, f)
                assert asyncio.run(mgr.search(q, "semantic_index", top_k=top_k, filters=expr, search_params=p)) == want
                # the blocking path: the mask never leaves the device; and the query already in HBM (device form, no mask)
                assert mgr._search_blocking(q, "semantic_index", top_k, expr, p) == want
                if expr is None:
                    assert mgr._search_blocking(torch.from_numpy(q).cuda(), "semantic_index", top_k, None, p) == want
        both = _want(mgr, Xs, q, metric, 20, worse, better)
        assert len(both) == 10                                    # ranks 3 .. 12: top_k is an upper limit, not a quota
        assert mgr._front.stats["range_launches"] >= 8
        # tombstones: the deleted rows leave the range search as they leave every search
        gone = [h["_row"] for h in both[:3]]
        asyncio.run(mgr.delete_by_filter("semantic_index", 'chunk_id in [' + ', '.join(f'"c{r}"' for r in gone) + ']'))
        alive = np.ones(N, bool)
        alive[gone] = False
        want = _want(mgr, Xs, q, metric, 20, worse, better, alive)
        assert [h["_row"] for h in want] == [h["_row"] for h in both[3:]]
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=20, search_params=_params(metric, worse, better))) == want
        assert mgr._search_blocking(q, "semantic_index", 20, None, _params(metric, worse, better)) == want
        # without range params: what it always was
        plain = asyncio.run(mgr.search(q, "semantic_index", top_k=6))
        ids, sc = ry.range_search(Xs, q[None, :], 6, CODE[metric], None, None, mask=alive)
        assert plain == mgr._format_hits(ids[0], sc[0])
    finally:
        asyncio.run(mgr.close())


def test_domain_collection(gpu, corpus):
    X, Xdom, csr, payload, Q, _ = corpus
    Xs = Xdom.astype(np.float16)
    mgr = _manager(corpus, domain=True)
    try:
        q = np.random.default_rng(4).standard_normal(DD).astype(np.float32)
        s = ry.scores(Xs, q, ry.COSINE)
        worse, better = _between(s, ry.COSINE, 30), _between(s, ry.COSINE, 5)
        for top_k, r, f in ((10, worse, None), (10, None, better), (40, worse, better)):
            want = _want(mgr, Xs, q, "COSINE", top_k, r, f)
            p = _params("COSINE", r, f)
            assert asyncio.run(mgr.search(q, "domain_index", top_k=top_k, search_params=p)) == want
            assert mgr._search_blocking(q, "domain_index", top_k, None, p) == want
        assert len(want) == 25
    finally:
        asyncio.run(mgr.close())


def test_ranged_searches_with_different_bounds_share_one_launch(gpu, corpus):
    X, Xdom, csr, payload, Q, _ = corpus
    Xs = X.astype(np.float16)
    mgr, fresh = _manager(corpus), _manager(corpus)
    try:
        mgr._front = SearchCoalescer(mgr, window_s=5e-3)          # a round waits 5 ms for its next request: one tick fits
        queries = [Q[i] for i in range(32)]
        radii = [_between(ry.scores(Xs, q, ry.COSINE), ry.COSINE, 3 + i) for i, q in enumerate(queries)]
        assert len(set(radii)) == 32
        plain_q = Q[33]
        want_plain = asyncio.run(fresh.search(plain_q, "semantic_index", top_k=7))
        sequential = [mgr._search_blocking(q, "semantic_index", 40, None, _params("COSINE", r)) for q, r in zip(queries, radii)]
        assert [len(h) for h in sequential] == [4 + i for i in range(32)]

        async def burst():
            return await asyncio.gather(*[mgr.search(q, "semantic_index", top_k=40, search_params=_params("COSINE", r))
                                          for q, r in zip(queries, radii)],
                                        mgr.search(plain_q, "semantic_index", top_k=7))

        st = mgr._front.stats
        before = dict(st)
        together = asyncio.run(burst())
        assert together[:32] == sequential
        assert together[32] == want_plain                          # the unranged search of the burst: today's answer
        assert st["range_launches"] - before["range_launches"] == 1          # one ranged launch, not 32
        assert st["dense_launches"] - before["dense_launches"] == 2          # ... beside the unranged one: no shared launch
        assert st["rounds"] - before["rounds"] == 1 and st["max_batch_seen"] == 32
        for q, r, got in zip(queries, radii, together):
            assert got == _want(mgr, Xs, q, "COSINE", 40, r, None)
    finally:
        asyncio.run(mgr.close())
        asyncio.run(fresh.close())


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_two_shards_give_the_single_shard_lists(gpu, corpus, metric):
    X, Xdom, csr, payload, Q, _ = corpus
    Xs = X.astype(np.float16)
    one, two = _manager(corpus, metric), _manager(corpus, metric, devices=[0, 0])
    try:
        assert two._main.n_shards == 2 and two._coalescer(two.collections["semantic_index"]) is None
        chunk = np.arange(N) % 7
        for i in range(3):
            q = Q[i]
            s = ry.scores(Xs, q, CODE[metric])
            worse, better = _between(s, CODE[metric], 25 + i), _between(s, CODE[metric], 4 + i)
            for expr, mask in ((None, None), ("chunk_index >= 2", chunk >= 2)):
                for top_k, r, f in ((10, worse, None), (10, None, better), (30, worse, better)):
                    p = _params(metric, r, f)
                    a = asyncio.run(one.search(q, "semantic_index", top_k=top_k, filters=expr, search_params=p))
                    b = asyncio.run(two.search(q, "semantic_index", top_k=top_k, filters=expr, search_params=p))
                    assert a == b == _want(one, Xs, q, metric, top_k, r, f, mask), (i, expr, top_k)
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


class _OneQueryGen:
    def __init__(self, q, sq):
        self.q, self.sq = q, sq

    def encode_semantic(self, text):
        return self.q

    def encode_sparse(self, text):
        return self.sq

    def encode_domain(self, text, domain=None):
        return np.zeros(DD, np.float32)


def test_retrieve_thresholds_the_semantic_list_before_fusion(gpu, long_timeout, corpus):
    X, Xdom, csr, payload, Q, sq = corpus
    Xs = X.astype(np.float16)
    mgr = _manager(corpus)
    try:
        q = Q[5]
        mgr.embedding_generator = _OneQueryGen(q, sq)
        top_k = 8
        initialize_caches()
        plain = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k)).retrieve("a statement"))
        assert any("semantic" in h["retrieval_methods"] for h in plain)
        launches = mgr._front.stats["hybrid_launches"]
        assert launches >= 1
        # a radius above every score: nothing semantic survives, the fused list is the sparse list
        initialize_caches()
        cfg = RetrievalConfig(top_k=top_k, semantic_search_params={"metric_type": "COSINE", "params": {"radius": 2.0}})
        got = asyncio.run(HybridRetriever(mgr, cfg).retrieve("a statement"))
        assert len(got) == top_k and all(h["retrieval_methods"] == ["sparse"] for h in got)
        spa = asyncio.run(mgr.search(sq, "sparse_index", top_k=2 * top_k, search_params=RetrievalConfig().sparse_search_params))
        assert [h["id"] for h in got] == [h["id"] for h in spa[:top_k]]
        assert mgr._front.stats["hybrid_launches"] == launches     # the one-round path declined
        # a radius that keeps the three best semantic rows: they are the only semantic hits of the fused list
        s = ry.scores(Xs, q, ry.COSINE)
        initialize_caches()
        cfg = RetrievalConfig(top_k=top_k, semantic_search_params=_params("COSINE", _between(s, ry.COSINE, 2)))
        got = asyncio.run(HybridRetriever(mgr, cfg).retrieve("a statement"))
        best3 = {f"c{r}" for r in np.lexsort((np.arange(N), -s))[:3]}
        assert {h["id"] for h in got if "semantic" in h["retrieval_methods"]} == best3
    finally:
        asyncio.run(mgr.close())


def test_hybrid_search_declines_a_semantic_range(gpu, corpus):
    X, Xdom, csr, payload, Q, sq = corpus
    mgr = _manager(corpus)
    try:
        kw = dict(top_k=5, filters=None, weights=(0.7, 0.3))

        async def both():
            return (await mgr.hybrid_search(Q[0], sq, semantic_params=_params("COSINE"), **kw),
                    await mgr.hybrid_search(Q[0], sq, semantic_params=_params("COSINE", 0.1), **kw),
                    await mgr.hybrid_search(Q[0], sq, semantic_params=_params("COSINE", None, 0.9), **kw))

        plain, with_radius, with_filter = asyncio.run(both())
        assert plain is not None and len(plain) == 5
        assert with_radius is None and with_filter is None
        # a range in the SPARSE params is declined too: the general path refuses it, whichever path retrieve() takes
        ranged_sparse = {"metric_type": "IP", "params": {"drop_ratio_search": 0.2, "radius": 0.5}}
        assert asyncio.run(mgr.hybrid_search(Q[0], sq, sparse_params=ranged_sparse, **kw)) is None
        with pytest.raises(ValueError, match="sparse"):
            asyncio.run(mgr.search(sq, "sparse_index", top_k=5, search_params=ranged_sparse))
    finally:
        asyncio.run(mgr.close())


def test_refusals_name_their_reason(gpu, corpus):
    X, Xdom, csr, payload, Q, sq = corpus
    mgr = _manager(corpus)
    try:
        for via in ("front", "blocking"):
            def search(query, coll, params, **kw):
                if via == "front":
                    return asyncio.run(mgr.search(query, coll, top_k=5, search_params=params, **kw))
                return mgr._search_blocking(query, coll, 5, None, params, kw.get("group_by_field"))
            with pytest.raises(ValueError, match="sparse"):
                search(sq, "sparse_index", {"metric_type": "IP", "params": {"radius": 0.5}})
            with pytest.raises(ValueError, match="group_by_field"):
                search(Q[0], "semantic_index", _params("COSINE", 0.1), group_by_field="doc_id")
            with pytest.raises(ValueError, match="empty range"):
                search(Q[0], "semantic_index", _params("COSINE", 0.9, 0.5))
            with pytest.raises(ValueError, match="NaN"):
                search(Q[0], "semantic_index", _params("COSINE", float("nan")))
        # the torchrun form: a collection whose shard set answers in rounds
        spread = SimpleNamespace(kind="dense", metric="COSINE", name="semantic_index", handle=SimpleNamespace(round=lambda *a: None))
        with pytest.raises(NotImplementedError, match="torchrun"):
            mgr._range_request(spread, _params("COSINE", 0.1), None)
        assert mgr._range_request(spread, _params("COSINE"), None) is None
        with pytest.raises(NotImplementedError, match="torchrun"):
            CollectiveShardSet.search_dense(SimpleNamespace(), Q[:1], 5, None, bounds=(0.1, 0.9))
    finally:
        asyncio.run(mgr.close())
