"""Deep search end to end: MilvusIndexManager.search(top_k, offset=) with offset + top_k up to 16 384 against the oracle's
ranking mapped through the payload, hit dict for hit dict (id, score, _row) — one shard with the mask in HBM, two shards
merged on the host, the sparse collection, filters, tombstones, paging across the 256 boundary, and the refusals."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from advanced_rag import MilvusIndexManager
from advanced_rag import _native as nat

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
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"text {r}" for r in range(N)],
                   doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 7 for r in range(N)])
    Q = rng.standard_normal((4, D)).astype(np.float32)
    sq = {"indices": list(range(0, V, 2)), "values": [1.0] * (V // 2)}
    return X, csr, payload, Q, sq


def _manager(corpus, metric="COSINE", **kw):
    X, csr, payload, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, semantic_metric=metric, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr.finalize()
    return mgr


def _ranking(corpus, q, metric, depth, mask=None):
    X = corpus[0].astype(np.float16)                              # what the shard stores
    packed = None if mask is None else np.packbits(mask, bitorder="little")
    if metric == "L2":
        return l2_search(X, q[None, :], depth, packed)
    return oracle.dense_search(X, q[None, :], depth, CODE[metric], packed)


def _want(mgr, corpus, q, metric, top_k, offset=0, mask=None):
    ids, sc = _ranking(corpus, q, metric, offset + top_k, mask)
    return mgr._format_hits(ids[0][offset:], sc[0][offset:])


@pytest.mark.parametrize("metric", ["COSINE", "L2", "IP"])
def test_deep_hits_paging_filters_and_tombstones(gpu, corpus, metric):
    X, csr, payload, Q, _ = corpus
    mgr = _manager(corpus, metric)
    try:
        q = Q[0]
        want = _want(mgr, corpus, q, metric, 1000)
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=1000))
        assert len(got) == 1000 and got == want                   # ids, scores, _row and the payload of every hit
        assert [h["_row"] for h in got] == [h["_row"] for h in want] and mgr.stats["deep_searches"] == 1
        # paging across the 256 boundary: W = 300 is deep, W = 200 is the plain search at top_k = 200 with 100 hits cut
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=100, offset=200)) == want[200:300]
        assert mgr.stats["deep_searches"] == 2
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=100, offset=100)) == want[100:200]
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=56, offset=200)) == want[200:256]   # W = 256: still plain
        assert mgr.stats["deep_searches"] == 2
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=20)) == want[:20]
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=N + 500))[:N] == _want(mgr, corpus, q, metric, N)
        assert len(asyncio.run(mgr.search(q, "semantic_index", top_k=N + 500))) == N     # a short ranking: no padding hits
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=50, offset=N - 10)) == _want(mgr, corpus, q, metric, 10, N - 10)
        # a filter expression (evaluated on the device, the mask never leaves HBM)
        chunk = np.arange(N) % 7
        want_f = _want(mgr, corpus, q, metric, 700, 0, chunk >= 2)
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=700, filters="chunk_index >= 2")) == want_f
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=300, offset=400, filters="chunk_index >= 2")) == want_f[400:]
        # tombstones
        gone = [h["_row"] for h in want[:3]] + [h["_row"] for h in want[300:303]]
        asyncio.run(mgr.delete_by_filter("semantic_index", 'chunk_id in [' + ', '.join(f'"c{r}"' for r in gone) + ']'))
        alive = np.ones(N, bool)
        alive[gone] = False
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=600)) == _want(mgr, corpus, q, metric, 600, 0, alive)
        assert asyncio.run(mgr.search(q, "semantic_index", top_k=300, offset=290, filters="chunk_index >= 2")) == \
            _want(mgr, corpus, q, metric, 300, 290, alive & (chunk >= 2))
    finally:
        asyncio.run(mgr.close())


def test_sparse_collection(gpu, corpus):
    X, (indptr, idx, val), payload, Q, sq = corpus
    mgr = _manager(corpus)
    try:
        ids, sc = oracle.sparse_search(indptr, idx, val, [(sq["indices"], sq["values"])], 1200)
        want = mgr._format_hits(ids[0], sc[0])
        assert len(want) > 600
        assert asyncio.run(mgr.search(sq, "sparse_index", top_k=1200)) == want
        assert asyncio.run(mgr.search(sq, "sparse_index", top_k=300, offset=250)) == want[250:550]
        assert asyncio.run(mgr.search(sq, "sparse_index", top_k=50, offset=100)) == want[100:150]
        assert mgr.stats["deep_searches"] == 2
    finally:
        asyncio.run(mgr.close())


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_two_shards_give_the_single_shard_lists(gpu, corpus, metric):
    X, csr, payload, Q, sq = corpus
    one, two = _manager(corpus, metric), _manager(corpus, metric, devices=[0, 0])
    try:
        assert two._main.n_shards == 2
        chunk = np.arange(N) % 7
        for i in range(2):
            for top_k, offset, expr, mask in ((1000, 0, None, None), (300, 700, None, None), (100, 200, None, None),
                                              (600, 100, "chunk_index >= 2", chunk >= 2)):
                want = _want(one, corpus, Q[i], metric, top_k, offset, mask)
                assert asyncio.run(one.search(Q[i], "semantic_index", top_k=top_k, offset=offset, filters=expr)) == want
                assert asyncio.run(two.search(Q[i], "semantic_index", top_k=top_k, offset=offset, filters=expr)) == want
        a = asyncio.run(one.search(sq, "sparse_index", top_k=400, offset=300))
        assert len(a) == 400 and asyncio.run(two.search(sq, "sparse_index", top_k=400, offset=300)) == a
        assert one.stats["deep_searches"] == two.stats["deep_searches"] == 9
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


def test_refusals(gpu, corpus):
    X, csr, payload, Q, sq = corpus
    mgr = _manager(corpus)
    try:
        def search(**kw):
            return asyncio.run(mgr.search(Q[0], "semantic_index", **kw))
        # the window rule
        for kw, word in ((dict(top_k=16385), r"offset \+ top_k"), (dict(top_k=16384, offset=1), r"offset \+ top_k"),
                         (dict(top_k=10, offset=16380), r"offset \+ top_k"), (dict(top_k=10, offset=-1), "offset"),
                         (dict(top_k=0, offset=5), "top_k"), (dict(top_k=10, offset=True), "offset"),
                         (dict(top_k=10, offset=2.0), "offset"), (dict(top_k=300.0, offset=1), "top_k")):
            with pytest.raises(ValueError, match=word):
                search(**kw)
        # a deep window with grouping, and with range params
        with pytest.raises(ValueError, match="group_by_field"):
            search(top_k=300, group_by_field="doc_id")
        with pytest.raises(ValueError, match="group_by_field"):
            search(top_k=100, offset=200, group_by_field="doc_id")
        for params in ({"radius": 0.1}, {"range_filter": 0.9}, {"radius": 0.1, "range_filter": 0.9}):
            with pytest.raises(ValueError, match="range search"):
                search(top_k=300, search_params={"metric_type": "COSINE", "params": params})
        # the torchrun form: a collection whose shard set answers in rounds
        spread = SimpleNamespace(kind="dense", metric="COSINE", name="semantic_index", handle=SimpleNamespace(round=lambda *a: None))
        with pytest.raises(NotImplementedError, match="torchrun"):
            mgr._deep_request(spread, 300, 0, None, None, 1)
        assert mgr._deep_request(spread, 200, 56, None, None, 1) == 256          # a plain window is not its business
        assert mgr.stats["deep_searches"] == 0                                   # nothing was launched for any of them
        # the limit itself is served
        assert len(search(top_k=16384)) == N
        assert len(search(top_k=1, offset=16383)) == 0
    finally:
        asyncio.run(mgr.close())
