"""multi_search and retrieve_multi end to end on the device: the fused ranking against the restatements
(retrieval.rrf_rank_lists / score_fuse_lists) applied to the manager's own search() results — ids, score bits, requests —
for both rankers, the cut at `limit`, the launches the batching front makes for same-key wordings, and two shards."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.multi_search import RRFRanker, SearchRequest, WeightedRanker
from advanced_rag.retrieval import norm_code, rrf_rank_lists, score_fuse_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, DD, V, NQ = 3001, 64, 32, 512, 8


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


class KeyedGen:
    """Embeddings keyed by the trailing query number of the text ("... q<i>")."""

    def __init__(self, Q, SQ):
        self.Q, self.SQ = Q, SQ

    def encode_semantic(self, text):
        return self.Q[int(text.rsplit("q", 1)[1])]

    def encode_sparse(self, text):
        qi, qv = self.SQ[int(text.rsplit("q", 1)[1])]
        return {"indices": qi.tolist(), "values": qv.astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(DD, np.float32)


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(47)
    X = rng.standard_normal((N, D)).astype(np.float32)
    XD = rng.standard_normal((N, DD)).astype(np.float32)
    nnz = 6
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(N)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((N, nnz))) * 3 + 0.1).astype(np.float32)
    csr = (np.arange(N + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(N)],
                   doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 7 for r in range(N)],
                   entropy=[(r % 13) / 13.0 for r in range(N)])
    base = rng.standard_normal(D).astype(np.float32)
    Q = (base[None, :] + 0.6 * rng.standard_normal((NQ, D))).astype(np.float32)      # wordings of one question: lists overlap
    SQ = [(np.sort(rng.choice(V, 60, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(60)) + 0.5).astype(np.float32))
          for _ in range(NQ)]
    QD = rng.standard_normal((2, DD)).astype(np.float32)
    return X, XD, csr, payload, Q, SQ, QD


def manager(corpus, **kw):
    X, XD, csr, payload, Q, SQ, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, domain_dim=DD, enable_domain=True, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr._domain.add(XD)                      # row-aligned with the main collections, as index_chunks keeps it
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(Q, SQ)
    return mgr


@pytest.fixture(scope="module")
def one_shard(corpus):
    mgr = manager(corpus)
    yield mgr
    asyncio.run(mgr.close())


def requests(corpus, ranged=False):
    _, _, _, _, Q, SQ, QD = corpus
    sparse = {"indices": SQ[0][0].tolist(), "values": SQ[0][1].astype(float).tolist()}
    reqs = [SearchRequest(Q[i], "semantic_index", 40, filters="chunk_index >= 1") for i in range(5)]
    reqs.append(SearchRequest(sparse, "sparse_index", 25, filters="chunk_index <= 5",
                              search_params={"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
    reqs.append(SearchRequest(QD[0], "domain_index", 30, filters="entropy < 0.8"))
    if ranged:
        reqs.append(SearchRequest(Q[5], "semantic_index", 50, search_params={"metric_type": "COSINE", "params": {"radius": 0.05}}))
    return reqs


def expected(mgr, reqs, ranker, limit):
    """The restatement over the search() results of the requests -> [(row, id, score hex, original score, requests)]."""
    lists = [asyncio.run(mgr.search(r.data, r.collection_name, r.limit, r.filters, r.search_params)) for r in reqs]
    assert all(lists)
    rows = [[h["_row"] for h in hits] for hits in lists]
    if isinstance(ranker, RRFRanker):
        fused = rrf_rank_lists(rows, ranker.weights or [1.0] * len(reqs), ranker.k)
    else:
        norms = [norm_code("IP" if r.collection_name == "sparse_index" else "COSINE", ranker.normalization) for r in reqs]
        fused = score_fuse_lists([(rw, [h["score"] for h in hits]) for rw, hits in zip(rows, lists)], ranker.weights, norms)
    out = []
    for row, score, held in fused[:limit]:
        first = next(h for h in lists[held[0]] if h["_row"] == row)
        out.append((row, first["id"], float(score).hex(), first["score"], held))
    return out, len(fused)


def got(hits):
    return [(h["_row"], h["id"], float(h["score"]).hex(), h["original_score"], h["requests"]) for h in hits]


RANKERS = [RRFRanker(), RRFRanker(20, [1.0, 0.9, 0.8, 0.7, 0.6, 1.5, 0.5]), WeightedRanker(0.3, 0.3, 0.2, 0.1, 0.1, 0.5, 0.25),
           WeightedRanker(1.0, 1.0, 1.0, 1.0, 1.0, 2.0, -0.5, normalization="minmax")]


@pytest.mark.parametrize("ranker", RANKERS, ids=repr)
def test_multi_search_equals_the_restatement_over_seven_searches(gpu, corpus, one_shard, ranker):
    mgr = one_shard
    reqs = requests(corpus)
    want, n_fused = expected(mgr, reqs, ranker, 768)
    assert 60 < n_fused < 768 and any(len(w[4]) >= 3 for w in want) and {5, 6} <= {l for w in want for l in w[4]}
    before = mgr.stats["multi_searches"]
    for limit in (1, 10, 768):                       # the cut at `limit`; fewer fused rows than limit: a shorter list
        hits = asyncio.run(mgr.multi_search(reqs, ranker, limit))
        assert got(hits) == want[:limit] and len(hits) == min(limit, n_fused)
    assert set(hits[0]) >= {"id", "content", "metadata", "score", "original_score", "requests", "_row"}
    assert mgr.stats["multi_searches"] == before + 3 and mgr._front.stats["fuse_n_launches"] >= 3


def test_a_range_request_and_refusals(gpu, corpus, one_shard):
    mgr = one_shard
    reqs = requests(corpus, ranged=True)
    ranker = RRFRanker(60, [1.0] * 8)
    want, _ = expected(mgr, reqs, ranker, 30)
    assert any(7 in w[4] for w in want)
    assert got(asyncio.run(mgr.multi_search(reqs, ranker, 30))) == want
    launches = dict(mgr._front.stats)
    ok = reqs[0]
    for bad, kw in (([], {}), ([ok] * 17, {}), ([ok, "x"], {}), ([SearchRequest(ok.data, "nope", 5)], {}), ([ok], dict(limit=769)),
                    ([ok], dict(limit=2.0)), ([ok], dict(ranker="rrf")), ([ok, ok], dict(ranker=WeightedRanker(1.0))),
                    ([SearchRequest(ok.data, "semantic_index", 5, search_params={"metric_type": "L2"})], {}),
                    ([SearchRequest(ok.data, "semantic_index", 5, search_params={"params": {"radius": 0.9, "range_filter": 0.1}})], {}),
                    ([SearchRequest(reqs[5].data, "sparse_index", 5, search_params={"metric_type": "IP", "params": {"radius": 1.0}})], {})):
        with pytest.raises(ValueError):
            asyncio.run(mgr.multi_search(bad, kw.get("ranker", RRFRanker()), kw.get("limit", 10)))
    assert {k: v for k, v in mgr._front.stats.items() if k.endswith("launches")} == \
        {k: v for k, v in launches.items() if k.endswith("launches")}            # nothing was searched


def test_five_same_key_wordings_cost_one_dense_launch_and_one_fusion_launch(gpu, corpus, one_shard):
    mgr = one_shard
    reqs = requests(corpus)[:5]
    asyncio.run(mgr.multi_search(reqs, RRFRanker(), 10))                  # (the worker, the streams and the row mask exist)
    front = mgr._front
    old, front.window_s = front.window_s, 5e-3                           # a round waits for its stragglers
    try:
        st0 = dict(front.stats)
        hits = asyncio.run(mgr.multi_search(reqs, RRFRanker(), 10))
        st = {k: front.stats[k] - st0[k] for k in ("dense_launches", "sparse_launches", "fuse_n_launches", "fuse_launches",
                                                     "score_fuse_launches", "hybrid_launches", "requests")}
        assert st == {"dense_launches": 1, "sparse_launches": 0, "fuse_n_launches": 1, "fuse_launches": 0,
                      "score_fuse_launches": 0, "hybrid_launches": 0, "requests": 6}, st
        assert got(hits) == expected(mgr, reqs, RRFRanker(), 10)[0]

        # concurrent calls with different weights (and different limits of the fusion: another key) share what they can
        async def burst():
            return await asyncio.gather(*[mgr.multi_search(reqs, RRFRanker(60, [1.0, 0.5 + 0.1 * i, 1.0, 1.0, 1.0]), 10)
                                          for i in range(4)])
        st0 = dict(front.stats)
        outs = asyncio.run(burst())
        assert front.stats["fuse_n_launches"] - st0["fuse_n_launches"] == 1 and front.stats["dense_launches"] - st0["dense_launches"] == 1
        for i, o in enumerate(outs):
            assert got(o) == expected(mgr, reqs, RRFRanker(60, [1.0, 0.5 + 0.1 * i, 1.0, 1.0, 1.0]), 10)[0]
    finally:
        front.window_s = old


def _fused_key(hits):
    return [(h["id"], float(h["score"]).hex(), h["retrieval_methods"]) for h in hits]


@pytest.mark.parametrize("fusion", ["rrf", "weighted"])
def test_retrieve_multi_against_the_restatement_and_against_retrieve(gpu, long_timeout, corpus, one_shard, fusion):
    mgr = one_shard
    gen = mgr.embedding_generator
    top_k = 10
    texts = [f"wording q{i}" for i in (0, 3, 1, 6)]
    qw = [1.0, 0.75, 0.5, 0.25]
    initialize_caches()
    retr = HybridRetriever(mgr, RetrievalConfig(top_k=top_k, fusion=fusion))
    st0 = mgr._front.stats["fuse_n_launches"]
    hits = asyncio.run(retr.retrieve_multi(texts, filters={"chunk_index": {"$gte": 1}}, profile_hint="default", query_weights=qw))
    assert mgr._front.stats["fuse_n_launches"] == st0 + 1
    lists = []
    for t in texts:
        lists.append(asyncio.run(mgr.search(gen.encode_semantic(t), "semantic_index", 2 * top_k, "chunk_index >= 1",
                                            retr.config.semantic_search_params)))
        lists.append(asyncio.run(mgr.search(gen.encode_sparse(t), "sparse_index", 2 * top_k, "chunk_index >= 1",
                                            retr.config.sparse_search_params)))
    w = [x * q for q in qw for x in (0.7, 0.3)]
    if fusion == "rrf":
        want = rrf_rank_lists([[h["id"] for h in l] for l in lists], w, 60)[:top_k]
    else:
        want = score_fuse_lists([([h["id"] for h in l], [h["score"] for h in l]) for l in lists], w, [0, 1] * 4)[:top_k]
    names = ("semantic", "sparse")
    assert _fused_key(hits) == [(i, float(s).hex(), [names[m] for m in sorted({l % 2 for l in ls})]) for i, s, ls in want]
    assert [h["queries"] for h in hits] == [[texts[i] for i in sorted({l // 2 for l in ls})] for _, _, ls in want]
    assert any(len(h["queries"]) > 1 for h in hits) and all("_row" not in h for h in hits)
    # one wording: what retrieve() gives (the one-round path), with and without MMR
    for mmr in (False, True):
        for q in (2, 5):
            cfg = dict(top_k=top_k, fusion=fusion, enable_mmr=mmr, mmr_lambda=0.6)
            initialize_caches()
            one = asyncio.run(HybridRetriever(mgr, RetrievalConfig(**cfg)).retrieve(f"wording q{q}", profile_hint="default"))
            many = asyncio.run(HybridRetriever(mgr, RetrievalConfig(**cfg)).retrieve_multi([f"wording q{q}"], profile_hint="default"))
            assert _fused_key(one) == _fused_key(many) and len(one) == top_k


def test_a_search_keeps_its_shard_mask_while_another_filter_takes_the_cache(gpu, corpus):
    """The requests of one multi_search run in threads of their own, and the semantic and the sparse collection share one
    ShardSet, which keeps the packed device mask of the filter used LAST.  A search is handed a raw device pointer into
    that entry: when another thread's filter replaces the entry, the mask under the pointer must stay allocated and
    intact until the first thread's search is over.  (It was freed, and the next upload or allocation of that size got
    its block: searches of two shards then ran under another filter's, or another shard's, mask now and then.)"""
    import threading
    Q = corpus[4]
    two = manager(corpus, devices=[0, 0])
    try:
        ss = two._main
        a = np.random.default_rng(3).random(N) < 0.5
        b = ~a
        h = ss.handles[0]
        own = np.packbits(a[ss.rows_of[0]], bitorder="little")
        want = h.search_dense(Q[:1], 40, own)                    # the host form under a's local mask, uploaded by the call
        args = ss._local_mask(0, a)                              # what a search of THIS thread is handed
        assert args[0] is None and args[1]
        t = threading.Thread(target=ss._local_mask, args=(0, b))  # another thread's filter takes the cache entry
        t.start()
        t.join()
        grab = [torch.zeros(own.size, dtype=torch.uint8, device="cuda") for _ in range(16)]   # a freed block would be handed out here
        torch.cuda.synchronize()
        assert all(g.data_ptr() != args[1] for g in grab)
        have = h.search_dense(Q[:1], 40, *args)
        assert np.array_equal(have[0], want[0]) and np.array_equal(have[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        asyncio.run(two.close())


def test_two_shards_give_the_same_answer(gpu, long_timeout, corpus, one_shard):
    reqs = requests(corpus)
    texts = [f"wording q{i}" for i in (0, 3, 1)]
    two = manager(corpus, devices=[0, 0])
    try:
        assert two._coalescer(two.collections["semantic_index"]) is None
        for ranker in (RANKERS[1], RANKERS[3]):
            assert got(asyncio.run(two.multi_search(reqs, ranker, 100))) == got(asyncio.run(one_shard.multi_search(reqs, ranker, 100)))
        for fusion in ("rrf", "weighted"):
            answers = []
            for mgr in (one_shard, two):
                initialize_caches()
                retr = HybridRetriever(mgr, RetrievalConfig(top_k=10, fusion=fusion))
                answers.append(_fused_key(asyncio.run(retr.retrieve_multi(texts, profile_hint="default"))))
            assert answers[0] == answers[1] and len(answers[0]) == 10
    finally:
        asyncio.run(two.close())
