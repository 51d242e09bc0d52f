"""Vector MMR end to end on one GPU shard: search(ranker=MMRRanker(...)) against the host restatement over the plain search
at depth W and the stored rows, concurrent requests with different lambdas in shared launches, a two-shard manager against
the one-shard one, search_by_ids, and retrieve() with mmr_similarity="embedding" without a token-set build."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.mmr import MMRRanker, vector_mmr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, DIM, DD, V, K, NQ = 3000, 8, 8, 64, 10, 4
HEADS = (0, 1000, 2500)          # every cluster: the head and five near-copies, 13 rows apart


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
        return self.SQ

    def encode_domain(self, text, domain=None):
        return np.zeros(DD, np.float32)


def _planted(rng, n, dim):
    X = rng.standard_normal((n, dim)).astype(np.float32)
    for c0 in HEADS:
        for j in range(1, 6):
            X[c0 + 13 * j] = X[c0] + np.float32(0.03) * rng.standard_normal(dim).astype(np.float32)
    return X


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(77)
    X, Xdom = _planted(rng, N, DIM), _planted(rng, N, DD)
    val = np.abs(rng.standard_normal((N, 4))).astype(np.float32) + 0.1
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, (N, 4))).astype(np.int32)
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(N)],
                   doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 7 for r in range(N)])
    Q = np.stack([X[c0] + np.float32(0.1) * rng.standard_normal(DIM).astype(np.float32) for c0 in HEADS]
                 + [rng.standard_normal(DIM).astype(np.float32)])
    sq = {"indices": list(range(0, V, 2)), "values": [1.0] * (V // 2)}
    return X, Xdom, (idx, val), payload, Q, sq


def manager(corpus, domain=False, **kw):
    """The collection appended in three pieces."""
    X, Xdom, (idx, val), payload, Q, sq = corpus
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, domain_dim=DD, enable_domain=domain, **kw)
    for lo in range(0, N, 1000):
        hi = lo + 1000
        csr = (np.arange(hi - lo + 1, dtype=np.int64) * 4, idx[lo:hi].reshape(-1), val[lo:hi].reshape(-1))
        mgr.add_rows(X[lo:hi], csr, **{k: v[lo:hi] for k, v in payload.items()})
        if domain:
            mgr._domain.add(Xdom[lo:hi])
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(Q, sq)
    return mgr


@pytest.fixture(scope="module")
def one_shard(gpu, corpus):
    mgr = manager(corpus, domain=True)
    yield mgr
    asyncio.run(mgr.close())


def entity(hit):
    return int(hit["id"][1:])


def sig(hits):
    return [(h["id"], float(h["score"]).hex(), float(h["mmr_value"]).hex()) for h in hits]


def want_search(mgr, Xs, q, coll, ranker, top_k=K, metric="COSINE", **kw):
    """The restatement over the plain search at depth W and the stored rows (looked up by entity id: rows are renumbered
    by a compaction) -> (signature, the plain prefix's ids)."""
    plain = asyncio.run(mgr.search(q, coll, ranker.window(top_k), **kw))
    pos, val = vector_mmr([h["score"] for h in plain], Xs[[entity(h) for h in plain]], ranker.lambda_mult, top_k,
                          ranker.norm_code(metric))
    return [(plain[p]["id"], float(plain[p]["score"]).hex(), float(v).hex()) for p, v in zip(pos, val)], \
        [h["id"] for h in plain[:top_k]]


RANKERS = [MMRRanker(), MMRRanker(0.3, candidates=40), MMRRanker(0.7, 64, "activation"), MMRRanker(0.5, 100, "minmax"),
           MMRRanker(1.0, 30)]


def test_search_with_a_ranker_equals_the_restatement(one_shard, corpus):
    X, Xdom, _, _, Q, sq = corpus
    mgr = one_shard
    assert mgr._front is None or mgr._front.stats["mmr_launches"] == 0                   # nothing asked for it yet
    launches = moved = 0
    for coll, Xs, queries in (("semantic_index", X.astype(np.float16), Q),
                              ("domain_index", Xdom.astype(np.float16), Xdom[list(HEADS)] + np.float32(0.05))):
        for i, ranker in enumerate(RANKERS):
            q = queries[i % len(queries)]
            want, prefix = want_search(mgr, Xs, q, coll, ranker)
            got = asyncio.run(mgr.search(q, coll, K, ranker=ranker))
            assert sig(got) == want and len(got) == K, (coll, ranker)
            assert ([w[0] for w in want] == prefix) if ranker.lambda_mult == 1.0 else True
            moved += [w[0] for w in want] != prefix
            launches += 1
    assert moved >= 6                                                                    # it diversifies, it is no identity
    # a filter, and range params: applied by the plain search as ever
    Xs, ranker = X.astype(np.float16), RANKERS[1]
    for kw in (dict(filters="chunk_index != 2"),
               dict(search_params={"metric_type": "COSINE", "params": {"ef": 64, "radius": 0.2}}),
               dict(filters="chunk_index >= 1", search_params={"metric_type": "COSINE", "params": {"ef": 64, "range_filter": 0.95}})):
        want, _ = want_search(mgr, Xs, Q[0], "semantic_index", ranker, **kw)
        got = asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=ranker, **kw))
        assert sig(got) == want and 0 < len(got) <= K
        if kw.get("filters") == "chunk_index != 2":
            assert all(h["metadata"]["chunk_index"] != 2 for h in got)
        launches += 1
    assert mgr._front.stats["mmr_launches"] == launches and mgr.stats["mmr_host_selects"] == 0      # the device answered
    for bad in (dict(group_by_field="doc_id"), dict(offset=2)):
        with pytest.raises(ValueError):
            asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=ranker, **bad))
    with pytest.raises(ValueError, match="dense embeddings"):
        asyncio.run(mgr.search(sq, "sparse_index", K, ranker=ranker))
    with pytest.raises(ValueError):
        asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=MMRRanker(candidates=257)))
    with pytest.raises(ValueError):
        asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=object()))
    assert mgr._front.stats["mmr_launches"] == launches


def test_concurrent_searches_with_different_lambdas_share_launches(one_shard, corpus):
    X, _, _, _, Q, _ = corpus
    mgr, Xs = one_shard, X.astype(np.float16)
    specs = [MMRRanker(i / 16.0, candidates=40) for i in range(16)]
    serial = [sig(asyncio.run(mgr.search(Q[i % NQ], "semantic_index", K, ranker=r))) for i, r in enumerate(specs)]
    for i in (0, 5, 15):
        assert serial[i] == want_search(mgr, Xs, Q[i % NQ], "semantic_index", specs[i])[0]
    assert len({tuple(s) for s in serial}) >= 10

    async def burst():
        return await asyncio.gather(*(mgr.search(Q[i % NQ], "semantic_index", K, ranker=r) for i, r in enumerate(specs)))

    before = mgr._front.stats["mmr_launches"]
    out = asyncio.run(burst())
    launches = mgr._front.stats["mmr_launches"] - before
    assert [sig(o) for o in out] == serial
    assert 1 <= launches < 16


def test_search_by_ids_passes_the_ranker_through(one_shard, corpus):
    X, _, _, _, Q, _ = corpus
    mgr, ranker = one_shard, MMRRanker(0.4, candidates=50)
    got = asyncio.run(mgr.search_by_ids(["c1000", "c7"], "semantic_index", K, ranker=ranker))
    for e, hits in zip((1000, 7), got):
        stored = X.astype(np.float16)[e].astype(np.float32)
        assert sig(hits) == sig(asyncio.run(mgr.search(stored, "semantic_index", K, ranker=ranker))) and len(hits) == K
    with pytest.raises(ValueError):
        asyncio.run(mgr.search_by_ids(["c7"], "semantic_index", K, ranker=ranker, group_by_field="doc_id"))


def test_delete_and_compact(gpu, corpus):
    X, _, _, _, Q, _ = corpus
    Xs, ranker = X.astype(np.float16), MMRRanker(0.5, candidates=60)
    mgr = manager(corpus)
    try:
        first, _ = want_search(mgr, Xs, Q[1], "semantic_index", ranker)
        gone = [first[0][0], first[2][0]]
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_id in [" + ", ".join(f'"{g}"' for g in gone) + "]"))
        for compacted in (False, True):
            if compacted:
                mgr.compact()
            want, _ = want_search(mgr, Xs, Q[1], "semantic_index", ranker)
            before = mgr._front.stats["mmr_launches"]        # (read here: a compaction may start a new front)
            got = asyncio.run(mgr.search(Q[1], "semantic_index", K, ranker=ranker))
            assert sig(got) == want and not {g for g in gone} & {h["id"] for h in got} and len(got) == K
            assert mgr._front.stats["mmr_launches"] == before + 1 and mgr.stats["mmr_host_selects"] == 0      # on the device
    finally:
        asyncio.run(mgr.close())


def test_two_shards_equal_one(one_shard, corpus):
    X, _, _, _, Q, _ = corpus
    two = manager(corpus, devices=[0, 0])
    try:
        calls = 0
        for i, ranker in enumerate(RANKERS):
            for kw in ({}, dict(filters="chunk_index != 2")):
                a = asyncio.run(two.search(Q[i % NQ], "semantic_index", K, ranker=ranker, **kw))
                b = asyncio.run(one_shard.search(Q[i % NQ], "semantic_index", K, ranker=ranker, **kw))
                assert sig(a) == sig(b) and len(a) == K
                calls += 1
        assert two.stats["mmr_host_selects"] == calls
        assert two._front is None or two._front.stats["mmr_launches"] == 0
    finally:
        asyncio.run(two.close())


def test_retrieve_with_embedding_similarity(gpu, long_timeout, corpus):
    X, _, _, _, Q, _ = corpus
    Xs, lam = X.astype(np.float16), 0.5
    for on_device in (False, True):
        mgr = manager(corpus, mmr_on_device=on_device)
        try:
            plain = HybridRetriever(mgr, RetrievalConfig(top_k=K, enable_mmr=False))
            emb = HybridRetriever(mgr, RetrievalConfig(top_k=K, enable_mmr=True, mmr_lambda=lam, mmr_similarity="embedding"))
            moved = 0
            for qi in range(NQ):
                async def fused_list():
                    sem = await plain._search_semantic(Q[qi], None)
                    sp = await plain._search_sparse(mgr.embedding_generator.SQ, None)
                    return await plain._fuse_results_async(sem, sp, [])
                fused = asyncio.run(fused_list())                                        # the general path's fused list, whole
                assert len(fused) > 2 * K
                pos, _ = vector_mmr([h["score"] for h in fused], Xs[[entity(h) for h in fused]], lam, K)
                hybrid = mgr._front.stats["hybrid_launches"]
                initialize_caches()                      # the embedding cache goes by the text: other modules use the same
                got = asyncio.run(emb.retrieve(f"plain statement q{qi}", profile_hint="default"))
                assert [(h["id"], h["score"]) for h in got] == [(fused[p]["id"], fused[p]["score"]) for p in pos] and len(got) == K
                assert mgr._front.stats["hybrid_launches"] == hybrid                     # not the one-round path
                moved += pos != list(range(K))
            assert moved >= 2
            assert mgr._front.stats["mmr_launches"] == NQ and mgr.stats["mmr_host_selects"] == 0
            assert mgr._cols._token_sets is None and mgr._dev_tokens is None             # no token-set build
        finally:
            asyncio.run(mgr.close())


def test_a_default_manager_launches_no_mmr(gpu, long_timeout, corpus):
    X, _, _, _, Q, _ = corpus
    mgr = manager(corpus)
    try:
        hits = asyncio.run(mgr.search(Q[0], "semantic_index", K))
        assert len(hits) == K and all("mmr_value" not in h for h in hits)
        initialize_caches()
        got = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=K)).retrieve("plain statement q1", profile_hint="default"))
        assert len(got) == K
        assert mgr._front.stats["mmr_launches"] == 0 and mgr.stats["mmr_host_selects"] == 0
    finally:
        asyncio.run(mgr.close())
