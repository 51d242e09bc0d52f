"""The decay ranker end to end on one GPU shard: search(ranker=...) against the host restatement over the plain search at
depth W, concurrent requests with different curves in shared launches, retrieve(decay=...) through the one-round path against
the general path, the epoch mirror after an append and after a compaction, and a two-shard manager against the one-shard one."""
import asyncio
from datetime import datetime, timedelta

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag import decay as D
from advanced_rag.constants import RetrievalConstants
from advanced_rag.decay import DecayRanker
from advanced_rag.embedding_cache import initialize_caches

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, N_MORE, DIM, V, TOP_K, NQ = 2000, 150, 32, 256, 10, 4
T0 = datetime(2024, 5, 1)


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
        return np.zeros(8, np.float32)


def _rows(rng, lo, hi):
    """Vectors, sparse rows and payload of global rows [lo, hi): timestamps spread over 60 days, a few empty or unparsable."""
    n, nnz = hi - lo, 5
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(n)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((n, nnz))) + 0.1).astype(np.float32)
    csr = (np.arange(n + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    stamps = [(T0 - timedelta(minutes=int(m))).isoformat() for m in rng.integers(0, 60 * 1440, n)]
    for r in range(0, n, 37):
        stamps[r] = ("", "n/a", "2024-02-30")[r % 3]
    payload = dict(ids=[f"c{r}" for r in range(lo, hi)], contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(lo, hi)],
                   doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 7 for r in range(lo, hi)],
                   token_count=[20 + r % 90 for r in range(lo, hi)], entropy=[(r % 11) / 11.0 for r in range(lo, hi)], timestamp=stamps)
    return X, csr, payload


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(61)
    base, more = _rows(rng, 0, N), _rows(rng, N, N + N_MORE)
    Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 40, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(40)) + 0.5).astype(np.float32))
          for _ in range(NQ)]
    field_of = {}
    for _, _, p in (base, more):
        for i, name in enumerate(p["ids"]):
            field_of[name] = {"timestamp": D.epoch_seconds(p["timestamp"][i]), "chunk_index": float(p["chunk_index"][i]),
                              "token_count": float(p["token_count"][i]), "entropy": float(np.float32(p["entropy"][i]))}
    assert sum(np.isnan(f["timestamp"]) for f in field_of.values()) >= 50
    return base, more, Q, SQ, field_of


def manager(corpus, **kw):
    (X, csr, payload), _, Q, SQ, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, enable_domain=False, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(Q, SQ)
    return mgr


@pytest.fixture(scope="module")
def one_shard(gpu, corpus):
    mgr = manager(corpus)
    yield mgr
    asyncio.run(mgr.close())


def rankers(candidates=None):
    day = 86400.0
    at = lambda d: (T0 - timedelta(days=d)).isoformat()
    return [DecayRanker("timestamp", "gauss", at(7), 5 * day, 3600.0, 0.5, candidates=candidates),
            DecayRanker("timestamp", "exp", at(30), 10 * day, normalization="minmax", candidates=candidates),
            DecayRanker("timestamp", "linear", at(0), 20 * day, day, 0.25, candidates=candidates),
            DecayRanker("chunk_index", "linear", 3, 2, candidates=candidates),
            DecayRanker("token_count", "gauss", 60, 15.0, 2.0, 0.3, normalization="none", candidates=candidates),
            DecayRanker("entropy", "exp", 0.5, 0.25, candidates=candidates)]


def sig(hits):
    return [(h["id"], float(h["score"]).hex(), float(h.get("raw_score", h.get("fused_score", 0.0))).hex()) for h in hits]


def want_search(mgr, field_of, query, coll, ranker, top_k, metric):
    W = ranker.window(top_k)
    plain = asyncio.run(mgr.search(query, coll, W))
    pos, _, fin = D.decay_rerank([h["_row"] for h in plain], [h["score"] for h in plain],
                                 [field_of[h["id"]][ranker.field] for h in plain], ranker.operands(), ranker.norm_code(metric), W)
    return [(plain[p]["id"], float(f).hex(), float(plain[p]["score"]).hex()) for p, f in zip(pos[:top_k], fin[:top_k])], plain


@pytest.mark.parametrize("candidates", [None, 4 * TOP_K])
def test_search_with_a_ranker_equals_the_restatement(one_shard, corpus, candidates):
    _, _, Q, SQ, field_of = corpus
    mgr = one_shard
    before = mgr._front.stats["decay_launches"] if mgr._front is not None else 0
    moved = 0
    for i, ranker in enumerate(rankers(candidates)):
        want, plain = want_search(mgr, field_of, Q[i % NQ], "semantic_index", ranker, TOP_K, "COSINE")
        got = asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker))
        assert sig(got) == want, ranker
        moved += [w[0] for w in want] != [h["id"] for h in plain[:TOP_K]]
    assert moved >= 4                                   # the decay reorders, it is no identity
    ranker = rankers(candidates)[0]
    sq = {"indices": SQ[0][0].tolist(), "values": SQ[0][1].astype(float).tolist()}
    want, _ = want_search(mgr, field_of, sq, "sparse_index", ranker, TOP_K, "IP")
    assert sig(asyncio.run(mgr.search(sq, "sparse_index", TOP_K, ranker=ranker))) == want
    want, _ = want_search(mgr, field_of, Q[1], "semantic_index", ranker, TOP_K, "COSINE")       # (no filter in the helper)
    filtered = asyncio.run(mgr.search(Q[1], "semantic_index", TOP_K, filters="chunk_index != 2", ranker=ranker))
    assert all(h["metadata"]["chunk_index"] != 2 for h in filtered) and len(filtered) == TOP_K
    assert mgr._front.stats["decay_launches"] - before == len(rankers()) + 2      # the device answered, one launch each here
    assert mgr._decay_columns_on_device().nbytes >= 8 * N                         # the epoch mirror: 8 bytes per row


def test_concurrent_searches_with_different_curves_share_launches(one_shard, corpus):
    _, _, Q, _, field_of = corpus
    mgr = one_shard
    day = 86400.0
    specs = [DecayRanker("timestamp", ("gauss", "exp", "linear")[i % 3], (T0 - timedelta(days=3 * i)).isoformat(), (2 + i) * day,
                         (i % 2) * 3600.0, 0.2 + 0.04 * i, candidates=30) for i in range(16)]
    serial = [sig(asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r))) for i, r in enumerate(specs)]
    for i, r in enumerate(specs[:3]):
        assert serial[i] == want_search(mgr, field_of, Q[i % NQ], "semantic_index", r, TOP_K, "COSINE")[0]
    assert len({tuple(s) for s in serial}) >= 12

    async def burst():
        return await asyncio.gather(*(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r) for i, r in enumerate(specs)))

    before = mgr._front.stats["decay_launches"]
    out = asyncio.run(burst())
    launches = mgr._front.stats["decay_launches"] - before
    assert [sig(o) for o in out] == serial
    assert 1 <= launches < 16


@pytest.mark.parametrize("mmr", [False, True])
def test_retrieve_one_round_equals_the_general_path(gpu, long_timeout, corpus, mmr):
    ranker = DecayRanker("timestamp", "exp", (T0 - timedelta(days=12)).isoformat(), 6 * 86400.0)
    answers = {}
    for name, kw in {"one_round": {"mmr_on_device": mmr}, "general": {"coalesce": False}}.items():
        mgr = manager(corpus, **kw)
        try:
            initialize_caches()
            cfg = RetrievalConfig(top_k=TOP_K, decay=ranker, enable_mmr=mmr, mmr_lambda=0.6)
            retr = HybridRetriever(mgr, cfg)
            answers[name] = [asyncio.run(retr.retrieve(f"plain statement q{q}", profile_hint="default")) for q in range(NQ)]
            plain = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, enable_mmr=mmr, mmr_lambda=0.6)).retrieve(
                "plain statement q0", profile_hint="default"))
            assert [h["id"] for h in plain] != [h["id"] for h in answers[name][0]]        # the decay reorders the fused list
            if name == "one_round":
                st = mgr._front.stats
                assert st["hybrid_launches"] == NQ + 1 and st["decay_launches"] == NQ and st["mmr_launches"] == ((NQ + 1) if mmr else 0)
                assert st["fuse_launches"] == 0
            else:
                assert mgr._front is None
        finally:
            asyncio.run(mgr.close())
    for q in range(NQ):
        got, want = answers["one_round"][q], answers["general"][q]
        assert len(want) == TOP_K and all(h["score"] <= h["fused_score"] for h in want)
        assert sig(got) == sig(want), q
        assert [h["retrieval_methods"] for h in got] == [h["retrieval_methods"] for h in want]      # the method bits follow
        assert [h["original_score"] for h in got] == [h["original_score"] for h in want]


def test_answers_after_an_append_and_after_a_compaction(gpu, corpus):
    _, (X2, csr2, payload2), Q, _, field_of = corpus
    mgr = manager(corpus)
    try:
        stamp, chunk = rankers(30)[0], rankers(30)[3]
        for r in (stamp, chunk):
            assert sig(asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=r))) == \
                want_search(mgr, field_of, Q[0], "semantic_index", r, TOP_K, "COSINE")[0]
        mirror = mgr._decay_columns_on_device()
        uploaded = mirror.stats["uploaded_bytes"]
        assert uploaded == 8 * N
        mgr.add_rows(X2, csr2, **payload2)
        mgr.finalize()
        q_new = X2[3] + 0.1 * Q[1]                                     # near an appended row: the new rows reach the window
        for r in (stamp, chunk):
            want, plain = want_search(mgr, field_of, q_new, "semantic_index", r, TOP_K, "COSINE")
            assert any(h["_row"] >= N for h in plain)
            assert sig(asyncio.run(mgr.search(q_new, "semantic_index", TOP_K, ranker=r))) == want
        assert mgr._decay_columns_on_device() is mirror and mirror.stats["uploaded_bytes"] == uploaded + 8 * N_MORE      # extended
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 1"))
        mgr.compact()
        assert mgr.num_rows < N + N_MORE
        for r in (stamp, chunk):
            for q in (q_new, Q[2]):
                want, plain = want_search(mgr, field_of, q, "semantic_index", r, TOP_K, "COSINE")
                assert all(h["metadata"]["chunk_index"] != 1 for h in plain)
                assert sig(asyncio.run(mgr.search(q, "semantic_index", TOP_K, ranker=r))) == want
        rebuilt = mgr._decay_columns_on_device()
        assert rebuilt is not mirror and rebuilt.stats["uploaded_bytes"] == 8 * mgr.num_rows                              # rebuilt
    finally:
        asyncio.run(mgr.close())


def test_two_shards_equal_one_shard(one_shard, long_timeout, corpus):
    _, _, Q, SQ, _ = corpus
    two = manager(corpus, devices=[0, 0])
    try:
        assert two._front is None or two._coalescer(two.collections["semantic_index"]) is None
        for i, ranker in enumerate(rankers(25)):
            assert sig(asyncio.run(two.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker))) == \
                sig(asyncio.run(one_shard.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker)))
        cfg = dict(top_k=TOP_K, decay=rankers()[1])
        initialize_caches()
        a = asyncio.run(HybridRetriever(two, RetrievalConfig(**cfg)).retrieve("plain statement q1", profile_hint="default"))
        initialize_caches()
        b = asyncio.run(HybridRetriever(one_shard, RetrievalConfig(**cfg)).retrieve("plain statement q1", profile_hint="default"))
        assert sig(a) == sig(b) and len(a) == TOP_K
    finally:
        asyncio.run(two.close())
