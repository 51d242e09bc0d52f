"""Late interaction end to end on one GPU shard: search(ranker=MaxSimRanker) against the numpy restatement over the plain
search at depth W, concurrent requests with different token counts in shared launches, the HBM mirror after an append
and after a compaction, a two-shard manager (host form) against the one-shard one, retrieve(late_interaction=True), and a
manager without token_dim."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag import maxsim as M
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.maxsim import MaxSimRanker
from advanced_rag.retrieval import rrf_rank_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, N_MORE, DIM, V, TD, TOP_K, NQ = 2000, 150, 64, 256, 32, 10, 4


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


class KeyedGen:
    """Embeddings keyed by the trailing query number of the text ("... q<i>"); token vectors from that number too."""

    def __init__(self, Q, SQ):
        self.Q, self.SQ = Q, SQ

    def encode_semantic(self, text):
        return self.Q[int(text.rsplit("q", 1)[1])]

    def encode_sparse(self, text):
        qi, qv = self.SQ[int(text.rsplit("q", 1)[1])]
        return {"indices": qi.tolist(), "values": qv.astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)

    def encode_token_vectors(self, texts):
        toks = [query_tokens(100 + int(t.rsplit("q", 1)[1]), 5 + 7 * (int(t.rsplit("q", 1)[1]) % 4)) for t in texts]
        return np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int64), np.concatenate(toks)


def query_tokens(seed, tq):
    return np.random.default_rng(seed).standard_normal((tq, TD)).astype(np.float32)


def _rows(rng, lo, hi):
    """Vectors, sparse rows, payload and token vectors (0..40 per row, every ninth row none) of global rows [lo, hi)."""
    n, nnz = hi - lo, 5
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(n)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((n, nnz))) + 0.1).astype(np.float32)
    csr = (np.arange(n + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    T = rng.integers(0, 41, n)
    T[::9] = 0
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    tok = rng.standard_normal((int(indptr[-1]), TD)).astype(np.float32)
    payload = dict(ids=[f"c{r}" for r in range(lo, hi)], contents=[f"topic{r % 5} word{r % 7}" for r in range(lo, hi)],
                   doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 7 for r in range(lo, hi)])
    return X, csr, payload, (indptr, tok)


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(71)
    base, more = _rows(rng, 0, N), _rows(rng, N, N + N_MORE)
    Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 40, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(40)) + 0.5).astype(np.float32))
          for _ in range(NQ)]
    tokens_of = {}
    for _, _, p, (indptr, tok) in (base, more):
        for i, name in enumerate(p["ids"]):
            tokens_of[name] = tok[indptr[i]:indptr[i + 1]].astype(np.float16)
    return base, more, Q, SQ, tokens_of


def manager(corpus, token_dim=TD, **kw):
    (X, csr, payload, tv), _, Q, SQ, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, enable_domain=False, token_dim=token_dim, **kw)
    mgr.add_rows(X, csr, **payload, **({"token_vectors": tv} if token_dim is not None else {}))
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(Q, SQ)
    return mgr


@pytest.fixture(scope="module")
def one_shard(gpu, corpus):
    mgr = manager(corpus)
    yield mgr
    asyncio.run(mgr.close())


def sig(hits):
    return [(h["id"], h["score"], h.get("raw_score", h.get("fused_score"))) for h in hits]


def want_search(mgr, tokens_of, query, coll, ranker, top_k, **kw):
    W = ranker.window(top_k)
    plain = asyncio.run(mgr.search(query, coll, W, **kw))
    pos, _, fin = M.maxsim_rerank([h["_row"] for h in plain], ranker.query_tokens, [tokens_of[h["id"]] for h in plain], W)
    return [(plain[p]["id"], f, plain[p]["score"]) for p, f in zip(pos[:top_k], fin[:top_k])], plain


def test_search_with_the_ranker_equals_the_restatement(one_shard, corpus):
    _, _, Q, SQ, tokens_of = corpus
    mgr = one_shard
    before = mgr._front.stats["maxsim_launches"] if mgr._front is not None else 0
    moved = 0
    specs = [(1, None), (9, 40), (16, 4 * TOP_K), (33, 80), (64, 256)]
    for i, (tq, cand) in enumerate(specs):
        ranker = MaxSimRanker(query_tokens(i, tq), candidates=cand)
        want, plain = want_search(mgr, tokens_of, Q[i % NQ], "semantic_index", ranker, TOP_K)
        got = asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker))
        assert sig(got) == want, (tq, cand)
        assert all("raw_score" in h and isinstance(h["score"], float) for h in got)
        moved += [w[0] for w in want] != [h["id"] for h in plain[:TOP_K]]
    assert moved >= 4                                   # the rerank reorders, it is no identity
    ranker = MaxSimRanker(query_tokens(7, 12), candidates=50)
    sq = {"indices": SQ[0][0].tolist(), "values": SQ[0][1].astype(float).tolist()}
    want, _ = want_search(mgr, tokens_of, sq, "sparse_index", ranker, TOP_K)
    assert sig(asyncio.run(mgr.search(sq, "sparse_index", TOP_K, ranker=ranker))) == want
    want, _ = want_search(mgr, tokens_of, Q[1], "semantic_index", ranker, TOP_K, filters="chunk_index != 2")
    assert sig(asyncio.run(mgr.search(Q[1], "semantic_index", TOP_K, filters="chunk_index != 2", ranker=ranker))) == want
    assert mgr._front.stats["maxsim_launches"] - before == len(specs) + 2       # the device answered, one launch each here
    assert mgr.stats["maxsim_host_reranks"] == 0
    mirror = mgr._token_vectors_on_device()
    n_tok = int(corpus[0][3][0][-1])
    assert mirror.stats["uploaded_bytes"] == 8 * (N + 1) + 2 * TD * n_tok and mirror.nbytes >= 2 * TD * n_tok


def test_concurrent_searches_with_different_token_counts_share_launches(one_shard, corpus):
    _, _, Q, _, tokens_of = corpus
    mgr = one_shard
    specs = [MaxSimRanker(query_tokens(50 + i, 1 + (i * 21) // 5), candidates=30) for i in range(16)]      # Tq = 1 .. 64
    assert specs[0].query_tokens.shape[0] == 1 and specs[15].query_tokens.shape[0] == 64
    serial = [sig(asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r))) for i, r in enumerate(specs)]
    for i in (0, 7, 15):
        assert serial[i] == want_search(mgr, tokens_of, Q[i % NQ], "semantic_index", specs[i], TOP_K)[0]

    async def burst():
        return await asyncio.gather(*(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r) for i, r in enumerate(specs)))

    before = mgr._front.stats["maxsim_launches"]
    out = asyncio.run(burst())
    launches = mgr._front.stats["maxsim_launches"] - before
    assert [sig(o) for o in out] == serial
    assert 1 <= launches < 16


def test_answers_after_an_append_and_after_a_compaction(gpu, corpus):
    _, (X2, csr2, payload2, tv2), Q, _, tokens_of = corpus
    mgr = manager(corpus)
    try:
        r = MaxSimRanker(query_tokens(3, 20), candidates=30)
        assert sig(asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=r))) == \
            want_search(mgr, tokens_of, Q[0], "semantic_index", r, TOP_K)[0]
        mirror = mgr._token_vectors_on_device()
        uploaded = mirror.stats["uploaded_bytes"]
        mgr.add_rows(X2, csr2, **payload2, token_vectors=tv2)
        mgr.finalize()
        q_new = X2[3] + 0.1 * Q[1]                                     # near an appended row: the new rows reach the window
        want, plain = want_search(mgr, tokens_of, q_new, "semantic_index", r, TOP_K)
        assert any(h["_row"] >= N for h in plain)
        assert sig(asyncio.run(mgr.search(q_new, "semantic_index", TOP_K, ranker=r))) == want
        assert mgr._token_vectors_on_device() is mirror                                       # extended in place:
        assert mirror.stats["uploaded_bytes"] == uploaded + 8 * (N_MORE + 1) + 2 * TD * int(tv2[0][-1])      # every row once
        before = {q: asyncio.run(mgr.search(qv, "semantic_index", TOP_K, filters="chunk_index != 1", ranker=r))
                  for q, qv in (("new", q_new), ("old", Q[2]))}
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 1"))
        mgr.compact()
        assert mgr.num_rows < N + N_MORE
        for q, qv in (("new", q_new), ("old", Q[2])):
            want, plain = want_search(mgr, tokens_of, qv, "semantic_index", r, TOP_K)
            assert all(h["metadata"]["chunk_index"] != 1 for h in plain)
            got = asyncio.run(mgr.search(qv, "semantic_index", TOP_K, ranker=r))
            assert sig(got) == want
            assert [(h["id"], h["score"]) for h in got] == [(h["id"], h["score"]) for h in before[q]]      # same hits by id
        assert mgr._token_vectors_on_device() is not mirror                                   # rebuilt
    finally:
        asyncio.run(mgr.close())


def test_two_shards_equal_one_shard(one_shard, corpus):
    _, _, Q, _, _ = corpus
    two = manager(corpus, devices=[0, 0])
    try:
        for i, tq in enumerate((1, 17, 40)):
            ranker = MaxSimRanker(query_tokens(20 + i, tq), candidates=25)
            assert sig(asyncio.run(two.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker))) == \
                sig(asyncio.run(one_shard.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker)))
        assert two.stats["maxsim_host_reranks"] == 3           # the host form answered
    finally:
        asyncio.run(two.close())


def test_retrieve_with_late_interaction(one_shard, long_timeout, corpus):
    _, _, Q, SQ, tokens_of = corpus
    mgr = one_shard
    gen = mgr.embedding_generator
    for q in range(NQ):
        initialize_caches()
        text = f"plain statement q{q}"
        sem = asyncio.run(mgr.search(gen.encode_semantic(text), "semantic_index", 2 * TOP_K))
        spa = asyncio.run(mgr.search(gen.encode_sparse(text), "sparse_index", 2 * TOP_K, None,
                                     {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
        ranked = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa]], (0.7, 0.3))
        qt = gen.encode_token_vectors([text])[1].astype(np.float16)
        pos, _, fin = M.maxsim_rerank(list(range(len(ranked))), qt, [tokens_of[i] for i, _, _ in ranked], len(ranked))
        want = [(ranked[p][0], f, ranked[p][1]) for p, f in zip(pos, fin)][:TOP_K]
        before = mgr._front.stats["maxsim_launches"]
        got = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, late_interaction=True)).retrieve(text, profile_hint="default"))
        assert sig(got) == want and len(got) == TOP_K
        assert mgr._front.stats["maxsim_launches"] == before + 1
        assert [w[0] for w in want] != [i for i, _, _ in ranked][:TOP_K]


def test_a_manager_without_token_dim(gpu, corpus):
    _, _, Q, _, _ = corpus
    mgr = manager(corpus, token_dim=None)
    try:
        with pytest.raises(ValueError, match="token_dim"):
            asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=MaxSimRanker(query_tokens(1, 4))))
        hits = asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K))
        assert len(hits) == TOP_K and mgr._dev_tokvec is None and mgr._front.stats["maxsim_launches"] == 0
    finally:
        asyncio.run(mgr.close())
