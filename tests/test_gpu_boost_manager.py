"""The boost ranker end to end on one GPU shard: search(ranker=...) on the three collections against the host restatement over
the plain search at depth W, concurrent requests with different functions in shared launches, retrieve(boost=...) through the
one-round path against the general path, rows appended, deleted and compacted, and a two-shard manager against the one-shard
one."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag import boost as BO
from advanced_rag import decay as D
from advanced_rag.boost import BoostRanker, FunctionScore
from advanced_rag.constants import RetrievalConstants
from advanced_rag.decay import DecayRanker
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.retrieval import rrf_rank_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, N_MORE, DIM, DD, V, TOP_K, NQ = 2000, 150, 64, 16, 256, 10, 4

# what row r (named c{r}) holds: doc r // 10, chunk_index r % 7, token_count 20 + r % 90, content "topic{r % 5} word{r % 7} ..."
MATCH = {None: lambda r: True, "chunk_index >= 3": lambda r: r % 7 >= 3, "chunk_index == 1": lambda r: r % 7 == 1,
         'doc_id in ["doc3", "doc17", "doc42", "doc120", "doc205"]': lambda r: r // 10 in (3, 17, 42, 120, 205),
         'TEXT_MATCH(content, "topic2")': lambda r: r % 5 == 2, 'TEXT_MATCH(content, "topic1 word3", minimum_should_match=2)':
         lambda r: r % 5 == 1 and r % 7 == 3, "token_count < 40 or not chunk_index != 0": lambda r: r % 90 < 20 or r % 7 == 0,
         "token_count >= 100": lambda r: r % 90 >= 80}
DOCS, TOPIC2 = 'doc_id in ["doc3", "doc17", "doc42", "doc120", "doc205"]', 'TEXT_MATCH(content, "topic2")'


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
    n, nnz = hi - lo, 5
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    XD = rng.standard_normal((n, DD)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(n)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((n, nnz))) + 0.1).astype(np.float32)
    csr = (np.arange(n + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    payload = dict(ids=[f"c{r}" for r in range(lo, hi)], contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(lo, hi)],
                   doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 7 for r in range(lo, hi)],
                   token_count=[20 + r % 90 for r in range(lo, hi)], entropy=[(r % 11) / 11.0 for r in range(lo, hi)])
    return X, XD, csr, payload


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(67)
    base, more = _rows(rng, 0, N), _rows(rng, N, N + N_MORE)
    Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    QD = rng.standard_normal((NQ, DD)).astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 40, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(40)) + 0.5).astype(np.float32))
          for _ in range(NQ)]
    return base, more, Q, SQ, QD


def manager(corpus, rows=None, domain=False, **kw):
    X, XD, csr, payload = rows if rows is not None else corpus[0]
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, domain_dim=DD, enable_domain=domain, **kw)
    mgr.add_rows(X, csr, **payload)
    if domain:
        mgr._domain.add(XD)                  # row-aligned with the main collections, as index_chunks keeps it
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(corpus[2], corpus[3])
    return mgr


@pytest.fixture(scope="module")
def one_shard(gpu, corpus):
    mgr = manager(corpus, domain=True)
    yield mgr
    asyncio.run(mgr.close())


def specs(candidates=None):
    return [BoostRanker(DOCS, 4.0),
            FunctionScore(BoostRanker("chunk_index >= 3", 0.5), BoostRanker(TOPIC2, 3.0), candidates=candidates),
            FunctionScore(BoostRanker("chunk_index >= 3", 0.25), BoostRanker("token_count < 40 or not chunk_index != 0", -1.5),
                          BoostRanker("token_count >= 100", 50.0), BoostRanker('TEXT_MATCH(content, "topic1 word3", minimum_should_match=2)', 9.0),
                          function_mode="sum", boost_mode="sum", normalization="activation", candidates=candidates),
            FunctionScore(BoostRanker(None, 1.0, {"seed": 126, "field": "doc_id"}), boost_mode="sum", normalization="minmax",
                          candidates=candidates),
            FunctionScore(BoostRanker("chunk_index >= 3", 2.0, {"seed": 5, "field": None}),
                          BoostRanker(None, 0.5, {"seed": 2 ** 64 - 1, "field": "chunk_index"}),
                          BoostRanker(TOPIC2, 1.5, {"seed": 77, "field": "token_count"}), function_mode="sum", candidates=candidates)]


def sig(hits):
    return [(h["id"], float(h["score"]).hex(), float(h.get("raw_score", h.get("fused_score", 0.0))).hex(), h.get("boosted_by"))
            for h in hits]


def restate(mgr, names, rows, scores, spec, metric, fused=False):
    """boost_rerank over what the rows are known to hold (by their names c{r}: compaction renumbers the rows)."""
    orig = [int(name[1:]) for name in names]
    matches = [[MATCH[f.filter](r) for r in orig] for f in spec.functions]
    values = []
    for f in spec.functions:
        if f.seed is None:
            values.append(f.weight)
        else:
            keys = rows if f.field is None else [int(mgr._host_group_keys(f.field)[r]) for r in rows]
            values.append((f.weight, f.seed, keys))
    fm, bm, norm, asc = spec.launch_key(metric, fused)
    return BO.boost_rerank(rows, scores, matches, values, fm, bm, norm, bool(asc))


def want_search(mgr, query, coll, ranker, top_k, metric, **kw):
    spec = FunctionScore.of(ranker)
    plain = asyncio.run(mgr.search(query, coll, spec.window(top_k), **kw))
    pos, _, fin, hit = restate(mgr, [h["id"] for h in plain], [h["_row"] for h in plain], [h["score"] for h in plain], spec, metric)
    return [(plain[p]["id"], float(f).hex(), float(plain[p]["score"]).hex(), BO.matched_functions(m))
            for p, f, m in zip(pos[:top_k], fin[:top_k], hit[:top_k])], plain


@pytest.mark.parametrize("candidates", [None, 4 * TOP_K])
def test_search_with_a_boost_equals_the_restatement(one_shard, corpus, candidates):
    _, _, Q, SQ, QD = corpus
    mgr = one_shard
    before, host_before = mgr._front.stats["boost_launches"] if mgr._front is not None else 0, mgr.stats["boost_host_reranks"]
    moved = calls = 0
    sq = {"indices": SQ[0][0].tolist(), "values": SQ[0][1].astype(float).tolist()}
    for i, ranker in enumerate(specs(candidates)):
        for coll, query, metric in (("semantic_index", Q[i % NQ], "COSINE"), ("sparse_index", sq, "IP"), ("domain_index", QD[i % NQ], "COSINE")):
            want, plain = want_search(mgr, query, coll, ranker, TOP_K, metric)
            got = asyncio.run(mgr.search(query, coll, TOP_K, ranker=ranker))
            assert sig(got) == want, (coll, ranker)
            moved += [w[0] for w in want] != [h["id"] for h in plain[:TOP_K]]
            calls += 1
    assert moved >= 6                                   # the boost reorders, it is no identity
    # a search filter together with a boost filter
    ranker = specs(candidates)[1]
    want, plain = want_search(mgr, Q[1], "semantic_index", ranker, TOP_K, "COSINE", filters="chunk_index != 2")
    got = asyncio.run(mgr.search(Q[1], "semantic_index", TOP_K, filters="chunk_index != 2", ranker=ranker))
    assert sig(got) == want and all(h["metadata"]["chunk_index"] != 2 for h in got) and len(got) == TOP_K
    assert any(0 in h["boosted_by"] for h in got) and any(h["boosted_by"] == [] for h in got)
    assert mgr._front.stats["boost_launches"] - before == calls + 1      # the device answered, one launch each here
    assert mgr.stats["boost_host_reranks"] == host_before


def test_a_document_shares_a_draw_and_by_ids(one_shard, corpus):
    _, _, Q, _, _ = corpus
    mgr = one_shard
    spec = FunctionScore(BoostRanker(None, 1.0, {"seed": 9, "field": "doc_id"}), boost_mode="sum", candidates=200)
    hits = asyncio.run(mgr.search(Q[0], "semantic_index", 200, ranker=spec))
    draws = {}
    for h in hits:
        draws.setdefault(int(h["id"][1:]) // 10, []).append(h["score"] - h["raw_score"])
    assert sum(len(v) > 1 for v in draws.values()) >= 10
    assert all(max(v) - min(v) < 1e-12 for v in draws.values()) and len({round(v[0], 9) for v in draws.values()}) > 50
    assert all(h["boosted_by"] == [0] for h in hits)
    by_id = asyncio.run(mgr.search_by_ids(["c7", "c1999"], "semantic_index", 6, ranker=specs(30)[2]))
    for name, got in zip(("c7", "c1999"), by_id):
        stored = mgr.collections["semantic_index"].handle.get_dense_rows([int(name[1:])])[0]
        assert sig(got) == sig(asyncio.run(mgr.search(stored, "semantic_index", 6, ranker=specs(30)[2]))) and len(got) == 6


def test_an_l2_collection_sorts_raw_distances_ascending(gpu, corpus):
    _, _, Q, _, _ = corpus
    mgr = manager(corpus, semantic_metric="L2")
    try:
        for ranker in (BoostRanker("chunk_index >= 3", 0.5), specs(30)[2], specs(30)[3]):
            want, plain = want_search(mgr, Q[0], "semantic_index", ranker, TOP_K, "L2")
            got = asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=ranker))
            assert sig(got) == want
            scores = [h["score"] for h in got]
            assert scores == sorted(scores, reverse=FunctionScore.of(ranker).normalization != "none")
        got = asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=BoostRanker("chunk_index >= 3", 0.5)))
        halved = [h for h in got if h["boosted_by"] == [0]]
        assert halved and all(h["score"] == 0.5 * h["raw_score"] for h in halved)          # a weight below 1 promotes
        assert all(h["score"] == h["raw_score"] for h in got if h["boosted_by"] == [])
    finally:
        asyncio.run(mgr.close())


def test_concurrent_searches_with_different_functions_share_launches(one_shard, corpus):
    _, _, Q, _, _ = corpus
    mgr = one_shard
    filters = [k for k in MATCH if k is not None]
    many = [FunctionScore(*(BoostRanker(filters[(i + j) % len(filters)], 0.5 + 0.25 * ((i + 3 * j) % 7),
                                        {"seed": 100 * i + j, "field": ("doc_id", None, "chunk_index")[j % 3]} if (i + j) % 3 == 0 else None)
                            for j in range(1 + i % 4)), candidates=30) for i in range(16)]
    serial = [sig(asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r))) for i, r in enumerate(many)]
    for i, r in enumerate(many[:5]):
        assert serial[i] == want_search(mgr, Q[i % NQ], "semantic_index", r, TOP_K, "COSINE")[0]
    assert len({tuple((s[0], s[1]) for s in one) for one in serial}) >= 12

    async def burst():
        return await asyncio.gather(*(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=r) for i, r in enumerate(many)))

    before = mgr._front.stats["boost_launches"]
    out = asyncio.run(burst())
    launches = mgr._front.stats["boost_launches"] - before
    assert [sig(o) for o in out] == serial
    assert 1 <= launches < 16


@pytest.mark.parametrize("decay", [False, True])
def test_retrieve_one_round_equals_the_general_path(gpu, long_timeout, corpus, decay):
    spec = FunctionScore(BoostRanker("chunk_index >= 3", 0.5), BoostRanker(TOPIC2, 3.0),
                         BoostRanker(None, 1.0, {"seed": 11, "field": "doc_id"}), function_mode="sum",
                         normalization="minmax" if decay else "none")
    ranker = DecayRanker("chunk_index", "linear", 4, 6, 0, 0.5) if decay else None
    answers = {}
    for name, kw in {"one_round": {}, "general": {"coalesce": False}}.items():
        mgr = manager(corpus, **kw)
        try:
            initialize_caches()
            retr = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, boost=spec, decay=ranker))
            answers[name] = [asyncio.run(retr.retrieve(f"plain statement q{q}", profile_hint="default")) for q in range(NQ)]
            if name == "one_round":
                st = mgr._front.stats
                assert st["hybrid_launches"] == NQ and st["boost_launches"] == NQ and st["decay_launches"] == (NQ if decay else 0)
                assert st["fuse_launches"] == 0
            else:
                assert mgr._front is None and mgr.stats["boost_host_reranks"] == NQ
                # the restatement over the boost-free fused list
                gen = mgr.embedding_generator
                sem = asyncio.run(mgr.search(gen.encode_semantic("q0"), "semantic_index", 2 * TOP_K))
                spa = asyncio.run(mgr.search(gen.encode_sparse("q0"), "sparse_index", 2 * TOP_K, None,
                                             {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
                ranked = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa]], (0.7, 0.3))
                row_of = {h["id"]: h["_row"] for h in sem + spa}
                pos, _, fin, _ = restate(mgr, [i for i, _, _ in ranked], [row_of[i] for i, _, _ in ranked], [s for _, s, _ in ranked],
                                         spec, "COSINE", fused=True)
                want = [(ranked[p][0], f, ranked[p][1]) for p, f in zip(pos, fin)]
                assert [w[0] for w in want] != [i for i, _, _ in ranked]
                if decay:
                    pos2, _, fin2 = D.decay_rerank([w[0] for w in want], [w[1] for w in want], [float(int(w[0][1:]) % 7) for w in want],
                                                   ranker.operands(), -1, len(want))
                    want = [(want[p][0], f, want[p][2]) for p, f in zip(pos2, fin2)]
                assert [(h["id"], float(h["score"]).hex(), float(h["fused_score"]).hex()) for h in answers[name][0]] == \
                    [(i, float(s).hex(), float(f).hex()) for i, s, f in want[:TOP_K]]
        finally:
            asyncio.run(mgr.close())
    for q in range(NQ):
        got, want = answers["one_round"][q], answers["general"][q]
        assert len(want) == TOP_K
        assert sig(got) == sig(want), q
        assert [h["retrieval_methods"] for h in got] == [h["retrieval_methods"] for h in want]      # the method bits follow
        assert [h["original_score"] for h in got] == [h["original_score"] for h in want]


def test_answers_after_an_append_a_delete_and_a_compaction(gpu, corpus):
    base, more, Q, _, _ = corpus
    mgr = manager(corpus)
    try:
        docs, mixed = specs(30)[0], specs(30)[4]
        new_doc = FunctionScore(BoostRanker(f'doc_id in ["doc{N // 10}", "doc{N // 10 + 1}"]', 6.0),
                                BoostRanker(None, 1.0, {"seed": 3, "field": "doc_id"}), function_mode="sum", boost_mode="sum",
                                candidates=30)
        for r in (docs, mixed):
            assert sig(asyncio.run(mgr.search(Q[0], "semantic_index", TOP_K, ranker=r))) == \
                want_search(mgr, Q[0], "semantic_index", r, TOP_K, "COSINE")[0]
        mgr.add_rows(more[0], more[2], **more[3])
        mgr.finalize()
        q_new = more[0][3] + 0.1 * Q[1]                                 # near an appended row: the new rows reach the window
        MATCH[new_doc.functions[0].filter] = lambda r: r // 10 in (N // 10, N // 10 + 1)
        for r in (docs, mixed, new_doc):
            want, plain = want_search(mgr, q_new, "semantic_index", r, TOP_K, "COSINE")
            assert any(h["_row"] >= N for h in plain)
            assert sig(asyncio.run(mgr.search(q_new, "semantic_index", TOP_K, ranker=r))) == want
        got = asyncio.run(mgr.search(q_new, "semantic_index", TOP_K, ranker=new_doc))
        assert got[0]["boosted_by"] == [0, 1] and int(got[0]["id"][1:]) >= N              # the appended rows are in the mask
        assert f"c{N + 3}" in [h["id"] for h in got]
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 1"))
        for r in (docs, mixed, new_doc):                                 # deleted, not yet compacted
            for q in (q_new, Q[2]):
                want, plain = want_search(mgr, q, "semantic_index", r, TOP_K, "COSINE")
                assert all(h["metadata"]["chunk_index"] != 1 for h in plain)
                assert sig(asyncio.run(mgr.search(q, "semantic_index", TOP_K, ranker=r))) == want
        mgr.compact()
        assert mgr.num_rows < N + N_MORE
        keep = np.array([r % 7 != 1 for r in range(N + N_MORE)])
        both = [np.concatenate([base[0], more[0]])[keep], np.concatenate([base[1], more[1]])[keep], None,
                {k: [v for v, ok in zip(base[3][k] + more[3][k], keep) if ok] for k in base[3]}]
        nnz = 5
        idx = np.concatenate([base[2][1], more[2][1]]).reshape(-1, nnz)[keep]
        val = np.concatenate([base[2][2], more[2][2]]).reshape(-1, nnz)[keep]
        both[2] = (np.arange(int(keep.sum()) + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
        fresh = manager(corpus, rows=both)
        try:
            for r in (docs, mixed, new_doc):
                for q in (q_new, Q[2]):
                    want, _ = want_search(mgr, q, "semantic_index", r, TOP_K, "COSINE")
                    got = sig(asyncio.run(mgr.search(q, "semantic_index", TOP_K, ranker=r)))
                    assert got == want and got == sig(asyncio.run(fresh.search(q, "semantic_index", TOP_K, ranker=r)))
        finally:
            asyncio.run(fresh.close())
    finally:
        MATCH.pop(new_doc.functions[0].filter, None)
        asyncio.run(mgr.close())


def test_two_shards_equal_one_shard(one_shard, long_timeout, corpus):
    _, _, Q, SQ, _ = corpus
    two = manager(corpus, devices=[0, 0])
    try:
        assert two._front is None or two._coalescer(two.collections["semantic_index"]) is None
        for i, ranker in enumerate(specs(25)):
            assert sig(asyncio.run(two.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker))) == \
                sig(asyncio.run(one_shard.search(Q[i % NQ], "semantic_index", TOP_K, ranker=ranker)))
        assert two.stats["boost_host_reranks"] == len(specs())
        cfg = dict(top_k=TOP_K, boost=specs()[1])
        one = manager(corpus)
        try:
            initialize_caches()
            a = asyncio.run(HybridRetriever(two, RetrievalConfig(**cfg)).retrieve("plain statement q1", profile_hint="default"))
            initialize_caches()
            b = asyncio.run(HybridRetriever(one, RetrievalConfig(**cfg)).retrieve("plain statement q1", profile_hint="default"))
        finally:
            asyncio.run(one.close())
        assert sig(a) == sig(b) and len(a) == TOP_K and two.stats["boost_host_reranks"] == len(specs()) + 1
    finally:
        asyncio.run(two.close())


def test_refusals_on_the_device_manager(one_shard, corpus):
    _, _, Q, _, _ = corpus
    mgr = one_shard
    before = dict(mgr._front.stats) if mgr._front is not None else {}
    for bad in ("chunk_index >>> 3", "no_such_field == 1", 'TEXT_MATCH(content, "a", minimum_should_match=16385)'):
        with pytest.raises(ValueError):
            asyncio.run(mgr.search(Q[0], "semantic_index", 5, ranker=BoostRanker(bad, 2.0)))
    with pytest.raises(ValueError, match="offset"):
        asyncio.run(mgr.search(Q[0], "semantic_index", 5, ranker=BoostRanker(None, 2.0), offset=1))
    with pytest.raises(ValueError, match="ranker"):
        asyncio.run(mgr.search(Q[0], "semantic_index", 5, ranker=object()))
    if mgr._front is not None:
        after = mgr._front.stats
        assert all(after[k] == before[k] for k in ("dense_launches", "boost_launches"))      # refused before anything is searched
