"""multi_search / retrieve_multi without a GPU: the three spec classes and every refusal, the two restatements as the
contract of hr_fuse_lists_dev (generalisation of the three-list golden cases, accumulation in list order), multi_search and
retrieve_multi on the manager over oracle-backed stand-ins for the shard handles (the setup of test_decay_host.py), and
plan_and_execute(fuse=...)."""
import asyncio
import json
import os

import numpy as np
import pytest

import test_decay_host as dh
from advanced_rag import AdvancedRAGPipeline, HybridRetriever, PipelineConfig, RetrievalConfig
from advanced_rag import _native as nat
from advanced_rag import multi_search as ms
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.multi_search import RRFRanker, SearchRequest, WeightedRanker
from advanced_rag.retrieval import norm_code, rrf_rank_lists, score_fuse_lists

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_codes_limits_and_symbol():
    assert (nat.HR_MAX_FUSE_LISTS, nat.HR_FUSE_RRF, nat.HR_FUSE_WEIGHTED) == (16, 0, 1)
    assert "hr_fuse_lists_dev" in nat.EXPORTED_SYMBOLS and ms.MAX_FUSED == 3 * nat.HR_MAX_TOPK
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hbmrag.h")).read()
    assert "#define HR_MAX_FUSE_LISTS 16" in header and "enum { HR_FUSE_RRF = 0, HR_FUSE_WEIGHTED = 1 };" in header
    assert "HR_API int hr_fuse_lists_dev(" in header


# ---- the restatement is the contract -------------------------------------------------------------------------------------
def test_restatement_reproduces_the_three_list_golden_cases():
    with open(os.path.join(GOLD, "g1_fuse.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 20
    names = ("semantic", "sparse", "domain")
    for c in cases:
        fused = rrf_rank_lists([c[m] for m in names], [c["dense_weight"], c["sparse_weight"], 0.2], 60)
        assert [f[0] for f in fused] == c["ids"], c["label"]
        assert [float(f[1]).hex() for f in fused] == c["scores"], c["label"]
        assert all(ls == sorted(set(ls)) for _, _, ls in fused)              # the method list = the list indices, ascending
        assert [sorted(names[l] for l in f[2]) for f in fused] == c["methods"], c["label"]


def test_accumulation_is_in_list_order():
    lists = [["x"]] * 4
    assert rrf_rank_lists(lists, [1e16, 1.0, -1e16, 1.0])[0][1] == 0.047643442622950824
    assert rrf_rank_lists(lists, [1e16, -1e16, 1.0, 1.0])[0][1] == 0.03278688524590164
    assert rrf_rank_lists(lists, [1e16, 1.0, -1e16, 1.0])[0][2] == [0, 1, 2, 3]
    # the weighted restatement: the same order of additions (COSINE code: n = (1 + s) / 2 = 0.75 for s = 0.5)
    sl = [(["x"], [0.5])] * 4
    assert score_fuse_lists(sl, [1e16, 1.0, -1e16, 1.0], [0] * 4)[0][1] == ((0.0 + 0.75 * 1e16 + 0.75) - 0.75 * 1e16) + 0.75
    assert score_fuse_lists(sl, [1e16, -1e16, 1.0, 1.0], [0] * 4)[0][1] == 1.5


def test_host_fusion_of_a_request_is_the_restatement_cut_and_masked():
    rows = [[5, 3, 9], [9, 7, -1, 3], [], [3]]
    scores = [[0.9, 0.5, 0.1], [4.0, 2.0, 0.0, 9.0], [], [0.25]]
    w = [1.0, 0.5, 2.0, -0.25]
    payload, key = ms.check_fuse_lists(rows, scores, w, nat.HR_FUSE_WEIGHTED, [0, 3, 1, 1], 60, None)
    assert key == (1, 4, 8, (0, 3, 1, 1), 60, 6) and [len(r) for r, _ in payload[0]] == [3, 2, 0, 1]    # -1 ends list 1
    ids, sc, wq = ms.stage_fuse_lists([payload, payload], key)
    assert ids.shape == (2, 4, 8) and ids[1, 1].tolist() == [9, 7] + [-1] * 6 and sc.dtype == np.float32 and wq.tolist() == [w, w]
    want = score_fuse_lists([([5, 3, 9], scores[0]), ([9, 7], [4.0, 2.0]), ([], []), ([3], [0.25])], w, [0, 3, 1, 1])
    r, s, m = ms.fuse_lists_host(payload, key)
    assert r.tolist() == [f[0] for f in want] and s.tolist() == [f[1] for f in want]
    assert [ms.lists_of_mask(x) for x in m] == [f[2] for f in want]
    payload, key = ms.check_fuse_lists(rows, None, w, nat.HR_FUSE_RRF, None, 60, 2)
    r, s, m = ms.fuse_lists_host(payload, key)
    want = rrf_rank_lists([[5, 3, 9], [9, 7], [], [3]], w, 60)[:2]
    assert key[3] is None and r.tolist() == [f[0] for f in want] and s.tolist() == [f[1] for f in want]
    for bad in (dict(row_lists=[]), dict(row_lists=[[1]] * 17, weights=[1.0] * 17), dict(weights=[1.0]), dict(top_k=769),
                dict(top_k=0), dict(weights=[1.0, 1.0, float("inf"), 1.0]), dict(row_lists=[list(range(257)), [], [], []])):
        kw = dict(row_lists=rows, score_lists=None, weights=w, mode=nat.HR_FUSE_RRF, norms=None, rrf_k=60, top_k=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ms.check_fuse_lists(**kw)
    with pytest.raises(ValueError):
        ms.check_fuse_lists(rows, scores, w, nat.HR_FUSE_WEIGHTED, [0, 5, 1, 1], 60, None)
    with pytest.raises(ValueError):
        ms.check_fuse_lists(rows, None, w, nat.HR_FUSE_WEIGHTED, [0, 1, 1, 1], 60, None)


# ---- the spec classes -----------------------------------------------------------------------------------------------------
def test_spec_classes_validate():
    r = SearchRequest([0.0], "semantic_index")
    assert (r.limit, r.filters, r.search_params) == (20, None, None)
    assert SearchRequest([0.0], "sparse_index", np.int64(7)).limit == 7
    for bad in (0, -1, nat.HR_MAX_TOPK + 1, True, 5.0, "5", None):
        with pytest.raises(ValueError, match="limit"):
            SearchRequest([0.0], "semantic_index", bad)
    with pytest.raises(ValueError):
        SearchRequest([0.0], 3)
    with pytest.raises(ValueError):
        SearchRequest([0.0], "semantic_index", filters={"doc_id": "x"})
    with pytest.raises(ValueError):
        SearchRequest([0.0], "semantic_index", search_params="COSINE")
    assert (RRFRanker().k, RRFRanker().weights) == (60, None) and RRFRanker(10, [1, 2.5]).weights == (1.0, 2.5)
    for bad in (0, -3, True, 60.0):
        with pytest.raises(ValueError):
            RRFRanker(bad)
    for bad in ([1.0, float("nan")], [float("inf")], ["a"], [True]):
        with pytest.raises(ValueError):
            RRFRanker(60, bad)
        with pytest.raises(ValueError):
            WeightedRanker(*bad)
    w = WeightedRanker(0.7, 0.3)
    assert w.weights == (0.7, 0.3) and w.normalization == "activation"
    assert WeightedRanker(1, normalization="minmax").normalization == "minmax"
    with pytest.raises(ValueError, match="normalization"):
        WeightedRanker(1.0, normalization="zscore")
    with pytest.raises(ValueError):
        WeightedRanker()


# ---- multi_search on the manager --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    mgr, X, csr = dh._manager(dh.sq._OracleShard, 2)
    assert mgr._filters_on_device() is None
    yield mgr, X, csr
    asyncio.run(mgr.close())


def _sparse_q(csr, r):
    a, b = csr[0][r], csr[0][r + 1]
    return {"indices": csr[1][a:b].tolist(), "values": csr[2][a:b].tolist()}


def _requests(X, csr):
    return [SearchRequest(X[5] + 0.25 * X[40], "semantic_index", 12),
            SearchRequest(X[5] + 0.5 * X[41], "semantic_index", 12, filters="chunk_index >= 3"),
            SearchRequest(_sparse_q(csr, 12), "sparse_index", 9, search_params={"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}),
            SearchRequest(X[6], "semantic_index", 5, filters='doc_id != "doc1"', search_params={"metric_type": "COSINE", "params": {"ef": 32}}),
            SearchRequest(X[40], "semantic_index", 7)]


def _expected(mgr, reqs, ranker, limit):
    lists = [asyncio.run(mgr.search(r.data, r.collection_name, r.limit, r.filters, r.search_params)) for r in reqs]
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
    return out


@pytest.mark.parametrize("ranker", [RRFRanker(), RRFRanker(10, [1.0, 0.5, 2.0, 0.25, -1.0]), WeightedRanker(0.5, 0.2, 0.1, 0.1, 0.1),
                                    WeightedRanker(1.0, 1.0, 0.5, 2.0, 0.25, normalization="minmax")], ids=repr)
def test_multi_search_equals_the_restatement_over_the_searches(host, ranker):
    mgr, X, csr = host
    reqs = _requests(X, csr)
    before = mgr.stats["multi_searches"]
    for limit in (4, 100):
        got = asyncio.run(mgr.multi_search(reqs, ranker, limit))
        want = _expected(mgr, reqs, ranker, limit)
        assert [(h["_row"], h["id"], float(h["score"]).hex(), h["original_score"], h["requests"]) for h in got] == want
        assert len(got) == min(limit, len(want)) and set(got[0]) >= {"content", "metadata"}
    assert len(got) < 100 and any(len(h["requests"]) > 1 for h in got)          # fewer fused rows than limit: a shorter list
    assert mgr.stats["multi_searches"] == before + 2
    assert not hasattr(mgr.collections["semantic_index"], "multi_search")


def test_multi_search_refusals_come_before_any_search(host):
    mgr, X, csr = host
    ok = SearchRequest(X[0], "semantic_index", 5)
    calls = []
    real = mgr._search_lists_async

    async def spy(*a, **kw):
        calls.append(a)
        return await real(*a, **kw)
    mgr._search_lists_async = spy
    run = lambda reqs, ranker=RRFRanker(), limit=10: asyncio.run(mgr.multi_search(reqs, ranker, limit))
    try:
        cases = [([], {}), ([ok] * 17, {}), (ok, {}), ([ok, "semantic_index"], {}), ([ok, (X[0], "semantic_index", 5)], {}),
                 ([ok, SearchRequest(X[0], "nope", 5)], {}),
                 ([ok], dict(limit=0)), ([ok], dict(limit=3 * nat.HR_MAX_TOPK + 1)), ([ok], dict(limit=True)), ([ok], dict(limit=10.0)),
                 ([ok], dict(ranker=None)), ([ok], dict(ranker="rrf")), ([ok], dict(ranker=dh.DecayRanker("chunk_index", "exp", 0, 4))),
                 ([ok, ok], dict(ranker=RRFRanker(60, [1.0]))), ([ok], dict(ranker=WeightedRanker(0.5, 0.5))),
                 ([ok, SearchRequest(X[0], "semantic_index", 5, search_params={"metric_type": "L2"})], {}),
                 ([ok, SearchRequest(X[0], "semantic_index", 5, search_params={"params": {"radius": float("nan")}})], {}),
                 ([ok, SearchRequest(X[0], "semantic_index", 5, search_params={"params": {"radius": 0.5, "range_filter": 0.25}})], {}),
                 ([ok, SearchRequest(_sparse_q(csr, 3), "sparse_index", 5, search_params={"metric_type": "IP", "params": {"radius": 0.5}})], {})]
        for reqs, kw in cases:
            with pytest.raises(ValueError):
                run(reqs, **kw)
        # what is mutable is checked again by the call
        moved = SearchRequest(X[0], "semantic_index", 5)
        moved.limit = 300
        with pytest.raises(ValueError, match="limit"):
            run([moved])
        r = RRFRanker()
        r.weights = (1.0, float("nan"))
        with pytest.raises(ValueError, match="finite"):
            run([ok, ok], ranker=r)
        w = WeightedRanker(1.0)
        w.normalization = "zscore"
        with pytest.raises(ValueError, match="normalization"):
            run([ok], ranker=w)
        assert calls == []
        assert len(run([ok])) == 5 and len(calls) == 1

        class Collective:
            round = None
        coll = mgr.collections["semantic_index"]
        kept, coll.handle = coll.handle, Collective()
        try:
            with pytest.raises(NotImplementedError, match="torchrun"):
                run([ok])
        finally:
            coll.handle = kept
        assert len(calls) == 1
    finally:
        del mgr._search_lists_async


def test_a_failing_sub_search_fails_the_call(host):
    mgr, X, _ = host
    real = mgr._search_lists_blocking

    def broken(query, collection_name, top_k, *a, **kw):
        if top_k == 7:
            raise RuntimeError("shard lost")
        return real(query, collection_name, top_k, *a, **kw)
    mgr._search_lists_blocking = broken
    try:
        with pytest.raises(RuntimeError, match="shard lost"):
            asyncio.run(mgr.multi_search([SearchRequest(X[0], "semantic_index", 5), SearchRequest(X[1], "semantic_index", 7)],
                                         RRFRanker(), 5))
    finally:
        del mgr._search_lists_blocking


# ---- retrieve_multi ---------------------------------------------------------------------------------------------------------
class _FixedManager:
    """search() answers from a table keyed by (collection, embedding tag); no fusion entry point: the restatements serve."""
    LISTS = {("semantic_index", 0): ["a", "b"], ("sparse_index", 0): ["b", "c"],
             ("semantic_index", 1): ["c", "a"], ("sparse_index", 1): ["d"]}

    def __init__(self):
        self.calls = []

    async def _generate_semantic_embedding(self, text):
        return int(text[-1])

    async def _generate_sparse_embedding(self, text):
        return int(text[-1])

    async def search(self, query_embedding, collection_name, top_k=20, filters=None, search_params=None):
        self.calls.append((collection_name, query_embedding, top_k, filters))
        return [{"id": i, "content": f"{collection_name[:3]}{query_embedding} {i}", "score": 0.9 - 0.1 * r, "metadata": {}}
                for r, i in enumerate(self.LISTS[(collection_name, query_embedding)])]


def test_retrieve_multi_against_a_hand_written_expectation():
    mgr = _FixedManager()
    r = HybridRetriever(mgr, RetrievalConfig(top_k=3, dense_weight=0.7, sparse_weight=0.3))
    got = asyncio.run(r.retrieve_multi(["wording 0", "wording 1"], filters={"doc_id": "x"}, profile_hint="default",
                                       query_weights=[1.0, 0.5]))
    # lists: sem_0 = a b | spa_0 = b c | sem_1 = c a | spa_1 = d; weights 0.7, 0.3, 0.7 * 0.5, 0.3 * 0.5; k = 60
    a = (0.0 + (1.0 / 61) * 0.7) + (1.0 / 62) * (0.7 * 0.5)
    b = (0.0 + (1.0 / 62) * 0.7) + (1.0 / 61) * 0.3
    c = (0.0 + (1.0 / 62) * 0.3) + (1.0 / 61) * (0.7 * 0.5)
    d = 0.0 + (1.0 / 61) * (0.3 * 0.5)
    assert a > b > c > d
    assert [(h["id"], h["score"]) for h in got] == [("a", a), ("b", b), ("c", c)]                  # cut at top_k = 3
    assert [h["retrieval_methods"] for h in got] == [["semantic"], ["semantic", "sparse"], ["semantic", "sparse"]]
    assert [h["queries"] for h in got] == [["wording 0", "wording 1"], ["wording 0"], ["wording 0", "wording 1"]]
    assert [h["content"] for h in got] == ["sem0 a", "sem0 b", "sem1 c"]           # the payload: the first semantic hit
    assert all(h["metadata"]["retrieval_profile"] == "default" for h in got)
    assert mgr.calls == [("semantic_index", 0, 6, 'doc_id == "x"'), ("sparse_index", 0, 6, 'doc_id == "x"'),
                         ("semantic_index", 1, 6, 'doc_id == "x"'), ("sparse_index", 1, 6, 'doc_id == "x"')]
    r = HybridRetriever(_FixedManager(), RetrievalConfig(top_k=4, fusion="weighted"))
    got = asyncio.run(r.retrieve_multi(["wording 0", "wording 1"], profile_hint="default"))
    want = score_fuse_lists([(ids, [0.9 - 0.1 * i for i in range(len(ids))]) for ids in _FixedManager.LISTS.values()],
                            [0.7, 0.3, 0.7, 0.3], [0, 1, 0, 1])
    assert [(h["id"], h["score"]) for h in got] == [(i, s) for i, s, _ in want]


def test_retrieve_multi_refusals():
    r = HybridRetriever(_FixedManager(), RetrievalConfig(top_k=3))
    for bad in ([], ["q0"] * 9, "q0", [0], None):
        with pytest.raises(ValueError):
            asyncio.run(r.retrieve_multi(bad))
    for bad in ([1.0], [1.0, float("nan")], [1.0, "2"], [True, 1.0]):
        with pytest.raises(ValueError):
            asyncio.run(r.retrieve_multi(["q0", "q1"], query_weights=bad))
    big = HybridRetriever(_FixedManager(), RetrievalConfig(top_k=nat.HR_MAX_TOPK // 2 + 1))
    with pytest.raises(ValueError, match="top_k"):
        asyncio.run(big.retrieve_multi(["q0"], profile_hint="default"))
    assert r.index_manager.calls == []


@pytest.mark.parametrize("fusion", ["rrf", "weighted"])
def test_retrieve_multi_of_one_wording_equals_retrieve(host, fusion):
    mgr, X, csr = host
    mgr.embedding_generator = dh._Gen(X, csr)
    old, RetrievalConstants.TIMEOUT_SECONDS = RetrievalConstants.TIMEOUT_SECONDS, 60.0
    try:
        for mmr in (False, True):
            cfg = dict(top_k=6, fusion=fusion, enable_mmr=mmr, mmr_lambda=0.6)
            for qn in (10, 30):
                initialize_caches()
                text = f"plain statement q{qn}"
                one = asyncio.run(HybridRetriever(mgr, RetrievalConfig(**cfg)).retrieve(text, profile_hint="default"))
                many = asyncio.run(HybridRetriever(mgr, RetrievalConfig(**cfg)).retrieve_multi([text], profile_hint="default"))
                key = lambda hits: [(h["id"], float(h["score"]).hex(), h["retrieval_methods"]) for h in hits]
                assert key(one) == key(many) and len(one) == 6 and all(h["queries"] == [text] for h in many)
        # several wordings through the manager's fuse_lists_async (a stand-in: the restatement behind it) = the restatement
        texts = ["plain statement q10", "plain statement q30", "plain statement q11"]
        initialize_caches()
        r = HybridRetriever(mgr, RetrievalConfig(top_k=8, fusion=fusion))
        got = asyncio.run(r.retrieve_multi(texts, profile_hint="default", query_weights=[1.0, 0.5, 0.25]))
        gen, lists = mgr.embedding_generator, []
        for t in texts:
            lists.append(asyncio.run(mgr.search(gen.encode_semantic(t), "semantic_index", 16, None, r.config.semantic_search_params)))
            lists.append(asyncio.run(mgr.search(gen.encode_sparse(t), "sparse_index", 16, None, r.config.sparse_search_params)))
        w = [x * q for q in (1.0, 0.5, 0.25) for x in (0.7, 0.3)]
        if fusion == "rrf":
            want = rrf_rank_lists([[h["id"] for h in l] for l in lists], w, 60)
        else:
            want = score_fuse_lists([([h["id"] for h in l], [h["score"] for h in l]) for l in lists], w, [0, 1] * 3)
        assert [(h["id"], float(h["score"]).hex()) for h in got] == [(i, float(s).hex()) for i, s, _ in want[:8]]
        assert [h["queries"] for h in got] == [[texts[i] for i in sorted({l // 2 for l in ls})] for _, _, ls in want[:8]]
    finally:
        RetrievalConstants.TIMEOUT_SECONDS = old
        mgr.embedding_generator = None


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
def test_plan_and_execute_default_is_what_it_was_and_fuse_adds_the_fused_list():
    import test_host_logic as hl
    p = AdvancedRAGPipeline(connect_to_milvus=False, config=PipelineConfig(enable_audit_logging=False))
    p.index_manager = hl.FakeIndexManager()
    p.retriever.index_manager = p.index_manager
    plan = asyncio.run(p.plan_and_execute("alpha and beta"))
    assert sorted(plan) == ["decomposition", "subqueries"]
    assert plan["decomposition"]["sub_queries"] == ["alpha", "beta"] and len(plan["subqueries"]) == 2
    fused = asyncio.run(p.plan_and_execute("alpha and beta", fuse=True))
    assert sorted(fused) == ["decomposition", "fused", "subqueries"]
    assert {h["id"] for h in fused["fused"]} == {"S", "P"} and fused["fused"][0]["queries"] == ["alpha", "beta"]
    s = (0.0 + (1.0 / 61) * 0.7) + (1.0 / 61) * 0.7
    assert fused["fused"][0]["id"] == "S" and fused["fused"][0]["score"] == s
