"""Boost ranker and function score without a GPU: the draw, the restatement (advanced_rag/boost.py), spec validation, and
search(ranker=...) / retrieve(boost=...) on CPU stand-in managers (one shard and three) against the restatement."""
import asyncio
import math

import numpy as np
import pytest

import test_decay_host as dh
import test_sparse_query_host as sq
from advanced_rag import HybridRetriever, RetrievalConfig
from advanced_rag import _native as nat
from advanced_rag import boost as BO
from advanced_rag import decay as D
from advanced_rag.boost import BoostRanker, FunctionScore
from advanced_rag.constants import RetrievalConstants
from advanced_rag.decay import DecayRanker
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.pipeline import PipelineConfig
from advanced_rag.retrieval import rrf_rank_lists


def hexes(values):
    return [float(v).hex() for v in values]


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def test_codes_match_the_header():
    assert (nat.HR_MAX_BOOST_FUNCS, nat.HR_BOOST_ACTIVE, nat.HR_BOOST_RANDOM, nat.HR_BOOST_MULTIPLY, nat.HR_BOOST_SUM) == (8, 1, 2, 0, 1)
    assert nat.BOOST_FUNC_DTYPE.itemsize == 56
    assert "hr_boost_rerank_dev" in nat.EXPORTED_SYMBOLS


@pytest.mark.parametrize("seed, key, u", [(0, 0, 0.6524484863740322), (126, 0, 0.4642177690240783), (126, 1, 0.9170314847966232),
                                          (126, -1, 0.1269855469743124), (2 ** 64 - 1, 2 ** 62, 0.2569625771059303),
                                          (1, 126, 0.3342356104450862)])
def test_known_answers_of_the_draw(seed, key, u):
    assert BO.canonical_random(seed, key) == u


def test_the_draw_is_uniform_enough():
    us = [BO.canonical_random(7, k) for k in range(100_000)]
    assert all(0.0 <= u < 1.0 for u in us)
    assert abs(sum(us) / len(us) - 0.5) < 0.01
    assert BO.canonical_random(7, -1) == BO.canonical_random(7, 2 ** 64 - 1)      # the key is taken mod 2^64


# ---- the restatement ------------------------------------------------------------------------------------------------------------
WORKED = ([0, 1, 2], [0.5, 0.25, 0.125], [[False, True, True], [False, False, True]], [3.0, 0.5])


@pytest.mark.parametrize("modes, finals, pos", [(("multiply", "multiply"), [0.5, 0.75, 0.1875], [1, 0, 2]),
                                                (("sum", "multiply"), [0.5, 0.75, 0.4375], [1, 0, 2]),
                                                (("multiply", "sum"), [0.5, 3.25, 1.625], [1, 2, 0])])
def test_the_worked_list(modes, finals, pos):
    got = BO.boost_rerank(*WORKED, *modes)
    assert got[0] == pos and got[1] == pos and got[2] == [finals[p] for p in pos]
    assert got[3] == [[0, 1, 3][p] for p in pos]
    codes = BO.boost_rerank(*WORKED, BO.BOOST_MODES[modes[0]], BO.BOOST_MODES[modes[1]])
    assert codes == got
    assert BO.boost_rerank(*WORKED, *modes, k_out=2)[0] == pos[:2]


def test_sum_mode_depends_on_the_order_of_the_functions():
    every = [[True]] * 3
    for weights, factor in (([1e16, 1.0, -1e16], 0.0), ([1e16, -1e16, 1.0], 1.0)):
        _, _, fin, hit = BO.boost_rerank([5], [2.0], every, weights, "sum", "sum")
        assert fin == [2.0 + factor] and hit == [7]


def test_unmatched_entries_keep_their_score_bit_for_bit():
    scores = [0.1, -0.0, 5e-324, 1.0 / 3.0]
    none = [[False] * 4]
    for bm in ("multiply", "sum"):
        pos, _, fin, hit = BO.boost_rerank([1, 2, 3, 4], scores, none, [9.0], "multiply", bm)
        assert hexes(fin) == hexes(scores[p] for p in pos) and hit == [0] * 4
    # min-max normalised, then untouched: n(s) itself
    _, _, fin, _ = BO.boost_rerank([1, 2, 3], [3.0, 2.0, 1.0], [[False] * 3], [9.0], norm=nat.HR_NORM_MINMAX)
    assert fin == D.normalise([3.0, 2.0, 1.0], nat.HR_NORM_MINMAX) == [1.0, 0.5, 0.0]


def test_zero_weight_direction_and_nans():
    n = 12
    scores = [1.0 - i / 16 for i in range(n)]
    pos, _, fin, _ = BO.boost_rerank(list(range(n)), scores, [[True] * n], [0.0])
    assert pos == list(range(n)) and fin == [0.0] * n                        # all ties: the input order holds
    pos, _, fin, _ = BO.boost_rerank(list(range(n)), [-s for s in scores], [[True] * n], [0.0], ascending=True)
    assert pos == list(range(n)) and all(math.copysign(1.0, f) == -1.0 for f in fin)      # -0.0 ties with itself too
    # ascending: the smallest final first; a weight below 1 promotes a distance
    pos, _, fin, _ = BO.boost_rerank([7, 8, 9], [1.0, 2.0, 3.0], [[False, False, True]], [0.25], ascending=True)
    assert pos == [2, 0, 1] and fin == [0.75, 1.0, 2.0]
    # a NaN final ranks after every number in either direction; NaNs keep input order
    nan, inf = float("nan"), float("inf")
    for asc, want in ((False, [3, 1, 0, 2, 4]), (True, [1, 3, 0, 2, 4])):
        pos, _, fin, _ = BO.boost_rerank([0, 1, 2, 3, 4], [nan, 1.0, inf, 2.0, nan], [[False, False, True, False, False]], [0.0],
                                         ascending=asc)
        assert pos == want and all(f != f for f in fin[2:])


def test_a_draw_scales_the_weight_and_follows_the_key():
    keys = [10, 11, 10, -3]
    pos, _, fin, _ = BO.boost_rerank([0, 1, 2, 3], [1.0] * 4, [[True] * 4], [(2.0, 126, keys)], "multiply", "sum")
    want = [1.0 + 2.0 * BO.canonical_random(126, k) for k in keys]
    assert sorted(fin, reverse=True) == fin and {p: f for p, f in zip(pos, fin)} == dict(enumerate(want))
    assert want[0] == want[2]


# ---- the specs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, name", [
    (dict(filter=5), "filter"), (dict(filter="  "), "filter"),
    (dict(weight="2"), "weight"), (dict(weight=True), "weight"), (dict(weight=float("nan")), "weight"),
    (dict(weight=float("inf")), "weight"),
    (dict(random_score=7), "random_score"), (dict(random_score={}), "random_score"),
    (dict(random_score={"seed": 1, "fields": None}), "random_score"),
    (dict(random_score={"seed": True}), "seed"), (dict(random_score={"seed": -1}), "seed"),
    (dict(random_score={"seed": 2 ** 64}), "seed"), (dict(random_score={"seed": 1.0}), "seed"),
    (dict(random_score={"seed": 1, "field": "entropy"}), "field"), (dict(random_score={"seed": 1, "field": 3}), "field")])
def test_boost_ranker_refusals_name_their_argument(kw, name):
    with pytest.raises(ValueError, match=name):
        BoostRanker(**kw)


def test_function_score_refusals_and_codes():
    f = BoostRanker("chunk_index >= 3", 2)
    for args, kw, name in [((), {}, "functions"), ((f,) * 9, {}, "functions"), ((f, "x"), {}, "BoostRanker"),
                           ((f,), dict(function_mode="avg"), "function_mode"), ((f,), dict(boost_mode=True), "boost_mode"),
                           ((f,), dict(normalization="l2"), "normalization"), ((f,), dict(candidates=0), "candidates"),
                           ((f,), dict(candidates=True), "candidates"), ((f,), dict(candidates=2.0), "candidates")]:
        with pytest.raises(ValueError, match=name):
            FunctionScore(*args, **kw)
    s = FunctionScore(f, BoostRanker(None, 0.5, {"seed": 2 ** 64 - 1, "field": "doc_id"}), function_mode="sum", candidates=40)
    assert s.operands() == (("chunk_index >= 3", 2.0, None, None), (None, 0.5, 2 ** 64 - 1, "doc_id"))
    assert s.window(10) == 40 and s.window(64) == 64
    assert s.launch_key("COSINE") == (1, 0, nat.HR_NORM_NONE, 0)
    assert s.launch_key("L2") == (1, 0, nat.HR_NORM_NONE, 1)                  # raw distances: ascending
    assert s.launch_key("L2", fused=True) == (1, 0, nat.HR_NORM_NONE, 0)
    act = FunctionScore(f, normalization="activation", boost_mode="sum")
    assert act.launch_key("L2") == (0, 1, nat.HR_NORM_ATAN_DIST, 0) and act.launch_key("IP") == (0, 1, nat.HR_NORM_ATAN, 0)
    assert act.launch_key("COSINE") == (0, 1, nat.HR_NORM_COSINE, 0) and act.launch_key("L2", fused=True)[2] == nat.HR_NORM_NONE
    mm = FunctionScore(f, normalization="minmax")
    assert mm.launch_key("L2") == (0, 0, nat.HR_NORM_MINMAX_DIST, 0) and mm.launch_key("L2", fused=True)[2] == nat.HR_NORM_MINMAX
    assert FunctionScore.of(f).functions == (f,) and FunctionScore.of(s) is s
    with pytest.raises(ValueError, match="ranker"):
        FunctionScore.of(object())


def test_configs_carry_the_boost_field():
    f = BoostRanker("chunk_index >= 3", 2)
    assert RetrievalConfig().boost is None and PipelineConfig().boost is None
    assert RetrievalConfig(boost=f).boost is f and PipelineConfig(boost=FunctionScore(f)).boost.functions == (f,)
    for bad in ("boost", 2.0, object(), DecayRanker("chunk_index", scale=1.0, origin=0)):
        with pytest.raises(ValueError, match="boost"):
            RetrievalConfig(boost=bad)
    r = HybridRetriever(None, RetrievalConfig(boost=f))
    assert all(cfg.boost is f for cfg in r.profiles.values())


# ---- search(ranker=...) on the stand-in managers -------------------------------------------------------------------------------------------
# what the rows of test_decay_host._manager hold: doc r // 5, chunk_index r % 9, token_count 30 + r % 41, content topic{r % 5} ...
MATCH = {None: lambda r: True, "chunk_index >= 3": lambda r: r % 9 >= 3, 'doc_id in ["doc3", "doc7", "doc11"]': lambda r: r // 5 in (3, 7, 11),
         'TEXT_MATCH(content, "topic2")': lambda r: r % 5 == 2, "token_count < 40 or chunk_index == 0": lambda r: r % 41 < 10 or r % 9 == 0,
         "chunk_index > 100": lambda r: False}


@pytest.fixture(scope="module", params=[("COSINE", 1), ("L2", 3)], ids=["cosine-1", "l2-3"])
def host(request):
    metric, shards = request.param
    mgr, X, csr = dh._manager(sq._OracleShard if metric == "COSINE" else dh._L2Shard, shards)
    assert mgr.semantic_metric == metric and mgr._filters_on_device() is None
    yield mgr, X, csr, metric
    asyncio.run(mgr.close())


def restate(mgr, rows, scores, spec, metric, fused=False):
    """boost_rerank over what the rows are known to hold (not over the manager's masks)."""
    matches = [[MATCH[f.filter](r) for r in rows] for f in spec.functions]
    values = []
    for f in spec.functions:
        if f.seed is None:
            values.append(f.weight)
        else:
            keys = rows if f.field is None else [int(mgr._host_group_keys(f.field)[r]) for r in rows]
            values.append((f.weight, f.seed, keys))
    fm, bm, norm, asc = spec.launch_key(metric, fused)
    return BO.boost_rerank(rows, scores, matches, values, fm, bm, norm, bool(asc))


def check_search(mgr, query, coll, metric, ranker, top_k, **kw):
    spec = FunctionScore.of(ranker)
    W = spec.window(top_k)
    before = mgr.stats["boost_host_reranks"]
    plain = asyncio.run(mgr.search(query, coll, W, **kw))
    got = asyncio.run(mgr.search(query, coll, top_k, ranker=ranker, **kw))
    rows = [h["_row"] for h in plain]
    pos, _, fin, hit = restate(mgr, rows, [h["score"] for h in plain], spec, metric)
    assert [h["id"] for h in got] == [plain[p]["id"] for p in pos[:top_k]]
    assert hexes(h["score"] for h in got) == hexes(fin[:top_k])
    assert [h["raw_score"] for h in got] == [plain[p]["score"] for p in pos[:top_k]]
    assert [h["boosted_by"] for h in got] == [BO.matched_functions(m) for m in hit[:top_k]]
    assert mgr.stats["boost_host_reranks"] == before + 1
    return got, plain


SPECS = [
    BoostRanker('doc_id in ["doc3", "doc7", "doc11"]', 4.0),
    FunctionScore(BoostRanker("chunk_index >= 3", 0.5), BoostRanker('TEXT_MATCH(content, "topic2")', 3.0), candidates=40),
    FunctionScore(BoostRanker("chunk_index >= 3", 0.25), BoostRanker("token_count < 40 or chunk_index == 0", -1.5),
                  BoostRanker("chunk_index > 100", 50.0), function_mode="sum", boost_mode="sum", normalization="activation",
                  candidates=30),
    FunctionScore(BoostRanker(None, 1.0, {"seed": 126, "field": "doc_id"}), boost_mode="sum", normalization="minmax", candidates=25),
    FunctionScore(BoostRanker("chunk_index >= 3", 2.0, {"seed": 5, "field": None}),
                  BoostRanker(None, 0.5, {"seed": 2 ** 64 - 1, "field": "chunk_index"}), function_mode="sum", candidates=20),
]


@pytest.mark.parametrize("n_spec", range(len(SPECS)))
def test_search_with_a_boost_equals_the_restatement_over_the_plain_search(host, n_spec):
    mgr, X, csr, metric = host
    q = X[5] + 0.25 * X[40]
    got, plain = check_search(mgr, q, "semantic_index", metric, SPECS[n_spec], 10)
    if n_spec in (1, 2):
        assert [h["id"] for h in got] != [h["id"] for h in plain[:10]]                    # the boost says something
    check_search(mgr, q, "semantic_index", metric, SPECS[n_spec], 7, filters="chunk_index >= 1")
    a, b = csr[0][12], csr[0][13]
    sparse_q = {"indices": csr[1][a:b].tolist(), "values": csr[2][a:b].tolist()}
    check_search(mgr, sparse_q, "sparse_index", "IP", SPECS[n_spec], 5)


def test_l2_none_sorts_ascending_and_a_document_shares_a_draw(host):
    mgr, X, _, metric = host
    q = X[5] + 0.25 * X[40]
    got, _ = check_search(mgr, q, "semantic_index", metric, BoostRanker("chunk_index >= 3", 0.5), 12)
    scores = [h["score"] for h in got]
    assert scores == sorted(scores, reverse=metric != "L2")
    spec = FunctionScore(BoostRanker(None, 1.0, {"seed": 9, "field": "doc_id"}), boost_mode="sum", normalization="minmax",
                         candidates=60)
    hits = asyncio.run(mgr.search(q, "semantic_index", 60, ranker=spec))
    plain = {h["id"]: h for h in asyncio.run(mgr.search(q, "semantic_index", 60))}
    lo, hi = min(h["score"] for h in plain.values()), max(h["score"] for h in plain.values())
    code = nat.HR_NORM_MINMAX_DIST if metric == "L2" else nat.HR_NORM_MINMAX
    draws = {}
    for h in hits:      # final - n(raw) is the draw (up to the rounding of the sum): equal within a document
        ns = D.normalise([h["raw_score"], lo, hi], code)[0]
        draws.setdefault(h["_row"] // 5, []).append(h["score"] - ns)
    assert any(len(v) > 1 for v in draws.values())
    assert all(max(v) - min(v) < 1e-12 for v in draws.values()) and len({round(v[0], 9) for v in draws.values()}) > 5
    by_id = asyncio.run(mgr.search_by_ids(["c7"], "semantic_index", 6, ranker=spec))[0]
    direct = asyncio.run(mgr.search(mgr.collections["semantic_index"].handle.get_dense_rows([7])[0], "semantic_index", 6, ranker=spec))
    assert [(h["id"], h["score"]) for h in by_id] == [(h["id"], h["score"]) for h in direct] and len(by_id) == 6


def test_search_refusals(host):
    mgr, X, _, _ = host
    q, r = X[0], BoostRanker("chunk_index >= 3", 2.0)
    searched = []
    real = mgr._search_lists_async

    async def spy(*a, **kw):
        searched.append(a)
        return await real(*a, **kw)
    mgr._search_lists_async = spy
    run = lambda **kw: asyncio.run(mgr.search(q, "semantic_index", kw.pop("top_k", 5), **kw))
    try:
        with pytest.raises(ValueError, match="group_by_field"):
            run(ranker=r, group_by_field="doc_id")
        with pytest.raises(ValueError, match="offset"):
            run(ranker=r, offset=3)
        with pytest.raises(ValueError, match="deep window"):
            run(ranker=r, top_k=nat.HR_MAX_TOPK + 1)
        with pytest.raises(ValueError, match="deep window"):
            run(ranker=FunctionScore(r, candidates=nat.HR_MAX_TOPK + 1))
        with pytest.raises(ValueError, match="not found"):
            asyncio.run(mgr.search(q, "nope", 5, ranker=r))
        for bad in ("chunk_index >>> 3", "no_such_field == 1", 'TEXT_MATCH(content, "a", minimum_should_match=16385)',
                    "chunk_index >= "):
            with pytest.raises(ValueError):
                run(ranker=FunctionScore(r, BoostRanker(bad, 2.0)))
        with pytest.raises(ValueError, match="group_by_field"):
            asyncio.run(mgr.search_by_ids(["c1"], "semantic_index", 5, ranker=r, group_by_field="doc_id"))
        with pytest.raises(ValueError):
            asyncio.run(mgr.search_by_ids(["c1"], "semantic_index", 5, ranker=BoostRanker("chunk_index >>> 3")))
        assert not searched                                                       # refused before anything is searched
        for bad in (object(), "boost", 1.5):
            with pytest.raises(ValueError, match="ranker"):
                run(ranker=bad)
        assert len(run(ranker=None)) == 5 and len(searched) == 1                # the default: the call it was
    finally:
        del mgr._search_lists_async


def test_synthetic_collection(host):
    X, csr = sq._corpus()
    mgr = MilvusIndexManager(semantic_dim=sq.DIM, sparse_dim=sq.V, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([sq._OracleShard(sq.V)])
    mgr.add_rows_synthetic(X[:sq.N], csr)
    try:
        with pytest.raises(ValueError, match="only chunk_index"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=BoostRanker('TEXT_MATCH(content, "a")', 2.0)))
        with pytest.raises(ValueError, match="only chunk_index"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=BoostRanker("token_count > 3", 2.0)))
        for field in ("timestamp", "id", "token_count"):
            with pytest.raises(ValueError, match="doc_id"):
                asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=BoostRanker(None, 2.0, {"seed": 1, "field": field})))
        spec = FunctionScore(BoostRanker("chunk_index >= 5", 3.0), BoostRanker(None, 1.0, {"seed": 4, "field": "doc_id"}), candidates=30)
        plain = asyncio.run(mgr.search(X[0], "semantic_index", 30))
        rows = [h["_row"] for h in plain]
        pos, _, fin, hit = BO.boost_rerank(rows, [h["score"] for h in plain], [[r % 10 >= 5 for r in rows], [True] * 30],
                                           [3.0, (1.0, 4, [r // 10 for r in rows])])
        got = asyncio.run(mgr.search(X[0], "semantic_index", 8, ranker=spec))
        assert [(h["_row"], h["score"]) for h in got] == [(rows[p], f) for p, f in zip(pos[:8], fin[:8])]
        assert [h["boosted_by"] for h in got] == [BO.matched_functions(m) for m in hit[:8]]
    finally:
        asyncio.run(mgr.close())


def test_torchrun_form_is_not_built(host):
    mgr, X, _, _ = host

    class Collective:
        round = None
    coll = mgr.collections["semantic_index"]
    real, coll.handle = coll.handle, Collective()
    try:
        with pytest.raises(NotImplementedError, match="torchrun"):
            asyncio.run(mgr.search(X[0], "semantic_index", 5, ranker=BoostRanker("chunk_index >= 3", 2.0)))
    finally:
        coll.handle = real


# ---- retrieve(boost=...) on the general path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("normalization", ["none", "minmax"])
def test_retrieve_with_boost_equals_the_restatement_over_the_fused_list(host, decay, normalization):
    mgr, X, csr, metric = host
    mgr.embedding_generator = dh._Gen(X, csr)
    top_k = 6
    spec = FunctionScore(BoostRanker("chunk_index >= 3", 0.5), BoostRanker('TEXT_MATCH(content, "topic2")', 3.0),
                         BoostRanker(None, 1.0, {"seed": 11, "field": "doc_id"}), function_mode="sum", normalization=normalization)
    ranker = DecayRanker("chunk_index", "linear", 4, 6, 0, 0.5) if decay else None
    params = {"metric_type": metric, "params": {"ef": 64}}
    old, RetrievalConstants.TIMEOUT_SECONDS = RetrievalConstants.TIMEOUT_SECONDS, 60.0
    try:
        for qn in (10, 30):
            initialize_caches()
            text = f"plain statement q{qn}"
            gen = mgr.embedding_generator
            sem = asyncio.run(mgr.search(gen.encode_semantic(text), "semantic_index", 2 * top_k, None, params))
            spa = asyncio.run(mgr.search(gen.encode_sparse(text), "sparse_index", 2 * top_k, None,
                                         {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}))
            ranked = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa]], (0.7, 0.3))
            row_of = {h["id"]: h["_row"] for h in sem + spa}
            rows = [row_of[i] for i, _, _ in ranked]
            pos, _, fin, _ = restate(mgr, rows, [s for _, s, _ in ranked], spec, metric, fused=True)
            want = [(ranked[p][0], f, ranked[p][1]) for p, f in zip(pos, fin)]
            assert [w[0] for w in want] != [i for i, _, _ in ranked]        # the boost reorders the fused list
            if decay:
                r2 = [row_of[w[0]] for w in want]
                pos2, _, fin2 = D.decay_rerank(r2, [w[1] for w in want], [float(r % 9) for r in r2], ranker.operands(), -1, len(r2))
                want = [(want[p][0], f, want[p][2]) for p, f in zip(pos2, fin2)]
            cfg = RetrievalConfig(top_k=top_k, boost=spec, decay=ranker, semantic_search_params=params)
            got = asyncio.run(HybridRetriever(mgr, cfg).retrieve(text, profile_hint="default"))
            assert [(h["id"], float(h["score"]).hex(), float(h["fused_score"]).hex()) for h in got] == \
                [(i, float(s).hex(), float(f).hex()) for i, s, f in want[:top_k]]
            assert all(h["retrieval_methods"] for h in got)
    finally:
        RetrievalConstants.TIMEOUT_SECONDS = old
        mgr.embedding_generator = None
