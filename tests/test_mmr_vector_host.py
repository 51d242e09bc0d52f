"""Vector MMR on the host: the restatement (advanced_rag/mmr.py) against the oracle's cosine and on hand-worked lists, the
ranker spec's refusals, and a CPU manager on stand-in handles — search(ranker=MMRRanker(...)) and retrieve() with
mmr_similarity="embedding" against the restatement, the default configuration untouched."""
import asyncio
import math
import types

import numpy as np
import pytest

import oracle
from advanced_rag import HybridRetriever, MilvusIndexManager, PipelineConfig, RetrievalConfig
from advanced_rag import _native as nat
from advanced_rag.constants import RetrievalConstants
from advanced_rag.decay import DecayRanker
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.mmr import MMRRanker, canonical_cosine, relevance, vector_mmr


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- canonical_cosine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_dtype", [np.float16, np.float32])
@pytest.mark.parametrize("dim", [1, 7, 64, 65, 768])
def test_canonical_cosine_equals_the_oracle(dim, np_dtype):
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((12, dim)).astype(np_dtype)
    X[3] = 0                      # a zero row
    X[5] = -X[4]                  # anti-parallel
    X[7] = X[6]                   # a duplicate
    C = canonical_cosine(X, X)
    assert C.dtype == np.float64 and C.shape == (12, 12)
    for j in range(12):
        want = oracle.dense_scores(X, X[j].astype(np.float32), oracle.COSINE)
        assert np.array_equal(C[:, j].astype(np.float32).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(bits(canonical_cosine(X, X[j])), bits(C[:, j]))           # the 1-D form
    assert np.array_equal(bits(C), bits(C.T))                                           # symmetric bit for bit
    assert (C[3] == 0).all() and (C[:, 3] == 0).all()
    assert C[4, 5] < 0 and abs(C[4, 5] + 1) < 1e-6 and abs(C[6, 7] - 1) < 1e-6 and abs(C[0, 0] - 1) < 1e-6


# ---- vector_mmr on hand-worked lists --------------------------------------------------------------------------------------
E = np.eye(6, dtype=np.float32)


def test_lambda_one_keeps_list_order():
    rng = np.random.default_rng(1)
    V = rng.standard_normal((9, 5)).astype(np.float32)
    scores = [0.9 - 0.1 * i for i in range(9)]
    pos, val = vector_mmr(scores, V, 1.0, 9)
    assert pos == list(range(9)) and val == scores


def test_a_planted_cluster_yields_one_member_among_the_first_five():
    rng = np.random.default_rng(2)
    V = rng.standard_normal((30, 16)).astype(np.float32)
    for j in range(1, 5):
        V[j] = V[0] + np.float32(0.01) * rng.standard_normal(16).astype(np.float32)
    scores = [0.95 - 0.01 * i for i in range(30)]
    pos, _ = vector_mmr(scores, V, 0.5, 5)
    assert pos[0] == 0 and sum(p < 5 for p in pos) == 1
    assert vector_mmr(scores, V, 1.0, 5)[0] == [0, 1, 2, 3, 4]


def test_the_running_maximum_starts_at_the_first_similarity_not_at_zero():
    V = np.stack([E[0], E[1], -E[0]])
    scores = [0.9, 0.8, 0.5]
    # second pick: the anti-parallel row has m = -1: 0.5 * 0.5 + 0.5 = 0.75 beats the orthogonal row's 0.5 * 0.8 - 0 = 0.4
    assert vector_mmr(scores, V, 0.5, 3) == ([0, 2, 1], [0.9, 0.75, 0.4])
    assert vector_mmr(scores, V, 0.5, 3, m_starts_at_zero=True)[0] == [0, 1, 2]          # the Jaccard kernel's floor


def test_equal_values_take_the_first_and_nan_is_never_picked():
    V = np.stack([E[0], E[1], E[2], E[3]])
    pos, val = vector_mmr([0.5, 0.5, 0.5, 0.5], V, 0.5, 4)
    assert pos == [0, 1, 2, 3] and val == [0.5, 0.25, 0.25, 0.25]
    pos, _ = vector_mmr([0.9, math.nan, 0.7, 0.6], V, 0.5, 4)
    assert pos == [0, 2, 3]
    assert vector_mmr([math.nan, math.nan], V[:2], 0.5, 2) == ([], [])
    assert vector_mmr([-2e9, 1.0], V[:2], 0.5, 2) == ([1], [1.0])                        # only values above -1e9 qualify


def test_empty_and_short_lists():
    assert vector_mmr([], np.zeros((0, 4), np.float32), 0.5, 3) == ([], [])
    pos, val = vector_mmr([0.3, 0.2], E[:2], 0.25, 10)
    assert pos == [0, 1] and val == [0.3, 0.25 * 0.2 - 0.75 * 0.0]


def test_normalisations_are_the_decay_rankers():
    from advanced_rag.decay import normalise
    s = [float(np.float32(x)) for x in (3.5, 1.25, -0.5, 1.25)]
    for code in (nat.HR_NORM_NONE, nat.HR_NORM_COSINE, nat.HR_NORM_ATAN, nat.HR_NORM_ATAN_DIST, nat.HR_NORM_MINMAX,
                 nat.HR_NORM_MINMAX_DIST):
        assert np.array_equal(bits(relevance(s, code)), bits(normalise(s, code)))
    r = relevance([1.0, math.nan, 3.0], nat.HR_NORM_MINMAX)                              # a NaN never becomes lo or hi
    assert r[0] == 0.0 and r[2] == 1.0 and math.isnan(r[1])


# ---- MMRRanker ----------------------------------------------------------------------------------------------------------------
def test_ranker_validation():
    r = MMRRanker()
    assert (r.lambda_mult, r.candidates, r.normalization) == (0.5, None, "none")
    assert r.window(20) == 20 and MMRRanker(candidates=80).window(20) == 80 and MMRRanker(candidates=5).window(20) == 20
    for bad in (-0.1, 1.1, math.nan, math.inf, "0.5", True, None):
        with pytest.raises(ValueError):
            MMRRanker(lambda_mult=bad)
    for bad in (0, -3, 2.5, True, "3"):
        with pytest.raises(ValueError):
            MMRRanker(candidates=bad)
    for bad in ("zscore", None, 3):
        with pytest.raises(ValueError):
            MMRRanker(normalization=bad)
    assert MMRRanker(lambda_mult=0).lambda_mult == 0 and MMRRanker(lambda_mult=1).lambda_mult == 1
    for norm in ("none", "activation", "minmax"):
        for metric in ("COSINE", "IP", "L2"):
            if norm == "none" and metric == "L2":
                with pytest.raises(ValueError):
                    MMRRanker(normalization=norm).norm_code(metric)
            elif norm == "none":
                assert MMRRanker(normalization=norm).norm_code(metric) == nat.HR_NORM_NONE
            else:          # exactly DecayRanker's mapping
                assert MMRRanker(normalization=norm).norm_code(metric) == \
                    DecayRanker("chunk_index", origin=0, scale=1.0, normalization=norm).norm_code(metric)


def test_config_validation():
    assert RetrievalConfig().mmr_similarity == "tokens" and PipelineConfig().mmr_similarity == "tokens"
    assert RetrievalConfig(mmr_similarity="embedding").mmr_similarity == "embedding"
    for bad in ("cosine", None, "Embedding"):
        with pytest.raises(ValueError):
            RetrievalConfig(mmr_similarity=bad)
    mgr = types.SimpleNamespace()
    profiles = HybridRetriever(mgr, RetrievalConfig(mmr_similarity="embedding")).profiles
    assert all(p.mmr_similarity == "embedding" for p in profiles.values())               # the profiles carry it


# ---- a CPU manager ------------------------------------------------------------------------------------------------------------
class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given."""

    def __init__(self, metric=oracle.COSINE):
        self.X = None
        self.device, self.sparse_dim, self.metric = 0, 0, metric

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = 0
    device_bytes = property(lambda self: 0 if self.X is None else self.X.nbytes)
    dim = property(lambda self: self.X.shape[1])

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, self.metric, mask)

    def get_dense_rows(self, rows):
        return self.X[np.asarray(rows, dtype=np.int64)].astype(np.float32)

    def finalize(self):
        pass

    def close(self):
        pass


MN, DIM, K = 203, 12, 8


class _Gen:
    def __init__(self, Q):
        self.Q = Q

    def encode_semantic(self, text):
        return self.Q[int(text.rsplit("q", 1)[1])]

    def encode_sparse(self, text):
        return {"indices": [], "values": []}

    def encode_domain(self, text, domain=None):
        return np.zeros(DIM, np.float32)


@pytest.fixture(scope="module")
def cpu():
    rng = np.random.default_rng(23)
    X = rng.standard_normal((MN, DIM)).astype(np.float32)
    for c0 in (0, 100):                       # two clusters of near-copies, each spread over both stand-in shards' rows
        for j in range(1, 6):
            X[c0 + 17 * j] = X[c0] + np.float32(0.02) * rng.standard_normal(DIM).astype(np.float32)
    Q = np.stack([X[0] + np.float32(0.1) * rng.standard_normal(DIM).astype(np.float32),
                  X[100] + np.float32(0.1) * rng.standard_normal(DIM).astype(np.float32),
                  rng.standard_normal(DIM).astype(np.float32)])
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard() for _ in range(2)])
    for lo in range(0, MN, 80):
        hi = min(MN, lo + 80)
        mgr.add_rows(X[lo:hi], None, ids=[f"c{r}" for r in range(lo, hi)],
                     contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(lo, hi)],
                     doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 10 for r in range(lo, hi)])
    mgr.embedding_generator = _Gen(Q)
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield mgr, X, Q
    RetrievalConstants.TIMEOUT_SECONDS = old
    asyncio.run(mgr.close())


def row_of(hit):
    return int(hit["id"][1:])


@pytest.mark.parametrize("ranker", [MMRRanker(), MMRRanker(0.3, candidates=40), MMRRanker(0.7, 25, "activation"),
                                    MMRRanker(1.0, 30, "minmax"), MMRRanker(0.0, 20)], ids=str)
def test_cpu_search_with_a_ranker_equals_the_restatement(cpu, ranker):
    mgr, X, Q = cpu
    before = mgr.stats["mmr_host_selects"]
    moved = 0
    for qi, expr in ((0, None), (1, None), (2, None), (0, "chunk_index != 7")):
        W = ranker.window(K)
        plain = asyncio.run(mgr.search(Q[qi], "semantic_index", W, filters=expr))
        assert len(plain) == W and all("mmr_value" not in h for h in plain)
        pos, val = vector_mmr([h["score"] for h in plain], X[[row_of(h) for h in plain]], ranker.lambda_mult, K,
                              ranker.norm_code("COSINE"))
        got = asyncio.run(mgr.search(Q[qi], "semantic_index", K, filters=expr, ranker=ranker))
        assert [h["id"] for h in got] == [plain[p]["id"] for p in pos]                   # pick order
        assert [float(h["mmr_value"]).hex() for h in got] == [float(v).hex() for v in val]
        assert [h["score"] for h in got] == [plain[p]["score"] for p in pos]             # the search's own score stays
        moved += pos != list(range(K))
    assert mgr.stats["mmr_host_selects"] - before == 4
    assert (moved == 0) if ranker.lambda_mult == 1.0 else (moved >= 3)                   # it diversifies, it is no identity


def test_cpu_search_by_ids_passes_the_ranker_through(cpu):
    mgr, X, Q = cpu
    ranker = MMRRanker(0.4, candidates=30)
    got = asyncio.run(mgr.search_by_ids(["c100", "c3"], "semantic_index", K, ranker=ranker))
    for entity, hits in zip((100, 3), got):
        want = asyncio.run(mgr.search(X[entity], "semantic_index", K, ranker=ranker))
        assert [(h["id"], h["mmr_value"]) for h in hits] == [(h["id"], h["mmr_value"]) for h in want] and len(hits) == K


def test_cpu_refusals_come_before_any_search(cpu):
    mgr, X, Q = cpu
    searched = []
    real = mgr._search_blocking
    mgr._search_blocking = lambda *a, **k: searched.append(a) or real(*a, **k)
    try:
        r = MMRRanker()
        for kw in (dict(ranker=object()), dict(ranker="mmr"), dict(ranker=r, group_by_field="doc_id"), dict(ranker=r, offset=1),
                   dict(ranker=MMRRanker(candidates=nat.HR_MAX_TOPK + 1)), dict(ranker=r, top_k=nat.HR_MAX_TOPK + 1)):
            with pytest.raises(ValueError):
                asyncio.run(mgr.search(Q[0], "semantic_index", **{"top_k": K, **kw}))
        with pytest.raises(ValueError):
            asyncio.run(mgr.search(Q[0], "nowhere", K, ranker=r))
        with pytest.raises(ValueError):
            asyncio.run(mgr.search_by_ids(["c1"], "semantic_index", K, ranker=r, group_by_field="doc_id"))
        coll = mgr.collections["semantic_index"]
        kind, metric, handle = coll.kind, coll.metric, coll.handle
        try:
            coll.kind = "sparse"
            with pytest.raises(ValueError, match="dense embeddings"):
                asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=r))
            coll.kind, coll.metric = kind, "L2"
            with pytest.raises(ValueError, match="L2"):
                asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=r))
            coll.metric = metric
            coll.handle = types.SimpleNamespace(round=None)                              # the torchrun form's mark
            with pytest.raises(NotImplementedError):
                asyncio.run(mgr.search(Q[0], "semantic_index", K, ranker=r))
        finally:
            coll.kind, coll.metric, coll.handle = kind, metric, handle
        assert searched == []
    finally:
        mgr._search_blocking = real


def test_cpu_retrieve_with_embedding_similarity_equals_the_restatement(cpu):
    mgr, X, Q = cpu
    lam = 0.5
    plain = HybridRetriever(mgr, RetrievalConfig(top_k=K, enable_mmr=False))
    emb = HybridRetriever(mgr, RetrievalConfig(top_k=K, enable_mmr=True, mmr_lambda=lam, mmr_similarity="embedding"))
    tok = HybridRetriever(mgr, RetrievalConfig(top_k=K, enable_mmr=True, mmr_lambda=lam))
    moved = 0
    for qi in range(3):
        initialize_caches()                          # the embedding cache goes by the text: other modules use the same

        async def fused_list():
            hits = await plain._search_semantic(Q[qi], None)
            return await plain._fuse_results_async(hits, [], [])
        fused = asyncio.run(fused_list())                                                # the general path's fused list, whole
        assert len(fused) == 2 * K
        pos, _ = vector_mmr([h["score"] for h in fused], X[[row_of(h) for h in fused]], lam, K)
        before = dict(mgr.stats)
        got = asyncio.run(emb.retrieve(f"plain statement q{qi}", profile_hint="default"))
        assert [h["id"] for h in got] == [fused[p]["id"] for p in pos] and len(got) == K
        assert [h["score"] for h in got] == [fused[p]["score"] for p in pos]
        assert all("_row" not in h for h in got)
        assert mgr.stats["mmr_host_selects"] == before["mmr_host_selects"] + 1
        moved += pos != list(range(K))
        # the default similarity: today's token-Jaccard loop, and no vector selection is counted
        before = dict(mgr.stats)
        want = HybridRetriever._mmr_diversify([dict(h) for h in fused], K, lam)
        got = asyncio.run(tok.retrieve(f"plain statement q{qi}", profile_hint="default"))
        assert [(h["id"], h["score"]) for h in got] == [(h["id"], h["score"]) for h in want]
        assert mgr.stats == before
        got = asyncio.run(plain.retrieve(f"plain statement q{qi}", profile_hint="default"))
        assert [h["id"] for h in got] == [h["id"] for h in fused[:K]] and mgr.stats == before
    assert moved >= 2
    assert emb.profiles["troubleshooting"].mmr_similarity == "embedding"


def test_hits_without_a_row_number_have_the_zero_vector(cpu):
    mgr, X, Q = cpu
    rows, scores = [5, None, 22, 39, 500000], [0.9, 0.8, 0.7, 0.6, 0.5]
    V = np.zeros((5, DIM), dtype=np.float32)
    V[[0, 2, 3]] = X[[5, 22, 39]]
    want = vector_mmr(scores, V, 0.5, 4)[0]
    assert mgr.mmr_select_lists(rows, scores, 0.5, 4) == want
    assert asyncio.run(mgr.mmr_select_lists_async(rows, scores, 0.5, 4)) == want
    assert mgr.mmr_select_lists([], [], 0.5, 4) == []
    with pytest.raises(ValueError):
        mgr.mmr_select_lists([1, 2], [0.5], 0.5, 4)


def test_a_manager_without_vectors_gives_every_hit_the_zero_vector():
    retr = HybridRetriever(types.SimpleNamespace(), RetrievalConfig(top_k=3, enable_mmr=True, mmr_similarity="embedding"))
    fused = [{"id": f"x{i}", "score": s} for i, s in enumerate((0.5, 0.4, 0.4, 0.1))]
    assert [h["id"] for h in retr._mmr_embedding(fused, [None] * 4)] == ["x0", "x1", "x2"]
    assert [h["id"] for h in asyncio.run(retr._mmr_embedding_async(fused, [None] * 4))] == ["x0", "x1", "x2"]
