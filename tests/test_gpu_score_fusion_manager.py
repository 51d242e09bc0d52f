"""Weighted score fusion end to end: retrieve() with RetrievalConfig(fusion="weighted") through the one-round path, the
general path (front off) and two shards, against the restatement of tests/score_fusion_ref.py applied to the yardsticks' two
2 * top_k lists; concurrent weighted and RRF requests; MMR on the device over the weighted fused list."""
import asyncio

import numpy as np
import pytest

import oracle
import range_yardstick as ry
import score_fusion_ref as R
from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.retrieval import norm_code, rrf_rank_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V, TOP_K, NQ = 3001, 64, 512, 10, 6
CODE = {"COSINE": ry.COSINE, "L2": ry.L2}
DROP = 0.2          # RetrievalConfig's default drop_ratio_search


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


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(31)
    X = rng.standard_normal((N, D)).astype(np.float32)
    nnz = 6
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(N)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((N, nnz))) * 3 + 0.1).astype(np.float32)       # BM25-sized: sums well beyond 10
    csr = (np.arange(N + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"topic{r % 5} word{r % 7} text{r % 3} common" for r in range(N)],
                   doc_id=[f"doc{r // 10}" for r in range(N)], chunk_index=[r % 7 for r in range(N)])
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 60, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(60)) + 0.5).astype(np.float32))
          for _ in range(NQ)]
    return X, csr, payload, Q, SQ


@pytest.fixture(scope="module")
def yardstick_lists(corpus):
    """(metric, k) -> per query ((dense rows, fp32 scores), (sparse rows, fp32 scores)): computed once, never changed."""
    X, csr, _, Q, SQ = corpus
    Xs = X.astype(np.float16)                       # what the shard stores
    cache = {}

    def get(metric, k):
        if (metric, k) not in cache:
            di, ds = ry.range_search(Xs, Q, k, CODE[metric], None, None)
            si, ss = oracle.sparse_search(csr[0], csr[1], csr[2], SQ, k, DROP)
            assert (di >= 0).all() and (si >= 0).all()
            cache[metric, k] = [((di[q], ds[q]), (si[q], ss[q])) for q in range(NQ)]
        return cache[metric, k]
    return get


def manager(corpus, metric="COSINE", **kw):
    X, csr, payload, Q, SQ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, semantic_metric=metric, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr.finalize()
    mgr.embedding_generator = KeyedGen(Q, SQ)
    return mgr


def want_fused(lists, metric, normalization, top_k, weights=(0.7, 0.3)):
    norms = (norm_code(metric, normalization), norm_code("IP", normalization))
    fi, fs, fm = R.fuse(lists, weights, norms)
    return [f"c{int(r)}" for r in fi[:top_k]], [float(s).hex() for s in fs[:top_k]], fm[:top_k].tolist()


def got_fused(hits):
    mask = lambda h: sum(1 << ("semantic", "sparse", "domain").index(m) for m in h["retrieval_methods"])
    return [h["id"] for h in hits], [float(h["score"]).hex() for h in hits], [mask(h) for h in hits]


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("normalization", ["activation", "minmax"])
def test_retrieve_weighted_three_ways(gpu, long_timeout, corpus, yardstick_lists, normalization, metric):
    lists = yardstick_lists(metric, 2 * TOP_K)
    want = [want_fused(lists[q], metric, normalization, TOP_K) for q in range(NQ)]
    assert len({tuple(w[0]) for w in want}) == NQ and all(len(w[0]) == TOP_K for w in want)
    assert len({m for w in want for m in w[2]}) >= 2          # hits of one list and hits of both reach the top
    rrf = [[f"c{int(r)}" for r, _, _ in rrf_rank_lists([lists[q][0][0], lists[q][1][0]], (0.7, 0.3))][:TOP_K] for q in range(NQ)]
    if normalization == "minmax":      # ("activation" saturates on these BM25-sized sparse scores: the dense list leads, as in RRF)
        assert any(w[0] != r for w, r in zip(want, rrf))      # the scores say something the ranks do not
    ways = {"one_round": {}, "general": {"coalesce": False}, "two_shards": {"devices": [0, 0]}}
    for name, kw in ways.items():
        mgr = manager(corpus, metric, **kw)
        try:
            initialize_caches()
            cfg = RetrievalConfig(top_k=TOP_K, fusion="weighted", score_normalization=normalization,
                                  semantic_search_params={"metric_type": metric, "params": {"ef": 64}})
            retr = HybridRetriever(mgr, cfg)
            for q in range(NQ):
                hits = asyncio.run(retr.retrieve(f"plain statement q{q}", profile_hint="default"))
                assert got_fused(hits) == want[q], (name, q)
                assert all(h["metadata"]["retrieval_profile"] == "default" for h in hits)
            if name == "one_round":
                st = mgr._front.stats
                assert st["hybrid_launches"] == NQ and st["score_fuse_launches"] == 0 and st["fuse_launches"] == 0
            elif name == "general":
                assert mgr._front is None
        finally:
            asyncio.run(mgr.close())


def test_concurrent_weighted_and_rrf_requests_do_not_share_a_launch(gpu, long_timeout, corpus, yardstick_lists):
    lists = yardstick_lists("COSINE", 2 * TOP_K)
    mgr = manager(corpus)
    try:
        initialize_caches()
        weighted = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, fusion="weighted"))
        minmax = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, fusion="weighted", score_normalization="minmax"))
        plain = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K))

        async def burst():
            return await asyncio.gather(*([r.retrieve(f"plain statement q{q}", profile_hint="default")
                                           for q in range(NQ) for r in (weighted, plain, minmax)]))

        asyncio.run(weighted.retrieve("plain statement q0", profile_hint="default"))      # (the worker and the buffers exist)
        before = dict(mgr._front.stats)
        out = asyncio.run(burst())
        st = mgr._front.stats
        for q in range(NQ):
            assert got_fused(out[3 * q]) == want_fused(lists[q], "COSINE", "activation", TOP_K), q
            assert got_fused(out[3 * q + 2]) == want_fused(lists[q], "COSINE", "minmax", TOP_K), q
            want = rrf_rank_lists([lists[q][0][0], lists[q][1][0]], (0.7, 0.3))[:TOP_K]
            assert [h["id"] for h in out[3 * q + 1]] == [f"c{int(r)}" for r, _, _ in want], q
            assert [float(h["score"]).hex() for h in out[3 * q + 1]] == [float(s).hex() for _, s, _ in want], q
        # three keys (RRF, weighted by activation, weighted by min-max): at least three launches, however the burst arrives
        assert 3 <= st["hybrid_launches"] - before["hybrid_launches"] <= 3 * NQ

        # the fusion entry points of the general path: a kind of their own, so one launch each at the least
        rows = [[int(r) for r in lists[q][0][0]] for q in range(NQ)], [[int(r) for r in lists[q][1][0]] for q in range(NQ)]
        ids = [[f"c{r}" for r in rows[0][q]] for q in range(NQ)], [[f"c{r}" for r in rows[1][q]] for q in range(NQ)]
        scs = [lists[q][0][1].tolist() for q in range(NQ)], [lists[q][1][1].tolist() for q in range(NQ)]

        async def fusions():
            calls = []
            for q in range(NQ):
                calls.append(mgr.fuse_score_lists_async([rows[0][q], rows[1][q]], [ids[0][q], ids[1][q]],
                                                        [scs[0][q], scs[1][q]], [0.7 - 0.1 * q, 0.3, 0.2], [0, 1, 0]))
                calls.append(mgr.fuse_rank_lists_async([rows[0][q], rows[1][q]], [ids[0][q], ids[1][q]], [0.7, 0.3, 0.2], 60))
            return await asyncio.gather(*calls)

        before = dict(st)
        out = asyncio.run(fusions())
        for q in range(NQ):
            fi, fs, fm = R.fuse(lists[q], (0.7 - 0.1 * q, 0.3), (0, 1))       # per-request weights share the launch
            assert [(i, float(s).hex()) for i, s, _ in out[2 * q]] == [(f"c{int(r)}", float(s).hex()) for r, s in zip(fi, fs)]
            assert [sum(1 << b for b in m) for _, _, m in out[2 * q]] == fm.tolist()
            want = rrf_rank_lists([ids[0][q], ids[1][q]], (0.7, 0.3, 0.2))
            assert [(i, float(s).hex()) for i, s, _ in out[2 * q + 1]] == [(i, float(s).hex()) for i, s, _ in want]
        assert 1 <= st["score_fuse_launches"] - before["score_fuse_launches"] <= NQ
        assert 1 <= st["fuse_launches"] - before["fuse_launches"] <= NQ
        # the synchronous form (what a sharded manager uses): the host entry point, the same answer
        fi, fs, _ = R.fuse(lists[1], (0.5, 0.5), (3, 3))
        got = mgr.fuse_score_lists([rows[0][1], rows[1][1]], [ids[0][1], ids[1][1]], [scs[0][1], scs[1][1]], [0.5, 0.5], [3, 3])
        assert [(i, float(s).hex()) for i, s, _ in got] == [(f"c{int(r)}", float(s).hex()) for r, s in zip(fi, fs)]
    finally:
        asyncio.run(mgr.close())


def test_weighted_request_with_mmr_on_the_device_equals_the_host_mmr(gpu, long_timeout, corpus, yardstick_lists):
    """Profile "troubleshooting": top_k 30, MMR with lambda 0.5 over the whole weighted fused list of two 60-entry lists."""
    _, _, payload, _, _ = corpus
    top_k = 30
    lists = yardstick_lists("COSINE", 2 * top_k)
    answers = {}
    for on_device in (True, False):
        mgr = manager(corpus, mmr_on_device=on_device)
        try:
            initialize_caches()
            retr = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, fusion="weighted", score_normalization="minmax"))
            answers[on_device] = [asyncio.run(retr.retrieve(f"plain statement q{q}", profile_hint="troubleshooting"))
                                  for q in range(3)]
            assert (retr.config.enable_mmr, retr.config.top_k, retr.config.fusion) == (True, top_k, "weighted")
            assert mgr._front.stats["mmr_launches"] == (3 if on_device else 0)
            assert mgr._front.stats["hybrid_launches"] == (3 if on_device else 0)
        finally:
            asyncio.run(mgr.close())
    for q in range(3):
        fi, fs, _ = R.fuse(lists[q], (0.7, 0.3), (3, 3))
        ranked = [{"id": f"c{int(r)}", "score": float(s), "content": payload["contents"][int(r)]} for r, s in zip(fi, fs)]
        want = HybridRetriever._mmr_diversify(ranked, top_k, 0.5)
        assert [h["id"] for h in want] != [h["id"] for h in ranked[:top_k]]            # MMR changes the order here
        for on_device in (True, False):
            got = answers[on_device][q]
            assert [(h["id"], float(h["score"]).hex()) for h in got] == [(h["id"], float(h["score"]).hex()) for h in want]
