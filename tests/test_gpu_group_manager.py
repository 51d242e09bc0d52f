"""Grouping search end to end: MilvusIndexManager.search(..., group_by_field=F) against the ten-line restatement over the
manager's own ungrouped ranking (which the other suites hold to the oracle) — ids and scores bit for bit — through the
continuation loop, the window clamp, the batching front, a synthetic collection, two shards, and retrieve()."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.batching import SearchCoalescer
from advanced_rag.constants import RetrievalConstants
from advanced_rag.embedding_cache import initialize_caches
from advanced_rag.retrieval import rrf_rank_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V = 240, 32, 64


def first_k_distinct(ranked_rows, keys, k):
    """The first k rows of a ranking whose key differs from the key of every row before them."""
    seen, out = set(), []
    for r in ranked_rows:
        key = int(keys[r])
        if key not in seen:
            seen.add(key)
            out.append(int(r))
            if len(out) == k:
                break
    return out


@pytest.fixture()
def long_timeout():
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


@pytest.fixture(scope="module")
def corpus():
    """240 rows: document "big" (120 chunks) is nearest the query under COSINE, IP and L2 and heaviest under the sparse
    query; the other 120 rows are documents of 1 to 10 chunks.  Values come from a handful of levels: many tied scores.
    Rows are shuffled, so the big document's chunks lie all over the row space."""
    rng = np.random.default_rng(17)
    X = np.zeros((N, D), np.float32)
    X[:120, 0] = 2.0
    X[:120, 1] = rng.integers(0, 3, 120) * 0.25
    X[120:, 0] = rng.integers(0, 4, 120) * 0.5
    X[120:, 2] = 1.0
    docs, d = ["big"] * 120, 0
    while len(docs) < N:
        docs += [f"doc{d}"] * int(rng.integers(1, 11))
        d += 1
    docs = docs[:N]
    best = [1 if (r < 120 and X[r, 1] == 0) else 0 for r in range(N)]        # the big document's best chunks
    val = np.concatenate([rng.integers(3, 5, (120, 4)), rng.integers(1, 3, (120, 4))]).astype(np.float32)
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, (N, 4))).astype(np.int32)     # ascending within a row
    perm = rng.permutation(N)
    X, val, idx = X[perm], val[perm], idx[perm]
    payload = dict(ids=[f"c{r}" for r in range(N)], contents=[f"text {r}" for r in range(N)],
                   doc_id=[docs[o] for o in perm], chunk_index=[r % 7 for r in range(N)],
                   token_count=[best[o] for o in perm], timestamp=[f"2024-01-0{1 + r % 3}T00:00:00" for r in range(N)])
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    q = np.zeros(D, np.float32)
    q[0] = 2.0
    sq = {"indices": list(range(V)), "values": [1.0] * V}
    return X, csr, payload, q, sq


def _manager(corpus, metric="COSINE", **kw):
    X, csr, payload, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, semantic_metric=metric, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr.finalize()
    return mgr


def _lists(hits):
    return [h["_row"] for h in hits], [h["score"] for h in hits], [h["id"] for h in hits]


def _check(mgr, query, coll, field, top_k, expr=None):
    """search(group_by_field=field) == first_k_distinct of the same manager's ungrouped ranking.  -> the grouped hits"""
    rows, scores, ids = _lists(asyncio.run(mgr.search(query, coll, top_k=256, filters=expr)))
    assert 0 < len(rows) < 256                                    # the whole ranking of the qualifying rows
    keys = mgr._cols.group_keys(field)
    want = first_k_distinct(rows, keys, top_k)
    at = [rows.index(r) for r in want]
    got = asyncio.run(mgr.search(query, coll, top_k=top_k, filters=expr, group_by_field=field))
    assert _lists(got) == (want, [scores[i] for i in at], [ids[i] for i in at]), (coll, field, top_k, expr)
    assert len(got) == min(top_k, len(set(keys[rows].tolist())))
    shown = [h["id"] if field == "id" else h["metadata"][field] for h in got if field != "token_count"]
    assert len(set(shown)) == len(shown)
    return got


class _TextGen:
    """Embeddings of the chunks appended by index_chunks, keyed by their text."""

    def __init__(self, dense, sparse):
        self.dense, self.sparse = dense, sparse

    def encode_semantic_batch(self, texts):
        return [self.dense[t] for t in texts]

    def encode_semantic(self, text):
        return self.dense[text]

    def encode_sparse(self, text):
        return self.sparse[text]


def _chunk(text, chunk_id, doc_id, chunk_index):
    meta = SimpleNamespace(chunk_id=chunk_id, doc_id=doc_id, chunk_index=chunk_index, token_count=0, entropy=0.0,
                           redundancy=0.0, domain_density=0.0, timestamp="2024-02-01T00:00:00")
    meta.to_dict = lambda: {"doc_id": doc_id}
    return SimpleNamespace(text=text, metadata=meta)


@pytest.mark.parametrize("metric", ["COSINE", "IP", "L2"])
def test_grouped_search_equals_the_restatement_through_the_collection_life(gpu, corpus, metric):
    X, csr, payload, q, sq = corpus
    mgr = _manager(corpus, metric)
    try:
        def everything(first="big"):
            for coll, query in (("semantic_index", q), ("sparse_index", sq)):
                got = _check(mgr, query, coll, "doc_id", 5)       # window 20: the big document's 120 chunks fill it
                assert first is None or got[0]["metadata"]["doc_id"] == first
                _check(mgr, query, coll, "chunk_index", 5)
                assert len(_check(mgr, query, coll, "doc_id", 60)) < 60            # fewer documents than top_k: a short list
                _check(mgr, query, coll, "doc_id", 5, 'chunk_index >= 2 and doc_id != "doc3"')
                _check(mgr, query, coll, "timestamp", 3)
                _check(mgr, query, coll, "token_count", 2)

        before = mgr.stats["group_continuations"]
        everything()
        assert mgr.stats["group_continuations"] >= before + 5      # (120 rows of one document / windows of 20) per search
        assert mgr._front.stats["group_launches"] > 0 and mgr._front.stats["redone_grouped"] > 0
        # the big document's best chunks are deleted: other chunks of it take their place
        asyncio.run(mgr.delete_by_filter("semantic_index", 'doc_id == "big" and token_count == 1'))
        everything()
        stats = mgr.compact()
        assert stats["rows_after"] < stats["rows_before"] == N and mgr._dev_groups is None     # the mirror went with the masks
        everything()
        # twelve more chunks: six of a new document that ties with the best rows, six more of the big one
        texts = [f"late chunk {j}" for j in range(12)]
        dense = {t: np.asarray([2.0, 0.0 if j < 6 else 0.25] + [0.0] * (D - 2), np.float32) for j, t in enumerate(texts)}
        sparse = {t: {"indices": [0, 5, 10, 15], "values": [4.0, 4.0, 4.0, 3.0 + j % 2]} for j, t in enumerate(texts)}
        mgr.embedding_generator = _TextGen(dense, sparse)
        initialize_caches()
        uploaded = mgr._dev_groups.stats["uploaded_bytes"]
        n_before = mgr.num_rows
        summary = asyncio.run(mgr.index_chunks([_chunk(t, f"late{j}", "late" if j < 6 else "big", j) for j, t in enumerate(texts)]))
        assert summary["indexed_semantic"] == summary["indexed_sparse"] == 12 and not summary["errors"]
        got = _check(mgr, q, "semantic_index", "doc_id", 5)
        assert "late" in [h["metadata"]["doc_id"] for h in got]
        # the mirror grew in place: only the new rows of the one field went up
        assert mgr._dev_groups.stats["uploaded_bytes"] == uploaded + 8 * 12 and mgr.num_rows == n_before + 12
        everything(first=None)        # (the new document now ties with or beats the big one)
    finally:
        asyncio.run(mgr.close())


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_window_clamp_against_the_numpy_ranking(gpu, metric):
    """3 000 rows of small integers: every score is exact in the fp16 store, in fp64 and in fp32, so numpy's ranking with
    the row tie-break is the truth.  One document holds the 700 best rows; top_k = 100, so the window is clamped to 256."""
    n = 3000
    rng = np.random.default_rng(29)
    big = np.zeros(n, bool)
    big[rng.permutation(n)[:700]] = True
    X = rng.integers(-1, 2, (n, D)).astype(np.float32)
    X[big, 1:] = 0
    X[:, 0] = np.where(big, rng.integers(8, 11, n), rng.integers(0, 8, n))
    q = np.zeros(D, np.float32)
    q[0] = 2.0 if metric == "IP" else 10.0
    docs = np.where(big, -1, rng.integers(0, 230, n))
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, enable_domain=False, semantic_metric=metric)
    mgr.collections.pop("sparse_index", None)
    try:
        mgr.add_rows(X, None, ids=[f"c{r}" for r in range(n)], doc_id=[f"d{d}" for d in docs.tolist()])
        mgr.finalize()
        X64 = X.astype(np.float64)
        if metric == "IP":
            score = X64 @ q.astype(np.float64)
            order = np.lexsort((np.arange(n), -score))
        else:
            score = ((X64 - q.astype(np.float64)) ** 2).sum(axis=1)
            order = np.lexsort((np.arange(n), score))
        assert set(order[:700].tolist()) == set(np.nonzero(big)[0].tolist())
        want = first_k_distinct(order.tolist(), docs + 1, 100)
        assert len(want) == 100 and MilvusIndexManager.group_window(100) == 256
        before = mgr.stats["group_continuations"]
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=100, group_by_field="doc_id"))
        assert [h["_row"] for h in got] == want
        assert [h["score"] for h in got] == [float(np.float32(score[r])) for r in want]
        assert mgr.stats["group_continuations"] - before >= 1
    finally:
        asyncio.run(mgr.close())


def test_grouped_searches_share_one_launch_of_the_front(gpu, corpus):
    X, csr, payload, q, sq = corpus
    rng = np.random.default_rng(3)
    queries = [q] + [np.abs(rng.standard_normal(D)).astype(np.float32) for _ in range(7)]
    plain_q = [queries[1], queries[2]]
    mgr, fresh = _manager(corpus), _manager(corpus)
    try:
        mgr._front = SearchCoalescer(mgr, window_s=5e-3)          # a round waits 5 ms for its next request: one tick fits
        want_plain = [asyncio.run(fresh.search(p, "semantic_index", top_k=7)) for p in plain_q]
        assert fresh._dev_groups is None and fresh._front.stats["group_launches"] == 0
        blocking = [mgr._search_blocking(p, "semantic_index", 5, None, None, "doc_id") for p in queries]

        async def burst():
            return await asyncio.gather(*[mgr.search(p, "semantic_index", top_k=5, group_by_field="doc_id") for p in queries],
                                        *[mgr.search(p, "semantic_index", top_k=7) for p in plain_q])

        st = mgr._front.stats
        before = dict(st)
        together = asyncio.run(burst())
        assert together[:8] == blocking and all(len(t) == 5 for t in together[:8])
        assert together[8:] == want_plain
        assert st["group_launches"] - before["group_launches"] == 1          # one grouped batch, not eight
        assert st["dense_launches"] - before["dense_launches"] == 2          # ... beside one ungrouped batch: no shared launch
        assert st["rounds"] - before["rounds"] == 1 and st["max_batch_seen"] == 8
        assert st["redone_grouped"] - before["redone_grouped"] >= 1          # the query at the big document needed the loop
        keys = mgr._cols.group_keys("doc_id")
        for p, got in zip(queries, together[:8]):
            rows = [h["_row"] for h in asyncio.run(mgr.search(p, "semantic_index", top_k=256))]
            assert [h["_row"] for h in got] == first_k_distinct(rows, keys, 5)
    finally:
        asyncio.run(mgr.close())
        asyncio.run(fresh.close())


def test_synthetic_collection_groups_on_its_generated_keys(gpu):
    rng = np.random.default_rng(8)
    n = 500
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[100:140] += 3.0                                             # four "documents" (row // 10) crowd the top of the ranking
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, enable_domain=False)
    mgr.collections.pop("sparse_index", None)
    try:
        mgr.add_rows_synthetic(X)
        mgr.finalize()
        q = np.full(D, 1.0, np.float32)
        rows = [h["_row"] for h in asyncio.run(mgr.search(q, "semantic_index", top_k=256))]
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=12, group_by_field="doc_id"))
        assert [h["_row"] for h in got] == first_k_distinct(rows, np.arange(n) // 10, 12)
        assert len({h["_row"] // 10 for h in got}) == 12 == len({h["metadata"]["doc_id"] for h in got})
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=12, group_by_field="chunk_index"))
        assert [h["_row"] for h in got] == first_k_distinct(rows, np.arange(n) % 10, 12) and len(got) == 10
        with pytest.raises(ValueError, match="bulk-ingested without payload columns"):
            asyncio.run(mgr.search(q, "semantic_index", top_k=12, group_by_field="timestamp"))
    finally:
        asyncio.run(mgr.close())


def test_two_shards_give_the_single_shard_lists(gpu, corpus):
    X, csr, payload, q, sq = corpus
    one, two = _manager(corpus), _manager(corpus, devices=[0, 0])
    try:
        assert two._main.n_shards == 2 and two._coalescer(two.collections["semantic_index"]) is None
        for coll, query in (("semantic_index", q), ("sparse_index", sq)):
            for field, top_k, expr in (("doc_id", 5, None), ("chunk_index", 5, None), ("doc_id", 60, None),
                                       ("doc_id", 5, "chunk_index >= 2")):
                a = _check(one, query, coll, field, top_k, expr)
                b = _check(two, query, coll, field, top_k, expr)
                assert a == b, (coll, field, top_k, expr)
        assert two.stats["group_continuations"] >= 5 and two._dev_groups is None      # the host loop: no mirror
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


def test_device_loop_and_host_loop_answer_and_count_alike(gpu, corpus):
    """The one grouped loop on its two backends, for group_size 1 and 3: a manager on one shard without the front (every
    request takes the blocking loop with the masks in HBM) and one with the same rows on two shards of the same device
    (host masks) — equal lists, equal to the restatement over the ungrouped ranking, and equal counters request by request."""
    X, csr, payload, q, sq = corpus
    counters = ("group_searches", "group_rounds", "group_continuations", "group_fill_searches", "group_fill_rounds")
    one = _manager(corpus, coalesce=False, group_members=True)
    two = _manager(corpus, devices=[0, 0], group_members=True)

    def restated(rows, keys, k, g):
        groups = {}
        for r in rows:
            if int(keys[r]) in groups or len(groups) < k:
                groups.setdefault(int(keys[r]), []).append(r)
        return [r for members in groups.values() for r in members[:g]]

    def asked(mgr, *args, **kw):
        before = dict(mgr.stats)
        hits = asyncio.run(mgr.search(*args, **kw))
        return _lists(hits), tuple(mgr.stats[c] - before[c] for c in counters)

    try:
        assert one._coalescer(one.collections["semantic_index"]) is None and one._main.n_shards == 1
        assert two._coalescer(two.collections["semantic_index"]) is None and two._main.n_shards == 2
        for coll, query in (("semantic_index", q), ("sparse_index", sq)):
            for expr in (None, 'chunk_index >= 2 and doc_id != "doc3"', "chunk_index > 100"):
                rows, scores, ids = _lists(asyncio.run(one.search(query, coll, top_k=256, filters=expr)))
                assert _lists(asyncio.run(two.search(query, coll, top_k=256, filters=expr))) == (rows, scores, ids)
                assert (len(rows) == 0) == (expr == "chunk_index > 100") and len(rows) < 256
                for field in ("doc_id", "chunk_index"):
                    keys = one._cols.group_keys(field)
                    for g in (1, 3):
                        for top_k in (2, 5, 60):
                            what = (coll, expr, field, g, top_k)
                            want = restated(rows, keys, top_k, g)
                            at = [rows.index(r) for r in want]
                            a, used_a = asked(one, query, coll, top_k=top_k, filters=expr, group_by_field=field, group_size=g)
                            b, used_b = asked(two, query, coll, top_k=top_k, filters=expr, group_by_field=field, group_size=g)
                            assert a == b == (want, [scores[i] for i in at], [ids[i] for i in at]), what
                            assert used_a == used_b and used_a[0] == 1, (what, used_a, used_b)
                            if (expr, field, g, top_k) == (None, "doc_id", 1, 5):
                                assert used_a[2] >= 1, what       # a window of 20 rows against the big document's 120
        assert one._dev_groups is not None and two._dev_groups is None
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


class _OneQueryGen:
    def __init__(self, q, sq):
        self.q, self.sq = q, sq

    def encode_semantic(self, text):
        return self.q

    def encode_sparse(self, text):
        return self.sq

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


def test_retrieve_returns_one_hit_per_document(gpu, long_timeout, corpus):
    X, csr, payload, q, sq = corpus
    mgr = _manager(corpus)
    try:
        mgr.embedding_generator = _OneQueryGen(q, sq)
        top_k = 8
        params = RetrievalConfig().sparse_search_params

        def restated(field):
            group = {"group_by_field": field} if field else {}
            sem = asyncio.run(mgr.search(q, "semantic_index", top_k=2 * top_k, **group))
            spa = asyncio.run(mgr.search(sq, "sparse_index", top_k=2 * top_k, search_params=params, **group))
            doc_of = {h["id"]: h["metadata"]["doc_id"] for h in sem + spa}
            fused = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa], []], [0.7, 0.3, 0.2], 60)
            if field:
                seen, kept = set(), []
                for cid, score, lists in fused:
                    if doc_of[cid] not in seen:
                        seen.add(doc_of[cid])
                        kept.append((cid, score, lists))
                fused = kept
            return [(cid, score, [("semantic", "sparse", "domain")[i] for i in lists]) for cid, score, lists in fused[:top_k]]

        initialize_caches()
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=top_k, group_by_field="doc_id"))
        hybrid_before = mgr._front.stats["hybrid_launches"] if mgr._front is not None else 0
        got = asyncio.run(retr.retrieve("plain statement"))
        docs = [h["metadata"]["doc_id"] for h in got]
        # (the big document need not lead: RRF fuses by chunk id, and its best semantic chunk is not its best sparse chunk)
        assert len(got) == top_k and len(set(docs)) == top_k and "big" in docs
        assert [(h["id"], h["score"], h["retrieval_methods"]) for h in got] == restated("doc_id")
        assert mgr._front.stats["hybrid_launches"] == hybrid_before         # the one-round path declined
        # without the field: chunks, through the one-round path, as ever
        initialize_caches()
        plain = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k)).retrieve("plain statement"))
        assert [(h["id"], h["score"], h["retrieval_methods"]) for h in plain] == restated(None)
        assert {h["metadata"]["doc_id"] for h in plain} == {"big"}
        assert mgr._front.stats["hybrid_launches"] == hybrid_before + 1
    finally:
        asyncio.run(mgr.close())
