"""Grouping search with group_size > 1 end to end: MilvusIndexManager(group_members=True).search(..., group_by_field=F,
group_size=g) against the restatement "the first g rows of each of the first top_k groups" over the manager's own
ungrouped ranking (which the other suites hold to the oracle) — rows, ids and score bits — through the one-round answer,
the continuation loop and the fill phase, the batching front, two shards, a synthetic collection and retrieve()."""
import asyncio

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


def first_n_of_first_k_groups(ranked_rows, keys, k, g):
    """The first g rows of each of the first k groups of a ranking, groups in order of their first row -> flat list."""
    groups = {}
    for r in ranked_rows:
        key = int(keys[r])
        if key not in groups:
            if len(groups) == k:
                continue
            groups[key] = []
        if len(groups[key]) < g:
            groups[key].append(int(r))
    return [r for rows in groups.values() for r in rows]


def first_window_answers(ranked_rows, keys, k, g):
    """Whether the first window of K' rows proves the answer: the groups are final (k of them, or the ranking ended
    inside the window) and so are their members (g of each in the window, or the ranking ended inside it)."""
    window = MilvusIndexManager.group_window(k, g)
    head = ranked_rows[:window]
    if len(head) < window:
        return True
    groups = {}
    for r in head:
        groups.setdefault(int(keys[r]), []).append(r)
    first = list(groups.values())[:k]
    return len(groups) >= k and all(len(m) >= g for m in first)


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


def _manager(corpus, metric="COSINE", group_members=True, **kw):
    X, csr, payload, _, _ = corpus
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, enable_domain=False, semantic_metric=metric,
                             group_members=group_members, **kw)
    mgr.add_rows(X, csr, **payload)
    mgr.finalize()
    return mgr


def _lists(hits):
    return [h["_row"] for h in hits], [h["score"] for h in hits], [h["id"] for h in hits]


def _expected(mgr, query, coll, field, top_k, g, expr=None):
    """The restatement over the manager's own ungrouped ranking -> ((rows, scores, ids), the ranking, the keys)"""
    rows, scores, ids = _lists(asyncio.run(mgr.search(query, coll, top_k=256, filters=expr)))
    assert 0 < len(rows) < 256                                    # the whole ranking of the qualifying rows
    keys = mgr._cols.group_keys(field)
    want = first_n_of_first_k_groups(rows, keys, top_k, g)
    at = [rows.index(r) for r in want]
    return (want, [scores[i] for i in at], [ids[i] for i in at]), rows, keys


def _check(mgr, query, coll, field, top_k, g, expr=None):
    """search(group_by_field=field, group_size=g), through the front and through the blocking loop alone, == the
    restatement.  -> (the hits, what the blocking loop added to the manager's stats)"""
    want, rows, keys = _expected(mgr, query, coll, field, top_k, g, expr)
    what = (coll, field, top_k, g, expr)
    got = asyncio.run(mgr.search(query, coll, top_k=top_k, filters=expr, group_by_field=field, group_size=g))
    assert _lists(got) == want, what
    before = dict(mgr.stats)
    payload = mgr._as_sparse_payload(query) if coll == "sparse_index" else query
    alone = mgr._format_hits(*mgr._search_lists_blocking(payload, coll, top_k, expr, mgr._search_params(mgr.collections[coll], None),
                                                         field, None, g))
    assert _lists(alone) == want, what
    used = {k: mgr.stats[k] - before[k] for k in before}
    assert used["group_searches"] == 1
    # the shape of the answer: at most top_k groups of at most g adjacent hits
    shown = keys[[h["_row"] for h in got]].tolist()
    runs = [k for i, k in enumerate(shown) if i == 0 or shown[i - 1] != k]
    assert len(runs) == len(set(runs)) <= top_k and max(shown.count(k) for k in runs) <= g, what
    assert len(runs) == min(top_k, len(set(keys[rows].tolist()))), what
    for strict in (True, False):
        assert asyncio.run(mgr.search(query, coll, top_k=top_k, filters=expr, group_by_field=field, group_size=g,
                                      strict_group_size=strict)) == got
    return got, used


SIZES = [(5, 3), (2, 3), (1, 256), (128, 2)]
EXPR = 'chunk_index >= 2 and doc_id != "doc3"'


@pytest.mark.parametrize("metric", ["COSINE", "IP", "L2"])
def test_group_size_search_equals_the_restatement(gpu, corpus, metric):
    X, csr, payload, q, sq = corpus
    mgr = _manager(corpus, metric)
    try:
        asyncio.run(mgr.delete_by_filter("semantic_index", 'doc_id == "big" and token_count == 1'))   # tombstones
        outcomes = {"one_round": 0, "continued": 0, "filled": 0}
        short_group = fewer_groups = False
        for coll, query in (("semantic_index", q), ("sparse_index", sq)):
            for field, expr in (("doc_id", None), ("chunk_index", None), ("doc_id", EXPR), ("doc_id", 'doc_id != "big"')):
                for top_k, g in SIZES:
                    got, used = _check(mgr, query, coll, field, top_k, g, expr)
                    outcomes["continued"] += used["group_continuations"] > 0
                    outcomes["filled"] += used["group_fill_rounds"] > 0
                    outcomes["one_round"] += used["group_rounds"] == 1 and used["group_fill_rounds"] == 0
                    assert (used["group_fill_searches"] == 1) == (used["group_fill_rounds"] > 0)
                    assert used["group_fill_rounds"] <= top_k
                    if field == "doc_id":
                        docs = [h["metadata"]["doc_id"] for h in got]
                        n_groups = len(set(docs))
                        fewer_groups |= n_groups < top_k
                        short_group |= any(docs.count(d) < g for d in set(docs)) and g <= 3
                        if expr is None:
                            assert docs[0] == "big" and docs.count("big") > 1      # the big document leads, with more than one chunk
                    if field == "doc_id" and expr is None and (top_k, g) in ((5, 3), (2, 3)):
                        # the window (60 / 24 rows) is smaller than the big document, which leads the ranking
                        assert used["group_continuations"] >= 1, (coll, top_k, g)
        assert all(outcomes.values()), outcomes          # an answer in one round, phase-1 continuation, phase 2
        assert short_group and fewer_groups
        assert mgr._front.stats["group_launches"] > 0 and mgr._front.stats["redone_grouped"] > 0
        # group_size = 1 with the option on is the answer of a manager without it
        plain = _manager(corpus, metric, group_members=False)
        try:
            asyncio.run(plain.delete_by_filter("semantic_index", 'doc_id == "big" and token_count == 1'))
            for coll, query in (("semantic_index", q), ("sparse_index", sq)):
                a = asyncio.run(mgr.search(query, coll, top_k=5, group_by_field="doc_id", group_size=1))
                assert a == asyncio.run(plain.search(query, coll, top_k=5, group_by_field="doc_id"))
            with pytest.raises(ValueError, match="group_size=2 is not supported: only group_size=1"):
                asyncio.run(plain.search(q, "semantic_index", top_k=5, group_by_field="doc_id", group_size=2))
        finally:
            asyncio.run(plain.close())
    finally:
        asyncio.run(mgr.close())


def test_group_size_searches_share_one_launch_of_the_front(gpu, corpus):
    X, csr, payload, q, sq = corpus
    rng = np.random.default_rng(3)
    away = np.zeros(D, np.float32)
    away[2] = 1.0                                                 # nearest the small documents: the big one comes last
    queries = [q, away] + [np.abs(rng.standard_normal(D)).astype(np.float32) for _ in range(14)]
    top_k, g = 5, 2
    mgr = _manager(corpus)
    try:
        mgr._front = SearchCoalescer(mgr, window_s=5e-3)          # a round waits 5 ms for its next request: one tick fits
        want, finished = [], []
        for p in queries:
            w, rows, keys = _expected(mgr, p, "semantic_index", "doc_id", top_k, g)
            want.append(w)
            finished.append(first_window_answers(rows, keys, top_k, g))
        assert 0 < sum(finished) < len(queries)                   # mixed outcomes

        async def burst():
            return await asyncio.gather(*[mgr.search(p, "semantic_index", top_k=top_k, group_by_field="doc_id", group_size=g)
                                          for p in queries])

        st = mgr._front.stats
        before, before_mgr = dict(st), dict(mgr.stats)
        together = asyncio.run(burst())
        assert [_lists(t) for t in together] == want
        assert st["group_launches"] - before["group_launches"] == 1          # one grouped batch, not sixteen
        assert st["dense_launches"] - before["dense_launches"] == 1
        assert st["rounds"] - before["rounds"] == 1 and st["max_batch_seen"] == 16
        assert st["redone_grouped"] - before["redone_grouped"] == len(queries) - sum(finished)
        assert mgr.stats["group_searches"] - before_mgr["group_searches"] == len(queries) - sum(finished)
        # another group size is another key: no shared launch
        async def two_sizes():
            return await asyncio.gather(mgr.search(away, "semantic_index", top_k=top_k, group_by_field="doc_id", group_size=2),
                                        mgr.search(away, "semantic_index", top_k=top_k, group_by_field="doc_id", group_size=3),
                                        mgr.search(away, "semantic_index", top_k=top_k, group_by_field="doc_id"))

        before = dict(st)
        a, b, c = asyncio.run(two_sizes())
        assert st["group_launches"] - before["group_launches"] == 3
        assert _lists(a) == want[1] and _lists(b) == _expected(mgr, away, "semantic_index", "doc_id", top_k, 3)[0]
        assert _lists(c) == _expected(mgr, away, "semantic_index", "doc_id", top_k, 1)[0]
    finally:
        asyncio.run(mgr.close())


def test_two_shards_give_the_single_shard_lists(gpu, corpus):
    X, csr, payload, q, sq = corpus
    one, two = _manager(corpus), _manager(corpus, devices=[0, 0])
    try:
        assert two._main.n_shards == 2 and two._coalescer(two.collections["semantic_index"]) is None
        filled = 0
        for coll, query in (("semantic_index", q), ("sparse_index", sq)):
            for field, top_k, g, expr in (("doc_id", 5, 3, None), ("chunk_index", 5, 3, None), ("doc_id", 128, 2, None),
                                          ("doc_id", 2, 3, 'doc_id != "big"'), ("doc_id", 5, 3, "chunk_index >= 2")):
                a, used_a = _check(one, query, coll, field, top_k, g, expr)
                b, used_b = _check(two, query, coll, field, top_k, g, expr)
                assert a == b and used_a == used_b, (coll, field, top_k, g, expr)      # the same loop in both forms
                filled += used_b["group_fill_rounds"] > 0
        assert filled and two.stats["group_continuations"] >= 2 and two._dev_groups is None      # the host form: no mirror
    finally:
        asyncio.run(one.close())
        asyncio.run(two.close())


def test_synthetic_collection_groups_on_its_generated_keys(gpu):
    rng = np.random.default_rng(8)
    n = 250                                                       # the whole ranking fits one ungrouped search
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[100:140] += 3.0                                             # four "documents" (row // 10) crowd the top of the ranking
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, enable_domain=False, group_members=True)
    mgr.collections.pop("sparse_index", None)
    try:
        mgr.add_rows_synthetic(X)
        mgr.finalize()
        q = np.full(D, 1.0, np.float32)
        hits = asyncio.run(mgr.search(q, "semantic_index", top_k=256))
        rows, score_of = [h["_row"] for h in hits], {h["_row"]: h["score"] for h in hits}
        assert len(rows) == n
        before = dict(mgr.stats)
        for top_k, g in ((12, 3), (4, 10), (5, 12), (25, 10)):   # (5, 12): documents of 10 rows in a full window of 240 stay open
            got = asyncio.run(mgr.search(q, "semantic_index", top_k=top_k, group_by_field="doc_id", group_size=g))
            want = first_n_of_first_k_groups(rows, np.arange(n) // 10, top_k, g)
            assert [h["_row"] for h in got] == want and len(want) == top_k * min(g, 10)
            assert [h["score"] for h in got] == [score_of[r] for r in want]
            assert [h["metadata"]["doc_id"] for h in got] == [f"doc{r // 10}" for r in want]
        assert mgr.stats["group_fill_rounds"] > before["group_fill_rounds"]
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=10, group_by_field="chunk_index", group_size=4))
        assert [h["_row"] for h in got] == first_n_of_first_k_groups(rows, np.arange(n) % 10, 10, 4) and len(got) == 40
        with pytest.raises(ValueError, match="bulk-ingested without payload columns"):
            asyncio.run(mgr.search(q, "semantic_index", top_k=12, group_by_field="timestamp", group_size=2))
    finally:
        asyncio.run(mgr.close())


class _OneQueryGen:
    def __init__(self, q, sq):
        self.q, self.sq = q, sq

    def encode_semantic(self, text):
        return self.q

    def encode_sparse(self, text):
        return self.sq

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


def test_retrieve_returns_up_to_two_hits_per_document(gpu, long_timeout, corpus):
    X, csr, payload, q, sq = corpus
    mgr, plain = _manager(corpus), _manager(corpus, group_members=False)
    try:
        top_k, g = 8, 2
        params = RetrievalConfig().sparse_search_params
        sem = asyncio.run(mgr.search(q, "semantic_index", top_k=2 * top_k, group_by_field="doc_id", group_size=g))
        spa = asyncio.run(mgr.search(sq, "sparse_index", top_k=2 * top_k, search_params=params, group_by_field="doc_id",
                                     group_size=g))
        assert len(sem) > 2 * top_k and len(spa) > 2 * top_k      # more than one hit per document in both lists
        doc_of = {h["id"]: h["metadata"]["doc_id"] for h in sem + spa}
        fused = rrf_rank_lists([[h["id"] for h in sem], [h["id"] for h in spa], []], [0.7, 0.3, 0.2], 60)
        count, kept = {}, []
        for cid, score, lists in fused:
            if count.get(doc_of[cid], 0) < g:
                count[doc_of[cid]] = count.get(doc_of[cid], 0) + 1
                kept.append((cid, score, [("semantic", "sparse", "domain")[i] for i in lists]))
        assert len(kept) < len(fused)                             # the fused pass had something to drop
        for m in (mgr, plain):
            m.embedding_generator = _OneQueryGen(q, sq)
        initialize_caches()
        retr = HybridRetriever(mgr, RetrievalConfig(top_k=top_k, group_by_field="doc_id", group_size=g))
        hybrid_before = mgr._front.stats["hybrid_launches"]
        got = asyncio.run(retr.retrieve("plain statement"))
        assert [(h["id"], h["score"], h["retrieval_methods"]) for h in got] == kept[:top_k] and len(got) == top_k
        docs = [h["metadata"]["doc_id"] for h in got]
        assert max(docs.count(d) for d in docs) == g and len(set(docs)) < top_k
        assert mgr._front.stats["hybrid_launches"] == hybrid_before         # the general path served it
        # a manager without the option: its refusal surfaces
        initialize_caches()
        with pytest.raises(ValueError, match="group_size=2 is not supported: only group_size=1"):
            asyncio.run(HybridRetriever(plain, RetrievalConfig(top_k=top_k, group_by_field="doc_id", group_size=g))
                        .retrieve("plain statement"))
    finally:
        asyncio.run(mgr.close())
        asyncio.run(plain.close())
