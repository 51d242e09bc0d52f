"""Grouping search without a GPU: the group-key column (ordinals in first-seen order, extension, compaction, integer
fields), what a grouping request refuses, and the manager's continuation loop in its host form — over an oracle-backed
stand-in for the shard handles — against the ten-line restatement."""
import asyncio
import threading

import numpy as np
import pytest

import oracle
from advanced_rag.columns import GroupKeyColumn, PayloadColumns
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.retrieval import HybridRetriever, RetrievalConfig
from advanced_rag.shards import ShardSet


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


def _fill(cols, docs, base=0):
    for i, d in enumerate(docs):
        r = base + i
        cols["id"].append(f"id{r}")
        cols["doc_id"].append(d)
        cols["content"].append("")
        cols["timestamp"].append("t0" if r % 2 else "t1")
        cols["metadata_json"].append("{}")
        cols["chunk_index"].append(r % 4)
        cols["token_count"].append(-r)
        for k in ("entropy", "redundancy", "domain_density"):
            cols[k].append(0.5)


def test_group_keys_are_ordinals_in_first_seen_order():
    cols = PayloadColumns()
    docs = ["b", "a", "b", "ünï", "a", "", "ünï", "c"]
    _fill(cols, docs)
    keys = cols.group_keys("doc_id")
    assert keys.dtype == np.int64 and keys.tolist() == [0, 1, 0, 2, 1, 3, 2, 4]
    assert cols.group_keys("id").tolist() == list(range(8))              # every chunk its own group
    assert np.array_equal(cols.group_keys("chunk_id"), cols.group_keys("id"))
    assert cols.group_keys("timestamp").tolist() == [0, 1, 0, 1, 0, 1, 0, 1]


def test_group_keys_extend_after_first_use():
    cols = PayloadColumns()
    _fill(cols, ["x", "y", "x"])
    assert cols.group_keys("doc_id").tolist() == [0, 1, 0]
    _fill(cols, ["z", "y", "x", "w"], base=3)
    assert cols.group_keys("doc_id").tolist() == [0, 1, 0, 2, 1, 0, 3]   # old ordinals kept, new ones follow


def test_group_keys_compact_gathers_and_never_renumbers():
    cols = PayloadColumns()
    docs = ["a", "b", "a", "c", "b", "c", "d"]
    _fill(cols, docs)
    before = cols.group_keys("doc_id").copy()
    cols.group_keys("timestamp")
    keep = np.array([0, 1, 1, 0, 1, 1, 0], bool)
    cols.compact(keep)
    after = cols.group_keys("doc_id")
    assert after.tolist() == before[keep].tolist() == [1, 0, 1, 2]       # gathered: equal keys stay equal
    assert len(cols.group_keys("timestamp")) == 4
    _fill(cols, ["d", "a", "e"], base=4)
    # "d" was keyed before the compaction and keeps its ordinal although its row is gone; "e" is new
    assert cols.group_keys("doc_id").tolist() == [1, 0, 1, 2, 3, 0, 4]
    col = GroupKeyColumn()
    col.extend(["p", "q", "p"])
    with pytest.raises(ValueError):
        col.compact(np.ones(2, bool))


def test_group_keys_built_from_two_threads_equal_the_sequential_build():
    """The searches of one request ask for the same field at once (a sharded manager runs them in worker threads): the
    lazy build and a later extension must come out as one thread builds them."""
    n = 150_000                                   # more than one piece of the build
    docs = [f"doc{(r * 7919) % 20011}" for r in range(n)]

    def filled(values):
        cols = PayloadColumns()
        cols["doc_id"].extend(values)
        cols["id"].extend(f"c{r}" for r in range(len(values)))
        return cols

    want = filled(docs).group_keys("doc_id").copy()
    want_more = filled(docs + docs[:70_000][::-1]).group_keys("doc_id").copy()
    for _ in range(3):
        cols = filled(docs)
        for stage, expected in (("build", want), ("extend", want_more)):
            if stage == "extend":
                cols["doc_id"].extend(docs[:70_000][::-1])
            got, errors, gate = [], [], threading.Barrier(2)

            def worker():
                try:
                    gate.wait()
                    got.append(cols.group_keys("doc_id").copy())
                except Exception as e:           # noqa: BLE001 - the assertion below shows it
                    errors.append(e)

            threads = [threading.Thread(target=worker) for _ in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, (stage, errors)
            assert all(np.array_equal(g, expected) for g in got) and len(got) == 2, stage
            assert np.array_equal(cols.group_keys("doc_id"), expected)


def test_int_fields_are_their_own_keys():
    cols = PayloadColumns()
    _fill(cols, ["a"] * 6)
    assert cols.group_keys("chunk_index").tolist() == [0, 1, 2, 3, 0, 1]
    assert cols.group_keys("token_count").tolist() == [0, -1, -2, -3, -4, -5]
    cols["chunk_index"].append(7)                                        # a view of the column: later rows show up
    assert cols.group_keys("chunk_index").tolist()[-1] == 7


@pytest.mark.parametrize("field", ["entropy", "redundancy", "domain_density"])
def test_float_fields_are_refused(field):
    with pytest.raises(ValueError, match="float"):
        PayloadColumns().group_keys(field)
    with pytest.raises(ValueError, match="float"):
        asyncio.run(MilvusIndexManager(connect=False).search(np.zeros(4), "semantic_index", 5, group_by_field=field))


@pytest.mark.parametrize("field", ["nope", "content", "metadata_json", "", 3])
def test_unknown_fields_are_refused(field):
    if isinstance(field, str):
        with pytest.raises(ValueError, match="unknown group_by_field"):
            PayloadColumns().group_keys(field)
    with pytest.raises(ValueError, match="unknown group_by_field"):
        asyncio.run(MilvusIndexManager(connect=False).search(np.zeros(4), "semantic_index", 5, group_by_field=field))


def test_group_size_other_than_one_is_refused():
    m = MilvusIndexManager(connect=False)
    with pytest.raises(ValueError, match="group_size=2 is not supported: only group_size=1"):
        asyncio.run(m.search(np.zeros(4), "semantic_index", 5, group_by_field="doc_id", group_size=2))
    with pytest.raises(ValueError, match="group_size"):
        asyncio.run(m.search(np.zeros(4), "semantic_index", 5, group_size=0))
    with pytest.raises(ValueError, match="HR_MAX_TOPK"):
        MilvusIndexManager.group_window(257)
    assert MilvusIndexManager.group_window(5) == 20 and MilvusIndexManager.group_window(100) == 256


# ---------------------------------------------------------------------------------------------------------------------
# the host form of the continuation loop (what a sharded or a torchrun manager runs), over the oracle

class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given, with the handle's search signatures."""

    def __init__(self, sparse_dim):
        self.X = None
        self.ptr, self.idx, self.val = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
        self.device, self.sparse_dim = 0, sparse_dim

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = property(lambda self: len(self.ptr) - 1)

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def add_sparse(self, ptr, idx, val):
        self.idx = np.concatenate([self.idx, idx[ptr[0]:ptr[-1]]])
        self.val = np.concatenate([self.val, val[ptr[0]:ptr[-1]]])
        self.ptr = np.concatenate([self.ptr, ptr[1:] - ptr[0] + self.ptr[-1]])

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def search_sparse(self, queries, k, drop, mask=None):
        return oracle.sparse_search(self.ptr, self.idx, self.val, queries, k, drop, mask)

    def finalize(self):
        pass

    def close(self):
        pass


N, DIM, V = 240, 16, 64


@pytest.fixture(scope="module")
def host_manager():
    """240 rows on two oracle-backed shards: document "big" holds the 120 rows nearest the query, the rest are documents
    of 1 to 10 chunks; scores are heavily tied (rows repeat a handful of directions)."""
    rng = np.random.default_rng(5)
    q = np.zeros(DIM, np.float32)
    q[0] = 1.0
    X = np.zeros((N, DIM), np.float32)
    X[:120, 0] = 1.0
    X[:120, 1] = rng.integers(0, 3, 120) * 0.25            # three distinct cosines among the big document's chunks
    X[120:, 0] = rng.integers(0, 4, 120) * 0.25
    X[120:, 2] = 1.0
    perm = rng.permutation(N)
    X = X[perm]
    docs = np.empty(N, dtype=object)
    small, d = [], 0
    while len(small) < 120:
        small += [f"doc{d}"] * int(rng.integers(1, 11))
        d += 1
    docs_sorted = ["big"] * 120 + small[:120]
    for new, old in enumerate(perm):
        docs[new] = docs_sorted[old]
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, size=(N, 4))).astype(np.int32)    # ascending within a row
    val = (rng.integers(1, 3, size=(N, 4))).astype(np.float32)
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    sq = (np.arange(V, dtype=np.int32), np.ones(V, np.float32))
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, connect=False, enable_domain=False)
    mgr.attach_shards([_OracleShard(V), _OracleShard(V)])
    for lo in range(0, N, 100):
        hi = min(N, lo + 100)
        mgr.add_rows(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]), ids=[f"c{r}" for r in range(lo, hi)],
                     doc_id=list(docs[lo:hi]), chunk_index=[r % 7 for r in range(lo, hi)])
    assert isinstance(mgr._main, ShardSet) and mgr._filters_on_device() is None
    yield mgr, q, sq
    asyncio.run(mgr.close())


def _rows(hits):
    return [h["_row"] for h in hits], [h["score"] for h in hits], [h["id"] for h in hits]


@pytest.mark.parametrize("collection", ["semantic_index", "sparse_index"])
@pytest.mark.parametrize("field,top_k,expr", [("doc_id", 5, None), ("chunk_index", 5, None), ("doc_id", 60, None),
                                              ("doc_id", 5, "chunk_index >= 2"), ("id", 7, None)])
def test_host_loop_equals_the_restatement(host_manager, collection, field, top_k, expr):
    mgr, q, sq = host_manager
    query = {"indices": sq[0].tolist(), "values": sq[1].tolist()} if collection == "sparse_index" else q
    ranking = asyncio.run(mgr.search(query, collection, top_k=N, filters=expr))
    rows, scores, ids = _rows(ranking)
    keys = mgr._cols.group_keys(field)
    want = first_k_distinct(rows, keys, top_k)
    at = [rows.index(r) for r in want]
    before = dict(mgr.stats)
    got = asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr, group_by_field=field))
    assert _rows(got) == (want, [scores[i] for i in at], [ids[i] for i in at])
    n_groups = len(set(keys[rows].tolist()))
    assert len(got) == min(top_k, n_groups)
    if field == "doc_id" and top_k == 5 and expr is None and collection == "semantic_index":
        # the window is 20 rows and the big document fills the first 120: continuation rounds were needed
        assert mgr.stats["group_continuations"] > before["group_continuations"]
    # the ungrouped answer is what it was
    assert _rows(asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr)))[0] == rows[:top_k]


TABLE_FIELDS = ("doc_id", "chunk_index", "id", "token_count", "timestamp")       # (the last two hold one value: one group)
TABLE_TOP_K = (1, 2, 5, 20, 60, 256)
TABLE_EXPRS = (None, "chunk_index >= 2", 'doc_id != "big"', "chunk_index > 100")  # the last keeps no row
GROUP_COUNTERS = ("group_searches", "group_rounds", "group_continuations", "group_fill_searches", "group_fill_rounds")
# What one group_by_field request (group_size 1) added to GROUP_COUNTERS, recorded by running this table on commit e9d4c67
# (the parent of the change that made the grouped search one loop), whose group_size == 1 requests ran a loop of their own.
# There every request added (1, rounds, continuations, 0, 0); below is "rounds continuations" per request, the top_k values
# of a (collection, field) on one line each, the four expressions of a top_k together.
TABLE_ROUNDS = {
    ("semantic_index", "doc_id"): "1 0 1 0 1 0 1 0  2 1 2 1 1 0 1 0  2 1 2 1 1 0 1 0  2 1 2 1 1 0 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("semantic_index", "chunk_index"): "1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("semantic_index", "id"): "1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("semantic_index", "token_count"): "1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("semantic_index", "timestamp"): "1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("sparse_index", "doc_id"): "1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  2 1 2 1 1 0 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("sparse_index", "chunk_index"): "1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("sparse_index", "id"): "1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("sparse_index", "token_count"): "1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
    ("sparse_index", "timestamp"): "1 0 1 0 1 0 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 2 1 2 1 1 0  2 1 1 0 1 0 1 0  1 0 1 0 1 0 1 0",
}


def _table_request(mgr, query, collection, field, top_k, expr, rankings):
    """One request of the table: the grouped answer is the restatement over the ungrouped ranking -> the counters' delta."""
    if (collection, expr) not in rankings:
        rankings[collection, expr] = _rows(asyncio.run(mgr.search(query, collection, top_k=N, filters=expr)))
    rows, scores, ids = rankings[collection, expr]
    want = first_k_distinct(rows, mgr._cols.group_keys(field), top_k)
    at = [rows.index(r) for r in want]
    before = dict(mgr.stats)
    got = asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr, group_by_field=field))
    delta = tuple(mgr.stats[c] - before[c] for c in GROUP_COUNTERS)
    assert _rows(got) == (want, [scores[i] for i in at], [ids[i] for i in at]), (collection, field, top_k, expr)
    return delta


@pytest.mark.parametrize("collection", ["semantic_index", "sparse_index"])
@pytest.mark.parametrize("field", TABLE_FIELDS)
def test_host_loop_answers_and_counts_as_the_parent_did(host_manager, collection, field):
    mgr, q, sq = host_manager
    query = {"indices": sq[0].tolist(), "values": sq[1].tolist()} if collection == "sparse_index" else q
    rankings = {}
    expected = iter(TABLE_ROUNDS[collection, field].split())
    for top_k in TABLE_TOP_K:
        for expr in TABLE_EXPRS:
            delta = _table_request(mgr, query, collection, field, top_k, expr, rankings)
            assert delta == (1, int(next(expected)), int(next(expected)), 0, 0), (collection, field, top_k, expr, delta)
    assert rankings[collection, TABLE_EXPRS[-1]][0] == [] and next(expected, None) is None


def test_host_loop_after_delete(host_manager):
    mgr, q, _ = host_manager
    best = asyncio.run(mgr.search(q, "semantic_index", top_k=30))
    gone = [h["id"] for h in best[:25]]
    saved = (mgr._deleted, mgr._delete_epoch)
    try:
        for i in gone:
            asyncio.run(mgr.delete_by_filter("semantic_index", f'chunk_id == "{i}"'))
        rows, scores, _ = _rows(asyncio.run(mgr.search(q, "semantic_index", top_k=N)))
        assert not set(rows) & {h["_row"] for h in best[:25]}
        want = first_k_distinct(rows, mgr._cols.group_keys("doc_id"), 6)
        got = asyncio.run(mgr.search(q, "semantic_index", top_k=6, group_by_field="doc_id"))
        assert _rows(got)[0] == want and _rows(got)[1] == [scores[rows.index(r)] for r in want]
    finally:
        mgr._deleted, mgr._delete_epoch = saved[0], mgr._delete_epoch + 1
        mgr._forget_masks(rebuild_filters=False)


def test_synthetic_collection_groups_on_what_its_hits_show():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((95, DIM)).astype(np.float32)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard(0)])
    mgr.add_rows_synthetic(X)
    q = X[:30].sum(axis=0)
    rows = _rows(asyncio.run(mgr.search(q, "semantic_index", top_k=95)))[0]
    got = _rows(asyncio.run(mgr.search(q, "semantic_index", top_k=8, group_by_field="doc_id")))[0]
    assert got == first_k_distinct(rows, np.arange(95) // 10, 8) and len({r // 10 for r in got}) == 8
    got = _rows(asyncio.run(mgr.search(q, "semantic_index", top_k=20, group_by_field="chunk_index")))[0]
    assert got == first_k_distinct(rows, np.arange(95) % 10, 20) and len(got) == 10
    with pytest.raises(ValueError, match="bulk-ingested without payload columns"):
        asyncio.run(mgr.search(q, "semantic_index", top_k=8, group_by_field="timestamp"))
    asyncio.run(mgr.close())


# ---------------------------------------------------------------------------------------------------------------------
# the retriever's host pass

def test_first_per_group_keeps_the_first_hit_of_every_group():
    hits = [{"id": f"c{i}", "metadata": {"doc_id": d, "chunk_index": i % 2}} for i, d in enumerate("abacbd")]
    assert [h["id"] for h in HybridRetriever._first_per_group(list(hits), "doc_id")] == ["c0", "c1", "c3", "c5"]
    assert [h["id"] for h in HybridRetriever._first_per_group(list(hits), "chunk_index")] == ["c0", "c1"]
    assert len(HybridRetriever._first_per_group(list(hits), "chunk_id")) == 6
    assert RetrievalConfig().group_by_field is None
    profiles = HybridRetriever._build_default_profiles(RetrievalConfig(group_by_field="doc_id"))
    assert all(p.group_by_field == "doc_id" for p in profiles.values())


@pytest.mark.parametrize("field", ["token_count", "entropy", "nope", "content", 3])
def test_retrieval_config_refuses_what_the_fused_pass_cannot_group_on(field):
    with pytest.raises(ValueError, match="group_by_field"):
        RetrievalConfig(group_by_field=field)
    for ok in ("doc_id", "chunk_index", "timestamp", "id", "chunk_id"):
        assert RetrievalConfig(group_by_field=ok).group_by_field == ok


def test_retriever_passes_the_field_only_when_it_is_set():
    class Manager:
        def __init__(self):
            self.calls = []

        async def search(self, **kw):
            self.calls.append(kw)
            return []

    m = Manager()
    r = HybridRetriever(m, RetrievalConfig())
    asyncio.run(r._search_semantic(np.zeros(4), None))
    assert "group_by_field" not in m.calls[-1]                           # managers that never heard of grouping keep working
    r.config = RetrievalConfig(group_by_field="doc_id")
    asyncio.run(r._search_sparse({"indices": [1], "values": [1.0]}, None))
    assert m.calls[-1]["group_by_field"] == "doc_id" and m.calls[-1]["top_k"] == 40
