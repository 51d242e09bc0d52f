"""Grouping search with group_size > 1 without a GPU: the manager's two phases in their host form — over an oracle-backed
stand-in for the shard handles — against the restatement "walk the ranking, keep the first top_k groups and the first
group_size rows of each", what such a request refuses, the window rule, and the retriever's fused pass."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag.device_groups import group_select_n_host
from advanced_rag.indexing import MilvusIndexManager
from advanced_rag.retrieval import HybridRetriever, RetrievalConfig
from advanced_rag.shards import ShardSet


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


def _host_manager(X, docs, csr=None, **kw):
    n = X.shape[0]
    v = V if csr is not None else 0
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=v, connect=False, enable_domain=False, group_members=True, **kw)
    mgr.attach_shards([_OracleShard(v), _OracleShard(v)])
    for lo in range(0, n, 100):
        hi = min(n, lo + 100)
        mgr.add_rows(X[lo:hi], None if csr is None else (csr[0][lo:hi + 1], csr[1], csr[2]),
                     ids=[f"c{r}" for r in range(lo, hi)], doc_id=list(docs[lo:hi]), chunk_index=[r % 7 for r in range(lo, hi)])
    assert isinstance(mgr._main, ShardSet) and mgr._filters_on_device() is None
    return mgr


@pytest.fixture(scope="module")
def host_manager():
    """240 rows on two oracle-backed shards: document "big" holds the 120 rows nearest the query, the rest are documents
    of 1 to 10 chunks; scores are heavily tied (rows repeat a handful of directions)."""
    rng = np.random.default_rng(5)
    q = np.zeros(DIM, np.float32)
    q[0] = 1.0
    X = np.zeros((N, DIM), np.float32)
    X[:120, 0] = 1.0
    X[:120, 1] = rng.integers(0, 3, 120) * 0.25
    X[120:, 0] = rng.integers(0, 4, 120) * 0.25
    X[120:, 2] = 1.0
    perm = rng.permutation(N)
    X = X[perm]
    small, d = [], 0
    while len(small) < 120:
        small += [f"doc{d}"] * int(rng.integers(1, 11))
        d += 1
    docs_sorted = ["big"] * 120 + small[:120]
    docs = [docs_sorted[old] for old in perm]
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, size=(N, 4))).astype(np.int32)    # ascending within a row
    val = (rng.integers(1, 3, size=(N, 4))).astype(np.float32)
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    sq = {"indices": list(range(V)), "values": [1.0] * V}
    mgr = _host_manager(X, docs, csr)
    yield mgr, q, sq
    asyncio.run(mgr.close())


def _rows(hits):
    return [h["_row"] for h in hits], [h["score"] for h in hits], [h["id"] for h in hits]


def _check(mgr, query, collection, field, top_k, g, expr=None, **kw):
    """search(group_by_field, group_size) == the restatement over the same manager's whole ungrouped ranking, rows, score
    bits and ids.  -> (hits, what the request added to the manager's stats)"""
    n = mgr.num_rows
    rows, scores, ids = _rows(asyncio.run(mgr.search(query, collection, top_k=n, filters=expr)))
    keys = mgr._cols.group_keys(field)
    want = first_n_of_first_k_groups(rows, keys, top_k, g)
    at = [rows.index(r) for r in want]
    before = dict(mgr.stats)
    got = asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr, group_by_field=field, group_size=g, **kw))
    assert _rows(got) == (want, [scores[i] for i in at], [ids[i] for i in at]), (collection, field, top_k, g, expr)
    got_keys = keys[[h["_row"] for h in got]].tolist()
    assert all(a == b or b not in got_keys[:i] for i, (a, b) in enumerate(zip(got_keys, got_keys[1:]), 1))    # groups are adjacent
    return got, {k: mgr.stats[k] - before[k] for k in before}


CASES = [("doc_id", 5, 3, None), ("doc_id", 2, 3, None), ("doc_id", 1, 256, None), ("doc_id", 128, 2, None),
         ("chunk_index", 5, 3, None), ("doc_id", 5, 3, "chunk_index >= 2"), ("id", 7, 2, None), ("doc_id", 60, 4, None)]


@pytest.mark.parametrize("collection", ["semantic_index", "sparse_index"])
@pytest.mark.parametrize("field,top_k,g,expr", CASES)
def test_host_phases_equal_the_restatement(host_manager, collection, field, top_k, g, expr):
    mgr, q, sq = host_manager
    query = sq if collection == "sparse_index" else q
    got, used = _check(mgr, query, collection, field, top_k, g, expr)
    assert used["group_searches"] == 1
    if field == "doc_id" and expr is None and collection == "semantic_index":
        docs = [h["metadata"]["doc_id"] for h in got]
        assert docs[:min(g, 120)] == ["big"] * min(g, 120)
        if (top_k, g) == (5, 3):
            # the window (60 rows) lies inside the big document: continuation, and every later group closes in its window
            assert used["group_continuations"] >= 1
        if (top_k, g) == (1, 256):
            # the window is 256 rows and the ranking holds 240: not full, so the one group is closed with all it has
            assert used["group_fill_rounds"] == 0 and len(got) == 120
        if (top_k, g) == (60, 4):
            assert len(set(docs)) < 60                      # fewer groups than top_k
            assert any(docs.count(d) < 4 for d in set(docs))   # a group with fewer members than group_size
    # strict_group_size changes nothing, and group_size=1 is what it was
    for strict in (True, False):
        assert _check(mgr, query, collection, field, top_k, g, expr, strict_group_size=strict)[0] == got
    one = asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr, group_by_field=field))
    assert one == asyncio.run(mgr.search(query, collection, top_k=top_k, filters=expr, group_by_field=field, group_size=1))


def test_a_second_member_beyond_every_phase_one_window():
    """600 rows: documents a and b lead the ranking with one row each, then 500 rows of singletons, then the second and
    third rows of a and b.  top_k=2, group_size=3: the window is 24 rows, phase 1 ends after one window with both
    groups open, and only the fill phase can find their later members."""
    n = 600
    X = np.zeros((n, DIM), np.float32)
    X[:, 0] = 1.0
    X[:, 1] = np.arange(n) * 0.01                # cosine with the query falls with the row number: the ranking is 0, 1, 2, ...
    q = np.zeros(DIM, np.float32)
    q[0] = 1.0
    docs = [f"single{r}" for r in range(n)]
    for r in (0, 510, 530):
        docs[r] = "a"
    for r in (1, 520, 599):
        docs[r] = "b"
    docs[2] = docs[3] = "c"                      # a closed group behind them: it has no part in the answer
    mgr = _host_manager(X, docs)
    try:
        got, used = _check(mgr, q, "semantic_index", "doc_id", 2, 3)
        assert [h["_row"] for h in got] == [0, 510, 530, 1, 520, 599]
        assert used == {**{k: 0 for k in used}, "group_searches": 1, "group_rounds": 1, "group_fill_searches": 1, "group_fill_rounds": 1}
        # a has three members, b two and a half windows of singletons: b's group is short, the fill list is not full
        docs2 = list(docs)
        docs2[599] = "single599"
        mgr2 = _host_manager(X, docs2)
        try:
            got, used = _check(mgr2, q, "semantic_index", "doc_id", 2, 3)
            assert [h["_row"] for h in got] == [0, 510, 530, 1, 520] and used["group_fill_rounds"] == 1
            # top_k = 3 takes c, which closes in the first window: still one fill round for a and b only
            got, used = _check(mgr2, q, "semantic_index", "doc_id", 3, 3)
            assert [h["_row"] for h in got] == [0, 510, 530, 1, 520, 2, 3] and used["group_fill_rounds"] == 1
        finally:
            asyncio.run(mgr2.close())
    finally:
        asyncio.run(mgr.close())


def test_fill_rounds_repeat_while_a_full_list_leaves_groups_open():
    """Two open groups, one of which has 300 rows right behind the first window: the fill list of 256 rows is full of it,
    closes it alone, and a second round fills the other group."""
    n = 700
    X = np.zeros((n, DIM), np.float32)
    X[:, 0] = 1.0
    X[:, 1] = np.arange(n) * 0.01
    q = np.zeros(DIM, np.float32)
    q[0] = 1.0
    docs = [f"single{r}" for r in range(n)]
    docs[0] = "a"
    docs[1] = "b"
    for r in range(100, 400):
        docs[r] = "a"
    docs[650] = docs[651] = "b"
    mgr = _host_manager(X, docs)
    try:
        got, used = _check(mgr, q, "semantic_index", "doc_id", 2, 3)
        assert [h["_row"] for h in got] == [0, 100, 101, 1, 650, 651]
        assert used["group_fill_searches"] == 1 and used["group_fill_rounds"] == 2 and used["group_rounds"] == 1
    finally:
        asyncio.run(mgr.close())


def test_select_restatement_on_a_small_list():
    keys = np.array([7, 7, 8, 7, 9, 8, 9, 9, 7], np.int64)
    ids = np.array([0, 1, 2, 3, 4, 5, 6, -1, 8], np.int64)                # the list ends at the first id < 0
    at, sel, n = group_select_n_host(ids, keys, 2, 2)
    assert [a.tolist() for a in at] == [[0, 1], [2, 5]] and sel == [7, 8] and n == 7
    at, sel, n = group_select_n_host(ids[:7], keys, 5, 3)
    assert [a.tolist() for a in at] == [[0, 1, 3], [2, 5], [4, 6]] and sel == [7, 8, 9] and n == 7
    at, sel, n = group_select_n_host(np.full(4, -1, np.int64), keys, 3, 2)
    assert at == [] and sel == [] and n == 0


def test_what_a_group_size_request_refuses():
    m = MilvusIndexManager(connect=False, group_members=True)
    q = np.zeros(4)

    def search(**kw):
        return asyncio.run(m.search(q, "semantic_index", kw.pop("top_k", 5), **kw))

    for bad in (True, False, 2.0, 0, -1, "2", None):
        with pytest.raises(ValueError, match="group_size must be an integer >= 1"):
            search(group_by_field="doc_id", group_size=bad)
    with pytest.raises(ValueError, match="group_size=2 needs group_by_field"):
        search(group_size=2)
    with pytest.raises(ValueError, match="top_k \\* group_size <= HR_MAX_TOPK = 256"):
        search(top_k=129, group_by_field="doc_id", group_size=2)
    with pytest.raises(ValueError, match="top_k \\* group_size <= HR_MAX_TOPK = 256"):
        search(top_k=1, group_by_field="doc_id", group_size=257)
    with pytest.raises(ValueError, match="strict_group_size"):
        search(group_by_field="doc_id", group_size=2, strict_group_size="yes")
    with pytest.raises(ValueError, match="unknown group_by_field"):
        search(group_by_field="nope", group_size=2)
    with pytest.raises(ValueError, match="float"):
        search(group_by_field="entropy", group_size=2)
    # what passes the checks fails later, on the collection this unconnected manager does not have
    for ok in (dict(top_k=128, group_size=2), dict(top_k=1, group_size=256), dict(group_size=np.int64(3)),
               dict(group_size=2, strict_group_size=True), dict(group_size=2, strict_group_size=False), dict(group_size=1)):
        with pytest.raises(ValueError, match="Collection semantic_index not found"):
            search(group_by_field="doc_id", **ok)
    # without the option: today's refusal, word for word
    with pytest.raises(ValueError, match="group_size=2 is not supported: only group_size=1"):
        asyncio.run(MilvusIndexManager(connect=False).search(q, "semantic_index", 5, group_by_field="doc_id", group_size=2))
    assert MilvusIndexManager(connect=False).group_members is False


def test_range_bounds_with_grouping_stay_refused(host_manager):
    mgr, q, _ = host_manager
    with pytest.raises(ValueError, match="cannot be combined with group_by_field"):
        asyncio.run(mgr.search(q, "semantic_index", 5, search_params={"metric_type": "COSINE", "params": {"radius": 0.5}},
                               group_by_field="doc_id", group_size=2))


def test_group_window_values():
    w = MilvusIndexManager.group_window
    assert [w(k) for k in (1, 5, 64, 100, 256)] == [4, 20, 256, 256, 256] == [w(k, 1) for k in (1, 5, 64, 100, 256)]
    assert [w(k, 3) for k in (1, 5, 21, 22, 85)] == [12, 60, 252, 256, 256]
    with pytest.raises(ValueError, match="HR_MAX_TOPK"):
        w(257, 3)


def test_retrieval_config_validation():
    assert RetrievalConfig().group_size == 1 and RetrievalConfig(group_by_field="doc_id").group_size == 1
    assert RetrievalConfig(group_by_field="doc_id", group_size=3).group_size == 3
    with pytest.raises(ValueError, match="needs group_by_field"):
        RetrievalConfig(group_size=2)
    for bad in (0, -2, True, 2.0, "2"):
        with pytest.raises(ValueError, match="group_size must be an integer >= 1"):
            RetrievalConfig(group_by_field="doc_id", group_size=bad)
    profiles = HybridRetriever._build_default_profiles(RetrievalConfig(group_by_field="doc_id", group_size=2))
    assert all(p.group_size == 2 and p.group_by_field == "doc_id" for p in profiles.values())


class _Manager:
    def __init__(self, error=None):
        self.calls, self.error = [], error

    async def search(self, **kw):
        self.calls.append(kw)
        if self.error:
            raise self.error
        return []


class _Gen:
    def encode_semantic(self, text):
        return np.zeros(4, np.float32)

    def encode_sparse(self, text):
        return {"indices": [1], "values": [1.0]}


def test_retriever_passes_the_group_size_and_refuses_beyond_the_cap():
    m = _Manager()
    r = HybridRetriever(m, RetrievalConfig(group_by_field="doc_id"))
    asyncio.run(r._search_semantic(np.zeros(4), None))
    assert "group_size" not in m.calls[-1]                              # group_size = 1: the request of before
    r.config = RetrievalConfig(top_k=8, group_by_field="doc_id", group_size=4)
    asyncio.run(r._search_sparse({"indices": [1], "values": [1.0]}, None))
    assert m.calls[-1]["group_size"] == 4 and m.calls[-1]["top_k"] == 16 and m.calls[-1]["group_by_field"] == "doc_id"
    # 2 * top_k * group_size > 256: refused when the request is made, before any search
    m.embedding_generator = _Gen()
    r = HybridRetriever(m, RetrievalConfig(top_k=33, group_by_field="doc_id", group_size=4))
    n_calls = len(m.calls)
    with pytest.raises(ValueError, match="2 \\* top_k \\* group_size <= 256"):
        asyncio.run(r.retrieve("plain statement", profile_hint="default"))
    assert len(m.calls) == n_calls
    # the manager's refusal of group_size surfaces; with group_size = 1 a failing modality degrades to "no hits" as ever
    refusing = _Manager(ValueError("group_size=2 is not supported: only group_size=1"))
    r = HybridRetriever(refusing, RetrievalConfig(top_k=8, group_by_field="doc_id", group_size=2))
    with pytest.raises(ValueError, match="only group_size=1"):
        asyncio.run(r._search_semantic(np.zeros(4), None))
    r.config = RetrievalConfig(top_k=8, group_by_field="doc_id")
    assert asyncio.run(r._search_semantic(np.zeros(4), None)) == []


def test_fused_pass_keeps_the_first_g_hits_of_every_group():
    hits = [{"id": f"c{i}", "metadata": {"doc_id": d, "chunk_index": i % 2}} for i, d in enumerate("abacabbda")]
    f = HybridRetriever._first_per_group
    assert [h["id"] for h in f(list(hits), "doc_id", 2)] == ["c0", "c1", "c2", "c3", "c5", "c7"]
    assert [h["id"] for h in f(list(hits), "doc_id", 3)] == ["c0", "c1", "c2", "c3", "c4", "c5", "c6", "c7"]
    assert [h["id"] for h in f(list(hits), "chunk_index", 2)] == ["c0", "c1", "c2", "c3"]
    assert [h["id"] for h in f(list(hits), "doc_id", 1)] == [h["id"] for h in f(list(hits), "doc_id")] == ["c0", "c1", "c3", "c7"]
    assert len(f(list(hits), "chunk_id", 2)) == 9
    assert len(f([{"id": "x"}, {"id": "y", "metadata": None}], "doc_id", 2)) == 2     # no field: groups of their own


def test_pipeline_forwards_the_option_like_devices():
    from advanced_rag.pipeline import AdvancedRAGPipeline
    assert AdvancedRAGPipeline(connect_to_milvus=False, group_members=True).index_manager.group_members is True
    assert AdvancedRAGPipeline(connect_to_milvus=False).index_manager.group_members is False
