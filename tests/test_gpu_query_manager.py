"""MilvusIndexManager.query on the GPU: a one-shard manager (the mask stays in HBM, hr_mask_rows_dev makes the page) and a
devices=[0, 0] manager (host view of the mask, ShardSet.get_dense_rows) must return identical lists, payloads, vectors
and counts, and both must equal the numpy restatement — with doc_id values longer than 16 bytes that share their
prefixes (the filter's undecided path), tombstones, paging, limit=None, count(*), and after compact()."""
import asyncio

import numpy as np
import pytest

from advanced_rag import MilvusIndexManager, filters

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, DD = 2011, 32, 16
EXPRS = ['chunk_index >= 4 and entropy < 0.5 and doc_id >= "corpus/shared-prefix/doc-0100"',
         'doc_id in ["corpus/shared-prefix/doc-0007", "corpus/shared-prefix/doc-0150", "corpus/shared-prefix/doc-0200", "corpus/shared-prefix/doc-9999"]',
         '(doc_id == "corpus/shared-prefix/doc-0033" or token_count > 1900) and not (chunk_index in [1, 2])']
DELETE = 'chunk_index == 7 or doc_id == "corpus/shared-prefix/doc-0150"'
FIELDS = ["doc_id", "content", "chunk_index", "token_count", "entropy", "redundancy", "domain_density", "metadata_json", "timestamp"]


def _payload():
    return dict(ids=[f"chunk-{r:05d}" for r in range(N)], contents=[f"text {r}" for r in range(N)],
                doc_id=[f"corpus/shared-prefix/doc-{r // 10:04d}" for r in range(N)],      # 16 bytes alike, then the number
                chunk_index=[r % 10 for r in range(N)], token_count=list(range(N)), entropy=[(r % 8) / 8.0 for r in range(N)],
                redundancy=[(r % 4) / 4.0 for r in range(N)], domain_density=[(r % 16) / 16.0 for r in range(N)],
                timestamp=[f"2024-01-{1 + r % 28:02d}" for r in range(N)], metadata_json=[f"{{'r': {r}}}" for r in range(N)])


def _columns(p):
    cols = {k: np.asarray(p[k], dtype=np.int64) for k in ("chunk_index", "token_count")}
    cols.update({k: np.asarray(p[k], dtype=np.float32) for k in ("entropy", "redundancy", "domain_density")})
    cols.update(id=np.asarray(p["ids"]), chunk_id=np.asarray(p["ids"]), doc_id=np.asarray(p["doc_id"]), timestamp=np.asarray(p["timestamp"]))
    return cols


def _manager(X, XD, p, **kw):
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, domain_dim=DD, enable_domain=True, **kw)
    for lo in range(0, N, 700):
        hi = min(N, lo + 700)
        mgr.add_rows(X[lo:hi], None, ids=p["ids"][lo:hi], contents=p["contents"][lo:hi],
                     **{k: v[lo:hi] for k, v in p.items() if k not in ("ids", "contents")})
        mgr._domain.add(XD[lo:hi])
    mgr.finalize()
    return mgr


@pytest.fixture(scope="module")
def world(gpu):
    rng = np.random.default_rng(41)
    X = rng.standard_normal((N, D)).astype(np.float32)
    XD = rng.standard_normal((N, DD)).astype(np.float32)
    p = _payload()
    one = _manager(X, XD, p)
    two = _manager(X, XD, p, devices=[0, 0])
    assert one._main.n_shards == 1 and two._main.n_shards == 2

    def never(expr):
        raise AssertionError("the one-shard path read the mask back")
    one._row_mask = never
    yield one, two, X.astype(np.float16).astype(np.float32), XD.astype(np.float16).astype(np.float32), p
    for m in (one, two):
        asyncio.run(m.close())


def _want(p, expr, deleted, offset=0, limit=None):
    keep = filters.evaluate(expr, _columns(p), N) if expr else np.ones(N, bool)
    rows = np.flatnonzero(keep & ~deleted)
    return rows[offset:] if limit is None else rows[offset:offset + limit]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for k in x:
            assert (np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype) if k == "embedding" else x[k] == y[k], k


def _check(one, two, stored, stored_dom, p, deleted):
    """Every kind of query of this file on both managers against the restatement; -> the one-shard answers."""
    q = lambda m, coll, *a, **kw: asyncio.run(m.query(coll, *a, **kw))
    ids_of = lambda rows: [p["ids"][r] for r in rows]
    answers = []
    for expr in EXPRS + [None]:
        rows = _want(p, expr, deleted)
        assert len(rows) > 0
        before = dict(one.stats)
        a, b = q(one, "semantic_index", expr, limit=N), q(two, "semantic_index", expr, limit=N)
        assert one.stats["queries"] == before["queries"] + 1 and one.stats["query_device"] == before["query_device"] + 1
        assert two.stats["query_device"] == 0
        _same(a, b)
        assert [h["id"] for h in a] == ids_of(rows)
        for m in (one, two):
            assert q(m, "semantic_index", expr, ["count(*)"]) == [{"count(*)": len(rows)}]
            assert q(m, "domain_index", expr, ["count(*)"]) == [{"count(*)": len(rows)}]
        if expr is not None:                       # limit=None: count first, then everything after the offset
            for offset in (0, 3, len(rows) - 1, len(rows), len(rows) + 9):
                a, b = q(one, "semantic_index", expr, offset=offset), q(two, "semantic_index", expr, offset=offset)
                _same(a, b)
                assert [h["id"] for h in a] == ids_of(rows[offset:])
        got, offset = [], 0                        # pages concatenate
        while True:
            a, b = q(one, "semantic_index", expr, ["token_count"], 64, offset), q(two, "semantic_index", expr, ["token_count"], 64, offset)
            _same(a, b)
            got += [h["id"] for h in a]
            offset += 64
            if len(a) < 64:
                break
        assert got == ids_of(rows)
        # payload and vectors of both dense collections
        a, b = q(one, "semantic_index", expr, FIELDS + ["embedding"], 100, 5), q(two, "semantic_index", expr, FIELDS + ["embedding"], 100, 5)
        _same(a, b)
        page = rows[5:105]
        assert len(a) == len(page)
        for h, r in zip(a, page):
            assert h["embedding"].dtype == np.float32 and np.array_equal(h["embedding"], stored[r])
            assert [h[f] for f in ("id", "doc_id", "chunk_index", "token_count", "timestamp", "metadata_json", "content")] == \
                [p["ids"][r], p["doc_id"][r], p["chunk_index"][r], p["token_count"][r], p["timestamp"][r], p["metadata_json"][r], p["contents"][r]]
            assert (h["entropy"], h["redundancy"], h["domain_density"]) == ((r % 8) / 8.0, (r % 4) / 4.0, (r % 16) / 16.0)
        c, d = q(one, "domain_index", expr, ["embedding"], 40), q(two, "domain_index", expr, ["embedding"], 40)
        _same(c, d)
        assert len(c) == min(40, len(rows)) and all(np.array_equal(h["embedding"], stored_dom[r]) for h, r in zip(c, rows[:40]))
        answers.append((a, c))
    return answers


def test_one_shard_and_two_shards_equal_the_restatement(world):
    one, two, stored, stored_dom, p = world
    none = np.zeros(N, bool)
    _check(one, two, stored, stored_dom, p, none)
    assert one._filters_on_device().stats["undecided_rows"] > 0           # the shared 16-byte prefixes were settled on the host
    # tombstones
    for m in (one, two):
        asyncio.run(m.delete_by_filter("semantic_index", DELETE))
    deleted = filters.evaluate(DELETE, _columns(p), N)
    assert 0 < deleted.sum() < N
    before = _check(one, two, stored, stored_dom, p, deleted)
    # compact(): the rows are renumbered, the same ids and the same vectors come back
    for m in (one, two):
        out = m.compact()
        assert out["rows_after"] == N - int(deleted.sum())
    survivors = np.flatnonzero(~deleted)
    assert asyncio.run(one.query("semantic_index", None, ["count(*)"])) == [{"count(*)": len(survivors)}]
    q = lambda m, *a, **kw: asyncio.run(m.query(*a, **kw))
    for (a_before, c_before), expr in zip(before, EXPRS + [None]):
        a, b = q(one, "semantic_index", expr, FIELDS + ["embedding"], 100, 5), q(two, "semantic_index", expr, FIELDS + ["embedding"], 100, 5)
        _same(a, b)
        _same(a, a_before)
        c, d = q(one, "domain_index", expr, ["embedding"], 40), q(two, "domain_index", expr, ["embedding"], 40)
        _same(c, d)
        _same(c, c_before)
    assert one.stats["query_device"] == one.stats["queries"] and two.stats["query_device"] == 0


def test_refusals(world):
    one, two, *_ = world
    for m in (one, two):
        with pytest.raises(ValueError):
            asyncio.run(m.query("semantic_index", None))
        with pytest.raises(ValueError):
            asyncio.run(m.query("semantic_index", "chunk_index == 1", ["nope"]))
        with pytest.raises(ValueError):
            asyncio.run(m.query("semantic_index", "chunk_index == 1", limit=16384, offset=1))
        with pytest.raises(ValueError):
            asyncio.run(m.query("semantic_index", "no_such_field == 1", limit=5))
