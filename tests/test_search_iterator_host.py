"""Search iterator, host side (no GPU): the key interval a cursor and range bounds become (indexing.cursor_key_interval, the
twin of deep_key_interval in csrc/deep.h) against the order it stands for, the page restatement (indexing.iterate_ranking),
and MilvusIndexManager.search_iterator over oracle-backed stand-ins for the shard handles (as tests/test_query_host.py
builds them): two shards that share one cursor, filters, tombstones and appends between pages, compaction, the refusals."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from advanced_rag import SearchIterator
from advanced_rag._native import f32_bound
from advanced_rag.indexing import (MilvusIndexManager, ShardCollection, cursor_key_interval, iterate_ranking, ord_f32,
                                   rank_key)
from advanced_rag.shards import ShardSet

from test_query_host import _OracleShard      # the oracle over the rows it was given: a ShardHandle without the cursor forms

EVERYTHING = (0, 2 ** 64 - 1)


def key(score, row):
    return int(rank_key(np.float32(score), row))


def inside(iv, score, row):
    return iv[0] < key(score, row) < iv[1]


# ---- cursor_key_interval ---------------------------------------------------------------------------------------------
def test_keys_order_as_the_ranking_does():
    f = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 0.25, 7.0, np.inf], np.float32)
    assert (np.diff(ord_f32(f).astype(np.int64)) > 0).all()                 # -0.0 below +0.0, everything else as floats
    assert key(0.5, 3) > key(0.5, 4) > key(0.25, 0)                         # score desc, then row asc <=> key desc
    assert key(-0.0, 0) < key(0.0, 2 ** 31 - 1)


def test_no_cursor_and_no_bounds_is_everything():
    for metric in ("COSINE", "IP", "L2"):
        assert cursor_key_interval(None, None, metric) == EVERYTHING
        assert cursor_key_interval(None, (None, None), metric) == EVERYTHING
    assert cursor_key_interval(None, (-np.inf, np.inf), "IP") == EVERYTHING
    assert cursor_key_interval(None, (np.inf, -np.inf), "L2") == EVERYTHING
    for s in (-3.0e38, -1.0, -0.0, 0.0, 1.0, 3.0e38):                       # every finite score, every row
        assert inside(EVERYTHING, s, 0) and inside(EVERYTHING, s, 2 ** 31 - 1)


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_rows_around_the_cursor_fall_on_the_right_sides(metric):
    sign = -1.0 if metric == "L2" else 1.0                                  # under L2 the cursor is a distance
    r = 1000
    iv = cursor_key_interval((sign * 0.5, r), None, metric)
    assert iv[0] == 0
    assert not inside(iv, 0.5, r - 1) and not inside(iv, 0.5, r) and inside(iv, 0.5, r + 1)
    assert not inside(iv, np.nextafter(np.float32(0.5), np.float32(1)), r + 1)      # a better score: before the cursor
    assert inside(iv, np.nextafter(np.float32(0.5), np.float32(0)), 0)              # a worse one: after it, whatever the row
    assert not inside(iv, 0.5, 0) and inside(iv, 0.5, 2 ** 31 - 1)


def test_a_cursor_is_a_position_not_a_row():
    off = 1_000_000
    below = cursor_key_interval((0.5, off - 5), None, "IP", off)            # a row below row_offset: every row of the score follows
    assert inside(below, 0.5, 0) and inside(below, 0.5, 2 ** 31 - 1)
    assert not inside(below, np.nextafter(np.float32(0.5), np.float32(1)), 2 ** 31 - 1)
    assert below == cursor_key_interval((0.5, -(2 ** 62)), None, "IP", off)
    beyond = cursor_key_interval((0.5, off + 2 ** 32 + 9), None, "IP", off)  # beyond the 32-bit rows: none of the score does
    assert not inside(beyond, 0.5, 2 ** 31 - 1) and inside(beyond, np.nextafter(np.float32(0.5), np.float32(0)), 0)
    assert beyond == cursor_key_interval((0.5, 2 ** 62), None, "IP", off)
    edge = cursor_key_interval((0.5, off + 2 ** 32 - 1), None, "IP", off)   # the last row of the key space
    assert edge[1] == int(ord_f32(0.5)) << 32
    mid = cursor_key_interval((0.5, off + 7), None, "IP", off)              # ids are rows + row_offset
    assert not inside(mid, 0.5, 7) and inside(mid, 0.5, 8)


def test_l2_negates_cursor_and_bounds():
    iv = cursor_key_interval((2.0, 5), (3.0, 1.0), "L2")                    # kept: 1 <= distance < 3, after (2.0, row 5)
    for d, row, want in ((2.0, 5, False), (2.0, 6, True), (2.0, 4, False), (1.5, 9, False), (2.5, 0, True), (3.0, 0, False),
                         (np.nextafter(np.float32(3), np.float32(0)), 0, True)):
        assert inside(iv, -np.float32(d), row) == want, (d, row)
    iv = cursor_key_interval(None, (3.0, 1.0), "L2")
    assert inside(iv, -1.0, 0) and not inside(iv, -np.nextafter(np.float32(1), np.float32(0)), 0) and not inside(iv, -3.0, 0)
    assert cursor_key_interval((0.0, 3), None, "L2") != cursor_key_interval((-0.0, 3), None, "L2")   # the cursor: bit for bit


def test_similarity_bounds_and_the_zero_rule():
    iv = cursor_key_interval(None, (0.25, 0.75), "COSINE")                  # kept: 0.25 < score <= 0.75
    assert not inside(iv, 0.25, 0) and inside(iv, np.nextafter(np.float32(0.25), np.float32(1)), 2 ** 31 - 1)
    assert inside(iv, 0.75, 0) and inside(iv, 0.75, 2 ** 31 - 1) and not inside(iv, np.nextafter(np.float32(0.75), np.float32(1)), 0)
    for zero in (0.0, -0.0):
        above = cursor_key_interval(None, (zero, None), "IP")               # score > 0: neither zero
        assert not inside(above, 0.0, 0) and not inside(above, -0.0, 0) and inside(above, 1e-45, 0)
        upto = cursor_key_interval(None, (None, zero), "IP")                # score <= 0: both zeros
        assert inside(upto, 0.0, 0) and inside(upto, -0.0, 2 ** 31 - 1) and not inside(upto, 1e-45, 0)
        near = cursor_key_interval(None, (None, zero), "L2")                # distance >= 0: both zeros (keys of -distance)
        assert inside(near, 0.0, 0) and inside(near, -0.0, 0) and inside(near, -1.0, 0)
        none = cursor_key_interval(None, (1.0, zero), "L2")
        assert inside(none, -0.0, 0) and inside(none, 0.0, 0) and not inside(none, -1.0, 0)
    assert cursor_key_interval(None, (0.0, None), "IP") == cursor_key_interval(None, (-0.0, None), "IP")


def test_a_float64_bound_cuts_the_fp32_scores_where_it_stands():
    s = np.float32(0.6)                                                     # 0.60000002..., the fp32 next to 0.6
    assert float(s) > 0.6 and f32_bound(0.6, False)[0] < s and f32_bound(0.6, True)[0] == s
    assert inside(cursor_key_interval(None, (0.6, None), "COSINE"), s, 0)            # 0.6 < score
    assert not inside(cursor_key_interval(None, (None, 0.6), "COSINE"), s, 0)        # score <= 0.6
    assert inside(cursor_key_interval(None, (None, 0.6), "L2"), -s, 0)               # distance >= 0.6
    assert not inside(cursor_key_interval(None, (0.6, None), "L2"), -np.nextafter(s, np.float32(1)), 0)
    assert inside(cursor_key_interval(None, (float(s) + 1e-12, None), "L2"), -s, 0)  # distance < a hair above s
    assert f32_bound(0.5, False)[0] == f32_bound(0.5, True)[0] == np.float32(0.5)
    assert f32_bound(1e300, False)[0] == np.finfo(np.float32).max and f32_bound(1e300, True)[0] == np.inf


def test_interval_refusals():
    for after in ((np.nan, 3), (np.inf, 3), (-np.inf, 3), (1e39, 3)):
        with pytest.raises(ValueError, match="non-finite"):
            cursor_key_interval(after, None, "IP")
    for bounds in ((np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError, match="NaN"):
            cursor_key_interval(None, bounds, "COSINE")
    for metric, bounds in (("COSINE", (0.5, 0.5)), ("IP", (0.7, 0.2)), ("L2", (1.0, 1.0)), ("L2", (1.0, 2.0)), ("IP", (np.inf, None)),
                           ("COSINE", (0.6, 0.6 + 1e-12))):                 # (the last: no fp32 between the two)
        with pytest.raises(ValueError, match="empty range"):
            cursor_key_interval(None, bounds, metric)
    with pytest.raises(ValueError, match="metric"):
        cursor_key_interval(None, None, "HAMMING")


def test_the_interval_is_the_walk_on_a_ranking_with_ties():
    """Feeding the last key back walks a tied ranking exactly once, in order (what the device selection is asked to do)."""
    rng = np.random.default_rng(3)
    scores = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0], np.float32), 400)
    keys = rank_key(scores, np.arange(400))
    order = np.argsort(keys)[::-1]
    seen, after = [], None
    while True:
        lo, hi = cursor_key_interval(after, None, "IP")
        page = [r for r in order if lo < int(keys[r]) < hi][:37]
        if not page:
            break
        seen += page
        after = (scores[page[-1]], page[-1])
    assert seen == order.tolist()


# ---- iterate_ranking ---------------------------------------------------------------------------------------------------
def test_iterate_ranking_pages():
    ids, sc = np.arange(10, 20), np.linspace(1, 0, 10, dtype=np.float32)
    pages = list(iterate_ranking(ids, sc, 4))
    assert [p[0].tolist() for p in pages] == [[10, 11, 12, 13], [14, 15, 16, 17], [18, 19]]
    assert np.array_equal(np.concatenate([p[1] for p in pages]), sc)
    assert [p[0].tolist() for p in iterate_ranking(ids, sc, 4, limit=6)] == [[10, 11, 12, 13], [14, 15]]
    assert [p[0].tolist() for p in iterate_ranking(ids, sc, 3, limit=3)] == [[10, 11, 12]]
    assert [len(p[0]) for p in iterate_ranking(ids, sc, 16384, limit=100)] == [10]
    padded = np.array([5, 6, 7, -1, -1])
    assert [p[0].tolist() for p in iterate_ranking(padded, np.zeros(5, np.float32), 2)] == [[5, 6], [7]]
    assert list(iterate_ranking(np.zeros(0, np.int64), np.zeros(0, np.float32), 5)) == []
    assert list(iterate_ranking(np.full(4, -1), np.zeros(4, np.float32), 5, limit=2)) == []
    for bad in (dict(batch_size=0), dict(batch_size=16385), dict(batch_size=2.0), dict(batch_size=True),
                dict(batch_size=2, limit=0), dict(batch_size=2, limit=1.5), dict(batch_size=2, limit=False)):
        with pytest.raises(ValueError):
            list(iterate_ranking(ids, sc, **bad))


# ---- the manager over stand-in shards ------------------------------------------------------------------------------------
N, DIM = 203, 12


def _rows(n, seed=17):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    X[rng.permutation(n)[: n // 4]] = X[3]                                  # a run of equal scores, spread over the shards
    return X


def _add(mgr, X, first):
    n = X.shape[0]
    mgr.add_rows(X, None, ids=[f"c{first + r}" for r in range(n)], contents=[f"text {first + r}" for r in range(n)],
                 doc_id=[f"doc{(first + r) // 10}" for r in range(n)], chunk_index=[(first + r) % 7 for r in range(n)])


def _manager(shards=2):
    X = _rows(N)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=0, connect=False, enable_domain=False, coalesce=False)
    mgr.attach_shards([_OracleShard() for _ in range(shards)])
    for lo in range(0, N, 80):                                              # several appends: the pieces interleave over the shards
        _add(mgr, X[lo:lo + 80], lo)
    assert isinstance(mgr._main, ShardSet) and mgr._filters_on_device() is None
    return mgr, X


def _want(mgr, X, q, mask=None):
    packed = None if mask is None else np.packbits(mask, bitorder="little")
    ids, sc = oracle.dense_search(X, q[None, :], X.shape[0], oracle.COSINE, packed)
    return mgr._format_hits(ids[0], sc[0])


def _walk(it):
    pages = []
    while True:
        page = it.next_blocking()
        if not page:
            return pages
        pages.append(page)


@pytest.fixture(scope="module")
def host():
    mgr, X = _manager()
    q = np.random.default_rng(5).standard_normal(DIM).astype(np.float32)
    yield mgr, X, q
    asyncio.run(mgr.close())


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("batch,limit", [(1, 9), (7, None), (50, 120), (203, None), (16384, None), (64, 203)])
def test_pages_concatenate_to_the_ranking(shards, batch, limit):
    mgr, X = _manager(shards)
    q = X[3] + np.float32(0.01)
    want = _want(mgr, X, q)[:limit]
    it = mgr.search_iterator(q, "semantic_index", batch_size=batch, limit=limit)
    assert isinstance(it, SearchIterator)
    pages = _walk(it)
    assert [h for p in pages for h in p] == want
    assert all(len(p) == batch for p in pages[:-1]) and it.returned == len(want)
    assert mgr.stats["iterator_pages"] >= len(pages) and it.next_blocking() == []
    ids = np.array([h["_row"] for h in want])
    assert [[h["_row"] for h in p] for p in pages] == [p[0].tolist() for p in iterate_ranking(ids, ids, batch, limit)]


def test_filters_range_async_and_the_collection_form(host):
    mgr, X, q = host
    chunk = np.arange(N) % 7
    want = _want(mgr, X, q, chunk >= 2)
    it = mgr.collections["semantic_index"].search_iterator(q, batch_size=40, filters="chunk_index >= 2")
    assert [h for p in _walk(it) for h in p] == want

    async def collect(**kw):
        return [page async for page in mgr.search_iterator(q, "semantic_index", **kw)]
    pages = asyncio.run(collect(batch_size=60, limit=150))
    assert [len(p) for p in pages] == [60, 60, 30] and [h for p in pages for h in p] == _want(mgr, X, q)[:150]
    # a range: every row with 0.1 < cosine <= 0.5, a result that has no top_k
    full = _want(mgr, X, q)
    ranged = [h for h in full if 0.1 < h["score"] <= 0.5]
    assert 10 < len(ranged) < N
    got = asyncio.run(collect(batch_size=9, search_params={"metric_type": "COSINE", "params": {"radius": 0.1, "range_filter": 0.5}}))
    assert [h for p in got for h in p] == ranged
    edge = ranged[4]["score"]                                               # bounds that sit on a score: exclusive below, inclusive above
    got = asyncio.run(collect(batch_size=16, search_params={"params": {"radius": edge, "range_filter": ranged[0]["score"]}}))
    assert [h for p in got for h in p] == [h for h in full if edge < h["score"] <= ranged[0]["score"]]


def test_mutations_between_pages():
    mgr, X = _manager()
    q = X[3] + np.float32(0.01)
    want = _want(mgr, X, q)
    it = mgr.search_iterator(q, "semantic_index", batch_size=30)
    first = it.next_blocking()
    assert first == want[:30]
    # a delete between pages: one row already returned, one not yet
    gone = [want[5]["_row"], want[40]["_row"]]
    asyncio.run(mgr.delete_by_filter("semantic_index", 'chunk_id in [' + ', '.join(f'"c{r}"' for r in gone) + ']'))
    second = it.next_blocking()
    assert second == [h for h in want[30:] if h["_row"] != gone[1]][:30]
    # an append between pages: a copy of the best row (before the cursor) and a copy of the worst (after it)
    extra = np.stack([X[want[0]["_row"]], X[want[-1]["_row"]]])
    _add(mgr, extra, N)
    alive = np.ones(N + 2, bool)
    alive[gone] = False
    now = _want(mgr, np.concatenate([X, extra]), q, alive)
    rest = [h for p in _walk(it) for h in p]
    seen = first + second + rest
    assert len({h["_row"] for h in seen}) == len(seen)                      # no hit twice
    assert N + 1 in [h["_row"] for h in rest] and N not in [h["_row"] for h in seen]
    cut = next(i for i, h in enumerate(now) if h["_row"] == second[-1]["_row"])
    assert rest == now[cut + 1:]                                            # the ranking as it is now, after the cursor
    # compact() renumbers the rows: an iterator from before refuses, a new one walks the new numbering
    it = mgr.search_iterator(q, "semantic_index", batch_size=50)
    assert len(it.next_blocking()) == 50
    generation = mgr._row_space_generation
    mgr.compact()
    assert mgr._row_space_generation == generation + 1
    with pytest.raises(RuntimeError, match=r"compact\(\)"):
        it.next_blocking()
    with pytest.raises(RuntimeError, match=r"compact\(\)"):
        asyncio.run(it.next())
    it.close()
    assert it.next_blocking() == [] and it.returned == 50
    fresh = [h for p in _walk(mgr.search_iterator(q, "semantic_index", batch_size=77)) for h in p]
    assert [h["id"] for h in fresh] == [h["id"] for h in now] and [h["score"] for h in fresh] == [h["score"] for h in now]
    asyncio.run(mgr.close())


def test_close_and_exhaustion(host):
    mgr, X, q = host
    it = mgr.search_iterator(q, "semantic_index", batch_size=10)
    assert len(it.next_blocking()) == 10
    pages = mgr.stats["iterator_pages"]
    it.close()
    assert it.next_blocking() == [] and asyncio.run(it.next()) == [] and it.returned == 10
    assert mgr.stats["iterator_pages"] == pages                             # a closed iterator launches nothing
    it = mgr.search_iterator(q, "semantic_index", batch_size=N)             # a full last page: the next one is empty, then none
    assert len(it.next_blocking()) == N and it.next_blocking() == [] and it.next_blocking() == []
    it = mgr.search_iterator(q, "semantic_index", batch_size=10, limit=10)  # limit reached: no further page is fetched
    pages = mgr.stats["iterator_pages"]
    assert len(it.next_blocking()) == 10 and it.next_blocking() == [] and mgr.stats["iterator_pages"] == pages + 1
    # bounds that differ as float64 with no fp32 score between them: an empty ranking, as search() finds it
    it = mgr.search_iterator(q, "semantic_index", search_params={"params": {"radius": 0.6, "range_filter": 0.6 + 1e-12}})
    assert it.next_blocking() == []


def test_creation_refusals(host):
    mgr, X, q = host
    for kw, word in ((dict(batch_size=0), "batch_size"), (dict(batch_size=16385), "batch_size"), (dict(batch_size=-1), "batch_size"),
                     (dict(batch_size=True), "batch_size"), (dict(batch_size=100.0), "batch_size"), (dict(batch_size="9"), "batch_size"),
                     (dict(batch_size=None), "batch_size"), (dict(limit=0), "limit"), (dict(limit=-4), "limit"),
                     (dict(limit=2.5), "limit"), (dict(limit=False), "limit"),
                     (dict(search_params={"metric_type": "L2"}), "metric_type"),
                     (dict(search_params={"params": {"radius": 0.9, "range_filter": 0.1}}), "empty range"),
                     (dict(search_params={"params": {"radius": float("nan")}}), "NaN"),
                     (dict(search_params={"params": {"radius": "0.3"}}), "radius")):
        with pytest.raises(ValueError, match=word):
            mgr.search_iterator(q, "semantic_index", **kw)
        with pytest.raises(ValueError, match=word):
            mgr.collections["semantic_index"].search_iterator(q, **kw)
    with pytest.raises(ValueError, match="not found"):
        mgr.search_iterator(q, "no_such_index")
    assert mgr.search_iterator(q, "semantic_index", batch_size=np.int64(16384), limit=np.int32(1)).batch_size == 16384
    pages = mgr.stats["iterator_pages"]
    # range params on the sparse collection, and the torchrun form
    mgr.collections["sparse_index"] = ShardCollection(mgr, "sparse_index", "sparse", mgr._main, 16, "IP")
    try:
        with pytest.raises(ValueError, match="sparse"):
            mgr.search_iterator({"indices": [1], "values": [1.0]}, "sparse_index", search_params={"params": {"radius": 0.1}})
    finally:
        del mgr.collections["sparse_index"]
    mgr.collections["spread"] = SimpleNamespace(kind="dense", metric="COSINE", name="spread", handle=SimpleNamespace(round=lambda *a: None))
    try:
        with pytest.raises(NotImplementedError, match="torchrun"):
            mgr.search_iterator(q, "spread")
    finally:
        del mgr.collections["spread"]
    assert mgr.stats["iterator_pages"] == pages                             # nothing was launched for any of them
