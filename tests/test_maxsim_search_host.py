"""MaxSim as a first-stage search without a GPU: the restatement (maxsim.maxsim_search_csr) against an exactly rounded
chain built with `fractions`, the ties the fp32 score makes, exclusions, paging, and manager.maxsim_search over the
oracle-backed stand-ins of test_maxsim_host.py (one shard and three), which take the restatement over the host column."""
import asyncio
import types
from fractions import Fraction

import numpy as np
import pytest

import test_maxsim_host as mh
from advanced_rag import _native as nat
from advanced_rag import maxsim as M
from advanced_rag.indexing import QUERY_MAX_WINDOW

TD = mh.TD


def _store(T, dim, rng, scale=1.0):
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    return indptr, (rng.standard_normal((int(indptr[-1]), dim)) * scale).astype(np.float16)


def _exact_ranking(q, indptr, vals, mask):
    """[(row, fp32 score)] by (score desc, row asc): every fma of the chain rounded once from the exact rational, the fp64
    sum in Python floats, one exact rounding to fp32 at the end."""
    hits = []
    for r in range(len(indptr) - 1):
        doc = vals[indptr[r]:indptr[r + 1]]
        if len(doc) == 0 or (mask is not None and not mask[r]):
            continue
        S = 0.0
        for t in range(len(q)):
            S = S + float(max(mh._exact_chain(q[t], doc[u]) for u in range(len(doc))))
        hits.append((r, mh._round_f32(Fraction(S))))
    return sorted(hits, key=lambda h: (-h[1], h[0]))


def test_search_equals_the_exactly_rounded_chain():
    rng = np.random.default_rng(17)
    T = [2, 0, 3, 1, 5, 0, 4, 1, 2, 3, 1, 2]                     # 12 rows, two of them without vectors
    for scale in (1.0, 37.0, 0.01):
        indptr, vals = _store(T, 8, rng, scale)
        q = (rng.standard_normal((3, 8)) * scale).astype(np.float16)
        for mask in (None, rng.random(12) < 0.6):
            want = _exact_ranking(q, indptr, vals, mask)
            ids, sc = M.maxsim_search_csr(q, indptr, vals, mask, 12)
            assert ids.dtype == np.int64 and sc.dtype == np.float32
            assert ids.tolist() == [r for r, _ in want] and sc.tolist() == [s for _, s in want]
            ids, sc = M.maxsim_search_csr(q, indptr, vals, mask, 4, offset=2, first_row=100)
            assert ids.tolist() == [r + 100 for r, _ in want[2:6]] and sc.tolist() == [s for _, s in want[2:6]]


def planted_tie(dim=8, rows=12):
    """Row 3 has S = 1.0, row 7 has S = 1 + 2^-30 (m_0 = 1.0; m_1 = 2^-30 from two fp16 elements of 2^-15, whose product is
    exact in fp32): both score 1.0f.  The other rows with tokens score 0.5 or 0.25; rows 1 and 5 hold no vectors."""
    tiny = np.float16(2.0 ** -15)
    assert float(tiny) == 2.0 ** -15
    q = np.zeros((2, dim), np.float16)
    q[0, 0], q[1, 1] = 1.0, tiny
    T = np.ones(rows, dtype=np.int64)
    T[[1, 5]] = 0
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    vals = np.zeros((int(indptr[-1]), dim), np.float16)
    for r in range(rows):
        if T[r]:
            vals[indptr[r], 0] = 0.5 if r % 2 else 0.25
    vals[indptr[3], 0] = 1.0
    vals[indptr[7], 0], vals[indptr[7], 1] = 1.0, tiny
    return q, indptr, vals


def test_planted_fp32_tie_orders_by_row_and_the_rerank_by_fp64():
    q, indptr, vals = planted_tie()
    S = M.maxsim_scores_csr(q, indptr, vals, [3, 7])
    assert S.tolist() == [1.0, 1.0 + 2.0 ** -30] and S[0] < S[1]
    ids, sc = M.maxsim_search_csr(q, indptr, vals, None, 2)
    assert ids.tolist() == [3, 7] and sc.tolist() == [1.0, 1.0]              # the first stage: a tie, row ascending
    pos, rid, fin = M.maxsim_rerank_csr([3, 7], q, indptr, vals, 0, 2)
    assert pos == [1, 0] and rid == [7, 3] and fin == [1.0 + 2.0 ** -30, 1.0]   # the rerank: the fp64 order


def duplicate_rows(dim=16, rows=20, seed=2):
    """Rows 4, 9, 10 and 15 hold the same token vectors; the rest are random."""
    rng = np.random.default_rng(seed)
    T = np.full(rows, 3)
    indptr, vals = _store(T, dim, rng)
    for r in (9, 10, 15):
        vals[indptr[r]:indptr[r + 1]] = vals[indptr[4]:indptr[5]]
    q = vals[indptr[4]:indptr[5]].copy()                         # the duplicates' own tokens: they rank at the top
    return q, indptr, vals


def test_duplicate_rows_straddling_the_cut():
    q, indptr, vals = duplicate_rows()
    full, fs = M.maxsim_search_csr(q, indptr, vals, None, 20)
    assert full[:4].tolist() == [4, 9, 10, 15] and len(set(fs[:4].tolist())) == 1 and fs[4] < fs[3]
    for k in (1, 2, 3):
        ids, sc = M.maxsim_search_csr(q, indptr, vals, None, k)
        assert ids.tolist() == [4, 9, 10][:k] and sc.tolist() == fs[:k].tolist()
    ids, _ = M.maxsim_search_csr(q, indptr, vals, None, 2, offset=2)
    assert ids.tolist() == [10, 15]


def test_exclusions_paging_and_a_short_ranking():
    rng = np.random.default_rng(3)
    T = np.array([0, 1, 15, 16, 17, 33, 100] * 5)
    indptr, vals = _store(T, 24, rng)
    q = rng.standard_normal((17, 24)).astype(np.float16)
    mask = rng.random(len(T)) < 0.5
    ids, sc = M.maxsim_search_csr(q, indptr, vals, mask, 1000)
    allowed = np.flatnonzero(mask & (T > 0))
    assert sorted(ids.tolist()) == allowed.tolist() and len(ids) < len(T)         # a short ranking gives a short list
    assert sc.tolist() == M.maxsim_scores_csr(q, indptr, vals, ids).astype(np.float32).tolist()
    assert all((sc[i] > sc[i + 1]) or (sc[i] == sc[i + 1] and ids[i] < ids[i + 1]) for i in range(len(ids) - 1))
    pages = [M.maxsim_search_csr(q, indptr, vals, mask, 4, offset=o) for o in range(0, len(ids) + 4, 4)]
    assert np.concatenate([p[0] for p in pages]).tolist() == ids.tolist()
    assert np.concatenate([p[1] for p in pages]).tolist() == sc.tolist()
    assert len(pages[-1][0]) == 0
    assert len(M.maxsim_search_csr(q, indptr, vals, np.zeros(len(T), bool), 5)[0]) == 0
    short = M.maxsim_search_csr(q, indptr, vals, np.ones(10, bool), 1000)[0]       # rows beyond the mask do not pass
    assert sorted(short.tolist()) == np.flatnonzero(T[:10] > 0).tolist()
    empty = M.maxsim_search_csr(q, np.zeros(1, np.int64), vals[:0], None, 5)
    assert len(empty[0]) == 0 and empty[1].dtype == np.float32
    zero = M.maxsim_search_csr(q[:0], indptr, vals, None, 1000)                     # no query tokens: every hit scores +0.0
    assert zero[0].tolist() == np.flatnonzero(T > 0).tolist() and not zero[1].any() and not np.signbit(zero[1]).any()


# ---- the manager over stand-ins -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 3])
def host(request):
    mgr, X, csr, indptr, vals = mh._manager(request.param)
    assert mgr._filters_on_device() is None
    yield mgr
    asyncio.run(mgr.close())


def _want(mgr, qt, keep, top_k, offset=0):
    col = mgr._cols.token_vectors()
    return M.maxsim_search_csr(np.asarray(qt, np.float32).astype(np.float16), col.indptr(), col.values(), keep, top_k, offset)


def _check(mgr, qt, keep, top_k, offset=0, **kw):
    before = dict(mgr.stats)
    hits = asyncio.run(mgr.maxsim_search(qt, top_k, offset=offset, **kw))
    ids, sc = _want(mgr, qt, keep, top_k, offset)
    assert [h["_row"] for h in hits] == ids.tolist() and [h["score"] for h in hits] == sc.astype(np.float64).tolist()
    assert [h["id"] for h in hits] == [mgr._cols["id"][r] for r in ids.tolist()]
    assert mgr.stats["maxsim_host_searches"] == before["maxsim_host_searches"] + 1
    assert mgr.stats["maxsim_searches"] == before["maxsim_searches"]
    return hits


def test_manager_returns_the_restatements_rows(host):
    mgr = host
    n = mgr.num_rows
    qt = mh._query_tokens(21, 9)
    hits = _check(mgr, qt, None, 20)
    assert len(hits) == 20 and set(hits[0]) >= {"id", "content", "score", "metadata", "_row"}
    plain = asyncio.run(mgr.search(np.ones(mgr.semantic_dim, np.float32), "semantic_index", 1))[0]
    assert set(hits[0]) == set(plain)                                          # the dicts search() returns
    assert not any(60 <= h["_row"] < 120 or h["_row"] % 7 == 0 for h in hits)  # rows without vectors are no hits
    _check(mgr, mh._query_tokens(22, 1), None, 7, offset=3)
    _check(mgr, mh._query_tokens(23, 64), None, n)                             # deeper than the ranking: a short list
    keep = np.arange(n) % 10 < 5
    filtered = _check(mgr, qt, keep, 15, filters="chunk_index < 5")
    assert filtered and all(h["metadata"]["chunk_index"] < 5 for h in filtered)
    pages = [asyncio.run(mgr.maxsim_search(qt, 6, "chunk_index < 5", offset=o)) for o in (0, 6, 12)]
    whole = asyncio.run(mgr.maxsim_search(qt, 18, "chunk_index < 5"))
    assert [h["id"] for p in pages for h in p] == [h["id"] for h in whole]
    assert _check(mgr, qt, np.zeros(n, bool), 5, filters="chunk_index > 50") == []


def test_manager_honours_tombstones():
    mgr, *_ = mh._manager(3)
    try:
        n = mgr.num_rows
        qt = mh._query_tokens(31, 12)
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 2"))
        alive = np.arange(n) % 10 != 2
        hits = _check(mgr, qt, alive, 40)
        assert all(h["metadata"]["chunk_index"] != 2 for h in hits)
        _check(mgr, qt, alive & (np.arange(n) % 10 < 5), 40, filters="chunk_index < 5")
    finally:
        asyncio.run(mgr.close())


def test_refusals(host):
    mgr = host
    qt = mh._query_tokens(1, 4)
    run = lambda *a, **kw: asyncio.run(mgr.maxsim_search(*a, **kw))
    before = dict(mgr.stats)
    for bad in (np.ones(TD), np.ones((0, TD)), np.ones((65, TD)), np.ones((2, TD + 8)), np.full((2, TD), np.nan),
                np.full((2, TD), 1e6), [["a"] * TD]):
        with pytest.raises(ValueError):
            run(bad)
    for kw in (dict(top_k=0), dict(top_k=True), dict(top_k=2.0), dict(offset=-1), dict(offset=1.5),
               dict(top_k=QUERY_MAX_WINDOW, offset=1), dict(top_k=QUERY_MAX_WINDOW + 1)):
        with pytest.raises(ValueError):
            run(qt, **kw)
    for expr in ("chunk_index <", "no_such_field == 3", "chunk_index == 'x' and"):
        with pytest.raises(ValueError):
            run(qt, 5, expr)
    coll = mgr.collections["semantic_index"]
    real, coll.handle = coll.handle, types.SimpleNamespace(round=None)          # the torchrun form's mark
    try:
        with pytest.raises(NotImplementedError):
            run(qt)
    finally:
        coll.handle = real
    assert mgr.stats == before                                                  # nothing ran
    assert len(run(qt, QUERY_MAX_WINDOW)) <= mgr.num_rows                       # the cap itself is served
    assert "hr_maxsim_scan_dev" in nat.EXPORTED_SYMBOLS and QUERY_MAX_WINDOW == nat.HR_MAX_DEEP_K


def test_a_manager_without_token_dim_refuses():
    mgr, *_ = mh._manager(1, token_dim=None)
    try:
        with pytest.raises(ValueError, match="token_dim"):
            asyncio.run(mgr.maxsim_search(mh._query_tokens(1, 4)))
        assert mgr.stats["maxsim_host_searches"] == 0 and mgr.stats["maxsim_searches"] == 0
    finally:
        asyncio.run(mgr.close())
