"""MaxSim as a first-stage search on the device: hr_maxsim_scan_dev against np.float32(maxsim_scores_csr) for every cell
of its two outputs, the scan followed by hr_deep_topk_dev against maxsim.maxsim_search_csr, the entry point's refusals, and
manager.maxsim_search on a real one-shard manager.  Every comparison is == / array_equal: the inputs are finite fp16 by
construction, so the restatement alone decides every value.  Outputs are sentinel-filled before every launch."""
import asyncio
import functools

import numpy as np
import pytest

from advanced_rag import MilvusIndexManager
from advanced_rag import _native as nat
from advanced_rag import maxsim as M
from advanced_rag.maxsim import MaxSimRanker
from test_maxsim_search_host import duplicate_rows, planted_tie

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7
ROW_TOKENS = (0, 1, 15, 16, 17, 33, 100)         # an empty row, both sides of the 16-token tile, a long row
QN = (1, 16, 17, 64, 0)                          # d_qn of the five queries; tq_stride = 64


def make_store(rng, rows, dim):
    """`rows` rows whose token counts cycle through ROW_TOKENS in a shuffled order."""
    T = np.array([ROW_TOKENS[i % len(ROW_TOKENS)] for i in range(rows)])
    rng.shuffle(T)
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    return indptr, rng.standard_normal((int(indptr[-1]), dim)).astype(np.float16)


def pack(bits):
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")


def bits_at(n, rows):
    m = np.zeros(n, dtype=bool)
    m[[r for r in rows if r < n]] = True
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def token_tensors(indptr, vals, tok_rows):
    """(indptr, values) of the first tok_rows rows on the device; a store without tokens still gets a pointer."""
    if tok_rows == 0:
        return None, None
    t_v = dev(vals[:max(int(indptr[tok_rows]), 1)].view(np.int16).reshape(-1)) if len(vals) else torch.zeros(8, dtype=torch.int16, device="cuda")
    return dev(indptr[:tok_rows + 1]), t_v


def run_scan(qtok, qn, indptr, vals, tok_rows, n_rows, mask):
    """-> (scores fp32 [B, n_rows], rows int32 [B, n_rows]) of one launch over sentinel-filled outputs."""
    B = qtok.shape[0]
    t_q, t_qn = dev(qtok.view(np.int16)), dev(np.asarray(qn, dtype=np.int32))
    t_ip, t_v = token_tensors(indptr, vals, tok_rows)
    t_m = dev(pack(mask)) if mask is not None else None
    sc = torch.full((B, n_rows), float(SENT), dtype=torch.float32, device="cuda")
    rw = torch.full((B, n_rows), SENT, dtype=torch.int32, device="cuda")
    nat.maxsim_scan_dev(t_q.data_ptr(), t_qn.data_ptr(), B, qtok.shape[1], qtok.shape[2], t_ip.data_ptr() if tok_rows else 0,
                        t_v.data_ptr() if tok_rows else 0, tok_rows, n_rows, t_m.data_ptr() if mask is not None else 0,
                        sc.data_ptr(), rw.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), rw.cpu().numpy()


def all_scores(qtok, qn, indptr, vals):
    """S (fp64 [B, store rows]) of every query and every row of the store, by the restatement."""
    rows = np.arange(len(indptr) - 1)
    return np.stack([M.maxsim_scores_csr(qtok[q, :min(max(int(qn[q]), 0), qtok.shape[1])], indptr, vals, rows) for q in range(len(qn))])


def want_scan(S, indptr, tok_rows, n_rows, mask):
    """The header's table from S: a hit writes (i, (float)S), everything else (-1, 0.0f)."""
    hit = np.zeros(n_rows, dtype=bool)
    m = min(n_rows, tok_rows)
    hit[:m] = np.diff(indptr)[:m] > 0
    if mask is not None:
        hit &= np.asarray(mask, dtype=bool)[:n_rows]
    S_n = np.zeros((S.shape[0], n_rows), dtype=np.float64)
    c = min(n_rows, S.shape[1])
    S_n[:, :c] = S[:, :c]
    sc = np.where(hit, S_n.astype(np.float32), np.float32(0.0))
    rw = np.where(hit, np.arange(n_rows, dtype=np.int32), np.int32(-1))
    return sc, np.broadcast_to(rw, sc.shape)


def check_scan(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    assert not (np.signbit(got[0]) & (got[0] == 0)).any()          # never -0.0


@functools.lru_cache(maxsize=None)
def small_case(dim):
    rng = np.random.default_rng(dim)
    indptr, vals = make_store(rng, 70, dim)
    qtok = rng.standard_normal((5, 64, dim)).astype(np.float16)
    return qtok, indptr, vals, all_scores(qtok, QN, indptr, vals)


@functools.lru_cache(maxsize=None)
def large_case():
    rng = np.random.default_rng(1000)
    indptr, vals = make_store(rng, 1100, 72)
    qtok = rng.standard_normal((5, 64, 72)).astype(np.float16)
    return qtok, indptr, vals, all_scores(qtok, QN, indptr, vals)


def test_version(gpu):
    assert nat.load_library().hr_version() >= 12200


@pytest.mark.parametrize("dim", [8, 72, 256])
def test_scan_equals_the_restatement(gpu, dim):
    """B = 5 with d_qn = 1, 16, 17, 64 and 0 at tq_stride 64; n_rows on both sides of a wave's 64 lanes; tok_rows larger
    and smaller than n_rows; the four kinds of mask."""
    qtok, indptr, vals, S = small_case(dim)
    rng = np.random.default_rng(dim + 1)
    for n_rows in (1, 63, 64, 65, 70):
        masks = [None, np.zeros(n_rows, bool), rng.random(n_rows) < 0.5, bits_at(n_rows, (63, 64, 65, n_rows - 1))]
        for tok_rows in (70, 40):
            for mask in masks:
                got = run_scan(qtok, QN, indptr, vals, tok_rows, n_rows, mask)
                check_scan(got, want_scan(S, indptr, tok_rows, n_rows, mask))
    got = run_scan(qtok[:1], QN[:1], indptr, vals, 70, 70, None)                 # B = 1
    check_scan(got, want_scan(S[:1], indptr, 70, 70, None))
    assert (got[1][0] >= 0).sum() == (np.diff(indptr) > 0).sum() and got[0].any()
    zero_q = run_scan(qtok[4:], QN[4:], indptr, vals, 70, 70, None)              # d_qn = 0: hits stay hits, scored +0.0f
    assert np.array_equal(zero_q[1], got[1]) and not zero_q[0].any()


@pytest.mark.parametrize("B", [1, 5])
def test_scan_of_a_thousand_rows(gpu, B):
    """n_rows = 1 000 over a store of 1 100 rows and of 900 rows (n_rows beyond the store), many blocks."""
    qtok, indptr, vals, S = large_case()
    rng = np.random.default_rng(B)
    n_rows = 1000
    for tok_rows, mask in ((1100, None), (1100, rng.random(n_rows) < 0.3), (900, bits_at(n_rows, (63, 64, 65, n_rows - 1))),
                           (900, None), (1100, np.zeros(n_rows, bool))):
        got = run_scan(qtok[:B], QN[:B], indptr, vals, tok_rows, n_rows, mask)
        check_scan(got, want_scan(S[:B], indptr, tok_rows, n_rows, mask))


def test_a_walk_of_several_trips(gpu):
    """About 3 000 rows with the grid capped at 3 blocks per query behind hr_debug_option(HR_DEBUG_MAXSIM_SCAN_BLOCKS): the
    range size follows the cap (256 rows, a full 64-lane piece per wave), so every block walks four ranges.  The default
    launch of the same store (ranges of 32 rows, one per block) must give the same cells."""
    rng = np.random.default_rng(30)
    indptr, vals = make_store(rng, 3001, 24)
    qtok = rng.standard_normal((2, 20, 24)).astype(np.float16)
    qn = (20, 7)
    S = all_scores(qtok, qn, indptr, vals)
    mask = rng.random(3001) < 0.7
    try:
        nat.debug_option(nat.HR_DEBUG_MAXSIM_SCAN_BLOCKS, 3)
        capped = [run_scan(qtok, qn, indptr, vals, 3001, 3001, m) for m in (None, mask)]
    finally:
        nat.debug_option(nat.HR_DEBUG_MAXSIM_SCAN_BLOCKS, 0)
    plain = [run_scan(qtok, qn, indptr, vals, 3001, 3001, m) for m in (None, mask)]
    for got_c, got_p, m in zip(capped, plain, (None, mask)):
        want = want_scan(S, indptr, 3001, 3001, m)
        check_scan(got_c, want)
        check_scan(got_p, want)
    with pytest.raises(ValueError):
        nat.debug_option(nat.HR_DEBUG_MAXSIM_SCAN_BLOCKS, -1)


# ---- scan + selection -------------------------------------------------------------------------------------------------------
FIRST_ROW = 1000


@functools.lru_cache(maxsize=None)
def ranked_store():
    """400 rows, dim 8.  Query 0 is the planted-tie query (column 0, and 2^-15 times column 1): rows 3 and 7 tie at 1.0f
    (ranks 0 and 1), six single rows follow, then four identical rows (ranks 8 .. 11: a cut at 10 splits them); every
    other row's column 0 lies below 0.9.  Query 1 is random."""
    rng = np.random.default_rng(8)
    q0, _, _ = planted_tie(dim=8)
    indptr, vals = make_store(rng, 400, 8)
    vals[:, 0] = (rng.random(len(vals)) * 0.85).astype(np.float16)
    vals[:, 1] = 0
    T = np.diff(indptr)
    single = np.flatnonzero(T == 1)
    assert len(single) > 20
    tie_a, tie_b = single[0], single[1]
    vals[indptr[tie_a], 0] = 1.0
    vals[indptr[tie_b], 0], vals[indptr[tie_b], 1] = 1.0, np.float16(2.0 ** -15)
    for j, r in enumerate(single[2:8]):
        vals[indptr[r], 0] = np.float16(0.99 - 0.01 * j)
    dup = single[[8, 11, 12, 19]]
    for r in dup:
        vals[indptr[r]] = vals[indptr[dup[0]]]
        vals[indptr[r], 0] = np.float16(0.92)
    qtok = np.zeros((2, 8, 8), np.float16)
    qtok[0, :2] = q0
    qtok[1] = rng.standard_normal((8, 8)).astype(np.float16)
    return qtok, (2, 5), indptr, vals, (int(tie_a), int(tie_b)), [int(r) for r in dup]


def run_search(qtok, qn, indptr, vals, mask, k, offset):
    B, n = qtok.shape[0], len(indptr) - 1
    t_q, t_qn = dev(qtok.view(np.int16)), dev(np.asarray(qn, dtype=np.int32))
    t_ip, t_v = token_tensors(indptr, vals, n)
    t_m = dev(pack(mask)) if mask is not None else None
    sc = torch.full((B, n), float(SENT), dtype=torch.float32, device="cuda")
    rw = torch.full((B, n), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(nat.deep_topk_scratch_bytes(n, B, k + offset) // 8 + 1, dtype=torch.int64, device="cuda")
    oi = torch.full((B, k), SENT, dtype=torch.int64, device="cuda")
    os_ = torch.full((B, k), float(SENT), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nat.maxsim_scan_dev(t_q.data_ptr(), t_qn.data_ptr(), B, qtok.shape[1], qtok.shape[2], t_ip.data_ptr(), t_v.data_ptr(), n, n,
                        t_m.data_ptr() if mask is not None else 0, sc.data_ptr(), rw.data_ptr(), s)
    nat.deep_topk_dev(sc.data_ptr(), rw.data_ptr(), n, B, k, offset, False, FIRST_ROW, oi.data_ptr(), os_.data_ptr(),
                      scratch.data_ptr(), s)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), os_.cpu().numpy()


@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("top_k", [1, 10, 256, 300])
def test_scan_then_deep_topk_equals_the_search_restatement(gpu, top_k, offset):
    qtok, qn, indptr, vals, tie, dup = ranked_store()
    rng = np.random.default_rng(top_k + offset)
    for mask in (None, rng.random(len(indptr) - 1) < 0.4):          # the masked ranking is shorter than 256: padding
        ids, sc = run_search(qtok, qn, indptr, vals, mask, top_k, offset)
        for q in range(2):
            wi, ws = M.maxsim_search_csr(qtok[q, :qn[q]], indptr, vals, mask, top_k, offset, FIRST_ROW)
            assert np.array_equal(ids[q, :len(wi)], wi) and np.array_equal(sc[q, :len(wi)], ws)
            assert (ids[q, len(wi):] == -1).all() and not sc[q, len(wi):].any()
    full, fs = M.maxsim_search_csr(qtok[0, :2], indptr, vals, None, 12, 0, FIRST_ROW)     # what the store was built to show
    assert full[:2].tolist() == [tie[0] + FIRST_ROW, tie[1] + FIRST_ROW] and fs[0] == fs[1] == np.float32(1.0)
    assert M.maxsim_rerank_csr(full[:2].tolist(), qtok[0, :2], indptr, vals, FIRST_ROW, 2)[1] == [tie[1] + FIRST_ROW, tie[0] + FIRST_ROW]
    assert full[8:12].tolist() == [r + FIRST_ROW for r in dup] and len(set(fs[8:12].tolist())) == 1


def test_duplicate_rows_through_the_device(gpu):
    q, indptr, vals = duplicate_rows()
    qtok = q[None]
    for k in (1, 2, 3, 20):
        ids, sc = run_search(qtok, (len(q),), indptr, vals, None, k, 0)
        wi, ws = M.maxsim_search_csr(q, indptr, vals, None, k, 0, FIRST_ROW)
        assert np.array_equal(ids[0], wi) and np.array_equal(sc[0], ws)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu):
    rng = np.random.default_rng(7)
    B, dim, tq, n = 2, 16, 8, 16
    indptr, vals = make_store(rng, n, dim)
    t = {"q": dev(rng.standard_normal((B, tq, dim)).astype(np.float16).view(np.int16)),
         "qn": torch.full((B,), tq, dtype=torch.int32, device="cuda"), "ip": dev(indptr), "v": dev(vals.view(np.int16)),
         "m": dev(pack(np.ones(n, bool)))}
    sc = torch.full((B, n), float(SENT), dtype=torch.float32, device="cuda")
    rw = torch.full((B, n), SENT, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(d_qtok=t["q"].data_ptr(), d_qn=t["qn"].data_ptr(), B=B, tq_stride=tq, dim=dim, d_indptr=t["ip"].data_ptr(),
                 d_tok=t["v"].data_ptr(), tok_rows=n, n_rows=n, d_rowmask=t["m"].data_ptr(), d_scores=sc.data_ptr(),
                 d_rows=rw.data_ptr())
        a.update(kw)
        nat.maxsim_scan_dev(**a)

    for kw in (dict(d_qtok=0), dict(d_qn=0), dict(d_scores=0), dict(d_rows=0), dict(d_indptr=0), dict(d_tok=0), dict(dim=4),
               dict(dim=0), dict(dim=12), dict(dim=20), dict(d_qtok=t["q"].data_ptr() + 2), dict(d_tok=t["v"].data_ptr() + 8),
               dict(B=-1), dict(tok_rows=-1), dict(n_rows=-1), dict(tq_stride=0)):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(tq_stride=nat.HR_MAX_QUERY_TOKENS + 1), dict(dim=nat.HR_MAX_TOKEN_DIM + 8), dict(n_rows=1 << 31), dict(B=65536)):
        with pytest.raises(nat.HbmRagError) as e:      # HR_ELIMIT
            call(**kw)
        assert e.value.status == 5
    call(B=0)
    call(n_rows=0)                                      # HR_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((sc == SENT).all()) and bool((rw == SENT).all())
    call(d_indptr=0, d_tok=0, tok_rows=0)               # no token store: allowed, every cell is (0.0f, -1)
    torch.cuda.synchronize()
    assert bool((sc == 0).all()) and bool((rw == -1).all())
    call()                                              # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert np.array_equal(rw.cpu().numpy()[0], np.where(np.diff(indptr) > 0, np.arange(n), -1))


# ---- through a real manager ---------------------------------------------------------------------------------------------------
N, N_MORE, DIM, V, TD = 2000, 150, 64, 256, 64


def query_tokens(seed, tq):
    return np.random.default_rng(seed).standard_normal((tq, TD)).astype(np.float32)


def _rows(rng, lo, hi):
    n, nnz = hi - lo, 5
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(n)]).astype(np.int32)
    val = (np.abs(rng.standard_normal((n, nnz))) + 0.1).astype(np.float32)
    csr = (np.arange(n + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
    T = rng.integers(0, 41, n)
    T[::9] = 0
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    tok = rng.standard_normal((int(indptr[-1]), TD)).astype(np.float32)
    payload = dict(ids=[f"c{r}" for r in range(lo, hi)], contents=[f"topic{r % 5}" for r in range(lo, hi)],
                   doc_id=[f"doc{r // 10}" for r in range(lo, hi)], chunk_index=[r % 7 for r in range(lo, hi)])
    return X, csr, payload, (indptr, tok)


def want_hits(mgr, qt, keep, top_k, offset=0):
    """The restatement over the manager's host column; keep = bool over the manager's rows or None."""
    col = mgr._cols.token_vectors()
    ids, sc = M.maxsim_search_csr(np.asarray(qt, np.float32).astype(np.float16), col.indptr(), col.values(), keep, top_k, offset)
    return [(mgr._cols["id"][r], float(s)) for r, s in zip(ids.tolist(), sc.tolist())]


def got_hits(mgr, qt, top_k, filters=None, offset=0):
    return [(h["id"], h["score"]) for h in asyncio.run(mgr.maxsim_search(qt, top_k, filters, offset=offset))]


def chunk_index(mgr):
    return np.array([mgr._cols["chunk_index"][r] for r in range(mgr.num_rows)])


def test_manager_search_equals_the_restatement(gpu):
    rng = np.random.default_rng(64)
    (X, csr, payload, tv), (X2, csr2, payload2, tv2) = _rows(rng, 0, N), _rows(rng, N, N + N_MORE)
    mgr = MilvusIndexManager(semantic_dim=DIM, sparse_dim=V, enable_domain=False, token_dim=TD)
    try:
        mgr.add_rows(X, csr, **payload, token_vectors=tv)
        mgr.finalize()
        assert mgr._device_shard(mgr._main) is not None
        ranker = MaxSimRanker(query_tokens(5, 12), candidates=40)
        rerank_before = [(h["id"], h["score"], h["raw_score"]) for h in asyncio.run(mgr.search(X[3], "semantic_index", 10, ranker=ranker))]
        qt = query_tokens(1, 9)
        assert np.array_equal(mgr._cols.token_vectors().indptr(), tv[0])
        # plain
        plain = got_hits(mgr, qt, 20)
        assert plain == want_hits(mgr, qt, None, 20) and len(plain) == 20
        assert got_hits(mgr, query_tokens(2, 64), 300, offset=7) == want_hits(mgr, query_tokens(2, 64), None, 300, 7)
        hit = asyncio.run(mgr.maxsim_search(qt, 1))[0]
        assert set(hit) == set(asyncio.run(mgr.search(X[0], "semantic_index", 1))[0]) and isinstance(hit["score"], float)
        # filtered, and pages of the filtered ranking
        keep = chunk_index(mgr) < 5
        whole = got_hits(mgr, qt, 30, "chunk_index < 5")
        assert whole == want_hits(mgr, qt, keep, 30)
        assert sum((got_hits(mgr, qt, 10, "chunk_index < 5", offset=o) for o in (0, 10, 20)), []) == whole
        deep = got_hits(mgr, qt, nat.HR_MAX_DEEP_K)                                        # deeper than the ranking: all hits
        assert deep == want_hits(mgr, qt, None, nat.HR_MAX_DEEP_K) and len(deep) == int((np.diff(tv[0]) > 0).sum())
        assert mgr.stats["maxsim_searches"] == 8 and mgr.stats["maxsim_host_searches"] == 0
        # the rerank on the same manager returns what it returned before, and what the restatement says
        hits = asyncio.run(mgr.search(X[3], "semantic_index", 10, ranker=ranker))
        assert [(h["id"], h["score"], h["raw_score"]) for h in hits] == rerank_before
        first = asyncio.run(mgr.search(X[3], "semantic_index", 40))
        col = mgr._cols.token_vectors()
        pos, _, fin = M.maxsim_rerank_csr([h["_row"] for h in first], ranker.query_tokens, col.indptr(), col.values(), 0, 40)
        assert rerank_before == [(first[p]["id"], f, first[p]["score"]) for p, f in zip(pos[:10], fin[:10])]
        # tombstones
        asyncio.run(mgr.delete_by_filter("semantic_index", "chunk_index == 1"))
        alive = chunk_index(mgr) != 1
        got = got_hits(mgr, qt, 50)
        assert got == want_hits(mgr, qt, alive, 50) and not any(int(i[1:]) % 7 == 1 for i, _ in got)
        assert any(int(i[1:]) % 7 == 1 for i, _ in want_hits(mgr, qt, None, 50))          # the tombstones decide something
        assert got_hits(mgr, qt, 50, "chunk_index < 5") == want_hits(mgr, qt, alive & keep, 50)
        # an append that extends the mirror in place (the new rows are alive whatever their chunk_index)
        mirror = mgr._token_vectors_on_device()
        mgr.add_rows(X2, csr2, **payload2, token_vectors=tv2)
        mgr.finalize()
        alive = np.concatenate([alive, np.ones(N_MORE, dtype=bool)])
        r_new = int(np.argmax(np.diff(tv2[0])))                                            # the longest appended row
        q_new = tv2[1][tv2[0][r_new]:tv2[0][r_new + 1]][:8]                                # its own tokens find it
        got = got_hits(mgr, q_new, 40)
        assert got == want_hits(mgr, q_new, alive, 40) and got[0][0] == f"c{N + r_new}"
        assert mgr._token_vectors_on_device() is mirror
        # compaction renumbers the rows and rebuilds the mirror
        before = got_hits(mgr, qt, 60, "chunk_index < 5")
        mgr.compact()
        assert mgr.num_rows == int(alive.sum()) < N + N_MORE
        assert got_hits(mgr, qt, 60, "chunk_index < 5") == want_hits(mgr, qt, chunk_index(mgr) < 5, 60) == before
        assert got_hits(mgr, qt, 60) == want_hits(mgr, qt, None, 60)
        assert mgr._token_vectors_on_device() is not mirror
        assert mgr.stats["maxsim_searches"] == 14 and mgr.stats["maxsim_host_searches"] == 0
        for bad in (dict(top_k=0), dict(top_k=nat.HR_MAX_DEEP_K, offset=1), dict(filters="no_such_field == 1")):
            with pytest.raises(ValueError):
                asyncio.run(mgr.maxsim_search(qt, **bad))
        with pytest.raises(ValueError):
            asyncio.run(mgr.maxsim_search(np.ones((65, TD))))
    finally:
        asyncio.run(mgr.close())
