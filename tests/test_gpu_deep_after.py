"""The search iterator's pages through the C ABI.  hr_deep_topk_window_dev, the selection with a key interval, on arrays
of the test's making against numpy's lexsort, the intervals made by indexing.cursor_key_interval (the library's own
interval function restated); hr_search_dense_deep_after / hr_search_sparse_deep_after against the deep forms at the same
position, the oracle, tests/l2_yardstick.py and tests/range_yardstick.py.  Ids equal, score bits equal."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.indexing import cursor_key_interval, rank_key
from advanced_rag.staging import csr_of_queries

import range_yardstick as ry
from l2_yardstick import bits, l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EVERYTHING = (0, 2 ** 64 - 1)
METRICS = {"COSINE": nat.HR_METRIC_COSINE, "IP": nat.HR_METRIC_IP, "L2": nat.HR_METRIC_L2}


# ---------------------------------------------------------------------------------------------------------------- selection
def run_window(scores, rows, k, intervals, ascending=False, row_offset=0):
    """scores / rows [B, n], intervals [(lo, hi)] * B (None: a NULL d_bounds) -> (ids [B, k], scores [B, k])."""
    scores = np.ascontiguousarray(np.atleast_2d(scores), dtype=np.float32)
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.int32)
    B, n = scores.shape
    ds, dr = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda()
    ids = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    sc = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(max(nat.deep_topk_scratch_bytes(n, B, k), 8), dtype=torch.uint8, device="cuda")
    db = None if intervals is None else torch.from_numpy(np.array(intervals, dtype=np.uint64).reshape(B, 2).view(np.int64)).cuda()
    st = torch.cuda.current_stream()
    nat.deep_topk_window_dev(ds.data_ptr(), dr.data_ptr(), n, B, k, ascending, row_offset, db.data_ptr() if db is not None else 0,
                             ids.data_ptr(), sc.data_ptr(), scratch.data_ptr(), st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def tied():
    """n = 5000, B = 4: three queries whose scores are drawn from 8 values (long runs of ties, both signs and both zeros),
    one whose scores are all equal; a twentieth of the slots invalid; rows a shuffled permutation.  -> scores, rows, and per
    query the ranking (rows, scores) by numpy's lexsort on (key domain score desc, row asc)."""
    rng = np.random.default_rng(2024)
    n, B = 5000, 4
    values = np.array([-2.5, -0.75, -0.0, 0.0, 0.125, 0.5, 0.5000001, 3.0], np.float32)
    scores = values[rng.integers(0, 8, (B, n))]
    scores[3] = np.float32(0.25)
    rows = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)
    rows[rng.random((B, n)) < 0.05] = -1
    ranking = []
    for b in range(B):
        ok = np.flatnonzero(rows[b] >= 0)
        order = ok[np.argsort(rank_key(scores[b][ok], rows[b][ok]))[::-1]]     # keys are unique: the order is total
        lex = ok[np.lexsort((rows[b][ok], -scores[b][ok].astype(np.float64)))]
        zero = scores[b][order] == 0                                          # (lexsort cannot tell -0.0 from +0.0; the key can)
        assert np.array_equal(order[~zero], lex[~(scores[b][lex] == 0)])
        ranking.append((rows[b][order].astype(np.int64), scores[b][order]))
    return scores, rows, ranking


@pytest.mark.parametrize("k", [257, 1000])
def test_walk_by_feeding_the_last_key_back(gpu, k):
    scores, rows, ranking = tied()
    B = scores.shape[0]
    after, got, short = [None] * B, [([], []) for _ in range(B)], [False] * B
    for _ in range(5000 // k + 3):
        ids, sc = run_window(scores, rows, k, [cursor_key_interval(a, None, "IP") for a in after])
        for b in range(B):
            m = int((ids[b] >= 0).sum())
            assert (ids[b][m:] == -1).all() and (bits(sc[b][m:]) == 0).all()
            assert not (short[b] and m), "an exhausted query writes only padding"
            got[b][0].extend(ids[b][:m].tolist())
            got[b][1].extend(sc[b][:m].tolist())
            short[b] |= m < k
            if m:
                after[b] = (sc[b][m - 1], ids[b][m - 1])
        if all(short):
            break
    assert all(short)
    for b in range(B):
        want_rows, want_sc = ranking[b]
        assert np.array_equal(np.array(got[b][0]), want_rows), b
        assert np.array_equal(bits(np.array(got[b][1], np.float32)), bits(want_sc)), b
        assert len(set(got[b][0])) == len(got[b][0])


@pytest.mark.parametrize("held", [0, 1, 256])
def test_one_launch_of_mixed_queries(gpu, held):
    """No cursor, a cursor in the middle of a run of ties, an exhausted query, and an interval that holds exactly `held`
    keys (0, 1, k - 1), in one launch."""
    scores, rows, ranking = tied()
    k = 257
    keys = [rank_key(sc, r) for r, sc in ranking]
    mid = 1234
    assert bits(ranking[1][1][mid]) == bits(ranking[1][1][mid + 1]) == bits(ranking[1][1][mid - 1])
    p = 2000
    intervals = [EVERYTHING,
                 cursor_key_interval((ranking[1][1][mid], ranking[1][0][mid]), None, "IP"),
                 cursor_key_interval((ranking[2][1][-1], ranking[2][0][-1]), None, "IP"),
                 (int(keys[3][p + held + 1]), int(keys[3][p]))]
    ids, sc = run_window(scores, rows, k, intervals)
    want = [(ranking[0][0][:k], ranking[0][1][:k]), (ranking[1][0][mid + 1:mid + 1 + k], ranking[1][1][mid + 1:mid + 1 + k]),
            (ranking[2][0][:0], ranking[2][1][:0]), (ranking[3][0][p + 1:p + 1 + held], ranking[3][1][p + 1:p + 1 + held])]
    for b, (wr, ws) in enumerate(want):
        m = len(wr)
        assert np.array_equal(ids[b][:m], wr) and np.array_equal(bits(sc[b][:m]), bits(ws)), b
        assert (ids[b][m:] == -1).all() and (bits(sc[b][m:]) == 0).all(), b
    again = run_window(scores, rows, k, intervals)
    assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == sc.tobytes()      # the same launch twice: the same bits


def test_open_bounds_are_the_plain_selection_and_the_small_cases(gpu):
    scores, rows, ranking = tied()
    B, n = scores.shape
    for k in (1, 300, 16384):
        ds, dr = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda()
        ids = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
        sc = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
        scratch = torch.empty(nat.deep_topk_scratch_bytes(n, B, k), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream()
        nat.deep_topk_dev(ds.data_ptr(), dr.data_ptr(), n, B, k, 0, False, 11, ids.data_ptr(), sc.data_ptr(), scratch.data_ptr(),
                          st.cuda_stream)
        st.synchronize()
        for intervals in ([EVERYTHING] * B, None):
            wi, ws = run_window(scores, rows, k, intervals, row_offset=11)
            assert wi.tobytes() == ids.cpu().numpy().tobytes() and ws.tobytes() == sc.cpu().numpy().tobytes()
    ids, sc = run_window(scores, rows, 1, [cursor_key_interval((ranking[b][1][0], ranking[b][0][0]), None, "IP") for b in range(B)])
    assert [int(i) for i in ids[:, 0]] == [int(ranking[b][0][1]) for b in range(B)]      # k = 1: the second of every ranking
    ids, sc = run_window(np.zeros((2, 0), np.float32), np.zeros((2, 0), np.int32), 5, [EVERYTHING] * 2)     # n = 0
    assert (ids == -1).all() and (bits(sc) == 0).all()
    # negated distances: written out as distances, the interval in the key domain
    dist = -np.abs(scores)
    ids, sc = run_window(dist[:1], rows[:1], 50, [cursor_key_interval((0.5, -1), None, "L2")], ascending=True)
    assert (sc[0][ids[0] >= 0] >= 0.5).all() and (np.diff(sc[0][ids[0] >= 0]) >= 0).all() and sc[0][0] == 0.5
    for bad_k in (0, 16385):
        with pytest.raises((ValueError, nat.HbmRagError)):
            run_window(scores, rows, bad_k, [EVERYTHING] * B)


# ---------------------------------------------------------------------------------------------------------------- dense host forms
N, D, V = 3000, 32, 64


@functools.lru_cache(maxsize=None)
def corpus():
    """The corpus shape of tests/test_gpu_deep_manager.py: 3 000 x 32 with 200 copies of one row; fp16 values."""
    rng = np.random.default_rng(41)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X[rng.permutation(N)[:200]] = X[7]
    X[11] = 0                                                     # a row whose inner product is +0.0
    X = X.astype(np.float16)
    Q = rng.standard_normal((2, D)).astype(np.float32)
    Q[1] = X[7].astype(np.float32)                                # at distance 0 of the 200 copies
    val = (rng.integers(1, 16, (N, 4)) / 4).astype(np.float32)
    idx = (np.arange(4) * (V // 4) + rng.integers(0, V // 4, (N, 4))).astype(np.int32)
    csr = (np.arange(N + 1, dtype=np.int64) * 4, idx.reshape(-1), val.reshape(-1))
    return X, Q, csr


def dense_want(X, Q, k, metric, mask=None, row_offset=0):
    if metric == nat.HR_METRIC_L2:
        return l2_search(X, Q, k, mask, row_offset)
    return oracle.dense_search(X, Q, k, metric, mask, row_offset)


@pytest.fixture(scope="module", params=list(METRICS))
def dense_case(request):
    X, Q, csr = corpus()
    metric = METRICS[request.param]
    h = nat.ShardHandle(D, nat.HR_F16, metric, V)
    h.add_dense(X.astype(np.float32))
    h.add_sparse(*csr)
    h.finalize()
    yield h, X, Q, metric, dense_want(X, Q, N, metric)
    h.close()


def same(got, want_ids, want_sc):
    assert np.array_equal(got[0], want_ids), f"ids differ at {np.argwhere(got[0] != want_ids)[:5]}"
    assert np.array_equal(bits(got[1]), bits(want_sc))


def after_ref(rid, rsc, cursor, k, ascending):
    """One query: the first k entries of the complete ranking (rid, rsc) strictly after cursor = (score, id), -1 / 0 padded."""
    live = rid >= 0
    if cursor is not None:
        s, i = np.float32(cursor[0]), int(cursor[1])
        worse = rsc > s if ascending else rsc < s
        live &= worse | ((rsc == s) & (rid > i))
    take = np.flatnonzero(live)[:k]
    ids, sc = np.full(k, -1, np.int64), np.zeros(k, np.float32)
    ids[:len(take)], sc[:len(take)] = rid[take], rsc[take]
    return ids, sc


def test_pages_are_the_deep_lists_at_the_same_position(gpu, dense_case):
    h, X, Q, metric, (rid, rsc) = dense_case
    k = 700
    same(h.search_dense_deep_after(Q, k), *h.search_dense_deep(Q, k, 0))
    same(h.search_dense_deep_after(Q, k, (np.zeros(2, np.float32), np.zeros(2, np.int64), np.zeros(2, bool))),
         *h.search_dense_deep(Q, k, 0))
    rid_p = np.pad(rid, ((0, 0), (0, 6 * k - N)), constant_values=-1)
    rsc_p = np.pad(rsc, ((0, 0), (0, 6 * k - N)))
    page, both = h.search_dense_deep(Q, k, 0), np.arange(2)
    for p in range(1, 6):                                         # page 4 is short, page 5 all padding
        last = np.maximum((page[0] >= 0).sum(1) - 1, 0)
        nxt = h.search_dense_deep_after(Q, k, (page[1][both, last], page[0][both, last]))
        same(nxt, rid_p[:, p * k:(p + 1) * k], rsc_p[:, p * k:(p + 1) * k])
        same(nxt, *h.search_dense_deep(Q, k, p * k))
        if p < 5:
            page = nxt
    # one query with a cursor, one without, in one call
    mixed = h.search_dense_deep_after(Q, 300, (rsc[:, 999], rid[:, 999], np.array([True, False])))
    same((mixed[0][:1], mixed[1][:1]), rid[:1, 1000:1300], rsc[:1, 1000:1300])
    same((mixed[0][1:], mixed[1][1:]), rid[1:, :300], rsc[1:, :300])


def test_masks_row_offset_and_cursors_that_name_no_row(gpu, dense_case):
    h, X, Q, metric, _ = dense_case
    asc = metric == nat.HR_METRIC_L2
    rng = np.random.default_rng(6)
    keep = rng.random(N) < 0.5
    packed = np.packbits(keep, bitorder="little")
    off = 1_000_000
    h.set_row_offset(off)
    try:
        rid, rsc = dense_want(X, Q, N, metric, packed, off)
        d_mask = torch.zeros(8 * ((N + 63) // 64), dtype=torch.uint8, device="cuda")
        d_mask[:packed.size] = torch.from_numpy(packed).cuda()
        k = 400
        same(h.search_dense_deep_after(Q, k, None, None, packed), rid[:, :k], rsc[:, :k])
        same(h.search_dense_deep_after(Q, k, (rsc[:, k - 1], rid[:, k - 1]), None, packed), rid[:, k:2 * k], rsc[:, k:2 * k])
        same(h.search_dense_deep_after(Q, k, (rsc[:, k - 1], rid[:, k - 1]), None, None, d_mask.data_ptr()), rid[:, k:2 * k], rsc[:, k:2 * k])
        run = int(np.flatnonzero(bits(rsc[1]) == bits(rsc[1][0]))[-1])        # query 1: the run of copies leads its ranking
        assert run > 50
        masked_in_run = next(r for r in np.flatnonzero((X == X[7]).all(1)) if not keep[r])
        for score, rid_c in ((rsc[:, 10], np.array([off - 5, off - 5])),        # below the row offset: the whole run of that score
                             (rsc[:, 10], np.array([-2 ** 62, 2 ** 62])),        # as far out as int64 goes, either side
                             (rsc[:, 10], np.array([off + N + 77, off + 2 ** 33])),   # beyond the last row: none of that score
                             (rsc[:, 3], np.array([off + masked_in_run] * 2)),   # on a masked row inside the run of copies
                             (rsc[:, 3], np.array([off + 7, off + 8]))):         # next to one another inside the run
            got = h.search_dense_deep_after(Q, k, (score, rid_c), None, packed)
            for b in range(2):
                wi, ws = after_ref(rid[b], rsc[b], (score[b], rid_c[b]), k, asc)
                same((got[0][b], got[1][b]), wi, ws)
    finally:
        h.set_row_offset(0)


def test_bounds_against_the_range_yardstick(gpu, dense_case):
    h, X, Q, metric, (rid, rsc) = dense_case
    asc = metric == nat.HR_METRIC_L2
    code = {nat.HR_METRIC_IP: ry.IP, nat.HR_METRIC_COSINE: ry.COSINE, nat.HR_METRIC_L2: ry.L2}[metric]
    s = [ry.scores(X, Q[b], code) for b in range(2)]
    lo, hi = float(rsc[0][1800]), float(rsc[0][300])              # bounds that sit on scores of query 0 (lo worse than hi)
    cases = [(lo, hi), (lo, None), (None, hi), (np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf))]    # (radius, range_filter)
    cases += [(None, -0.0), (None, 0.0)] if asc else [(-0.0, None), (0.0, None), (None, -0.0)]
    for radius, range_filter in cases:
        got = h.search_dense_deep_after(Q, N, None, (radius, range_filter))
        for b in range(2):
            wi, ws = ry.topk_in_range(s[b], code, N, radius, range_filter)
            same((got[0][b], got[1][b]), wi, ws)
        # the same ranking in pages of 450: cursor and bounds in one interval
        b, seen_i, seen_s, cursor = 0, [], [], None
        want_i, want_s = ry.topk_in_range(s[0], code, N, radius, range_filter)
        for _ in range(N // 450 + 2):
            pi, ps = h.search_dense_deep_after(Q[:1], 450, cursor, (radius, range_filter))
            m = int((pi[0] >= 0).sum())
            seen_i += pi[0][:m].tolist()
            seen_s += ps[0][:m].tolist()
            if m < 450:
                break
            cursor = (ps[0][-1:], pi[0][-1:])
        n_in = int((want_i >= 0).sum())
        assert seen_i == want_i[:n_in].tolist() and np.array_equal(bits(np.array(seen_s, np.float32)), bits(want_s[:n_in]))
    # what the zero bounds are about: the zero row's inner product is +0.0 and must not pass radius = -0.0; a row at
    # distance 0 (key score -0.0) must pass range_filter = +-0.0
    if metric == nat.HR_METRIC_IP:
        assert s[0][11] == 0 and 11 not in h.search_dense_deep_after(Q[:1], N, None, (-0.0, None))[0][0]
        assert 11 in h.search_dense_deep_after(Q[:1], N, None, (None, -0.0))[0][0]
    if asc:
        for zero in (0.0, -0.0):
            got = h.search_dense_deep_after(Q[1:], 300, None, (None, zero))
            assert (got[1][0][:200] == 0).all() and (X[got[0][0][:200]] == X[7]).all()


def test_float64_bounds_keep_their_meaning(gpu, dense_case):
    """A bound between two fp32 numbers, and one an fp32 score rounds ONTO: the rows kept are those the float64 rule keeps."""
    h, X, Q, metric, (rid, rsc) = dense_case
    asc = metric == nat.HR_METRIC_L2
    code = {nat.HR_METRIC_IP: ry.IP, nat.HR_METRIC_COSINE: ry.COSINE, nat.HR_METRIC_L2: ry.L2}[metric]
    s = ry.scores(X, Q[0], code)
    x = float(rsc[0][500])
    for bound in (x * (1 + 1e-9), x * (1 - 1e-9)):
        for bounds in ((bound, None), (None, bound)):
            got = h.search_dense_deep_after(Q[:1], N, None, bounds)
            same((got[0][0], got[1][0]), *ry.topk_in_range(s, code, N, *bounds))


# ---------------------------------------------------------------------------------------------------------------- sparse, past the cap
def test_sparse_walk_against_the_oracle(gpu, dense_case):
    h, X, Q, metric, _ = dense_case
    _, _, (indptr, idx, val) = corpus()
    queries = [(list(range(0, V, 2)), [1.0] * (V // 2)), ([3, 40], [1.0, 0.5])]
    rid, rsc = oracle.sparse_search(indptr, idx, val, queries, N)
    n_pos = (rid >= 0).sum(1)
    assert n_pos[0] > 2000 and 0 < n_pos[1] < 600                 # positive scores only: the second ranking is short
    k = 600
    same(h.search_sparse_deep_after(queries, k), *h.search_sparse_deep(queries, k, 0))
    cursor, pages = None, []
    for _ in range(N // k + 2):
        pi, ps = h.search_sparse_deep_after(queries, k, cursor)
        pages.append((pi, ps))
        last = np.maximum((pi >= 0).sum(1) - 1, 0)
        prev = cursor
        cursor = (ps[np.arange(2), last].copy(), pi[np.arange(2), last].copy())
        for b in range(2):                                        # an exhausted query keeps its cursor and writes padding
            if pi[b][0] < 0:
                cursor[0][b], cursor[1][b] = prev[0][b], prev[1][b]
        if (pi[:, -1] < 0).all():
            break
    got_i, got_s = np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)
    for b in range(2):
        m = got_i[b] >= 0
        assert np.array_equal(got_i[b][m], rid[b][:n_pos[b]]) and np.array_equal(bits(got_s[b][m]), bits(rsc[b][:n_pos[b]]))
        assert (bits(got_s[b][~m]) == 0).all()
    keep = np.random.default_rng(9).random(N) < 1 / 3
    packed = np.packbits(keep, bitorder="little")
    wi, ws = oracle.sparse_search(indptr, idx, val, queries, N, 0.0, packed)
    same(h.search_sparse_deep_after(queries[:1], 200, (ws[:1, 99], wi[:1, 99]), 0.0, packed), wi[:1, 100:300], ws[:1, 100:300])


def test_a_walk_past_the_deep_cap(gpu):
    rng = np.random.default_rng(77)
    n, k = 20_011, 4096
    X = rng.standard_normal((n, D)).astype(np.float16)
    X[rng.permutation(n)[:300]] = X[5]                            # a run of ties that straddles a page edge somewhere
    Q = rng.standard_normal((1, D)).astype(np.float32)
    h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, 0)
    try:
        h.add_dense(X.astype(np.float32))
        h.finalize()
        rid, rsc = oracle.dense_search(X, Q, n, nat.HR_METRIC_COSINE)
        cursor, got_i, got_s = None, [], []
        for _ in range(n // k + 2):
            pi, ps = h.search_dense_deep_after(Q, k, cursor)
            m = int((pi[0] >= 0).sum())
            got_i.append(pi[0][:m])
            got_s.append(ps[0][:m])
            if m < k:
                break
            cursor = (ps[:, -1], pi[:, -1])
        assert [len(p) for p in got_i] == [k, k, k, k, n - 4 * k]
        assert np.array_equal(np.concatenate(got_i), rid[0]) and np.array_equal(bits(np.concatenate(got_s)), bits(rsc[0]))
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(gpu, dense_case):
    h, X, Q, metric, _ = dense_case
    lib = nat.load_library()
    asc = metric == nat.HR_METRIC_L2
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)         # noqa: E731
    f32 = lambda *v: np.array(v, np.float32)                                       # noqa: E731
    one, yes = np.array([5, 5], np.int64), np.ones(2, np.uint8)
    empty = (f32(1.0, 1.0), f32(1.0, 2.0)) if asc else (f32(0.5, 0.7), f32(0.5, 0.2))          # radius, range_filter
    cases = [(300, f32(np.nan, 0.5), one, yes, None, None, 1), (300, f32(0.5, np.inf), one, yes, None, None, 1),
             (300, f32(0.5, -np.inf), one, yes, None, None, 1), (300, None, None, None, f32(np.nan, 0.1), None, 1),
             (300, None, None, None, None, f32(0.1, np.nan), 1), (300, None, None, None, empty[0], empty[1], 1),
             (300, None, None, None, f32(0.3, 0.3), f32(0.3, 0.9), 1),
             (0, None, None, None, None, None, 1), (-4, None, None, None, None, None, 1), (16385, None, None, None, None, None, 5)]
    for k, a_sc, a_id, a_has, radius, range_filter, status in cases:
        ids, sc = np.full((2, 300), 7, np.int64), np.full((2, 300), 7.0, np.float32)
        rc = lib.hr_search_dense_deep_after(h._h, vp(Q), 2, k, vp(a_sc), vp(a_id), vp(a_has), vp(radius), vp(range_filter), None, 0,
                                            vp(ids), vp(sc))
        assert rc == status, (k, a_sc, radius, range_filter, rc)
        assert (ids == 7).all() and (sc == 7.0).all()
    # a non-finite after_score where has_after is NOT set is no cursor at all
    ids, sc = np.full((2, 300), 7, np.int64), np.full((2, 300), 7.0, np.float32)
    assert lib.hr_search_dense_deep_after(h._h, vp(Q), 2, 300, vp(f32(np.nan, np.inf)), vp(one), vp(np.zeros(2, np.uint8)), None, None,
                                          None, 0, vp(ids), vp(sc)) == 0
    same((ids, sc), *h.search_dense_deep(Q, 300))
    queries = [([3, 40], [1.0, 0.5])] * 2
    indptr, idx, val = csr_of_queries(queries)
    for k, a_sc, status in ((300, f32(np.nan, 1.0), 1), (300, f32(1.0, np.inf), 1), (16385, None, 5), (0, None, 1)):
        ids, sc = np.full((2, 300), 7, np.int64), np.full((2, 300), 7.0, np.float32)
        rc = lib.hr_search_sparse_deep_after(h._h, vp(indptr), vp(idx), vp(val), 2, k, vp(a_sc), vp(one) if a_sc is not None else None,
                                             vp(yes) if a_sc is not None else None, 0.0, None, 0, vp(ids), vp(sc))
        assert rc == status and (ids == 7).all() and (sc == 7.0).all()
    with pytest.raises(ValueError, match="after_score"):
        h.search_dense_deep_after(Q, 300, (f32(np.nan, 0.1), one))
    with pytest.raises(nat.HbmRagError) as ei:
        h.search_dense_deep_after(Q, 16385)
    assert ei.value.status == 5
    assert lib.hr_version() >= 11700
