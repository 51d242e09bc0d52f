"""Range search through the C ABI (hr_search_dense_range, hr_search_dense_range_dev) against the numpy yardstick
(tests/range_yardstick.py): ids equal, score bits equal, no tolerance anywhere.  fp16 and fp32 shards, all three metrics,
16- and 64-row candidate groups, both finish paths.

What the clamp in the scan is for is shown on the planted "annulus" corpus: per query 1 500 rows lie ABOVE range_filter,
so without the clamp every candidate group is one of theirs and no device list is proven; with it every list is."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import range_yardstick as ry
from advanced_rag import _native as nat
from l2_yardstick import bits

pytestmark = pytest.mark.gpu

assert (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE, nat.HR_METRIC_L2) == (ry.IP, ry.COSINE, ry.L2)
DTYPES = [(nat.HR_F16, np.float16), (nat.HR_F32, np.float32)]
METRICS = [ry.COSINE, ry.IP, ry.L2]
METRIC_IDS = ["COSINE", "IP", "L2"]
PATHS = [(16, 1), (16, 2), (64, 1), (64, 2)]          # (HR_DEBUG_GROUP_ROWS, HR_DEBUG_FINISH_MODE)


@contextlib.contextmanager
def option(key, value):
    nat.debug_option(key, value)
    try:
        yield
    finally:
        nat.debug_option(key, 0)


def _shard(X, dtype, metric):
    h = nat.ShardHandle(X.shape[1], dtype, metric, 0)
    h.add_dense(np.ascontiguousarray(X, dtype=np.float32))
    h.finalize()
    return h


def _dev_range(h, Q, k, radius, range_filter, mask=None):
    """hr_search_dense_range_dev -> (ids, scores, flags); radius / range_filter: float64 arrays or None (NULL)."""
    import torch
    B = Q.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(radius, dtype=np.float64)).cuda() if radius is not None else None
    df = torch.from_numpy(np.ascontiguousarray(range_filter, dtype=np.float64)).cuda() if range_filter is not None else None
    dm = torch.from_numpy(np.packbits(mask, bitorder="little")).cuda() if mask is not None else None
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    h.search_dense_range_dev(dq.data_ptr(), B, k, dr.data_ptr() if dr is not None else 0, df.data_ptr() if df is not None else 0,
                             ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), dm.data_ptr() if dm is not None else 0, st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def _dev_plain(h, Q, k):
    import torch
    B = Q.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    h.search_dense_dev(dq.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def _same(got, want, what):
    ids, sc = got[0], got[1]
    assert np.array_equal(ids, want[0]), f"{what}: ids differ at {np.argwhere(ids != want[0])[:5].tolist()}"
    assert np.array_equal(bits(sc), bits(want[1])), f"{what}: score bits differ"


def _same_where_proven(got, want, what):
    ids, sc, fl = got
    assert set(np.unique(fl)) <= {0, 1}, f"{what}: flags {np.unique(fl)}"
    for b in np.nonzero(fl == 1)[0]:
        assert np.array_equal(ids[b], want[0][b]), f"{what}: proven list of query {b} differs"
        assert np.array_equal(bits(sc[b]), bits(want[1][b])), f"{what}: proven scores of query {b} differ"
    return fl


def _score_rows(X, Q, metric):
    if metric == ry.L2:
        return ry.l2_dist_batch(X, Q)
    return np.stack([ry.scores(X, q, metric) for q in np.atleast_2d(Q)])


# ---- 1. the annulus -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _annulus_case(np_dtype, metric):
    """-> (stored rows, queries, radius [B], range_filter [B], expectations {k: (ids, scores)}, gap, eps): computed once per
    (dtype, metric) and shared by the group-size / finish-path cases."""
    a = ry.ANNULUS
    X32, Qh, _ = ry.annulus()
    X = X32.astype(np_dtype)
    B = Qh.shape[0]
    if metric == ry.L2:
        Q = Qh.copy()
        radius = np.full(B, a["l2_radius"])
        rfilter = np.full(B, a["l2_range_filter"])
    else:
        Q = (Qh * np.linspace(0.5, 3.0, B, dtype=np.float32)[:, None]).astype(np.float32)
        qn = np.array([np.sqrt(ry.canonical_qn2(q)) for q in Q])
        scale = qn if metric == ry.IP else np.ones(B)          # IP: each bound scaled by that query's |q|
        radius, rfilter = a["radius"] * scale, a["range_filter"] * scale
    S = _score_rows(X, Q, metric)
    want = {k: ry.range_search(X, Q, k, metric, radius, rfilter, score_rows=S) for k in (10, 64)}
    # distance of every row from both bounds in the scan's domain, against the scan's own error bound
    M = ry.max_row_norm(X)
    gap, eps = np.inf, 0.0
    for b in range(B):
        qn2 = ry.canonical_qn2(Q[b])
        nq = np.sqrt(qn2)
        s = S[b].astype(np.float64)
        if metric == ry.COSINE:
            t, tb = s, (radius[b], rfilter[b])
        elif metric == ry.IP:
            t, tb = s / nq, (radius[b] / nq, rfilter[b] / nq)
        else:
            t, tb = (qn2 - s) / (2 * nq), ((qn2 - radius[b]) / (2 * nq), (qn2 - rfilter[b]) / (2 * nq))
        gap = min(gap, np.abs(t - tb[0]).min(), np.abs(t - tb[1]).min())
        eps = max(eps, ry.scan_eps(metric, np_dtype == np.float16, X.shape[1], M, qn2))
    return X, Q, radius, rfilter, want, gap, eps


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_annulus(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    a = ry.ANNULUS
    X, Q, radius, rfilter, want, gap, eps = _annulus_case(np_dtype, metric)
    print(f"annulus: gap {gap:.4g}, eps {eps:.4g}, gap / eps {gap / eps:.1f}")
    assert gap > 4 * eps                                   # the construction is honest: no row within the slack of a bound
    n_hits = (want[64][0] >= 0).sum(axis=1)
    assert np.all(n_hits == a["n_in"]) and np.all(want[10][0] >= 0)
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(X, dtype, metric)
        try:
            for k in (10, 64):                             # full lists; 40 hits, padded
                _same(h.search_dense_range(Q, k, radius, rfilter), want[k], f"host k={k}")
                got = _dev_range(h, Q, k, radius, rfilter)
                _same(got, want[k], f"device k={k}")
                assert np.all(got[2] == 1), f"device flags k={k}: {got[2]}"
            with option(nat.HR_DEBUG_NO_RANGE_CLAMP, 1):
                # exactness never rests on the clamp: the host form escalates to the same lists; what the clamp buys is the
                # proof — the k-th in-range score (<= 0.8) lies far below an a_cut of about 0.95
                for k in (10, 64):
                    _same(h.search_dense_range(Q, k, radius, rfilter), want[k], f"host, no clamp, k={k}")
                fl = _same_where_proven(_dev_range(h, Q, 10, radius, rfilter), want[10], "device, no clamp")
                assert np.all(fl == 0), f"unclamped device flags: {fl}"
        finally:
            h.close()


# ---- 2. bounds on the scores themselves -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_case(np_dtype, metric):
    """3 000 x 64 rows, 4 queries.  Per query range_filter = the canonical score of its rank-5 row (closed side: kept) and
    radius = that of its rank-30 row (strict side: dropped).  Query 0: three more copies of both rows, so several rows tie
    on each bound.  IP and L2: small-integer vectors, every score exact.  L2, query 1: a row equal to the query and
    range_filter = 0."""
    rng = np.random.default_rng(64 + metric)
    n, d, B = 3000, 64, 4
    if metric == ry.COSINE:
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((B, d)).astype(np.float32)
    else:
        X = rng.integers(-3, 4, (n, d)).astype(np.float32)
        Q = rng.integers(-3, 4, (B, d)).astype(np.float32)
    X = X.astype(np_dtype)
    order = lambda s: np.lexsort((np.arange(n), s if metric == ry.L2 else -s))   # noqa: E731
    o0 = order(ry.scores(X, Q[0], metric))
    spare = np.setdiff1d(np.arange(n), o0[:200])[:7]               # rows far down query 0's ranking
    X[spare[:3]] = X[o0[5]]
    X[spare[3:6]] = X[o0[30]]
    if metric == ry.L2:
        X[spare[6]] = Q[1].astype(np_dtype)                        # integers: exact in fp16
    S = _score_rows(X, Q, metric)
    radius, rfilter = np.empty(B), np.empty(B)
    ties = []
    for b in range(B):
        o = order(S[b])
        closed, strict = float(S[b][o[5]]), float(S[b][o[30]])
        if b == 0:                                                 # the scores of the two rows that were copied
            closed, strict = float(S[0][o0[5]]), float(S[0][o0[30]])
        if metric == ry.L2 and b == 1:
            closed = 0.0
            assert S[b][o[0]] == 0.0
        assert closed != strict
        rfilter[b], radius[b] = closed, strict
        ties.append((np.flatnonzero(S[b] == np.float32(closed)), np.flatnonzero(S[b] == np.float32(strict))))
    assert len(ties[0][0]) >= 4 and len(ties[0][1]) >= 4
    want = ry.range_search(X, Q, 40, metric, radius, rfilter, score_rows=S)
    return X, Q, radius, rfilter, want, ties


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_bounds_on_the_scores_themselves(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    X, Q, radius, rfilter, want, ties = _edge_case(np_dtype, metric)
    for b, (on_closed, on_strict) in enumerate(ties):              # what the expectation itself says about the two sides
        assert set(on_closed) <= set(want[0][b]) and not set(on_strict) & set(want[0][b])
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(X, dtype, metric)
        try:
            _same(h.search_dense_range(Q, 40, radius, rfilter), want, "host")
            _same_where_proven(_dev_range(h, Q, 40, radius, rfilter), want, "device")
        finally:
            h.close()


# ---- 3. batch shapes that cross the routing -------------------------------------------------------------------------
BATCHES = (1, 16, 64, 65, 128, 130)


def _bounds_per_query(S, metric):
    """A different pair per query, between two neighbouring scores of that query's ranking; some sides unbounded."""
    B, n = S.shape
    radius, rfilter = [], []
    for b in range(B):
        s = np.sort(S[b].astype(np.float64))
        s = s if metric == ry.L2 else s[::-1]                      # best first
        i_better, i_worse = 1 + b % 5, 12 + (7 * b) % 40
        better = 0.5 * (s[i_better] + s[i_better + 1])
        worse = 0.5 * (s[i_worse] + s[i_worse + 1])
        rfilter.append(None if b % 4 == 2 or b % 8 == 7 else better)
        radius.append(None if b % 4 == 1 or b % 8 == 7 else worse)
    return radius, rfilter


@functools.lru_cache(maxsize=None)
def _batch_case(np_dtype, metric, n, d):
    rng = np.random.default_rng(n + d + metric)
    X = rng.standard_normal((n, d)).astype(np.float32).astype(np_dtype)
    Q = rng.standard_normal((max(BATCHES), d)).astype(np.float32)
    S = _score_rows(X, Q, metric)
    radius, rfilter = _bounds_per_query(S, metric)
    want = ry.range_search(X, Q, 20, metric, radius, rfilter, score_rows=S)
    return X, Q, ry.bounds_arrays(metric, radius, rfilter, len(Q)), want


def _check_batches(h, case, metric):
    X, Q, (r, f), want = case
    for B in BATCHES:
        w = (want[0][:B], want[1][:B])
        _same(h.search_dense_range(Q[:B], 20, r[:B], f[:B]), w, f"host B={B}")
        fl = _same_where_proven(_dev_range(h, Q[:B], 20, r[:B], f[:B]), w, f"device B={B}")
        print(f"B={B}: {int(fl.sum())} of {B} device lists proven")


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_batch_shapes(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    case = _batch_case(np_dtype, metric, 3001, 200)                # the LDS-resident pass up to 64 queries, 128-query passes beyond
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(case[0], dtype, metric)
        try:
            _check_batches(h, case, metric)
        finally:
            h.close()


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
def test_long_fp32_rows_take_the_k_chunked_pass(gpu, metric, group_rows, finish_mode):
    case = _batch_case(np.float32, metric, 2000, 2560)             # KT = 160 > 156: no LDS-resident query tile at any B
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(case[0], nat.HR_F32, metric)
        try:
            _check_batches(h, case, metric)
        finally:
            h.close()


# ---- 4. corner cases ------------------------------------------------------------------------------------------------
def _random(n, d, B, np_dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)).astype(np.float32).astype(np_dtype), rng.standard_normal((B, d)).astype(np.float32))


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_unbounded_is_the_plain_search_bit_for_bit(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    X, Q = _random(5003, 96, 70, np_dtype, 5003 + metric)
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(X, dtype, metric)
        try:
            for B in (70, 9):                                      # the batch-size default would fuse one and chain the other
                inf = np.full(B, np.inf)
                forms = [(None, None), (-inf, inf) if metric != ry.L2 else (inf, -inf)]
                if metric == ry.L2:
                    forms.append((inf, np.zeros(B)))               # every distance is >= 0
                plain = h.search_dense(Q[:B], 30)
                d_plain = _dev_plain(h, Q[:B], 30)
                for r, f in forms:
                    _same(h.search_dense_range(Q[:B], 30, r, f), plain, "host")
                    got = _dev_range(h, Q[:B], 30, r, f)
                    _same(got, d_plain, "device")
                    assert np.array_equal(got[2], d_plain[2]), "flags differ from hr_search_dense_dev's"
        finally:
            h.close()


@functools.lru_cache(maxsize=None)
def _random_scored(n, d, B, np_dtype, seed, metric):
    X, Q = _random(n, d, B, np_dtype, seed)
    return X, Q, _score_rows(X, Q, metric)


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_no_row_in_range_is_all_padding_and_proven(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    X, Q, S = _random_scored(4001, 64, 5, np_dtype, 41, metric)
    best, worst = (S.min(axis=1), S.max(axis=1)) if metric == ry.L2 else (S.max(axis=1), S.min(axis=1))
    sign = -1.0 if metric == ry.L2 else 1.0
    span = np.abs(S).max()
    # beyond the best row (nothing reaches the floor) and beyond the worst (every row is above the ceiling: all clamped)
    beyond_best = (best + sign * 0.05 * span, best + sign * 0.5 * span)
    beyond_worst = (worst - sign * 0.5 * span, worst - sign * 0.05 * span)
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(X, dtype, metric)
        try:
            for worse, better in (beyond_best, beyond_worst):
                r, f = worse.astype(np.float64), better.astype(np.float64)
                want = ry.range_search(X, Q, 12, metric, r, f, score_rows=S)
                assert np.all(want[0] == -1)
                _same(h.search_dense_range(Q, 12, r, f), want, "host")
                got = _dev_range(h, Q, 12, r, f)
                _same(got, want, "device")
                assert np.all(got[2] == 1), got[2]
        finally:
            h.close()


@functools.lru_cache(maxsize=None)
def _mask_case(np_dtype, metric):
    """1003 = 62 * 16 + 11 rows (a ragged last group), 6 queries of which query 3 is zero, a row mask that keeps 60 % of
    the rows -> (X, Q, mask, bound arrays, {masked?: expectation at k = 50})."""
    X, Q = _random(1003, 128, 6, np_dtype, 1003 + metric)
    Q[3] = 0.0                                                      # a zero query: no ceiling, no floor, the refine decides
    S = _score_rows(X, Q, metric)
    rng = np.random.default_rng(9)
    mask = rng.random(1003) < 0.6
    mask[-11:] = True                                               # the ragged group's rows are candidates
    radius, rfilter = _bounds_per_query(S, metric)
    if metric == ry.L2:                                             # zero query: D = |x|^2; keep the middle of the ranking
        radius[3], rfilter[3] = float(np.sort(S[3])[700]), float(np.sort(S[3])[300])
    else:                                                           # every canonical score is 0
        radius[3], rfilter[3] = -0.5, 0.5
    want = {masked: ry.range_search(X, Q, 50, metric, radius, rfilter, mask=mask if masked else None, score_rows=S)
            for masked in (False, True)}
    return X, Q, mask, ry.bounds_arrays(metric, radius, rfilter, len(Q)), want


@pytest.mark.parametrize("group_rows,finish_mode", PATHS)
@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_row_mask_ragged_last_group_and_zero_query(gpu, dtype, np_dtype, metric, group_rows, finish_mode):
    X, Q, mask, (r, f), wants = _mask_case(np_dtype, metric)
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        h = _shard(X, dtype, metric)
        try:
            for m in (None, mask):
                want = wants[m is not None]
                assert (want[0][3] >= 0).all()
                packed = None if m is None else np.packbits(m, bitorder="little")
                _same(h.search_dense_range(Q, 50, r, f, packed), want, "host, host mask")
                _same_where_proven(_dev_range(h, Q, 50, r, f, m), want, "device")
                if m is not None:
                    import torch
                    dm = torch.from_numpy(packed).cuda()
                    _same(h.search_dense_range(Q, 50, r, f, None, dm.data_ptr()), want, "host, device mask")
        finally:
            h.close()


@pytest.mark.parametrize("metric", METRICS, ids=METRIC_IDS)
def test_nan_and_empty_intervals_are_refused_and_write_nothing(gpu, metric):
    X, Q = _random(500, 32, 3, np.float16, 500)
    h = _shard(X, nat.HR_F16, metric)
    lib = nat.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    good = (1.0, 0.2) if metric == ry.L2 else (0.2, 1.0)
    try:
        for bad_q, (r, f) in ((1, (np.nan, good[1])), (2, (good[0], np.nan)), (0, (good[1], good[0])), (1, (0.5, 0.5))):
            radius, rfilter = np.full(3, good[0]), np.full(3, good[1])
            radius[bad_q], rfilter[bad_q] = r, f
            ids = np.full((3, 8), 123456789, np.int64)
            sc = np.full((3, 8), 7.5, np.float32)
            rc = lib.hr_search_dense_range(h._h, vp(Q), 3, 8, None, 0, vp(radius), vp(rfilter), vp(ids), vp(sc))
            assert rc == 1                                      # HR_EINVAL
            assert f"query {bad_q}" in lib.hr_last_error(h._h).decode()
            assert np.all(ids == 123456789) and np.all(sc == 7.5)
        with pytest.raises(ValueError):
            h.search_dense_range(Q, 8, good[1], good[0])
        with pytest.raises(ValueError):
            h.search_dense_range(Q, 8, np.array([0.1, np.nan, 0.1]), None)
    finally:
        h.close()
