"""Deep search through the C ABI (hr_search_dense_deep, hr_search_sparse_deep) against the oracle at k = W sliced [offset:]:
oracle.dense_search / oracle.sparse_search, and for L2 the numpy yardstick over oracle.topk (tests/l2_yardstick.py).  Ids
equal, score bits equal."""
import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat

from l2_yardstick import bits, l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, B = 20_011, 128, 3          # not a multiple of 64 (nor of 16)
WS = [257, 1000, 16384]
METRICS = {"COSINE": nat.HR_METRIC_COSINE, "IP": nat.HR_METRIC_IP, "L2": nat.HR_METRIC_L2}
DTYPES = {"f16": (nat.HR_F16, np.float16), "f32": (nat.HR_F32, np.float32)}


def dense_want(Xs, Q, k, metric, mask=None, row_offset=0):
    if metric == nat.HR_METRIC_L2:
        return l2_search(Xs, Q, k, mask, row_offset)
    return oracle.dense_search(Xs, Q, k, metric, mask, row_offset)


def shard(Xs, dtype, metric, sparse_dim=0):
    h = nat.ShardHandle(Xs.shape[1], dtype, metric, sparse_dim)
    h.add_dense(Xs.astype(np.float32))
    h.finalize()
    return h


@pytest.fixture(scope="module")
def base():
    rng = np.random.default_rng(77)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)


def planted(X, Q, np_dtype, metric):
    """X in the shard's dtype with duplicates planted for query 0: the rows ranked 256 and 993 are copied over six rows of
    the ranking's tail each, which then rank beside them: runs of seven equal scores at positions 256 .. 262 and (the first
    run having moved the second source six places down) 999 .. 1005 — across the edges `offset` and W of the windows below."""
    Xs = X.astype(np_dtype)
    order = dense_want(Xs, Q[:1], N, metric)[0][0]
    tail = list(order[-12:])
    for pos in (256, 993):
        for _ in range(6):
            Xs[tail.pop()] = Xs[order[pos]]
    return Xs


@pytest.fixture(scope="module", params=[(d, m) for d in DTYPES for m in METRICS], ids=lambda p: f"{p[0]}-{p[1]}")
def dense_case(request, base):
    """One shard per (dtype, metric), its oracle ranking at depth 16384 for every query computed once."""
    dname, mname = request.param
    dtype, np_dtype = DTYPES[dname]
    X, Q = base
    Xs = planted(X, Q, np_dtype, METRICS[mname])
    h = shard(Xs, dtype, METRICS[mname])
    ref = dense_want(Xs, Q, nat.HR_MAX_DEEP_K, METRICS[mname])
    yield h, Xs, Q, METRICS[mname], ref
    h.close()


def same(got, want_ids, want_sc):
    assert np.array_equal(got[0], want_ids), f"ids differ at {np.argwhere(got[0] != want_ids)[:5]}"
    assert np.array_equal(bits(got[1]), bits(want_sc))


@pytest.mark.parametrize("W", WS)
def test_dense_deep_lists(gpu, dense_case, W):
    h, Xs, Q, metric, (rid, rsc) = dense_case
    same(h.search_dense_deep(Q, W), rid[:, :W], rsc[:, :W])                      # B = 3
    same(h.search_dense_deep(Q[:1], W), rid[:1, :W], rsc[:1, :W])                # one query
    for offset in sorted({1, 256, W - 1}):
        same(h.search_dense_deep(Q, W - offset, offset), rid[:, offset:W], rsc[:, offset:W])


def test_planted_ties_straddle_the_window_edges(gpu, dense_case):
    h, Xs, Q, metric, (rid, rsc) = dense_case
    sc0 = bits(rsc[0])
    assert sc0[256] == sc0[255] or sc0[256] == sc0[257]          # the case is what it claims: position 256 inside a run
    assert sc0[999] == sc0[998] or sc0[999] == sc0[1000]
    same(h.search_dense_deep(Q[:1], 744, 256), rid[:1, 256:1000], rsc[:1, 256:1000])
    same(h.search_dense_deep(Q[:1], 257), rid[:1, :257], rsc[:1, :257])
    same(h.search_dense_deep(Q[:1], 1, 256), rid[:1, 256:257], rsc[:1, 256:257])


def test_head_is_the_plain_list_and_pages_concatenate(gpu, dense_case):
    h, Xs, Q, metric, (rid, rsc) = dense_case
    deep = h.search_dense_deep(Q, 600)
    plain = h.search_dense(Q, 256)
    assert np.array_equal(deep[0][:, :256], plain[0]) and np.array_equal(bits(deep[1][:, :256]), bits(plain[1]))
    a, b = h.search_dense_deep(Q, 300, 0), h.search_dense_deep(Q, 300, 300)
    assert np.array_equal(np.concatenate([a[0], b[0]], 1), deep[0])
    assert np.array_equal(bits(np.concatenate([a[1], b[1]], 1)), bits(deep[1]))


def test_masks_host_and_device_and_device_bytes(gpu, dense_case):
    h, Xs, Q, metric, _ = dense_case
    rng = np.random.default_rng(5)
    keep = rng.random(N) < 1 / 3
    packed = np.packbits(keep, bitorder="little")
    want_ids, want_sc = dense_want(Xs, Q, 1000, metric, packed)
    held = h.device_bytes
    same(h.search_dense_deep(Q, 1000, 0, packed), want_ids, want_sc)
    d_mask = torch.zeros(8 * ((N + 63) // 64), dtype=torch.uint8, device="cuda")
    d_mask[:packed.size] = torch.from_numpy(packed).cuda()
    same(h.search_dense_deep(Q, 700, 300, None, d_mask.data_ptr()), want_ids[:, 300:], want_sc[:, 300:])
    assert h.device_bytes == held
    few = np.zeros(N, bool)
    few[rng.permutation(N)[:500]] = True                          # fewer rows pass than the window is long
    packed = np.packbits(few, bitorder="little")
    want_ids, want_sc = dense_want(Xs, Q, 1000, metric, packed)
    assert (want_ids[:, 500:] == -1).all()
    same(h.search_dense_deep(Q, 1000, 0, packed), want_ids, want_sc)


@pytest.mark.parametrize("mname", list(METRICS))
def test_short_shard_and_row_offset(gpu, base, mname):
    X, Q = base
    Xs = X[:300].astype(np.float16)
    h = shard(Xs, nat.HR_F16, METRICS[mname])
    try:
        h.set_row_offset(1_000_000)
        want_ids, want_sc = dense_want(Xs, Q, 1000, METRICS[mname], None, 1_000_000)
        assert (want_ids[:, 300:] == -1).all()
        same(h.search_dense_deep(Q, 1000), want_ids, want_sc)
        same(h.search_dense_deep(Q, 800, 200), want_ids[:, 200:], want_sc[:, 200:])
        same(h.search_dense_deep(Q, 10, 400), want_ids[:, 400:410], want_sc[:, 400:410])   # a window past the end: padding
    finally:
        h.close()


@pytest.mark.parametrize("dname", list(DTYPES))
def test_l2_near_duplicates_far_from_the_origin(gpu, dname):
    """Rows within a few ulps of one another at distance ~1e3 from the origin: the scan's bound cannot separate them (its
    error grows with the row norms); the deep path refines every row and does not care."""
    dtype, np_dtype = DTYPES[dname]
    rng = np.random.default_rng(11)
    n, d = 3001, 64
    centre = (rng.standard_normal(d) * 4 + 1000).astype(np.float32)
    X = (centre + rng.integers(-2, 3, (n, d)).astype(np.float32)).astype(np_dtype)   # exact in fp16: integers below 2048
    X[rng.permutation(n)[:40]] = X[0]                                               # and true duplicates
    Q = (centre + rng.standard_normal((2, d))).astype(np.float32)
    h = shard(X, dtype, nat.HR_METRIC_L2)
    try:
        want_ids, want_sc = l2_search(X, Q, 1000)
        same(h.search_dense_deep(Q, 1000), want_ids, want_sc)
        same(h.search_dense_deep(Q, 300, 700), want_ids[:, 700:], want_sc[:, 700:])
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------ sparse
NS_, V = 20_000, 1000


def sparse_corpus(signed):
    rng = np.random.default_rng(31 + signed)
    lens = rng.integers(15, 26, NS_)
    indptr = np.zeros(NS_ + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    step = np.array([1, 3, 7, 9, 11, 13, 17, 19])[rng.integers(0, 8, NS_)]        # coprime to 1000: distinct terms in a row
    start = rng.integers(0, V, NS_)
    idx = np.concatenate([np.sort((start[r] + step[r] * np.arange(lens[r])) % V) for r in range(NS_)]).astype(np.int32)
    val = (rng.integers(1, 64, idx.size) / 16).astype(np.float32)                  # coarse: equal scores are common
    if signed:
        val[rng.random(idx.size) < 0.3] *= -1
    return indptr, idx, val


@pytest.fixture(scope="module", params=[False, True], ids=["unsigned", "signed"])
def sparse_case(request):
    indptr, idx, val = sparse_corpus(request.param)
    h = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    h.add_sparse(indptr, idx, val)
    h.finalize()
    queries = [([3, 500], [1.0, 0.5]),                                             # some 800 docs hold one of the two terms
               (list(range(0, 40)), [1.0 + 0.25 * (i % 3) for i in range(40)]),
               ([7, 8, 900], [2.0, -1.0, 0.5])]
    ref = oracle.sparse_search(indptr, idx, val, queries, nat.HR_MAX_DEEP_K)
    yield h, (indptr, idx, val), queries, ref
    h.close()


@pytest.mark.parametrize("W", WS)
def test_sparse_deep_lists(gpu, sparse_case, W):
    h, csr, queries, (rid, rsc) = sparse_case
    assert 0 < (rid[0] >= 0).sum() < 1000                                          # fewer than W docs score above 0
    same(h.search_sparse_deep(queries, W), rid[:, :W], rsc[:, :W])
    same(h.search_sparse_deep(queries[:1], W), rid[:1, :W], rsc[:1, :W])
    for offset in sorted({1, 256, W - 1}):
        same(h.search_sparse_deep(queries, W - offset, offset), rid[:, offset:W], rsc[:, offset:W])


def test_sparse_head_pages_masks_and_drop_ratio(gpu, sparse_case):
    h, (indptr, idx, val), queries, (rid, rsc) = sparse_case
    deep = h.search_sparse_deep(queries, 600)
    plain = h.search_sparse(queries, 256)
    assert np.array_equal(deep[0][:, :256], plain[0]) and np.array_equal(bits(deep[1][:, :256]), bits(plain[1]))
    a, b = h.search_sparse_deep(queries, 300, 0), h.search_sparse_deep(queries, 300, 300)
    assert np.array_equal(np.concatenate([a[0], b[0]], 1), deep[0])
    keep = np.random.default_rng(9).random(NS_) < 1 / 3
    packed = np.packbits(keep, bitorder="little")
    held = h.device_bytes
    want = oracle.sparse_search(indptr, idx, val, queries, 1000, 0.0, packed)
    same(h.search_sparse_deep(queries, 1000, 0, 0.0, packed), *want)
    d_mask = torch.zeros(8 * ((NS_ + 63) // 64), dtype=torch.uint8, device="cuda")
    d_mask[:packed.size] = torch.from_numpy(packed).cuda()
    same(h.search_sparse_deep(queries, 700, 300, 0.0, None, d_mask.data_ptr()), want[0][:, 300:], want[1][:, 300:])
    want = oracle.sparse_search(indptr, idx, val, queries, 1000, 0.4)
    same(h.search_sparse_deep(queries, 1000, 0, 0.4), *want)
    assert h.device_bytes == held


def test_refusals_through_the_abi(gpu, dense_case, sparse_case):
    h, Xs, Q, metric, _ = dense_case
    for k, offset in ((16385, 0), (16000, 385)):
        with pytest.raises(nat.HbmRagError) as ei:
            h.search_dense_deep(Q, k, offset)
        assert ei.value.status == 5
    with pytest.raises(ValueError):
        h.search_dense_deep(Q, 10, -1)
    with pytest.raises(ValueError):
        h.search_dense_deep(Q, 0, 5)
    bad = Q.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        h.search_dense_deep(bad, 300)
    with pytest.raises(nat.HbmRagError):                                           # the plain forms keep their limit
        h.search_dense(Q, 300)
    hs = sparse_case[0]
    with pytest.raises(nat.HbmRagError) as ei:
        hs.search_sparse_deep(sparse_case[2], 16384, 1)
    assert ei.value.status == 5
    with pytest.raises(ValueError, match="non-finite"):
        hs.search_sparse_deep([([1, 2], [1.0, float("inf")])], 300)
    with pytest.raises(nat.HbmRagError):                                           # no dense collection on this handle
        hs.search_dense_deep(np.zeros((1, 0), np.float32), 300)
