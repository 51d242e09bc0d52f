"""HR_METRIC_L2 through the C ABI against the numpy yardstick (tests/l2_yardstick.py): ids equal, score bits equal,
no tolerance anywhere.  L2 routing: dense_scan_kernel up to 16 * G queries (G = 4 groups while the query tile fits LDS),
dense_scan_bigq_kernel in passes of 128 beyond and for rows too long for the tile."""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat

from l2_yardstick import bits, l2_search

pytestmark = pytest.mark.gpu

DTYPES = [(nat.HR_F16, np.float16), (nat.HR_F32, np.float32)]


@contextlib.contextmanager
def option(key, value):
    nat.debug_option(key, value)
    try:
        yield
    finally:
        nat.debug_option(key, 0)


def _shard(X, dtype, sparse_dim=0):
    h = nat.ShardHandle(X.shape[1], dtype, nat.HR_METRIC_L2, sparse_dim)
    h.add_dense(X)
    h.finalize()
    return h


def _check(h, X, Q, k, mask=None):
    ids, sc = h.search_dense(Q, k, mask)
    oids, osc = l2_search(X, Q, k, mask)
    assert np.array_equal(ids, oids), f"ids differ: {np.argwhere(ids != oids)[:5]}"
    assert np.array_equal(bits(sc), bits(osc))


def _dev_search(h, Q, k):
    import torch
    B = Q.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((B,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    h.search_dense_dev(dq.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def _check_flagged(h, X, Q, k):
    """Device form: wherever the flag is 1 the list is the yardstick's.  -> the flags."""
    ids, sc, fl = _dev_search(h, Q, k)
    oids, osc = l2_search(X, Q, k)
    for b in np.nonzero(fl == 1)[0]:
        assert np.array_equal(ids[b], oids[b]), f"query {b}: proven list differs"
        assert np.array_equal(bits(sc[b]), bits(osc[b])), f"query {b}: proven scores differ"
    return fl


def _data(n, d, B, np_dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32).astype(np_dtype)
    Q = rng.standard_normal((B, d)).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
@pytest.mark.parametrize("n,d,B,k", [(1000, 384, 1, 40), (1000, 384, 7, 20), (5000, 96, 33, 40), (64, 128, 3, 100),
                                     (20000, 768, 64, 40), (3, 100, 2, 5)])
def test_l2_matches_yardstick(gpu, dtype, np_dtype, n, d, B, k):
    X, Q = _data(n, d, B, np_dtype, n + d + B)
    h = _shard(X, dtype)
    _check(h, X, Q, k)
    h.close()


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 16, 17, 64, 65, 128, 129, 256, 300])
def test_l2_batch_sizes_across_kernel_boundaries(gpu, dtype, np_dtype, B):
    X, Q = _data(3000, 200, B, np_dtype, 100 + B)
    h = _shard(X, dtype)
    _check(h, X, Q, 20)
    fl = _check_flagged(h, X, Q, 20)
    assert fl.shape == (B,)
    h.close()


@pytest.mark.parametrize("B", [5, 48, 49, 130])
def test_l2_d1024_fp16(gpu, B):
    X, Q = _data(4000, 1024, B, np.float16, 1024 + B)
    h = _shard(X, nat.HR_F16)
    _check(h, X, Q, 40)
    h.close()


@pytest.mark.parametrize("B", [1, 20])
def test_l2_long_fp32_rows_take_the_k_chunked_pass(gpu, B):
    X, Q = _data(700, 3000, B, np.float32, 3000 + B)     # KT > 156: no LDS-resident query tile
    h = _shard(X, nat.HR_F32)
    _check(h, X, Q, 30)
    _check_flagged(h, X, Q, 30)
    h.close()


@pytest.mark.parametrize("group_rows", [16, 64])
@pytest.mark.parametrize("finish_mode", [1, 2])
@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_l2_group_rows_and_finish_paths(gpu, group_rows, finish_mode, dtype, np_dtype):
    with option(nat.HR_DEBUG_GROUP_ROWS, group_rows), option(nat.HR_DEBUG_FINISH_MODE, finish_mode):
        for n, d, B, k in ((9001, 128, 9, 40), (9001, 128, 140, 40), (30, 128, 4, 40), (6000, 64, 3, 256)):
            X, Q = _data(n, d, B, np_dtype, n + B + group_rows)
            h = _shard(X, dtype)
            _check(h, X, Q, k)                      # n < k: -1 / +0 padding; k = 256
            _check_flagged(h, X, Q, k)
            h.close()


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_l2_incremental_add_and_rowmask(gpu, dtype, np_dtype):
    rng = np.random.default_rng(7)
    X, Q = _data(3001, 200, 5, np_dtype, 7)
    h = nat.ShardHandle(200, dtype, nat.HR_METRIC_L2)
    done = 0
    for a, b in ((0, 1), (1, 18), (18, 1500), (1500, 3001)):  # ragged appends, a finalize (and a search) between them
        h.add_dense(X[a:b])
        h.finalize()
        done = b
        _check(h, X[:done], Q, 40)
    allow = rng.random(3001) < 0.3
    mask = np.packbits(allow, bitorder="little")
    _check(h, X, Q, 40, mask)
    Qb = rng.standard_normal((150, 200)).astype(np.float32)
    _check(h, X, Qb, 40, mask)
    ids, sc = h.search_dense(Q, 10, np.zeros_like(mask))
    assert (ids == -1).all() and (bits(sc) == 0).all()
    h.close()


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_l2_ties_and_degenerate_inputs(gpu, dtype, np_dtype):
    rng = np.random.default_rng(3)
    base = rng.standard_normal((50, 64)).astype(np.float32).astype(np_dtype)
    X = np.concatenate([base, base, np.zeros((20, 64), np_dtype), base])
    Q = np.concatenate([base[:3].astype(np.float32), np.zeros((1, 64), np.float32)])   # duplicates of rows; a zero query
    h = _shard(X, dtype)
    _check(h, X, Q, 30)
    ids, sc = h.search_dense(Q, 30)
    for b in range(3):                                         # distance exactly +0 first, lowest id first
        assert ids[b, :3].tolist() == [b, 50 + b, 120 + b] and (bits(sc[b, :3]) == 0).all()
    assert ids[3, :20].tolist() == list(range(100, 120)) and (bits(sc[3, :20]) == 0).all()   # zero query: D = |x|^2
    _check_flagged(h, X, Q, 30)
    h.close()
    # many rows at ONE distance straddling the k-th place: +-e_j scaled, all at the same distance from the query
    d = 64
    E = np.zeros((2 * d, d), np.float32)
    E[np.arange(d), np.arange(d)] = 2.0
    E[d + np.arange(d), np.arange(d)] = -2.0
    X = np.concatenate([np.tile(E, (20, 1)), rng.standard_normal((500, d)).astype(np.float32) * 0.25]).astype(np_dtype)
    Q = np.zeros((2, d), np.float32)
    Q[1] = 1e-3
    h = _shard(X, dtype)
    for k in (10, 100, 256):
        _check(h, X, Q, k)
        _check_flagged(h, X, Q, k)
    h.close()
    # row norms from 1e-2 to 1e2 in one shard
    X = rng.standard_normal((6000, 96)).astype(np.float32)
    X *= (10.0 ** rng.uniform(-2, 2, size=(6000, 1)) / np.sqrt(96)).astype(np.float32)
    X = X.astype(np_dtype)
    Q = np.concatenate([rng.standard_normal((4, 96)).astype(np.float32) * s for s in (0.01, 1.0, 30.0)])
    h = _shard(X, dtype)
    _check(h, X, Q, 40)
    _check_flagged(h, X, Q, 40)
    h.close()


@pytest.mark.parametrize("dtype,np_dtype", DTYPES)
def test_l2_cancellation_far_from_the_origin(gpu, dtype, np_dtype):
    """Rows and queries c + 1e-3 * noise with |c| about 30: D is tiny against |x|^2.  The host form must still be exact;
    the device form may leave lists unproven (flags 0) and nothing is asserted about how many."""
    rng = np.random.default_rng(30)
    d = 128
    c = rng.standard_normal(d).astype(np.float32)
    c *= 30.0 / np.linalg.norm(c)
    X = (c + 1e-3 * rng.standard_normal((5000, d)).astype(np.float32)).astype(np_dtype)
    Q = (c + 1e-3 * rng.standard_normal((9, d)).astype(np.float32)).astype(np.float32)
    h = _shard(X, dtype)
    _check(h, X, Q, 40)
    fl = _check_flagged(h, X, Q, 40)
    print(f"cancellation case, dtype {dtype}: {int(fl.sum())} of {len(fl)} lists proven by the device form")
    h.close()


def test_l2_device_form_proves_lists_on_ordinary_data(gpu):
    n, d, B, k = 20000, 768, 64, 40
    X, Q = _data(n, d, B, np.float16, 2024)
    h = _shard(X, nat.HR_F16)
    fl = _check_flagged(h, X, Q, k)
    h.close()
    hip = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_IP)
    hip.add_dense(X)
    hip.finalize()
    _, _, fl_ip = _dev_search(hip, Q, k)
    hip.close()
    print(f"proven lists on N(0,1) 20000 x 768 fp16, B = 64, k = 40: L2 {fl.mean():.3f}, IP {fl_ip.mean():.3f}")
    assert fl.sum() >= 1


def test_l2_snapshot_round_trip(gpu, tmp_path):
    X, Q = _data(2500, 160, 6, np.float16, 99)
    h = _shard(X, nat.HR_F16)
    want = h.search_dense(Q, 25)
    path = str(tmp_path / "l2.hbmrag")
    h.save(path)
    h.close()
    h2 = nat.ShardHandle.load(path, 160, nat.HR_F16, nat.HR_METRIC_L2)
    metric = ctypes.c_int32(-1)
    assert nat.load_library().hr_get_info(h2._h, None, None, ctypes.byref(metric), None) == 0 and metric.value == nat.HR_METRIC_L2
    got = h2.search_dense(Q, 25)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    _check(h2, X, Q, 25)
    h2.add_dense(X[:100])                                      # the loaded shard keeps growing as an L2 shard
    h2.finalize()
    _check(h2, np.concatenate([X, X[:100]]), Q, 25)
    h2.close()
    with pytest.raises(ValueError):
        nat.ShardHandle.load(path, 160, nat.HR_F16, nat.HR_METRIC_COSINE)


def _sparse_corpus(n, V, nnz, B, seed):
    rng = np.random.default_rng(seed)
    idx = np.stack([np.sort(rng.choice(V, nnz, replace=False)) for _ in range(n)]).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(n * nnz)).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * nnz
    SQ = [(np.sort(rng.choice(V, nnz, replace=False)).astype(np.int32), np.abs(rng.standard_normal(nnz)).astype(np.float32))
          for _ in range(B)]
    return ptr, idx, val, SQ


@pytest.mark.parametrize("B", [6, 70])
def test_l2_hybrid_forms(gpu, B):
    import torch
    from advanced_rag.engine import pack_sparse_queries
    n, d, V, nnz, k = 5000, 96, 800, 12, 40
    X, Q = _data(n, d, B, np.float16, 500 + B)
    ptr, idx, val, SQ = _sparse_corpus(n, V, nnz, B, 600 + B)
    h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_L2, V)
    h.add_dense(X)
    h.add_sparse(ptr, idx, val)
    h.finalize()
    want_d = l2_search(X, Q, k)
    want_s = oracle.sparse_search(ptr, idx, val, SQ, k, 0.2)
    dq = torch.from_numpy(Q).cuda()
    p, i_, v_, mx = pack_sparse_queries(SQ, 0.2)
    dp, di_, dv_ = torch.from_numpy(p).cuda(), torch.from_numpy(i_).cuda(), torch.from_numpy(v_).cuda()
    st = torch.cuda.current_stream()

    def check(ids, sc, fl):
        ids, sc, fl = ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()
        for m, (wi, ws) in enumerate((want_d, want_s)):
            for b in np.nonzero(fl[m] == 1)[0]:
                assert np.array_equal(ids[m, b], wi[b]) and np.array_equal(bits(sc[m, b]), bits(ws[b]))
        assert fl[0].sum() >= 1 and fl[1].sum() >= 1

    ids = torch.empty((2, B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((2, B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((2, B), dtype=torch.int32, device="cuda")
    h.search_hybrid_dev(dq.data_ptr(), dp.data_ptr(), di_.data_ptr(), dv_.data_ptr(), B, len(i_), mx, k, ids.data_ptr(),
                        sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    check(ids, sc, fl)
    ids.fill_(-7)
    sc.fill_(-7.0)
    fl.zero_()
    h.hybrid_prep_dev(dq.data_ptr(), dp.data_ptr(), di_.data_ptr(), dv_.data_ptr(), B, len(i_), mx, k, 1, st.cuda_stream)
    h.hybrid_scan_dev(dq.data_ptr(), dp.data_ptr(), di_.data_ptr(), dv_.data_ptr(), B, len(i_), mx, k, 1, st.cuda_stream)
    h.hybrid_finish_dev(dq.data_ptr(), dp.data_ptr(), di_.data_ptr(), dv_.data_ptr(), B, mx, k, 1, ids.data_ptr(),
                        sc.data_ptr(), fl.data_ptr(), st.cuda_stream)
    st.synchronize()
    check(ids, sc, fl)
    # and the host forms of the same handle
    _check(h, X, Q, k)
    si, ss = h.search_sparse(SQ, k, 0.2)
    assert np.array_equal(si, want_s[0]) and np.array_equal(bits(ss), bits(want_s[1]))
    h.close()
