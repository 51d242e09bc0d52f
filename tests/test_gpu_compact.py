"""hr_compact through the C ABI (include/hbmrag.h, csrc/compact.h): a compacted handle against a handle built from the
surviving rows alone — byte-identical snapshots, the oracle's search results, the bounds of the exactness proofs, the
contract's edges, and the HBM that comes back.  Snapshot layout as in tests/test_gpu_store_lifecycle.py."""
import ctypes
import hashlib

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.engine import pack_sparse_queries

from l2_yardstick import l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, V = 1025, 300   # off the 16- and 64-row grids
OFFSET = 1000      # hr_set_row_offset of every handle here: ids must carry it unchanged


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np_dtype(dtype):
    return np.float16 if dtype == nat.HR_F16 else np.float32


def _dense(rng, n, d, dtype):
    return rng.standard_normal((n, d)).astype(np.float32).astype(_np_dtype(dtype))


def _sparse(rng, n, v=V, max_nnz=6, signed=True):
    """CSR of n rows with 0 .. max_nnz entries each (some rows empty), indices ascending and unique in a row."""
    lens = rng.integers(0, max_nnz + 1, size=n)
    lens[::17] = 0
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(v, m, replace=False)) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = (np.abs(rng.standard_normal(int(ptr[-1]))) + 0.01).astype(np.float32)
    if signed:
        val[rng.random(val.shape[0]) < 0.1] *= -1
    return ptr, idx, val


def _csr_rows(csr, keep):
    """The rows of a CSR that the boolean `keep` names, as a CSR from 0."""
    ptr, idx, val = csr
    rows = np.nonzero(keep)[0]
    lens = (ptr[1:] - ptr[:-1])[rows]
    new_ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=new_ptr[1:])
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    return new_ptr, idx[take], val[take]


def _build(X, csr, dtype, metric, v=V, offset=OFFSET):
    h = nat.ShardHandle(0 if X is None else X.shape[1], dtype, metric, v if csr is not None else 0)
    h.set_row_offset(offset)
    if X is not None and len(X):
        h.add_dense(X)
    if csr is not None and len(csr[0]) > 1:
        h.add_sparse(*csr)
    h.finalize()
    return h


def _saved(h, path):
    h.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def _header(blob):
    """Fields of the snapshot header by name."""
    i64 = lambda at: int(np.frombuffer(blob, np.int64, 1, at)[0])
    f32 = lambda at: np.frombuffer(blob, np.float32, 1, at)[0]
    return {"n_rows": i64(40), "cap_rows": i64(48), "n_sparse": i64(56), "nnz": i64(64), "row_offset": i64(72),
            "max_row_norm": f32(80), "max_sparse_abs": f32(84)}


def _device_mask(keep):
    """8 * ceil(n / 64) bytes in HBM, as hr_filter_eval_dev writes its masks."""
    buf = np.zeros(8 * ((len(keep) + 63) // 64), np.uint8)
    packed = np.packbits(keep, bitorder="little")
    buf[: packed.size] = packed
    return torch.from_numpy(buf).cuda()


def _leave_used_blocks(rng, d, dtype):
    """Stores filled to their last row at the capacities the compacted handles will take, then closed: the allocator
    hands freed blocks out again, so a new buffer that was not zeroed beyond the survivors shows what these held."""
    for m in (64, 128, 512, 768, 1088):
        h = nat.ShardHandle(d, dtype, nat.HR_METRIC_IP)
        h.reserve(m)
        h.add_dense(_dense(rng, m, d, dtype) + _np_dtype(dtype)(3))
        h.finalize()
        h.close()


def _masks(rng, n):
    random70 = rng.random(n) < 0.7
    every_other = np.arange(n) % 2 == 0
    edges = np.ones(n, bool)
    edges[:64] = False                  # the whole first super-group
    edges[n - n % 16 if n % 16 else n - 16:] = False   # the ragged last row block
    last = np.zeros(n, bool)
    last[-1] = True
    k64 = np.zeros(n, bool)
    k64[rng.choice(n, 64, replace=False)] = True
    k65 = np.zeros(n, bool)
    k65[rng.choice(n, 65, replace=False)] = True
    return {"random70": random70, "every_other": every_other, "edges": edges, "last_only": last, "keep64": k64, "keep65": k65}


@pytest.mark.parametrize("metric", [nat.HR_METRIC_COSINE, nat.HR_METRIC_IP, nat.HR_METRIC_L2], ids=["COSINE", "IP", "L2"])
@pytest.mark.parametrize("d,dtype", [(32, nat.HR_F16), (200, nat.HR_F16), (40, nat.HR_F32)], ids=["d32_f16", "d200_f16", "d40_f32"])
def test_compacted_equals_fresh_build_byte_for_byte(gpu, tmp_path, d, dtype, metric):
    rng = np.random.default_rng(1000 + d + metric)
    X = _dense(rng, N, d, dtype)
    csr = _sparse(rng, N)
    for name, keep in _masks(rng, N).items():
        _leave_used_blocks(rng, d, dtype)
        fresh = _build(X[keep], _csr_rows(csr, keep), dtype, metric)
        want = _saved(fresh, tmp_path / "fresh.hbmrag")
        fresh.close()
        for form in ("host", "device"):
            h = _build(X, csr, dtype, metric)
            if form == "host":
                got_counts = h.compact(keep)
            else:
                d_keep = _device_mask(keep)
                got_counts = h.compact(d_keep=d_keep.data_ptr())
            assert got_counts == (int(keep.sum()), int(keep.sum())), (name, form)
            assert (h.num_rows, h.num_sparse_rows) == got_counts, (name, form)
            got = _saved(h, tmp_path / "compacted.hbmrag")
            h.close()
            assert _header(got) == _header(want), (name, form)
            assert len(got) == len(want), (name, form)
            assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest(), (name, form)


def test_scans_that_span_blocks(gpu, tmp_path):
    """70 001 rows: the row map's scan runs over 1 094 mask words (two blocks of 1 024) and the CSR's over about 49 000
    surviving rows (48 blocks), so the block sums and their prefix carry real values; the first block keeps nothing and
    one block keeps everything."""
    rng = np.random.default_rng(23)
    n, d = 70_001, 32
    X = _dense(rng, n, d, nat.HR_F16)
    csr = _sparse(rng, n)
    keep = rng.random(n) < 0.7
    keep[:2048] = False
    keep[4096:4096 + 1024 * 3] = True
    h = _build(X, csr, nat.HR_F16, nat.HR_METRIC_COSINE)
    m = int(keep.sum())
    assert h.compact(d_keep=_device_mask(keep).data_ptr()) == (m, m)
    fresh = _build(X[keep], _csr_rows(csr, keep), nat.HR_F16, nat.HR_METRIC_COSINE)
    got, want = _saved(h, tmp_path / "a.hbmrag"), _saved(fresh, tmp_path / "b.hbmrag")
    assert _header(got) == _header(want)
    assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest()
    h.close()
    fresh.close()


def _sparse_dev(h, SQ, k):
    p, i_, v_, mx = pack_sparse_queries(SQ, 0.0)
    dp, di, dv = (torch.from_numpy(a).cuda() for a in (p, i_, v_))
    B = len(SQ)
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((B,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    h.search_sparse_dev(dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, len(i_), mx, k, ids.data_ptr(), sc.data_ptr(),
                        fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def test_bounds_shrink_with_the_dropped_rows(gpu, tmp_path):
    """The row with the largest norm, the entry with the largest |weight| and the only negative weights are dropped: the
    header's bounds and the sparse device form's exactness flags are those of the fresh build."""
    rng = np.random.default_rng(7)
    d, k = 32, 10
    X = _dense(rng, N, d, nat.HR_F16)
    X[7] *= np.float16(40)
    ptr, idx, val = _sparse(rng, N, signed=False)
    big = int(ptr[300])          # first entry of a row that has entries
    row_big = int(np.searchsorted(ptr, big, side="right") - 1)
    val[big] = 900.0
    neg_rows = [r for r in (500, 501, 502, 503, 504, 505) if ptr[r + 1] > ptr[r]][:2]
    assert neg_rows
    for r in neg_rows:
        val[ptr[r]:ptr[r + 1]] *= -1
    keep = rng.random(N) < 0.8
    keep[[7, row_big] + neg_rows] = False
    keep[[8, row_big + 1]] = True
    csr = (ptr, idx, val)
    fresh = _build(X[keep], _csr_rows(csr, keep), nat.HR_F16, nat.HR_METRIC_IP)
    h = _build(X, csr, nat.HR_F16, nat.HR_METRIC_IP)
    before = _header(_saved(h, tmp_path / "before.hbmrag"))
    h.compact(keep)
    got, want = _header(_saved(h, tmp_path / "after.hbmrag")), _header(_saved(fresh, tmp_path / "fresh.hbmrag"))
    print("max_row_norm", before["max_row_norm"], "->", got["max_row_norm"], "fresh", want["max_row_norm"])
    print("max_sparse_abs", before["max_sparse_abs"], "->", got["max_sparse_abs"], "fresh", want["max_sparse_abs"])
    assert got["max_row_norm"] == want["max_row_norm"] and got["max_row_norm"] < before["max_row_norm"]
    assert got["max_sparse_abs"] == want["max_sparse_abs"] and got["max_sparse_abs"] < before["max_sparse_abs"] == 900.0
    SQ = [(np.sort(rng.choice(V, 8, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(8)) + 0.1).astype(np.float32))
          for _ in range(12)]
    a, b = _sparse_dev(h, SQ, k), _sparse_dev(fresh, SQ, k)
    assert np.array_equal(a[2], b[2]), "exactness flags differ from the fresh build's"
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    h.close()
    fresh.close()


def _check_all_forms(h, X, csr, Q, SQ, k, metric):
    """Host forms, hr_search_hybrid_dev and the phased form against the oracle over (X, csr), ids with OFFSET."""
    if metric == nat.HR_METRIC_L2:
        want_d = l2_search(X, Q, k, None, OFFSET)
    else:
        want_d = oracle.dense_search(X, Q, k, oracle.COSINE if metric == nat.HR_METRIC_COSINE else oracle.IP, None, OFFSET)
    want_s = oracle.sparse_search(*csr, SQ, k, 0.0, None, OFFSET)
    ids, sc = h.search_dense(Q, k)
    assert np.array_equal(ids, want_d[0]) and np.array_equal(_bits(sc), _bits(want_d[1]))
    ids, sc = h.search_sparse(SQ, k, 0.0)
    assert np.array_equal(ids, want_s[0]) and np.array_equal(_bits(sc), _bits(want_s[1]))
    B = Q.shape[0]
    dq = torch.from_numpy(Q).cuda()
    p, i_, v_, mx = pack_sparse_queries(SQ, 0.0)
    dp, di, dv = (torch.from_numpy(a).cuda() for a in (p, i_, v_))
    st = torch.cuda.current_stream()
    ids = torch.empty((2, B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((2, B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((2, B), dtype=torch.int32, device="cuda")

    def check():
        i, s, f = ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()
        for m, (wi, ws) in enumerate((want_d, want_s)):
            for b in np.nonzero(f[m] == 1)[0]:
                assert np.array_equal(i[m, b], wi[b]) and np.array_equal(_bits(s[m, b]), _bits(ws[b])), (m, b)
        assert f[0].sum() >= 1 and f[1].sum() >= 1
    h.search_hybrid_dev(dq.data_ptr(), dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, len(i_), mx, k, ids.data_ptr(),
                        sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    check()
    ids.fill_(-7)
    sc.fill_(-7.0)
    fl.zero_()
    h.hybrid_scan_dev(dq.data_ptr(), dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, len(i_), mx, k, 1, st.cuda_stream)
    h.hybrid_finish_dev(dq.data_ptr(), dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, mx, k, 1, ids.data_ptr(),
                        sc.data_ptr(), fl.data_ptr(), st.cuda_stream)
    st.synchronize()
    check()


@pytest.mark.parametrize("metric", [nat.HR_METRIC_COSINE, nat.HR_METRIC_L2], ids=["COSINE", "L2"])
def test_searches_after_compaction_and_after_a_later_append(gpu, tmp_path, metric):
    rng = np.random.default_rng(11 + metric)
    d, k, B = 200, 10, 6
    X = _dense(rng, N, d, nat.HR_F16)
    csr = _sparse(rng, N)
    keep = rng.random(N) < 0.7
    Q = rng.standard_normal((B, d)).astype(np.float32)
    Q[0] = X[np.nonzero(keep)[0][5]].astype(np.float32)
    SQ = [(np.sort(rng.choice(V, 8, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(8)) + 0.1).astype(np.float32))
          for _ in range(B)]
    h = _build(X, csr, nat.HR_F16, metric)
    h.search_dense(Q, k)     # workspaces sized for the old shard exist
    h.compact(keep)
    Xs, csr_s = X[keep], _csr_rows(csr, keep)
    _check_all_forms(h, Xs, csr_s, Q, SQ, k, metric)
    # 100 more rows: the dense store grows from the exact capacity, the CSR from its exact size
    X2 = _dense(rng, 100, d, nat.HR_F16)
    csr2 = _sparse(rng, 100)
    h.add_dense(X2)
    h.add_sparse(*csr2)
    h.finalize()
    Xa = np.concatenate([Xs, X2])
    csr_a = (np.concatenate([csr_s[0], csr2[0][1:] + csr_s[0][-1]]), np.concatenate([csr_s[1], csr2[1]]),
             np.concatenate([csr_s[2], csr2[2]]))
    _check_all_forms(h, Xa, csr_a, Q, SQ, k, metric)
    fresh = _build(Xa, csr_a, nat.HR_F16, metric)
    assert _saved(h, tmp_path / "a.hbmrag") == _saved(fresh, tmp_path / "b.hbmrag")
    h.close()
    fresh.close()


@pytest.fixture(scope="module")
def range_corpus():
    """40 000 sparse-only rows, V = 64, 3 entries per row; term 0 sits in more than half of the rows (the dense-run form
    of the postings)."""
    rng = np.random.default_rng(13)
    n, v = 40_000, 64
    idx = np.empty((n, 3), np.int32)
    has0 = rng.random(n) < 0.7
    idx[:, 0] = np.where(has0, 0, rng.integers(1, 20, n))
    idx[:, 1] = rng.integers(20, 40, n)
    idx[:, 2] = rng.integers(40, 64, n)
    val = (np.abs(rng.standard_normal(n * 3)) + 0.01).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * 3
    SQ = [(np.array([0, 25, 50], np.int32), np.array([1.0, 0.5, 0.25], np.float32)),
          (np.array([3, 30, 41, 63], np.int32), np.array([0.3, 1.5, 0.7, 0.2], np.float32))]
    return (ptr, idx.reshape(-1), val), SQ, rng.permutation(n)


@pytest.mark.parametrize("survivors", [16384, 16385, 32769])
def test_sparse_range_edges(gpu, tmp_path, range_corpus, survivors):
    csr, SQ, order = range_corpus
    n, k = len(csr[0]) - 1, 10
    keep = np.zeros(n, bool)
    keep[order[:survivors]] = True
    h = _build(None, csr, nat.HR_F16, nat.HR_METRIC_COSINE, v=64)
    assert h.compact(keep) == (0, survivors)
    csr_s = _csr_rows(csr, keep)
    want = oracle.sparse_search(*csr_s, SQ, k, 0.0, None, OFFSET)
    ids, sc = h.search_sparse(SQ, k, 0.0)
    assert np.array_equal(ids, want[0]) and np.array_equal(_bits(sc), _bits(want[1]))
    fresh = _build(None, csr_s, nat.HR_F16, nat.HR_METRIC_COSINE, v=64)
    a, b = _sparse_dev(h, SQ, k), _sparse_dev(fresh, SQ, k)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _saved(h, tmp_path / "a.hbmrag") == _saved(fresh, tmp_path / "b.hbmrag")
    h.close()
    fresh.close()


def test_contract_edges(gpu, tmp_path):
    rng = np.random.default_rng(17)
    d, k = 32, 5
    X = _dense(rng, N, d, nat.HR_F16)
    csr = _sparse(rng, N)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    SQ = [(np.array([1, 7, 100], np.int32), np.array([1.0, 0.5, 0.25], np.float32))] * 3
    lib = nat.load_library()

    # keep-all: nothing changes, capacity included
    h = _build(X, csr, nat.HR_F16, nat.HR_METRIC_COSINE)
    before, dev_bytes = _saved(h, tmp_path / "0.hbmrag"), h.device_bytes
    assert h.compact(np.ones(N, bool)) == (N, N)
    assert _saved(h, tmp_path / "1.hbmrag") == before and h.device_bytes == dev_bytes
    # NULL mask / NULL handle
    assert lib.hr_compact(h._h, None, 0, None, None) == 1
    assert lib.hr_compact(None, None, 0, None, None) == 1
    assert _saved(h, tmp_path / "2.hbmrag") == before
    # an unfinalized handle is refused and stays as it was
    h.add_dense(X[:3])
    h.add_sparse(*_csr_rows(csr, np.arange(N) < 3))
    with pytest.raises(nat.HbmRagError) as e:
        h.compact(np.zeros(N + 3, bool))
    assert e.value.status == 2
    assert (h.num_rows, h.num_sparse_rows) == (N + 3, N + 3)
    h.finalize()
    first3 = _csr_rows(csr, np.arange(N) < 3)
    again = _build(np.concatenate([X, X[:3]]), (np.concatenate([csr[0], first3[0][1:] + csr[0][-1]]),
                                                 np.concatenate([csr[1], first3[1]]), np.concatenate([csr[2], first3[2]])),
                   nat.HR_F16, nat.HR_METRIC_COSINE)
    assert _saved(h, tmp_path / "2a.hbmrag") == _saved(again, tmp_path / "2b.hbmrag")
    again.close()

    # keep-none: an empty finalized handle that answers with padded lists and takes appends
    assert h.compact(np.zeros(N + 3, bool)) == (0, 0)
    assert (h.num_rows, h.num_sparse_rows) == (0, 0)
    ids, sc = h.search_dense(Q, k)
    assert (ids == -1).all() and (sc == 0).all()
    ids, sc = h.search_sparse(SQ, k, 0.0)
    assert (ids == -1).all() and (sc == 0).all()
    empty = _build(X[:0], _csr_rows(csr, np.zeros(N, bool)), nat.HR_F16, nat.HR_METRIC_COSINE)
    assert _saved(h, tmp_path / "3.hbmrag") == _saved(empty, tmp_path / "4.hbmrag")
    empty.close()
    h.add_dense(X[:200])
    h.add_sparse(*_csr_rows(csr, np.arange(N) < 200))
    h.finalize()
    want = oracle.dense_search(X[:200], Q, k, oracle.COSINE, None, OFFSET)
    ids, sc = h.search_dense(Q, k)
    assert np.array_equal(ids, want[0]) and np.array_equal(_bits(sc), _bits(want[1]))
    want = oracle.sparse_search(*_csr_rows(csr, np.arange(N) < 200), SQ, k, 0.0, None, OFFSET)
    ids, sc = h.search_sparse(SQ, k, 0.0)
    assert np.array_equal(ids, want[0]) and np.array_equal(_bits(sc), _bits(want[1]))
    h.close()

    # dense-only and sparse-only handles
    keep = rng.random(N) < 0.5
    for Xp, cp in ((X, None), (None, csr)):
        h = _build(Xp, cp, nat.HR_F16, nat.HR_METRIC_COSINE)
        m = int(keep.sum())
        assert h.compact(keep) == ((m, 0) if cp is None else (0, m))
        fresh = _build(None if Xp is None else Xp[keep], None if cp is None else _csr_rows(cp, keep), nat.HR_F16, nat.HR_METRIC_COSINE)
        assert _saved(h, tmp_path / "5.hbmrag") == _saved(fresh, tmp_path / "6.hbmrag")
        h.close()
        fresh.close()


def test_hbm_comes_back(gpu):
    """400 000 x 64 fp16 rows (tiles + scale + norm2 about 56 MB), three quarters dropped: the driver's free memory rises
    by at least 32 MiB across the call (about 42 MB expected; the margin is allocation granularity), hr_device_bytes
    falls to at most a fresh reservation's, and eight create / compact / close cycles leak nothing (8 MiB, the bound of
    tests/test_gpu_store_lifecycle.py)."""
    rng = np.random.default_rng(19)
    n, d = 400_000, 64
    X = rng.standard_normal((n, d)).astype(np.float16)
    keep = np.arange(n) % 4 == 0
    torch.cuda.synchronize()
    free = []
    for cycle in range(8):
        h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_IP)
        h.add_dense(X)
        h.finalize()
        before, bytes_before = torch.cuda.mem_get_info()[0], h.device_bytes
        assert h.compact(keep) == (n // 4, 0)
        after = torch.cuda.mem_get_info()[0]
        if cycle == 0:
            ref = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_IP)
            ref.reserve(n // 4)
            print("free memory gained:", after - before, "device_bytes", bytes_before, "->", h.device_bytes, "fresh reservation",
                  ref.device_bytes)
            assert after - before >= 32 << 20
            assert h.device_bytes <= ref.device_bytes
            ref.close()
        h.close()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each close:", free)
    assert abs(free[7] - free[0]) <= 8 << 20, free
