"""hr_get_dense_rows / hr_get_dense_rows_dev (include/hbmrag.h, csrc/query.h): stored rows come back out of the tiles as
they were ingested — fp16 shards as X.astype(float16), whose rounding tests/test_gpu_dense_ingest_values.py pins — for
dimensions below one k-chunk group (8), with a ragged tile (24), at exact (128, 768) and ragged (136) multiples of four
tiles, and a row count that leaves the last row block ragged."""
import ctypes

import numpy as np
import pytest

from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 16 * 9 + 5
OFFSET = 1000
DIMS = [8, 24, 128, 136, 768]
DTYPES = [nat.HR_F16, nat.HR_F32]
SENTINEL = -77.25    # exact in fp16 and fp32, and far outside what standard normal rows hold


def _rows(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _stored(X, dtype):
    """What the shard holds, widened: the fp32 rows themselves, or their fp16 roundings."""
    return X.astype(np.float16).astype(np.float32) if dtype == nat.HR_F16 else X


def _build(X, dtype, reserve=0, finalize=True):
    h = nat.ShardHandle(X.shape[1], dtype, nat.HR_METRIC_IP)
    h.set_row_offset(OFFSET)
    if reserve:
        h.reserve(reserve)
    h.add_dense(X)
    if finalize:
        h.finalize()
    return h


def _id_lists(rng, n):
    asc = np.arange(n, dtype=np.int64)
    return {"ascending": asc, "reversed": asc[::-1].copy(), "twice": np.repeat(asc, 2), "permutation": rng.permutation(n).astype(np.int64),
            "ends": np.array([0, n - 1], dtype=np.int64)}


def _device_fetch(h, ids, out_dtype, stride=0, pad=0):
    """hr_get_dense_rows_dev into a sentinel-filled buffer -> (the flat buffer, missing count)."""
    np_t, t_t = (np.float16, torch.float16) if out_dtype == nat.HR_F16 else (np.float32, torch.float32)
    stride = stride or h.dim
    n = len(ids)
    out = torch.full((max(n - 1, 0) * stride + (h.dim if n else 0) + pad,), SENTINEL, dtype=t_t, device="cuda")
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda()
    missing = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    h.get_dense_rows_dev(d_ids.data_ptr(), n, out_dtype, out.data_ptr(), stride, missing.data_ptr(), 0)
    return out.cpu().numpy().astype(np_t, copy=False), int(missing.item())


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_come_back_as_stored(gpu, dtype, dim):
    rng = np.random.default_rng(dim * 2 + dtype)
    X = _rows(rng, N, dim)
    want = _stored(X, dtype)
    h = _build(X, dtype)
    try:
        for name, local in _id_lists(rng, N).items():
            ids = local + OFFSET
            got = h.get_dense_rows(ids)
            assert got.dtype == np.float32 and got.shape == (len(ids), dim)
            assert np.array_equal(got.view(np.uint32), want[local].view(np.uint32)), name
            flat, missing = _device_fetch(h, ids, nat.HR_F32)
            assert missing == 0 and np.array_equal(flat.reshape(len(ids), dim).view(np.uint32), want[local].view(np.uint32)), name
            if dtype == nat.HR_F16:      # the raw bits
                flat, missing = _device_fetch(h, ids, nat.HR_F16)
                assert missing == 0, name
                assert np.array_equal(flat.reshape(len(ids), dim).view(np.uint16), X[local].astype(np.float16).view(np.uint16)), name
        if dtype == nat.HR_F32:
            with pytest.raises(ValueError):
                _device_fetch(h, np.arange(3) + OFFSET, nat.HR_F16)
    finally:
        h.close()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_stride_leaves_the_gap_and_the_tail_alone(gpu, dtype, dim):
    rng = np.random.default_rng(100 + dim * 2 + dtype)
    X = _rows(rng, N, dim)
    want = _stored(X, dtype)
    h = _build(X, dtype)
    try:
        local = rng.permutation(N).astype(np.int64)
        stride = dim + 5
        for out_dtype in ([nat.HR_F32, nat.HR_F16] if dtype == nat.HR_F16 else [nat.HR_F32]):
            flat, missing = _device_fetch(h, local + OFFSET, out_dtype, stride=stride, pad=11)
            assert missing == 0
            body = np.full(N * stride, SENTINEL, dtype=flat.dtype)
            body[: (N - 1) * stride + dim] = flat[: (N - 1) * stride + dim]
            body = body.reshape(N, stride)
            assert np.array_equal(body[:, :dim].astype(np.float32), want[local])
            assert (body[:, dim:] == SENTINEL).all()                       # the gap between dim and the stride
            assert (flat[(N - 1) * stride + dim:] == SENTINEL).all()       # nothing after the last row's last element
        with pytest.raises(ValueError):
            _device_fetch(h, local + OFFSET, nat.HR_F32, stride=dim - 1, pad=N)
    finally:
        h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_outside_the_shard(gpu, dtype):
    dim = 24
    rng = np.random.default_rng(7 + dtype)
    X = _rows(rng, N, dim)
    want = _stored(X, dtype)
    h = _build(X, dtype)
    try:
        ids = np.array([OFFSET + 3, -1, OFFSET - 1, OFFSET + N, OFFSET + N - 1, OFFSET], dtype=np.int64)
        flat, missing = _device_fetch(h, ids, nat.HR_F32)
        got = flat.reshape(len(ids), dim)
        assert missing == 3
        assert np.array_equal(got[[0, 4, 5]], want[[3, N - 1, 0]]) and (got[[1, 2, 3]] == 0).all()
        # the host form refuses, names the first such id and writes nothing
        out = np.full((len(ids), dim), SENTINEL, dtype=np.float32)
        rc = h._lib.hr_get_dense_rows(h._h, ids.ctypes.data_as(ctypes.c_void_p), len(ids), out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 1 and (out == SENTINEL).all()
        assert "-1" in (h._lib.hr_last_error(h._h) or b"").decode()
        with pytest.raises(ValueError):
            h.get_dense_rows(ids)
        assert h.get_dense_rows(np.zeros(0, np.int64)).shape == (0, dim)
    finally:
        h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_survive_growth_and_compaction(gpu, dtype):
    dim = 136
    rng = np.random.default_rng(11 + dtype)
    X = _rows(rng, N, dim)
    h = _build(X, dtype, reserve=64)          # the first batch already outgrows the reserve
    try:
        more = _rows(rng, 300, dim)
        h.add_dense(more)                      # and the second one the capacity that growth left
        h.finalize()
        allX = np.concatenate([X, more])
        want = _stored(allX, dtype)
        n = allX.shape[0]
        assert h.num_rows == n
        local = rng.permutation(n).astype(np.int64)
        assert np.array_equal(h.get_dense_rows(local + OFFSET), want[local])
        keep = rng.random(n) < 0.6
        keep[0], keep[-1] = False, True
        kept, _ = h.compact(keep)
        assert kept == int(keep.sum())
        survivors = want[keep]
        got = h.get_dense_rows(np.arange(kept, dtype=np.int64) + OFFSET)   # row j is the j-th survivor
        assert np.array_equal(got, survivors)
        flat, missing = _device_fetch(h, np.array([OFFSET + kept - 1, OFFSET + kept], dtype=np.int64), nat.HR_F32)
        assert missing == 1 and np.array_equal(flat.reshape(2, dim)[0], survivors[-1]) and (flat.reshape(2, dim)[1] == 0).all()
    finally:
        h.close()


def test_state_errors(gpu):
    rng = np.random.default_rng(3)
    h = _build(_rows(rng, 20, 8), nat.HR_F16, finalize=False)
    try:
        with pytest.raises(nat.HbmRagError) as ei:
            h.get_dense_rows(np.array([OFFSET], dtype=np.int64))
        assert ei.value.status == 2
        out = torch.zeros(8, dtype=torch.float32, device="cuda")
        d_ids = torch.tensor([OFFSET], dtype=torch.int64, device="cuda")
        with pytest.raises(nat.HbmRagError) as ei:
            h.get_dense_rows_dev(d_ids.data_ptr(), 1, nat.HR_F32, out.data_ptr())
        assert ei.value.status == 2
        h.finalize()
        assert h.get_dense_rows(np.array([OFFSET + 19], dtype=np.int64)).shape == (1, 8)
    finally:
        h.close()
    s = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_IP, 50)      # no dense collection
    try:
        s.add_sparse(np.array([0, 1], np.int64), np.array([3], np.int32), np.array([1.0], np.float32))
        s.finalize()
        with pytest.raises(nat.HbmRagError) as ei:
            s.get_dense_rows(np.array([0], dtype=np.int64))
        assert ei.value.status == 2
    finally:
        s.close()
