"""hr_get_sparse_rows / hr_get_sparse_rows_dev (include/hbmrag.h, csrc/query.h): stored sparse rows come back out of the
device CSR as one CSR in request order, bit for bit what was ingested.  The oracle is numpy slicing of the CSR this file
ingested.  The shard is filled in three batches with a finalize between the second and the third (the stored row
pointers are absolute), and its row lengths are planted at 0, 1, the lane-stride edge (63, 64, 65), 200 and 1000."""
import ctypes

import numpy as np
import pytest

from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, N, OFFSET = 1000, 5003, 7_000
PLANTED = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 200, 6: 1000, 2500: 0, 2501: 65, 3999: 0, 4000: 1000 - 1, N - 1: 64}
BATCHES = (0, 1700, 3900, N)          # finalize after the second batch
GUARD, IDX_SENTINEL, VAL_SENTINEL, PTR_SENTINEL = 64, -7, -77.25, -5


def _corpus():
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 41, N)
    for r, n in PLANTED.items():
        lens[r] = n
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    idx = np.concatenate([np.sort(rng.choice(V, n, replace=False)) for n in lens]).astype(np.int32)
    val = (np.abs(rng.standard_normal(idx.shape[0])) + 0.01).astype(np.float32)
    return indptr, idx, val


def _build(csr, upto=N, finalize=True):
    indptr, idx, val = csr
    h = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_IP, V)
    h.set_row_offset(OFFSET)
    for b, (lo, hi) in enumerate(zip(BATCHES[:-1], BATCHES[1:])):
        hi = min(hi, upto)
        if lo >= hi:
            break
        h.add_sparse(indptr[lo:hi + 1], idx, val)       # hr_add_sparse reads idx / val at the absolute positions
        if b == 1:
            h.finalize()
    if finalize:
        h.finalize()
    return h


@pytest.fixture(scope="module")
def shard(gpu):
    csr = _corpus()
    h = _build(csr)
    assert h.num_sparse_rows == N
    yield h, csr
    h.close()


def _slice(csr, local, n_rows=N):
    """The oracle: rows `local` of the CSR as a CSR; a row outside [0, n_rows) is empty."""
    indptr, idx, val = csr
    local = np.asarray(local, dtype=np.int64)
    ok = (local >= 0) & (local < n_rows)
    safe = np.where(ok, local, 0)
    lens = np.where(ok, indptr[safe + 1] - indptr[safe], 0)
    out_ptr = np.zeros(len(local) + 1, np.int64)
    np.cumsum(lens, out=out_ptr[1:])
    take = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r, k in zip(safe, ok) if k] + [np.zeros(0, np.int64)]).astype(np.int64)
    return out_ptr, idx[take], val[take], int((~ok).sum())


def _fetch(h, ids, cap=None, null_entries=False, total_hint=None):
    """hr_get_sparse_rows_dev into sentinel-filled buffers with GUARD entries behind `cap` -> (indptr, idx buffer, val
    buffer, counts).  cap None: the count pass first, then cap = the total."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n = len(ids)
    d_ids = torch.from_numpy(ids).cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    indptr = torch.full((n + 1,), PTR_SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(nat.get_sparse_rows_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    if cap is None:
        h.get_sparse_rows_dev(d_ids.data_ptr(), n, indptr.data_ptr(), 0, 0, 0, counts.data_ptr(), scratch.data_ptr())
        cap = int(counts.cpu()[0])
        indptr.fill_(PTR_SENTINEL)
        counts.fill_(77)
    d_idx = torch.full((cap + GUARD,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    d_val = torch.full((cap + GUARD,), VAL_SENTINEL, dtype=torch.float32, device="cuda")
    h.get_sparse_rows_dev(d_ids.data_ptr(), n, indptr.data_ptr(), 0 if null_entries else d_idx.data_ptr(),
                          0 if null_entries else d_val.data_ptr(), cap, counts.data_ptr(), scratch.data_ptr())
    torch.cuda.synchronize()
    return indptr.cpu().numpy(), d_idx.cpu().numpy(), d_val.cpu().numpy(), counts.cpu().numpy()


def _assert_equals_slice(got, want, cap=None):
    indptr, idx, val, counts = got
    w_ptr, w_idx, w_val, w_missing = want
    total = int(w_ptr[-1])
    cap = total if cap is None else cap
    assert np.array_equal(indptr, w_ptr)
    assert counts.tolist() == [total, w_missing]
    m = min(cap, total)
    assert np.array_equal(idx[:m], w_idx[:m])
    assert np.array_equal(val[:m].view(np.uint32), w_val[:m].view(np.uint32))
    assert (idx[m:] == IDX_SENTINEL).all() and (val[m:] == VAL_SENTINEL).all()     # nothing at or beyond cap, or the total


def _request_lists():
    rng = np.random.default_rng(5)
    planted = np.array(sorted(PLANTED), dtype=np.int64)
    empty = np.array([r for r, n in PLANTED.items() if n == 0] * 3, dtype=np.int64)
    return {
        "one": np.array([6], dtype=np.int64),
        "three": np.array([6, 0, 4], dtype=np.int64),                        # a partly filled block of waves
        "1024": np.concatenate([planted, rng.integers(0, N, 1024 - len(planted))]),
        "1025": np.concatenate([rng.integers(0, N, 1025 - len(planted)), planted]),   # phase 2 sums two blocks
        "ascending": np.arange(N, dtype=np.int64),
        "shuffled": rng.permutation(N).astype(np.int64),
        "repeats": np.repeat(np.array([5, 6, 0, 3, 6, N - 1], dtype=np.int64), 3),
        "last": np.array([N - 1], dtype=np.int64),
        "empty rows": empty,
    }


@pytest.mark.parametrize("name", list(_request_lists()))
def test_rows_come_back_as_stored(shard, name):
    h, csr = shard
    local = _request_lists()[name]
    want = _slice(csr, local)
    if name == "empty rows":
        assert want[0][-1] == 0
    _assert_equals_slice(_fetch(h, local + OFFSET), want)
    # the binding's host form: the sizing call, then the fetch
    ptr, idx, val = h.get_sparse_rows(local + OFFSET)
    assert (ptr.dtype, idx.dtype, val.dtype) == (np.int64, np.int32, np.float32)
    assert np.array_equal(ptr, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(val.view(np.uint32), want[2].view(np.uint32))


def test_ids_outside_the_shard_are_empty_rows(shard):
    h, csr = shard
    ids = np.array([OFFSET + 5, OFFSET - 1, 5, OFFSET + 6, OFFSET + N, -1, OFFSET + N - 1, OFFSET + N + 10**12, 0, OFFSET + 4,
                    -2**63, 2**63 - 1], dtype=np.int64)
    want = _slice(csr, ids - OFFSET)
    assert want[3] == 8
    _assert_equals_slice(_fetch(h, ids), want)
    only_missing = np.array([-1, OFFSET - 1, OFFSET + N], dtype=np.int64)
    _assert_equals_slice(_fetch(h, only_missing), _slice(csr, only_missing - OFFSET))


def test_cap_bounds_the_writes(shard):
    h, csr = shard
    local = np.array([5, 0, 4, 6, 1, 3, 6, N - 1], dtype=np.int64)
    want = _slice(csr, local)
    total = int(want[0][-1])
    mid_row = int(want[0][3]) + 417                     # inside the row of 1000
    for cap in (total, total - 1, mid_row, 1, total + 9):
        _assert_equals_slice(_fetch(h, local + OFFSET, cap=cap), want, cap)
    indptr, idx, val, counts = _fetch(h, local + OFFSET, cap=0, null_entries=True)       # the count pass
    assert np.array_equal(indptr, want[0]) and counts.tolist() == [total, 0]
    assert (idx == IDX_SENTINEL).all() and (val == VAL_SENTINEL).all()


def test_empty_request_and_determinism(shard):
    h, csr = shard
    indptr, idx, val, counts = _fetch(h, np.zeros(0, np.int64), cap=0)
    assert indptr.tolist() == [0] and counts.tolist() == [0, 0] and (idx == IDX_SENTINEL).all()
    ptr, i2, v2 = h.get_sparse_rows(np.zeros(0, np.int64))
    assert ptr.tolist() == [0] and i2.shape == v2.shape == (0,)
    ids = np.random.default_rng(8).integers(-50, N + 50, 3000) + OFFSET
    a, b = _fetch(h, ids), _fetch(h, ids)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _assert_equals_slice(a, _slice(csr, ids - OFFSET))


def _host_call(h, ids, cap, null_entries=False):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    ptr = np.full(len(ids) + 1, PTR_SENTINEL, np.int64)
    idx = np.full(cap + GUARD, IDX_SENTINEL, np.int32)
    val = np.full(cap + GUARD, VAL_SENTINEL, np.float32)
    total = ctypes.c_int64(-9)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = h._lib.hr_get_sparse_rows(h._h, vp(ids), len(ids), vp(ptr), None if null_entries else vp(idx),
                                   None if null_entries else vp(val), cap, ctypes.byref(total))
    return rc, ptr, idx, val, total.value


def test_host_form(shard):
    h, csr = shard
    local = np.array([6, 5, 0, 2, 6, N - 1], dtype=np.int64)
    w_ptr, w_idx, w_val, _ = _slice(csr, local)
    total = int(w_ptr[-1])
    rc, ptr, idx, val, got_total = _host_call(h, local + OFFSET, 0, null_entries=True)       # the sizing call
    assert rc == 0 and got_total == total and np.array_equal(ptr, w_ptr)
    rc, ptr, idx, val, got_total = _host_call(h, local + OFFSET, total)                      # the fetch
    assert rc == 0 and got_total == total and np.array_equal(ptr, w_ptr)
    assert np.array_equal(idx[:total], w_idx) and np.array_equal(val[:total].view(np.uint32), w_val.view(np.uint32))
    assert (idx[total:] == IDX_SENTINEL).all() and (val[total:] == VAL_SENTINEL).all()
    # a total above cap: the indptr and the total, no entries
    rc, ptr, idx, val, got_total = _host_call(h, local + OFFSET, total - 1)
    assert rc == 0 and got_total == total and np.array_equal(ptr, w_ptr)
    assert (idx == IDX_SENTINEL).all() and (val == VAL_SENTINEL).all()
    # an id outside the shard: refused, named, nothing written
    bad = np.array([OFFSET + 3, OFFSET + N, OFFSET - 1], dtype=np.int64)
    rc, ptr, idx, val, got_total = _host_call(h, bad, 100)
    assert rc == 1 and got_total == -9 and (ptr == PTR_SENTINEL).all() and (idx == IDX_SENTINEL).all() and (val == VAL_SENTINEL).all()
    assert str(OFFSET + N) in (h._lib.hr_last_error(h._h) or b"").decode()
    with pytest.raises(ValueError):
        h.get_sparse_rows(bad)


def test_state_and_argument_errors(shard):
    h, csr = shard
    d_ids = torch.tensor([OFFSET], dtype=torch.int64, device="cuda")
    ptr = torch.zeros(2, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(nat.get_sparse_rows_scratch_bytes(1) + 8, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(8, dtype=torch.int32, device="cuda")
    val = torch.zeros(8, dtype=torch.float32, device="cuda")
    ok = [d_ids.data_ptr(), 1, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), 8, counts.data_ptr(), scratch.data_ptr()]
    h.get_sparse_rows_dev(*ok)
    torch.cuda.synchronize()
    for at, bad in ((1, -1), (5, -1), (2, 0), (6, 0), (7, 0), (3, 0), (4, 0), (7, scratch.data_ptr() + 4), (2, ptr.data_ptr() + 4),
                    (3, idx.data_ptr() + 2)):
        args = list(ok)
        args[at] = bad
        with pytest.raises(ValueError):
            h.get_sparse_rows_dev(*args)
    assert nat.get_sparse_rows_scratch_bytes(0) >= 16 and nat.get_sparse_rows_scratch_bytes(1025) >= 24
    assert nat.get_sparse_rows_scratch_bytes(16384) <= 256
    with pytest.raises(ValueError):
        _host_call_checked(h, -1)
    # rows added since the last finalize are staged on the host
    p = _build(csr, upto=3000)
    try:
        p.add_sparse(csr[0][3000:3101], csr[1], csr[2])
        with pytest.raises(nat.HbmRagError) as ei:
            p.get_sparse_rows_dev(*ok)
        assert ei.value.status == 2
        with pytest.raises(nat.HbmRagError) as ei:
            p.get_sparse_rows(np.array([OFFSET], dtype=np.int64))
        assert ei.value.status == 2
        p.finalize()
        got = p.get_sparse_rows(np.array([OFFSET + 3099, OFFSET + 6], dtype=np.int64))
        want = _slice(csr, [3099, 6])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        p.close()
    d = nat.ShardHandle(8, nat.HR_F16, nat.HR_METRIC_IP)            # no sparse collection
    try:
        d.add_dense(np.ones((4, 8), np.float32))
        d.finalize()
        with pytest.raises(nat.HbmRagError) as ei:
            d.get_sparse_rows_dev(*ok)
        assert ei.value.status == 2
        with pytest.raises(nat.HbmRagError) as ei:
            d.get_sparse_rows(np.array([0], dtype=np.int64))
        assert ei.value.status == 2
    finally:
        d.close()


def _host_call_checked(h, n):
    ids = np.zeros(1, np.int64)
    ptr = np.zeros(2, np.int64)
    total = ctypes.c_int64(0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h._check(h._lib.hr_get_sparse_rows(h._h, vp(ids), n, vp(ptr), None, None, 0, ctypes.byref(total)))


def test_rows_after_compaction(gpu):
    csr = _corpus()
    h = _build(csr)
    try:
        keep = np.ones(N, bool)
        keep[::3] = False                                  # drops every third row, the planted rows 0, 3 and 6 among them
        _, kept = h.compact(keep)
        survivors = np.flatnonzero(keep)
        assert kept == len(survivors) == h.num_sparse_rows
        rng = np.random.default_rng(12)
        for new in (np.arange(kept, dtype=np.int64), rng.permutation(kept).astype(np.int64)[:1500]):
            want = _slice(csr, survivors[new])             # new row j is the j-th survivor
            _assert_equals_slice(_fetch(h, new + OFFSET), want)
        got = _fetch(h, np.array([OFFSET + kept - 1, OFFSET + kept], dtype=np.int64))
        _assert_equals_slice(got, _slice(csr, [survivors[-1], N + 5]))
    finally:
        h.close()
