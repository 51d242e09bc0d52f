"""Lifecycle of the shard store (csrc/hbmrag.hip, grow_dense .. hr_load): the snapshot's bytes, the dense store's growth
paths, and what hr_destroy gives back.  The snapshot fixture (tests/golden/snapshot_v2.json) was recorded by
tests/golden/gen_snapshot_v2.py with the library as it was before the store's buffers became owning."""
import hashlib
import json
import os
import runpy

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.engine import pack_sparse_queries

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
gen = runpy.run_path(os.path.join(GOLDEN, "gen_snapshot_v2.py"))
with open(os.path.join(GOLDEN, "snapshot_v2.json")) as _f:
    RECORDED = {s["case"]: s for s in json.load(_f)["snapshots"]}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _saved(h, path):
    h.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def test_fixture_covers_the_cases():
    assert sorted(RECORDED) == sorted(gen["CASES"])
    assert all(RECORDED[name]["seed"] == c["seed"] for name, c in gen["CASES"].items())


@pytest.mark.parametrize("case", sorted(gen["CASES"]))
def test_snapshot_bytes_are_the_recorded_ones(gpu, tmp_path, case):
    """Header, section order, section lengths and every byte of the body (the zero rows between n_rows and the saved
    capacity included) are those of the recorded file; and the file loads again."""
    want = RECORDED[case]
    h = gen["build_case"](nat, case)
    path = tmp_path / "s.hbmrag"
    blob = _saved(h, path)
    got = gen["describe"](blob)
    assert got["header_hex"] == want["header_hex"]
    assert got["length"] == want["length"]
    assert got["sha256"] == want["sha256"]
    back = nat.ShardHandle.load(str(path), h.dim, h.dtype, h.metric, h.sparse_dim)
    assert (back.num_rows, back.num_sparse_rows) == (h.num_rows, h.num_sparse_rows)
    assert _saved(back, tmp_path / "again.hbmrag") == blob
    back.close()
    h.close()


APPENDS = (1000, 24, 1, 700, 275)  # cross the 1024-row first capacity, then the 1.5x step; 1, 24, 1000 are off the 64-row grid


def _leave_used_blocks(rng, d, dtype):
    """Stores filled to the last row of every capacity the test's handles will take (64, 1024, 1536, 2304; 2048), then
    closed.  The allocator hands freed blocks out again: a growth path that did not zero its new buffers would now show
    what these held, not the zeros of memory fresh from the driver."""
    def rows(m):
        return rng.standard_normal((m, d)).astype(np.float16 if dtype == nat.HR_F16 else np.float32)

    grown = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    for m in (1024, 512, 768):
        grown.add_dense(rows(m))
    exact = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    exact.reserve(2048)
    exact.add_dense(rows(2048))
    small = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    small.reserve(64)
    small.add_dense(rows(64))
    for h in (grown, exact, small):
        h.finalize()
        h.close()


def _rows_beyond_are_zero(blob, n):
    """The dense sections of a snapshot [header][tiles][scale][norm2] hold only zeros for the rows n .. cap_rows (n on the
    16-row grid of the tile layout)."""
    KT, = np.frombuffer(blob, np.int32, 1, 20)
    cap, = np.frombuffer(blob, np.int64, 1, 48)
    assert n % 16 == 0 and n < cap
    at = 96
    for per_row in (KT * 64, 4, 8):  # tiles: row blocks of 16 rows x KT KiB; scale fp32; norm2 fp64
        if any(blob[at + n * per_row:at + cap * per_row]):
            return False
        at += cap * per_row
    return at == len(blob)


@pytest.mark.parametrize("d,dtype", [(32, nat.HR_F16), (40, nat.HR_F32)], ids=["d32_f16", "d40_f32"])
def test_growth_leaves_what_a_fresh_build_leaves(gpu, tmp_path, d, dtype):
    """Appends that grow the store step by step, one exact reservation, and a reservation on a non-empty handle give
    the same shard: identical search results (the oracle's), snapshots whose rows between n_rows and the saved capacity
    are zero after every growth path, and byte-identical snapshots."""
    rng = np.random.default_rng(29)
    n, k = sum(APPENDS), 10
    X = rng.standard_normal((n, d)).astype(np.float16 if dtype == nat.HR_F16 else np.float32)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q[0] = X[990].astype(np.float32)  # a row appended before the second growth
    want = oracle.dense_search(X, Q, k, oracle.COSINE)
    _leave_used_blocks(rng, d, dtype)

    stepwise = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    lo = 0
    for m in APPENDS:
        stepwise.add_dense(X[lo:lo + m])
        stepwise.finalize()
        lo += m
    reserved = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    reserved.reserve(n)
    reserved.add_dense(X)
    reserved.finalize()
    regrown = nat.ShardHandle(d, dtype, nat.HR_METRIC_COSINE)
    regrown.reserve(10)
    regrown.add_dense(X[:n // 2])
    regrown.reserve(1500)  # non-empty handle: grows by the append rule
    regrown.add_dense(X[n // 2:])
    regrown.finalize()

    handles = {"stepwise": stepwise, "reserved": reserved, "regrown": regrown}
    for name, h in handles.items():
        assert h.num_rows == n, name
        ids, sc = h.search_dense(Q, k)
        assert np.array_equal(ids, want[0]), name
        assert np.array_equal(_bits(sc), _bits(want[1])), name
    blobs = {name: _saved(h, tmp_path / (name + ".hbmrag")) for name, h in handles.items()}
    assert len(blobs["stepwise"]) == len(blobs["reserved"]) == len(blobs["regrown"])
    for name, blob in blobs.items():
        assert _rows_beyond_are_zero(blob, n), name
    assert hashlib.sha256(blobs["stepwise"]).digest() == hashlib.sha256(blobs["reserved"]).digest(), "stepwise vs reserved"
    assert hashlib.sha256(blobs["regrown"]).digest() == hashlib.sha256(blobs["reserved"]).digest(), "regrown vs reserved"
    for h in handles.values():
        h.close()


def test_destroy_gives_back_what_a_handle_took(gpu):
    """Create, search through the host form, a `*_dev` form and the hybrid form (so that pooled and per-stream
    workspaces, sparse_ws, the side stream and the events exist), close; eight times.  A leak detector, not a
    measurement: 200 000 rows make one leaked tile buffer about 50 MB against a bound of 8 MiB."""
    rng = np.random.default_rng(31)
    n, d, V, nnz, B, k = 200_000, 32, 50, 3, 4, 10
    X = rng.standard_normal((n, d)).astype(np.float16)
    idx = (np.arange(nnz, dtype=np.int32) * 16 + rng.integers(0, 16, size=(n, nnz), dtype=np.int32)).reshape(-1)
    val = (np.abs(rng.standard_normal(n * nnz)) + 0.01).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * nnz
    Q = rng.standard_normal((B, d)).astype(np.float32)
    SQ = [(idx[b * nnz:(b + 1) * nnz], val[b * nnz:(b + 1) * nnz]) for b in range(B)]
    p, i_, v_, mx = pack_sparse_queries(SQ, 0.0)
    dq, dp, di, dv = (torch.from_numpy(a).cuda() for a in (Q, p, i_, v_))
    ids = torch.empty((2, B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((2, B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((2, B), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()

    free = []
    for _ in range(8):
        h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_COSINE, V)
        h.add_dense(X)
        h.add_sparse(ptr, idx, val)
        h.finalize()
        host_ids, _ = h.search_dense(Q, k)
        h.search_sparse(SQ, k, 0.0)
        h.search_dense_dev(dq.data_ptr(), B, k, ids[0].data_ptr(), sc[0].data_ptr(), fl[0].data_ptr(), 0, st.cuda_stream)
        st.synchronize()
        assert np.array_equal(ids[0].cpu().numpy(), host_ids)
        h.search_hybrid_dev(dq.data_ptr(), dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, len(i_), mx, k, ids.data_ptr(),
                            sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
        st.synchronize()
        assert np.array_equal(ids[0].cpu().numpy(), host_ids)
        h.close()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each close:", free)
    assert abs(free[7] - free[0]) <= 8 << 20, free
