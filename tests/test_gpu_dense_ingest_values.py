"""What the dense scans search: the rows as hr_add_dense / hr_add_dense_raw / hr_add_dense_raw_dev store them.

A. The stored values are numpy's.  On an IP shard a one-hot query e_j scores row r with exactly (float)x_stored[r, j], so
   k = n and Q = I make every stored element visible on its own: ties of the fp32 -> fp16 rounding, fp16 subnormals, the
   65504 edge, -0, and (through a COSINE pass, whose norms run over the whole padded row) the zero fill of the tail.
B. A batch with an element that is NaN or infinite AS STORED is refused with HR_EINVAL (ValueError) naming the row, and
   leaves the handle as it was: the shard-wide bound max_row_norm, and with it every later proof, is untouched.
"""
import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat

from l2_yardstick import l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENTRIES = ("f32", "raw", "raw_dev")        # hr_add_dense, hr_add_dense_raw, hr_add_dense_raw_dev
STORES = {nat.HR_F16: np.float16, nat.HR_F32: np.float32}
METRICS = (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE, nat.HR_METRIC_L2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _add(h, entry, rows32, bad_bits=None):
    """Append fp32-valued rows through one entry point.  The raw forms get them in the store's type, rounded by numpy;
    bad_bits = (row, col, uint16) then plants an fp16 bit pattern in what they are handed."""
    n = rows32.shape[0]
    if entry == "f32":
        rows = np.ascontiguousarray(rows32, dtype=np.float32)
        h._check(h._lib.hr_add_dense(h._h, nat._vp(rows), n))
        return
    with np.errstate(over="ignore"):
        rows = np.ascontiguousarray(rows32.astype(STORES[h.dtype]))
    if bad_bits is not None:
        rows.view(np.uint16)[bad_bits[0], bad_bits[1]] = bad_bits[2]
    if entry == "raw":
        h._check(h._lib.hr_add_dense_raw(h._h, nat._vp(rows), n))
    else:
        t = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        h.add_dense_dev(t.data_ptr(), n, torch.cuda.current_stream().cuda_stream)


def _dev_search(h, Q, k):
    B = Q.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    fl = torch.zeros((B,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    h.search_dense_dev(dq.data_ptr(), B, k, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def _reference(X, Q, k, metric):
    if metric == nat.HR_METRIC_L2:
        return l2_search(X, Q, k)
    return oracle.dense_search(X, Q, k, oracle.IP if metric == nat.HR_METRIC_IP else oracle.COSINE)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ at {np.argwhere(got[0] != want[0])[:5].tolist()}"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), f"{what}: score bits differ"


# ----------------------------------------------------------------------------------------------------------------- A
def _f16(bits):
    return np.array(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def _special_values():
    """fp32 values at which a rounding mode to fp16 shows.  For 64 fp16 values h over every binade (subnormals, the
    normal / subnormal border and the top binade included; an even and an odd h each time): the fp32 midpoint of h and
    its successor (a tie), that midpoint's fp32 neighbours on both sides, and the negatives of the three."""
    hs = {0x0001, 0x0002, 0x03FE, 0x03FF, 0x0400, 0x0401, 0x7BFD, 0x7BFE}    # 0x7BFE's successor is 65504
    for e in range(31):
        hs.add((e << 10) | ((e * 74) & 0x3FE))
        hs.add((e << 10) | ((e * 53) & 0x3FF) | 1)
    hs = sorted(b for b in hs if b < 0x7BFF)              # the successor of 0x7BFF is infinity: refused, see part B
    assert len(hs) >= 50 and any(b & 1 for b in hs) and any(not b & 1 for b in hs)
    out = [2.0 ** -25,                                    # a tie that rounds to 0
           np.nextafter(np.float32(2.0 ** -25), np.float32(1)),      # just above it: 2^-24
           1.5 * 2.0 ** -24,                              # a tie that rounds to 2^-23
           1e-10, -0.0, 65504.0,
           np.nextafter(np.float32(65520.0), np.float32(0)),         # the largest fp32 that still rounds to 65504
           -65504.0, -np.nextafter(np.float32(65520.0), np.float32(0)), -2.0 ** -25, 0.0]
    for b in hs:
        lo, hi = np.float64(_f16(b)), np.float64(_f16(b + 1))
        mid = np.float32((lo + hi) / 2)
        assert np.float64(mid) == (lo + hi) / 2           # 11 + 1 significant bits: exact in fp32
        for v in (mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))):
            out += [v, -v]
    return np.array(out, dtype=np.float32)


def _matrices(d, extra=()):
    """[n <= 200, d] fp32 matrices of seeded N(0,1) filler that between them hold every special value in the first
    element of a row and in the last element before the padding, a run of them in the last row and a sprinkling inside."""
    S = np.concatenate([_special_values(), np.array(extra, dtype=np.float32)])
    n = 200
    rng = np.random.default_rng(1000 + d)
    out = []
    for t in range((len(S) + n - 1) // n):
        X = rng.standard_normal((n, d)).astype(np.float32)
        inside = rng.random((n, d)) < 0.1
        X[inside] = S[rng.integers(0, len(S), size=int(inside.sum()))]
        X[n - 1, :] = np.roll(S, -t * 53)[np.arange(d) % len(S)]
        X[:, 0] = np.roll(S, -t * n)[:n]
        X[:, d - 1] = np.roll(S, -t * n - (0 if d == 1 else 97))[:n]
        out.append(X)
    first, last = np.concatenate([X[:, 0] for X in out]), np.concatenate([X[:, d - 1] for X in out])
    for v in S.view(np.uint32):
        assert v in first.view(np.uint32) and v in last.view(np.uint32)
    return out


@pytest.mark.parametrize("dtype,d", [(nat.HR_F16, d) for d in (1, 7, 8, 9, 33, 100)] +
                         [(nat.HR_F32, d) for d in (3, 4, 5, 100)])
def test_stored_values_are_numpys(gpu, dtype, d):
    """Every element, through every entry point, appended in ragged pieces (1, 17, the rest)."""
    extra = (1e-40, -1e-40, 1.4e-45) if dtype == nat.HR_F32 else ()      # fp32 subnormals stay what they are
    rng = np.random.default_rng(d)
    for X in _matrices(d, extra):
        n = X.shape[0]
        stored = X.astype(STORES[dtype])
        eye = np.eye(d, dtype=np.float32)
        Qr = rng.standard_normal((5, d)).astype(np.float32)
        want_ip, want_ipr = _reference(stored, eye, n, nat.HR_METRIC_IP), _reference(stored, Qr, n, nat.HR_METRIC_IP)
        want_cos = _reference(stored, Qr, n, nat.HR_METRIC_COSINE)
        got = {}
        for entry in ENTRIES:
            for metric in (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE):
                h = nat.ShardHandle(d, dtype, metric)
                for lo, hi in ((0, 1), (1, 18), (18, n)):
                    _add(h, entry, X[lo:hi])
                h.finalize()
                assert h.num_rows == n
                if metric == nat.HR_METRIC_IP:
                    got[entry] = (h.search_dense(eye, n), h.search_dense(Qr, n))
                    _same(got[entry][0], want_ip, f"{entry} one-hot")
                    _same(got[entry][1], want_ipr, f"{entry} IP")
                    for j in range(d):           # independently of the oracle: column j of the stored matrix, sorted
                        col = np.sort(stored[:, j].astype(np.float32))[::-1]
                        assert (got[entry][0][1][j] == col).all(), f"{entry}: stored column {j} is not numpy's"
                else:
                    _same(h.search_dense(Qr, n), want_cos, f"{entry} COSINE")
                h.close()
        for entry in ENTRIES[1:]:
            for a, b in zip(got[entry], got[ENTRIES[0]]):
                _same(a, b, f"{entry} vs {ENTRIES[0]}")


# ----------------------------------------------------------------------------------------------------------------- B
D, N0, N1, NBAD, K = 96, 3000, 1000, 50, 20
POSITIONS = {"first": (0, 0), "last": (NBAD - 1, D - 1), "inside": (23, 41)}

_cache = {}


def _good(dtype):
    """Good rows (fp32 values exact in the store's type), a batch to spoil, queries, and, per metric, the references over
    the first N0 rows and over all good rows plus the device-form answer of a handle that only ever saw good rows."""
    if dtype not in _cache:
        rng = np.random.default_rng(7 + dtype)
        G = rng.standard_normal((N0 + N1, D)).astype(np.float32).astype(STORES[dtype])
        batch = rng.standard_normal((NBAD, D)).astype(np.float32).astype(STORES[dtype]).astype(np.float32)
        Q = rng.standard_normal((8, D)).astype(np.float32)
        per_metric = {}
        for metric in METRICS:
            h = nat.ShardHandle(D, dtype, metric)
            h.add_dense(G[:N0])
            h.finalize()
            h.add_dense(G[N0:])
            h.finalize()
            per_metric[metric] = (_reference(G[:N0], Q, K, metric), _reference(G, Q, K, metric), _dev_search(h, Q, K))
            _same(h.search_dense(Q, K), per_metric[metric][1], "fresh handle")
            h.close()
        _cache[dtype] = (G, batch, Q, per_metric)
    return _cache[dtype]


def _refusal_cases():
    cases = []
    for dtype in STORES:
        for entry in ENTRIES:
            values = [float("nan"), float("inf"), float("-inf")]
            if dtype == nat.HR_F16:
                # finite fp32 input that rounds to infinity; the raw forms get the fp16 infinity / NaN bit patterns
                values += [65520.0, 1e5, -7e4] if entry == "f32" else [0x7C00, 0x7E00]
            for value in values:
                for pos in POSITIONS:
                    cases.append(pytest.param(entry, dtype, value, pos,
                                              id=f"{entry}-{'f16' if dtype == nat.HR_F16 else 'f32'}-{value}-{pos}"))
    return cases


def _spoiled(batch, value, pos):
    """-> (fp32 rows, bad_bits for the raw forms or None)."""
    r, c = POSITIONS[pos]
    rows = batch.copy()
    if isinstance(value, int):
        return rows, (r, c, value)
    rows[r, c] = value
    return rows, None


@pytest.mark.parametrize("entry,dtype,value,pos", _refusal_cases())
def test_non_finite_batch_is_refused_and_leaves_the_handle_as_it_was(gpu, tmp_path, entry, dtype, value, pos):
    G, batch, Q, per_metric = _good(dtype)
    rows, bad_bits = _spoiled(batch, value, pos)
    for metric in METRICS:
        want0, want, fresh_dev = per_metric[metric]
        h = nat.ShardHandle(D, dtype, metric)
        h.add_dense(G[:N0])
        h.finalize()
        with pytest.raises(ValueError, match=rf"row {POSITIONS[pos][0]}\b"):
            _add(h, entry, rows, bad_bits)
        assert h.num_rows == N0
        _same(h.search_dense(Q, K), want0, "after the refusal")       # still finalized, still the first N0 rows
        h.add_dense(G[N0:])
        h.finalize()
        assert h.num_rows == N0 + N1
        _same(h.search_dense(Q, K), want, "host form")
        ids, sc, fl = _dev_search(h, Q, K)
        assert np.array_equal(fl, fresh_dev[2]), f"flags {fl.tolist()} vs a fresh handle's {fresh_dev[2].tolist()}"
        assert np.array_equal(ids, fresh_dev[0]) and np.array_equal(_bits(sc), _bits(fresh_dev[1]))
        path = str(tmp_path / f"m{metric}.hbmrag")
        h.save(path)
        back = nat.ShardHandle.load(path, D, dtype, metric)
        _same(back.search_dense(Q, K), want, "after save / load")
        ids, sc, fl = _dev_search(back, Q, K)
        assert np.array_equal(fl, fresh_dev[2])
        assert np.array_equal(ids, fresh_dev[0]) and np.array_equal(_bits(sc), _bits(fresh_dev[1]))
        back.close()
        h.close()


@pytest.mark.parametrize("dtype", list(STORES))
def test_refused_batch_leaves_no_trace_in_the_snapshot(gpu, tmp_path, dtype):
    """The tiles a refused batch wrote beyond the last row are zero again: the snapshot is, byte for byte, the one of a
    handle that never saw it.  Also on an empty handle, which then takes good rows as if nothing had happened."""
    G, batch, Q, per_metric = _good(dtype)
    rows, _ = _spoiled(batch, float("nan"), "inside")
    h, fresh = nat.ShardHandle(D, dtype, nat.HR_METRIC_COSINE), nat.ShardHandle(D, dtype, nat.HR_METRIC_COSINE)
    with pytest.raises(ValueError, match=r"row 23\b"):
        _add(h, "f32", rows)
    assert h.num_rows == 0
    for x in (h, fresh):
        x.add_dense(G[:N0])
        x.finalize()
    with pytest.raises(ValueError, match=r"row 23\b"):
        _add(h, "raw_dev", rows)
    _same(h.search_dense(Q, K), per_metric[nat.HR_METRIC_COSINE][0])
    h.save(str(tmp_path / "a"))
    fresh.save(str(tmp_path / "b"))
    assert open(str(tmp_path / "a"), "rb").read() == open(str(tmp_path / "b"), "rb").read()
    h.close()
    fresh.close()


@pytest.mark.parametrize("value", [65520.0, 1e5, -7e4])
@pytest.mark.parametrize("entry", ENTRIES)
def test_fp32_shard_accepts_what_overflows_fp16(gpu, entry, value):
    G, batch, Q, _ = _good(nat.HR_F32)
    rows, _ = _spoiled(batch, value, "last")
    X = np.concatenate([G[:N0], rows])
    for metric in METRICS:
        h = nat.ShardHandle(D, nat.HR_F32, metric)
        h.add_dense(G[:N0])
        _add(h, entry, rows)
        h.finalize()
        assert h.num_rows == N0 + NBAD
        _same(h.search_dense(Q, K), _reference(X, Q, K, metric))
        h.close()


def test_fp16_shard_accepts_the_largest_value_that_rounds_to_65504(gpu):
    G, batch, Q, _ = _good(nat.HR_F16)
    edge = np.nextafter(np.float32(65520.0), np.float32(0))
    rows = batch.copy()
    rows[0, 0], rows[NBAD - 1, D - 1], rows[23, 41] = edge, -edge, edge
    X = np.concatenate([G[:N0], rows.astype(np.float16)])
    assert np.isfinite(X).all() and X[N0, 0] == 65504
    for metric in (nat.HR_METRIC_IP, nat.HR_METRIC_COSINE):
        h = nat.ShardHandle(D, nat.HR_F16, metric)
        h.add_dense(G[:N0])
        _add(h, "f32", rows)
        h.finalize()
        assert h.num_rows == N0 + NBAD
        _same(h.search_dense(Q, K), _reference(X, Q, K, metric))
        h.close()


def test_bad_row_in_a_later_staging_chunk_of_one_call(gpu):
    """hr_add_dense stages a call in pieces of 64 MiB: 4096 rows of 4096 floats.  The bad element sits in the second."""
    d, n0, n = 4096, 300, 4200
    rng = np.random.default_rng(11)
    G = rng.standard_normal((n0, d), dtype=np.float32)
    big = rng.random((n, d), dtype=np.float32)
    big[n - 1, d - 1] = np.inf
    Q = rng.standard_normal((3, d)).astype(np.float32)
    h = nat.ShardHandle(d, nat.HR_F32, nat.HR_METRIC_COSINE)
    h.add_dense(G)
    h.finalize()
    with pytest.raises(ValueError, match=rf"row {n - 1}\b"):
        _add(h, "f32", big)
    assert h.num_rows == n0
    _same(h.search_dense(Q, K), _reference(G, Q, K, nat.HR_METRIC_COSINE))
    more = rng.standard_normal((40, d), dtype=np.float32)
    h.add_dense(more)
    h.finalize()
    _same(h.search_dense(Q, K), _reference(np.concatenate([G, more]), Q, K, nat.HR_METRIC_COSINE))
    h.close()
