"""The host half of compaction, without a GPU: the payload columns' compact() against a plain Python rebuild, and
ShardSet.compact over oracle-backed stand-ins for the shard handles (in the style of tests/test_distributed_cpu.py):
when the row maps are renumbered, what a failing shard leaves behind, and that searches stay the oracle's."""
import numpy as np
import pytest

import oracle
from advanced_rag.columns import NumericColumn, PayloadColumns, StringColumn, TokenSetColumn
from advanced_rag.shards import CollectiveShardSet, ShardSet

STRINGS = ["", "plain", "ünïcödé ✓ 漢字", "a" * 40, "", "tail with spaces  ", "é", "x", "zebra zebra Zebra", "last ✓"]


def _fill(n):
    cols = PayloadColumns()
    for r in range(n):
        cols["id"].append(f"id{r}")
        cols["doc_id"].append(f"doc{r // 3}")
        cols["content"].append(STRINGS[r % len(STRINGS)] + (f" row{r}" if r % 4 else ""))
        cols["timestamp"].append("" if r % 5 == 0 else f"2024-01-{1 + r % 28:02d}")
        cols["metadata_json"].append("{}")
        cols["chunk_index"].append(r % 10)
        cols["token_count"].append(r * 7)
        for k, m in (("entropy", 8), ("redundancy", 4), ("domain_density", 16)):
            cols[k].append((r % m) / m)
    return cols


def _as_python(cols):
    return {k: list(cols[k]) for k in cols}


@pytest.mark.parametrize("mask", ["random", "none", "all", "first_and_last"])
def test_payload_columns_compact_equals_a_python_rebuild(mask):
    n = 57
    rng = np.random.default_rng(3)
    keep = {"random": rng.random(n) < 0.6, "none": np.zeros(n, bool), "all": np.ones(n, bool),
            "first_and_last": np.isin(np.arange(n), (0, n - 1))}[mask]
    cols = _fill(n)
    cols["doc_id"].keys()                      # prefix keys and token sets exist before the compaction
    tokens_before = [cols.token_sets().row(r).tolist() for r in range(n)]
    dictionary = dict(cols.token_sets().ids)
    want = {k: [v for v, kp in zip(vals, keep) if kp] for k, vals in _as_python(cols).items()}
    cols.compact(keep)
    assert cols.n_rows == int(keep.sum())
    assert _as_python(cols) == want
    for k in cols:
        assert len(cols[k]) == int(keep.sum()), k
    fresh = StringColumn()
    fresh.extend(want["doc_id"])
    assert np.array_equal(cols["doc_id"].keys(), fresh.keys())
    ts = cols.token_sets()
    assert ts.ids == dictionary                # the dictionary stays: an id never changes
    assert [ts.row(r).tolist() for r in range(len(ts))] == [t for t, kp in zip(tokens_before, keep) if kp]
    assert ts.indptr()[0] == 0 and ts.indptr()[-1] == len(ts.tokens())
    # the columns keep growing
    cols["id"].append("later")
    cols["content"].append("ünï later")
    assert cols["id"][len(cols["id"]) - 1] == "later" and cols["content"][len(cols["content"]) - 1] == "ünï later"
    with pytest.raises(ValueError):
        cols["chunk_index"].compact(np.ones(3, bool))


def test_token_set_column_compact():
    col = TokenSetColumn()
    contents = ["a b c", "", "c d", "A a", "e f g h", ""]
    col.extend(contents)
    keep = np.array([0, 1, 1, 0, 1, 1], bool)
    rows = [col.row(r).tolist() for r in range(len(contents))]
    col.compact(keep)
    assert len(col) == 4
    assert [col.row(r).tolist() for r in range(4)] == [rows[1], rows[2], rows[4], rows[5]]
    col.extend(["h a"])
    assert col.row(4).tolist() == sorted([col.ids["h"], col.ids["a"]])
    num = NumericColumn(np.int64)
    num.extend(range(6))
    num.compact(keep)
    assert num.tolist() == [1, 2, 4, 5]
    num.append(9)
    assert num.tolist() == [1, 2, 4, 5, 9]


class _OracleShard:
    """Stands in for a ShardHandle: the oracle over the rows it was given (local row numbers), with the handle's search
    signatures and compact()."""
    fail_compact = False

    def __init__(self, sparse_dim):
        self.X = None
        self.ptr, self.idx, self.val = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
        self.device, self.sparse_dim = 0, sparse_dim

    num_rows = property(lambda self: 0 if self.X is None else self.X.shape[0])
    num_sparse_rows = property(lambda self: len(self.ptr) - 1)
    device_bytes = property(lambda self: 0 if self.X is None else self.X.nbytes)

    def add_dense(self, rows):
        self.X = rows.copy() if self.X is None else np.concatenate([self.X, rows])

    def add_sparse(self, ptr, idx, val):
        self.idx = np.concatenate([self.idx, idx[ptr[0]:ptr[-1]]])
        self.val = np.concatenate([self.val, val[ptr[0]:ptr[-1]]])
        self.ptr = np.concatenate([self.ptr, ptr[1:] - ptr[0] + self.ptr[-1]])

    def compact(self, keep=None, d_keep=0):
        if self.fail_compact:
            raise MemoryError("the new store does not fit beside the old one")
        keep = np.asarray(keep, dtype=bool)
        rows = np.nonzero(keep)[0]
        take = np.concatenate([np.arange(self.ptr[r], self.ptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        lens = (self.ptr[1:] - self.ptr[:-1])[rows]
        self.ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.idx, self.val, self.X = self.idx[take], self.val[take], self.X[keep]
        return len(rows), len(rows)

    def search_dense(self, q, k, mask=None):
        return oracle.dense_search(self.X, q, k, oracle.COSINE, mask)

    def search_sparse(self, queries, k, drop, mask=None):
        return oracle.sparse_search(self.ptr, self.idx, self.val, queries, k, drop, mask)

    def finalize(self):
        pass

    def close(self):
        pass


def _corpus(n=700, d=16, v=200):
    rng = np.random.default_rng(41)
    X = rng.standard_normal((n, d)).astype(np.float32)
    idx = (np.arange(4) * 50 + rng.integers(0, 50, size=(n, 4))).astype(np.int32).reshape(-1)
    val = (np.abs(rng.standard_normal(n * 4)) + 0.01).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * 4
    Q = rng.standard_normal((3, d)).astype(np.float32)
    SQ = [((np.arange(4) * 50 + rng.integers(0, 50, size=4)).astype(np.int32), np.ones(4, np.float32)) for _ in range(3)]
    return X, (ptr, idx, val), Q, SQ


def _shard_set(X, csr, n_shards=3):
    s = ShardSet([_OracleShard(200) for _ in range(n_shards)])
    for lo in range(0, X.shape[0], 250):     # several batches: every shard holds interleaved global ranges
        hi = min(lo + 250, X.shape[0])
        s.add(X[lo:hi], (csr[0][lo:hi + 1], csr[1], csr[2]))
    return s


def _same_as_oracle(s, X, csr, Q, SQ, keep, k=10):
    packed = None if keep is None else np.packbits(keep, bitorder="little")
    for got, want in ((s.search_dense(Q, k, keep), oracle.dense_search(X, Q, k, oracle.COSINE, packed)),
                      (s.search_sparse(SQ, k, 0.0, keep), oracle.sparse_search(*csr, SQ, k, 0.0, packed))):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _csr_rows(csr, keep):
    ptr, idx, val = csr
    rows = np.nonzero(keep)[0]
    take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows]).astype(np.int64)
    lens = (ptr[1:] - ptr[:-1])[rows]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[take], val[take]


def test_shard_set_compact_renumbers_after_the_last_shard():
    X, csr, Q, SQ = _corpus()
    n = X.shape[0]
    s = _shard_set(X, csr)
    keep = np.random.default_rng(2).random(n) < 0.6
    _same_as_oracle(s, X, csr, Q, SQ, keep)
    seen = []
    for h in s.handles:       # what the maps look like while shard after shard is compacted
        inner = h.compact
        def spy(own, d_keep=0, inner=inner):
            seen.append([r.copy() for r in s.rows_of])
            return inner(own, d_keep)
        h.compact = spy
    old_maps = [r.copy() for r in s.rows_of]
    assert s.compact(keep) == int(keep.sum())
    for i, maps in enumerate(seen):           # shards before i are cut down, all in OLD numbers
        for j, m in enumerate(maps):
            assert np.array_equal(m, old_maps[j][keep[old_maps[j]]] if j < i else old_maps[j])
    new_of = np.cumsum(keep) - 1
    for j, m in enumerate(s.rows_of):
        assert np.array_equal(m, new_of[old_maps[j][keep[old_maps[j]]]])
    assert sorted(np.concatenate(s.rows_of).tolist()) == list(range(int(keep.sum())))
    assert s.num_rows == s.num_sparse_rows == int(keep.sum())
    Xs, csr_s = X[keep], _csr_rows(csr, keep)
    _same_as_oracle(s, Xs, csr_s, Q, SQ, None)
    sub = np.random.default_rng(4).random(int(keep.sum())) < 0.5
    _same_as_oracle(s, Xs, csr_s, Q, SQ, sub)
    # and appends go on from the new row count
    base, end, _ = s.add(X[:5], (csr[0][:6], csr[1], csr[2]))
    assert (base, end) == (int(keep.sum()), int(keep.sum()) + 5)


def test_failing_second_shard_leaves_the_old_numbering_valid():
    X, csr, Q, SQ = _corpus()
    n = X.shape[0]
    s = _shard_set(X, csr)
    keep = np.random.default_rng(6).random(n) < 0.5
    old_maps = [r.copy() for r in s.rows_of]
    s.handles[1].fail_compact = True
    with pytest.raises(MemoryError):
        s.compact(keep)
    assert np.array_equal(s.rows_of[0], old_maps[0][keep[old_maps[0]]])       # cut down, old numbers
    assert np.array_equal(s.rows_of[1], old_maps[1]) and np.array_equal(s.rows_of[2], old_maps[2])
    assert all(len(r) == h.num_rows for r, h in zip(s.rows_of, s.handles))
    _same_as_oracle(s, X, csr, Q, SQ, keep)       # the tombstone mask still hides exactly the dead rows
    s.handles[1].fail_compact = False
    assert s.compact(keep) == int(keep.sum())     # the retry finishes the job
    _same_as_oracle(s, X[keep], _csr_rows(csr, keep), Q, SQ, None)


def test_keep_mask_must_cover_the_set():
    X, csr, _, _ = _corpus(n=100)
    s = _shard_set(X, csr, n_shards=2)
    with pytest.raises(ValueError):
        s.compact(np.ones(50, bool))
    assert s.num_rows == 100


def test_collective_shard_set_refuses():
    cs = CollectiveShardSet.__new__(CollectiveShardSet)     # no process group on this box: the method needs none
    with pytest.raises(NotImplementedError):
        cs.compact(np.ones(4, bool))
