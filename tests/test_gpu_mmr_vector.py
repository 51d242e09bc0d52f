"""hr_mmr_select_vec_dev against the host restatement (advanced_rag/mmr.py): positions, the bits of every pick's value and the
counts are equal; padding is -1 / 0.0; nothing is written behind the outputs; refused calls write nothing.  The
restatement's similarities are themselves held to oracle.dense_scores once."""
import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag import mmr as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = 1500          # 93 row blocks and a last one of 12 rows
OFFSET = 7000        # hr_set_row_offset
CANARY = 8           # elements behind every output
SENT = -7
METRICS = {"COSINE": nat.HR_METRIC_COSINE, "IP": nat.HR_METRIC_IP, "L2": nat.HR_METRIC_L2}
# local rows that every list set draws from: the first tile's near-copies, zero rows, anti-parallel pairs, the last tile
CLUSTER = [0, 1, 2, 3, 4]
ZERO_ROWS = [9, 760]
ANTI = [(20, 21), (750, 1497)]
EDGE_ROWS = CLUSTER + ZERO_ROWS + [a for p in ANTI for a in p] + [15, 16, 751, 1488, 1499]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_rows(rng, dim, np_dtype):
    """ROWS x dim stored rows (values on a coarse grid, exact in fp16): a cluster of five near-copies at the head, two
    zero rows, two anti-parallel pairs."""
    X = (np.round(rng.standard_normal((ROWS, dim)) * 8) / 8).astype(np_dtype)
    X[np.all(X == 0, axis=1)] = 1             # only the planted rows are zero (dim 1 rounds many to 0)
    for j in CLUSTER[1:]:
        X[j] = X[0]
        X[j, (j * 3) % dim] += np_dtype(0.125)       # dim 1: a parallel row, cosine exactly 1
    X[ZERO_ROWS] = 0
    for a, b in ANTI:
        X[b] = -X[a]
    return X


_SHARDS = {}


def shard(dim, dtype, metric):
    """One shard per (dim, dtype, metric) for the whole module: (handle, stored rows)."""
    key = (dim, dtype, metric)
    if key not in _SHARDS:
        np_dtype = np.float16 if dtype == nat.HR_F16 else np.float32
        X = make_rows(np.random.default_rng(dim * 10 + dtype), dim, np_dtype)
        h = nat.ShardHandle(dim, dtype, METRICS[metric])
        h.set_row_offset(OFFSET)
        h.add_dense(X)
        h.finalize()
        _SHARDS[key] = (h, X)
    return _SHARDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shards():
    yield
    for h, _ in _SHARDS.values():
        h.close()
    _SHARDS.clear()


def make_lists(rng, B, k_in, norm, f64):
    """ids [B, k_in] from inside the shard (always some of EDGE_ROWS) and from both sides of it; scores as a list with that
    norm code holds them, on a grid so that some are equal.  d_n: with B >= 3 an empty list, a short one and one beyond k_in."""
    pool = np.concatenate([np.arange(OFFSET - 20, OFFSET + ROWS + 20)])
    ids = np.empty((B, k_in), dtype=np.int64)
    for q in range(B):
        ids[q] = rng.choice(pool, k_in, replace=k_in > len(pool))
        edge = rng.permutation(EDGE_ROWS)[:min(k_in, len(EDGE_ROWS))] + OFFSET
        ids[q, rng.choice(k_in, len(edge), replace=False)] = edge
    if norm in (nat.HR_NORM_ATAN_DIST, nat.HR_NORM_MINMAX_DIST):
        s = np.sort(np.round(rng.uniform(0, 6, (B, k_in)) * 16) / 16, axis=1)
    elif norm in (nat.HR_NORM_COSINE, nat.HR_NORM_NONE):
        s = -np.sort(-np.round(rng.uniform(-1, 1, (B, k_in)) * 64) / 64, axis=1)
    else:
        s = -np.sort(-np.round(rng.uniform(-20, 60, (B, k_in)) * 8) / 8, axis=1)
    if f64:
        s = s + rng.uniform(0, 1e-9, s.shape)      # not representable in fp32: a narrowing would show
    n = np.full(B, k_in, dtype=np.int32)
    if B >= 3:
        n[0], n[1], n[2] = 0, max(1, k_in // 3), k_in + 5
    lam = np.round(rng.uniform(0, 1, B) * 16) / 16
    lam[-1] = 0.5
    return ids, s.astype(np.float64 if f64 else np.float32), n, lam


class Out:
    """Garbage-filled outputs with a canary behind each."""

    def __init__(self, B, k_out):
        self.B, self.k_out = B, k_out
        self.pos = torch.full((B * k_out + CANARY,), SENT, dtype=torch.int32, device="cuda")
        self.val = torch.full((B * k_out + CANARY,), float(SENT), dtype=torch.float64, device="cuda")
        self.n = torch.full((B + CANARY,), SENT, dtype=torch.int32, device="cuda")

    def host(self):
        torch.cuda.synchronize()
        pos, val, n = self.pos.cpu().numpy(), self.val.cpu().numpy(), self.n.cpu().numpy()
        m = self.B * self.k_out
        assert (pos[m:] == SENT).all() and (val[m:] == SENT).all() and (n[self.B:] == SENT).all(), "written behind an output"
        return pos[:m].reshape(self.B, self.k_out), val[:m].reshape(self.B, self.k_out), n[:self.B]

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.pos == SENT).all() and (self.val == SENT).all() and (self.n == SENT).all())


def launch(h, t_ids, t_sc, f64, norm, t_n, B, k_in, t_lam, k_out, out, scratch=None):
    if scratch is None:
        scratch = torch.full((max(h.mmr_vec_scratch_bytes(B, k_in), 16),), 0xFF, dtype=torch.uint8, device="cuda")   # NaN bits
    h.mmr_select_vec_dev(t_ids.data_ptr(), t_sc.data_ptr(), f64, norm, t_n.data_ptr(), B, k_in, t_lam.data_ptr(), k_out,
                         scratch.data_ptr(), out.pos.data_ptr(), out.val.data_ptr(), out.n.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    return scratch


def run_dev(h, ids, scores, n, lam, norm, k_out):
    B, k_in = ids.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ids, scores, n, lam)]
    out = Out(B, k_out)
    keep = launch(h, dev[0], dev[1], scores.dtype == np.float64, norm, dev[2], B, k_in, dev[3], k_out, out)
    got = out.host()
    del keep
    return got


def vectors_of(X, ids):
    V = np.zeros((len(ids), X.shape[1]), dtype=X.dtype)
    inside = (ids >= OFFSET) & (ids < OFFSET + ROWS)
    V[inside] = X[ids[inside] - OFFSET]
    return V


def run_host(X, ids, scores, n, lam, norm, k_out):
    B, k_in = ids.shape
    wp = np.full((B, k_out), -1, dtype=np.int32)
    wv = np.zeros((B, k_out), dtype=np.float64)
    wn = np.zeros(B, dtype=np.int32)
    for q in range(B):
        m = int(min(max(n[q], 0), k_in))
        pos, val = M.vector_mmr([float(x) for x in scores[q, :m]], vectors_of(X, ids[q, :m]), float(lam[q]), k_out, norm)
        wp[q, :len(pos)], wv[q, :len(val)], wn[q] = pos, val, len(pos)
    return wp, wv, wn


def check(got, want):
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def test_restated_similarity_equals_the_oracle():
    """canonical_cosine over the planted rows of an fp16 and an fp32 shard's data = oracle.dense_scores(.., COSINE) bit for
    bit, and symmetric."""
    for np_dtype, dim in ((np.float16, 100), (np.float32, 8)):
        X = make_rows(np.random.default_rng(3), dim, np_dtype)[sorted(EDGE_ROWS)]
        C = M.canonical_cosine(X, X)
        for j in range(len(X)):
            want = oracle.dense_scores(X, X[j].astype(np.float32), oracle.COSINE)
            assert np.array_equal(C[:, j].astype(np.float32).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(bits(C), bits(C.T))


# dim, dtype, metric, norm codes, B, k_in, k_outs, fp64 scores
SHAPES = [
    (1, nat.HR_F16, "COSINE", (-1, 0, 3), 3, 2, (1, 2), False),
    (1, nat.HR_F32, "L2", (4,), 3, 1, (1,), False),
    (8, nat.HR_F32, "IP", (1, 3), 130, 40, (1, 20, 40), False),
    (8, nat.HR_F16, "COSINE", (0,), 1, 768, (20, 768), True),
    (100, nat.HR_F16, "L2", (2, 4), 3, 256, (20,), False),
    (100, nat.HR_F32, "COSINE", (3,), 3, 256, (256,), True),
    (384, nat.HR_F32, "COSINE", (-1,), 3, 40, (1, 20), False),
    (384, nat.HR_F16, "IP", (1,), 1, 40, (40,), True),
    (4096, nat.HR_F16, "COSINE", (-1,), 3, 4, (4,), False),
]


@pytest.mark.parametrize("dim,dtype,metric,norms,B,k_in,k_outs,f64", SHAPES,
                         ids=[f"d{s[0]}-{'f16' if s[1] == nat.HR_F16 else 'f32'}-{s[2]}-B{s[4]}-k{s[5]}" for s in SHAPES])
def test_kernel_equals_the_restatement(gpu, dim, dtype, metric, norms, B, k_in, k_outs, f64):
    h, X = shard(dim, dtype, metric)
    rng = np.random.default_rng(dim * 1000 + k_in)
    for norm in norms:
        ids, scores, n, lam = make_lists(rng, B, k_in, norm, f64)
        for k_out in k_outs:
            check(run_dev(h, ids, scores, n, lam, norm, k_out), run_host(X, ids, scores, n, lam, norm, k_out))


def planted_lists(k_in=40):
    """Five lists over the same ids, the cluster of near-copies at the head with the best scores:
    0 lambda 0.5 | 1 lambda 1 | 2 duplicate ids and equal scores | 3 a NaN score | 4 lambda 0 (diversity only)."""
    rng = np.random.default_rng(11)
    others = [r for r in rng.permutation(np.arange(30, 1400))[:k_in] if r not in EDGE_ROWS]
    tail = [ZERO_ROWS[0], ANTI[0][0], ANTI[0][1], ANTI[1][0], ANTI[1][1], 1499]
    row = np.array(CLUSTER + tail + others, dtype=np.int64)[:k_in] + OFFSET
    row[-1], row[-2] = OFFSET - 3, OFFSET + ROWS        # outside the shard, either side
    ids = np.tile(row, (5, 1))
    scores = np.tile((0.95 - 0.01 * np.arange(k_in)).astype(np.float32), (5, 1))
    ids[2, 7] = ids[2, 6]                                # a duplicate id
    ids[2, 12] = ids[2, 0]
    scores[2, 5:15] = scores[2, 5]                       # equal scores
    scores[3, 2] = np.nan
    n = np.full(5, k_in, dtype=np.int32)
    lam = np.array([0.5, 1.0, 0.5, 0.5, 0.0])
    return ids, scores, n, lam


@pytest.mark.parametrize("dtype", [nat.HR_F16, nat.HR_F32])
def test_planted_contents(gpu, dtype):
    """Near-duplicate clusters, duplicate ids, ids outside the shard, zero rows, anti-parallel pairs, equal scores, a NaN."""
    h, X = shard(8, dtype, "COSINE")
    ids, scores, n, lam = planted_lists()
    k_in = ids.shape[1]
    for k_out in (10, k_in):
        got = run_dev(h, ids, scores, n, lam, nat.HR_NORM_NONE, k_out)
        check(got, run_host(X, ids, scores, n, lam, nat.HR_NORM_NONE, k_out))
        pos, val, cnt = got
        assert list(pos[1, :k_out]) == list(range(k_out))                  # lambda = 1: the plain prefix
        assert np.array_equal(bits(val[1, :k_out]), bits(scores[1, :k_out].astype(np.float64)))   # 1 * rel - 0 * m
        assert list(pos[0, :5]) != [0, 1, 2, 3, 4]                         # lambda = 0.5 leaves it
        assert sum(p in (0, 1, 2, 3, 4) for p in pos[0, :5]) == 1          # one member of the cluster among the first five
        assert 2 not in pos[3]                                             # NaN is never picked
        assert cnt[3] == min(k_out, k_in - 1) and cnt[0] == k_out
    assert pos[3, k_in - 1] == -1 and val[3, k_in - 1] == 0.0              # the padding of the list that ran out


def test_negative_cosine_starts_the_running_maximum(gpu):
    """The one deviation from the Jaccard kernel: after the first pick an anti-parallel candidate has m = -1, not 0, and
    wins the second pick over a better-scored orthogonal one."""
    h, X = shard(8, nat.HR_F32, "COSINE")
    a, b = ANTI[0]
    ortho = next(r for r in range(30, 200) if abs(float(M.canonical_cosine(X[r:r + 1], X[a])[0])) < 0.3)
    ids = np.array([[a, ortho, b]], dtype=np.int64) + OFFSET
    scores = np.array([[0.9, 0.8, 0.5]], dtype=np.float32)
    n, lam = np.array([3], dtype=np.int32), np.array([0.5])
    V = vectors_of(X, ids[0])
    want = M.vector_mmr([float(x) for x in scores[0]], V, 0.5, 3)
    floor0 = M.vector_mmr([float(x) for x in scores[0]], V, 0.5, 3, m_starts_at_zero=True)
    assert want[0] == [0, 2, 1] and floor0[0] == [0, 1, 2]
    check(run_dev(h, ids, scores, n, lam, nat.HR_NORM_NONE, 3), run_host(X, ids, scores, n, lam, nat.HR_NORM_NONE, 3))


def test_two_runs_are_byte_identical(gpu):
    h, X = shard(100, nat.HR_F16, "L2")
    ids, scores, n, lam = make_lists(np.random.default_rng(5), 130, 80, nat.HR_NORM_MINMAX_DIST, False)
    a = run_dev(h, ids, scores, n, lam, nat.HR_NORM_MINMAX_DIST, 20)
    b = run_dev(h, ids, scores, n, lam, nat.HR_NORM_MINMAX_DIST, 20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def test_refusals_write_nothing(gpu):
    h, X = shard(8, nat.HR_F32, "COSINE")
    B, k_in, k_out = 3, 40, 20
    ids, scores, n, lam = make_lists(np.random.default_rng(6), B, k_in, nat.HR_NORM_NONE, False)
    t_ids = torch.from_numpy(np.concatenate([ids.reshape(-1), np.zeros(1, np.int64)])).cuda()
    t_sc, t_n, t_lam = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (scores, n, lam))
    out = Out(B, k_out)
    scratch = torch.zeros(h.mmr_vec_scratch_bytes(B, 769) + 64, dtype=torch.uint8, device="cuda")
    assert h.mmr_vec_scratch_bytes(B, k_in) >= B * k_in * 8 * 4 and h.mmr_vec_scratch_bytes(0, k_in) == 0

    class Null:
        @staticmethod
        def data_ptr():
            return 0

    class Shifted:
        def __init__(self, t, by):
            self.t, self.by = t, by

        def data_ptr(self):
            return self.t.data_ptr() + self.by

    def refused(status, **kw):
        a = dict(t_ids=t_ids, t_sc=t_sc, f64=False, norm=nat.HR_NORM_NONE, t_n=t_n, B=B, k_in=k_in, t_lam=t_lam, k_out=k_out,
                 out=out, scratch=scratch, h=h)
        a.update(kw)
        with pytest.raises(ValueError if status == 1 else nat.HbmRagError) as ei:
            launch(**a)
        if status != 1:
            assert ei.value.status == status
        assert out.untouched()

    refused(5, k_in=769)                                    # HR_ELIMIT
    refused(1, k_out=k_in + 1)                              # HR_EINVAL from here on
    refused(1, k_out=0)
    refused(1, B=-1)
    refused(1, norm=5)
    refused(1, norm=-2)
    refused(1, t_ids=Null)
    refused(1, t_lam=Null)
    refused(1, scratch=Null)
    refused(1, t_ids=Shifted(t_ids, 4))                     # misaligned
    refused(1, scratch=Shifted(scratch, 8))
    refused(1, t_sc=Shifted(t_sc, 4), f64=True)
    launch(h, t_ids, t_sc, False, nat.HR_NORM_NONE, t_n, 0, k_in, t_lam, k_out, out, scratch)      # B == 0: HR_OK, nothing
    assert out.untouched()
    fresh = nat.ShardHandle(8, nat.HR_F32, nat.HR_METRIC_COSINE)
    try:
        fresh.add_dense(X[:32])
        refused(2, h=fresh)                                 # HR_ESTATE: before hr_finalize
    finally:
        fresh.close()
    sparse = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_IP, 50)
    try:
        sparse.add_sparse(np.array([0, 1], np.int64), np.array([3], np.int32), np.array([1.0], np.float32))
        sparse.finalize()
        refused(2, h=sparse)                                # no dense collection
    finally:
        sparse.close()
    launch(h, t_ids, t_sc, False, nat.HR_NORM_NONE, t_n, B, k_in, t_lam, k_out, out, scratch)      # and the good call still runs
    check(out.host(), run_host(X, ids, scores, n, lam, nat.HR_NORM_NONE, k_out))
