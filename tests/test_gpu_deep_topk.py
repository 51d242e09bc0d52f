"""hr_deep_topk_dev, the deep search's selection alone, on arrays of the test's making against oracle.topk at k = W sliced
[offset:]: ids equal, score bits equal.  The candidates come in the refine kernels' layout (score fp32, row int32, row < 0 =
invalid); the rows are a shuffled permutation so that slot order and row order differ."""
import functools

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS = [0, 1, 255, 256, 257, 1023, 1025, 16384, 16385, 100_003]
WS = [1, 256, 257, 1000, 4096, 16383, 16384]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(scores, rows, k, offset, ascending=False, row_offset=0):
    """scores / rows [B, n] -> (ids [B, k], scores [B, k]) of hr_deep_topk_dev."""
    scores = np.ascontiguousarray(np.atleast_2d(scores), dtype=np.float32)
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.int32)
    B, n = scores.shape
    ds, dr = torch.from_numpy(scores).cuda(), torch.from_numpy(rows).cuda()
    ids = torch.full((B, k), 7, dtype=torch.int64, device="cuda")
    sc = torch.full((B, k), 7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(max(nat.deep_topk_scratch_bytes(n, B, k + offset), 8), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    nat.deep_topk_dev(ds.data_ptr(), dr.data_ptr(), n, B, k, offset, ascending, row_offset, ids.data_ptr(), sc.data_ptr(),
                      scratch.data_ptr(), st.cuda_stream)
    st.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def want(scores, rows, W, row_offset=0):
    """oracle.topk at depth W of one query's candidates (the scores laid out by row, the invalid ones masked)."""
    n_rows = int(rows.max()) + 1 if (rows >= 0).any() else 1
    by_row = np.zeros(n_rows, np.float32)
    keep = np.zeros(n_rows, bool)
    ok = rows >= 0
    by_row[rows[ok]] = scores[ok]
    keep[rows[ok]] = True
    return oracle.topk(by_row, W, np.packbits(keep, bitorder="little"), False, row_offset)


def check(scores, rows, W, offset, **kw):
    scores, rows = np.atleast_2d(scores), np.atleast_2d(rows)
    ids, sc = run(scores, rows, W - offset, offset, **kw)
    for b in range(scores.shape[0]):
        wi, ws = want(scores[b], rows[b], W, kw.get("row_offset", 0))
        if kw.get("ascending"):
            ws = np.where(wi >= 0, -ws, np.float32(0))
        assert np.array_equal(ids[b], wi[offset:]), f"query {b}: ids differ at {np.flatnonzero(ids[b] != wi[offset:])[:5]}"
        assert np.array_equal(bits(sc[b]), bits(ws[offset:])), f"query {b}: score bits differ"


@functools.lru_cache(maxsize=None)
def candidates(n, B=3):
    """B queries of n candidates: scores on a coarse grid on both sides of zero (ties everywhere, no zero: the oracle does
    not order -0 against +0), a tenth of the slots invalid, rows shuffled."""
    rng = np.random.default_rng(n + 1)
    scores = ((rng.integers(-2000, 2000, (B, n)) + 0.5) / 64).astype(np.float32)
    rows = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32) if n else np.zeros((B, 0), np.int32)
    rows[rng.random((B, n)) < 0.1] = -1
    return scores, rows


@functools.lru_cache(maxsize=None)
def reference(n, b):
    scores, rows = candidates(n)
    return want(scores[b], rows[b], nat.HR_MAX_DEEP_K)


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("n", NS)
def test_window_of_the_ranking(gpu, n, W):
    scores, rows = candidates(n)
    for B in (1, 3):
        for offset in sorted({0, 1, 255, 256, W - 1}):
            if offset >= W:
                continue
            ids, sc = run(scores[:B], rows[:B], W - offset, offset)
            for b in range(B):
                wi, ws = reference(n, b)                      # the depth-16384 ranking, computed once: R[:W] is its head
                assert np.array_equal(ids[b], wi[offset:W]), (n, W, offset, B, b)
                assert np.array_equal(bits(sc[b]), bits(ws[offset:W])), (n, W, offset, B, b)


def test_fewer_valid_rows_than_the_window_and_none(gpu):
    scores, rows = (a.copy() for a in candidates(1025))
    rows[:, 300:] = -1                                            # some 270 valid candidates
    for W, offset in ((1000, 0), (1000, 256), (257, 0), (16384, 255)):
        check(scores, rows, W, offset)
    for n in (1025, 100_003):
        s, r = candidates(n)
        ids, sc = run(s, np.full_like(r, -1), 300, 100)
        assert (ids == -1).all() and (bits(sc) == 0).all()


@pytest.mark.parametrize("n", [1025, 100_003])
def test_every_score_equal_the_row_bits_decide(gpu, n):
    rng = np.random.default_rng(n)
    rows = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    for value in (0.75, -3.0):
        scores = np.full((2, n), value, np.float32)
        for W, offset in ((257, 0), (1000, 999), (1000, 256)):
            check(scores, rows, W, offset)
        ids, _ = run(scores, rows, 744, 256)
        assert np.array_equal(ids[0], np.arange(256, 1000))       # row ascending, nothing else


@pytest.mark.parametrize("W,offset", [(1000, 0), (1000, 990), (600, 300), (4096, 256)])
def test_boundary_and_offset_inside_a_run_of_ties(gpu, W, offset):
    """Two distinct scores, the better one on n_hi rows.  n_hi < W puts position W inside the run of the worse score; n_hi
    a few rows off `offset` puts position offset next to the change of score, inside one run or the other."""
    n = 20_000
    rng = np.random.default_rng(W + offset)
    n_hi = {(1000, 0): 400, (1000, 990): 995, (600, 300): 290, (4096, 256): 250}[(W, offset)]
    scores = np.full(n, 0.25, np.float32)
    scores[rng.permutation(n)[:n_hi]] = 0.5
    rows = rng.permutation(n).astype(np.int32)
    check(scores, rows, W, offset)
    check(-scores, rows, W, offset)                               # the run of ties at the top instead


def test_ascending_writes_distances_and_row_offset_is_added(gpu):
    scores, rows = candidates(16385)
    dist = -np.abs(scores)                                        # negated distances
    check(dist, rows, 1000, 256, ascending=True)
    check(dist, rows, 300, 0, ascending=True, row_offset=5_000_000_000)
    check(scores, rows, 4096, 1, row_offset=123_456_789)
    ids, sc = run(dist[:1], rows[:1], 300, 0, ascending=True)
    assert (sc[0][ids[0] >= 0] >= 0).all() and (np.diff(sc[0]) >= 0).all()


def test_the_same_call_twice_gives_identical_bytes(gpu):
    scores, rows = candidates(100_003)
    a = run(scores, rows, 16384 - 255, 255)
    b = run(scores, rows, 16384 - 255, 255)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_limit_refusals(gpu):
    scores, rows = candidates(1025)
    for k, offset in ((16385, 0), (16384, 1), (1, 16384)):
        with pytest.raises(nat.HbmRagError) as ei:
            run(scores, rows, k, offset)
        assert ei.value.status == 5                               # HR_ELIMIT
    # HR_EINVAL: refused before a buffer is looked at (the pointers are never read)
    for n, k, offset in ((10, 0, 0), (10, -1, 5), (10, 10, -1), (-1, 10, 0)):
        with pytest.raises(ValueError):
            nat.deep_topk_dev(8, 8, n, 1, k, offset, False, 0, 8, 8, 8)
    ids, sc = run(scores, rows, 16384, 0)                         # the limit itself is served
    assert (ids[:, :900] >= 0).all()
