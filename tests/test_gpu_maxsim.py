"""hr_maxsim_rerank_dev against the host restatement (advanced_rag/maxsim.py): positions, ids and counts equal, scores
compared with ==, padding as the header states.  Refused calls launch nothing: sentinel-filled outputs stay as they were.
No tolerance anywhere: the inputs are finite fp16 by construction, so the restatement alone decides every value."""
import numpy as np
import pytest

from advanced_rag import _native as nat
from advanced_rag import maxsim as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7
FIRST_ROW = 1000
ROW_TOKENS = (0, 1, 15, 16, 17, 31, 33, 100)     # both sides of the 16-token tile, an empty row, a long row


def make_store(rng, rows, dim, scale=1.0):
    """`rows` rows whose token counts cycle through ROW_TOKENS in a shuffled order."""
    T = np.array([ROW_TOKENS[i % len(ROW_TOKENS)] for i in range(rows)])
    rng.shuffle(T)
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    vals = (rng.standard_normal((int(indptr[-1]), dim)) * scale).astype(np.float16)
    return indptr, vals


def make_queries(rng, B, tq_stride, dim, scale=1.0):
    return (rng.standard_normal((B, tq_stride, dim)) * scale).astype(np.float16)


def make_lists(rng, B, k_in, rows, lo=20, hi=20):
    """ids [B, k_in] drawn WITH repetition from the store's rows and `lo` / `hi` ids below / above it; list 0 is empty and
    list 1 short when B >= 3, the last is full."""
    ids = rng.integers(FIRST_ROW - lo, FIRST_ROW + rows + hi, (B, k_in)).astype(np.int64)
    n = np.full(B, k_in, dtype=np.int32)
    if B >= 3:
        n[0] = 0
        n[1] = max(1, k_in // 3) if k_in > 1 else 0
    return ids, n


def run_dev(ids, n, qtok, qn, indptr, vals, first_row, k_out, use_n=True):
    B, k_in = ids.shape
    ids = ids.copy()
    if not use_n:                                   # the prefix ends at the first id < 0 instead
        for q in range(B):
            ids[q, n[q]:] = -1
    t_ids = torch.from_numpy(ids).cuda()
    t_n = torch.from_numpy(np.ascontiguousarray(n)).cuda() if use_n else None
    t_q = torch.from_numpy(np.ascontiguousarray(qtok).view(np.int16)).cuda()
    t_qn = torch.from_numpy(np.ascontiguousarray(qn, dtype=np.int32)).cuda()
    tok_rows = 0 if indptr is None else len(indptr) - 1
    t_ip = torch.from_numpy(indptr).cuda() if tok_rows else None
    t_v = torch.from_numpy(np.ascontiguousarray(vals).view(np.int16).reshape(-1)).cuda() if tok_rows else None
    if t_v is not None and t_v.numel() == 0:
        t_v = torch.zeros(8, dtype=torch.int16, device="cuda")     # a store of empty rows still needs a pointer
    op = torch.full((B, k_out), SENT, dtype=torch.int32, device="cuda")
    oi = torch.full((B, k_out), SENT, dtype=torch.int64, device="cuda")
    os_ = torch.full((B, k_out), float(SENT), dtype=torch.float64, device="cuda")
    on = torch.full((B,), SENT, dtype=torch.int32, device="cuda")
    nat.maxsim_rerank_dev(t_ids.data_ptr(), t_n.data_ptr() if use_n else 0, B, k_in, t_q.data_ptr(), t_qn.data_ptr(),
                          qtok.shape[1], qtok.shape[2], t_ip.data_ptr() if tok_rows else 0, t_v.data_ptr() if tok_rows else 0,
                          tok_rows, first_row, k_out, op.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return op.cpu().numpy(), oi.cpu().numpy(), os_.cpu().numpy(), on.cpu().numpy()


def run_host(ids, n, qtok, qn, indptr, vals, first_row, k_out):
    B = ids.shape[0]
    wp = np.full((B, k_out), -1, dtype=np.int32)
    wi = np.full((B, k_out), -1, dtype=np.int64)
    ws = np.zeros((B, k_out), dtype=np.float64)
    wn = np.zeros(B, dtype=np.int32)
    if indptr is None:
        indptr, vals = np.zeros(1, dtype=np.int64), np.zeros((0, qtok.shape[2]), dtype=np.float16)
    for q in range(B):
        tq = int(min(max(int(qn[q]), 0), qtok.shape[1]))
        pos, oid, fin = M.maxsim_rerank_csr(ids[q, :n[q]].tolist(), qtok[q, :tq], indptr, vals, first_row, k_out)
        wp[q, :len(pos)], wi[q, :len(pos)], ws[q, :len(pos)], wn[q] = pos, oid, fin, len(pos)
    return wp, wi, ws, wn


def check(got, want):
    for g, w in zip((got[3], got[0], got[1]), (want[3], want[0], want[1])):
        assert np.array_equal(g, w)
    assert (got[2] == want[2]).all()
    assert not (np.signbit(got[2]) & (got[2] == 0)).any()      # S is never -0.0


def test_version(gpu):
    assert nat.load_library().hr_version() >= 12100


@pytest.mark.parametrize("dim", [8, 72, 128, 256])
def test_kernel_equals_the_restatement(gpu, dim):
    """Every Tq around the 16-token tile in one launch (tq_stride larger than most d_qn), rows of every length of
    ROW_TOKENS in one list, ids below and above the store, first_row != 0, d_n given and NULL, both cuts."""
    rng = np.random.default_rng(dim)
    indptr, vals = make_store(rng, 64, dim)
    qtok = make_queries(rng, 6, 64, dim)
    for qn in ([1, 15, 16, 17, 33, 64], [64, 33, 17, 16, 1, 15]):
        ids, n = make_lists(rng, 6, 40, 64)
        for k_out in (7, 40):
            want = run_host(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_out)
            check(run_dev(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_out, use_n=k_out == 7), want)
    qtok5 = make_queries(rng, 5, 40, dim)           # B = 5, five different token counts, one of them beyond the stride
    qn5 = [3, 40, 17, 99, 32]
    ids, n = make_lists(rng, 5, 40, 64)
    check(run_dev(ids, n, qtok5, qn5, indptr, vals, FIRST_ROW, 40), run_host(ids, n, qtok5, qn5, indptr, vals, FIRST_ROW, 40))


@pytest.mark.parametrize("k_in", [1, 40, 256, 768])
def test_list_lengths(gpu, k_in):
    """Lists of every size up to the cap (the long ones repeat ids: equal scores keep list order), d_n shorter than k_in
    and d_n == NULL with a -1 terminator, k_out below and above n."""
    rng = np.random.default_rng(k_in)
    dim = 24
    indptr, vals = make_store(rng, 48, dim)
    qtok = make_queries(rng, 3, 20, dim)
    qn = [20, 7, 17]
    ids, n = make_lists(rng, 3, k_in, 48, lo=5, hi=5)
    for k_out in sorted({1, max(1, k_in // 2), k_in}):
        want = run_host(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_out)
        check(run_dev(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_out, use_n=True), want)
        check(run_dev(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_out, use_n=False), want)


def test_all_negative_similarities(gpu):
    """Every document token is -(a query token) and the query tokens are positive, so every similarity is negative: a padded
    column of a short tile, scored as 0, would win a maximum; an empty row (S = 0.0 by the contract) outranks real rows."""
    rng = np.random.default_rng(3)
    dim, B, tq = 40, 2, 17
    qtok = (np.abs(rng.standard_normal((B, tq, dim))) + 0.125).astype(np.float16)
    T = np.array([ROW_TOKENS[i % len(ROW_TOKENS)] for i in range(32)])
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    vals = -qtok[0][rng.integers(0, tq, int(indptr[-1]))]
    ids = np.stack([rng.permutation(32) for _ in range(B)]).astype(np.int64) + FIRST_ROW
    n = np.full(B, 32, dtype=np.int32)
    qn = [tq, tq]
    got = run_dev(ids, n, qtok, qn, indptr, vals, FIRST_ROW, 32)
    check(got, run_host(ids, n, qtok, qn, indptr, vals, FIRST_ROW, 32))
    empty = set((np.flatnonzero(T == 0) + FIRST_ROW).tolist())
    for q in range(B):
        assert set(got[1][q, :len(empty)].tolist()) == empty and not got[2][q, :len(empty)].any()
        assert (got[2][q, len(empty):] < 0).all()


def test_ties_and_empty_rows(gpu):
    """A list of one id repeated keeps its order; so does a list of only empty or outside rows, with all-zero scores; a
    query without tokens scores everything 0.0."""
    rng = np.random.default_rng(4)
    dim = 16
    indptr, vals = make_store(rng, 40, dim)
    T = np.diff(indptr)
    qtok = make_queries(rng, 4, 16, dim)
    k_in = 30
    full = int(np.flatnonzero(T == 100)[0]) + FIRST_ROW
    empties = np.flatnonzero(T == 0) + FIRST_ROW
    ids = np.zeros((4, k_in), dtype=np.int64)
    ids[0] = full
    ids[1] = np.resize(np.concatenate([empties, [FIRST_ROW - 1, FIRST_ROW + 40, 0]]), k_in)
    ids[2] = rng.integers(FIRST_ROW, FIRST_ROW + 40, k_in)
    ids[3] = ids[2]
    n = np.full(4, k_in, dtype=np.int32)
    qn = [16, 16, 0, -5]
    got = run_dev(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_in)
    check(got, run_host(ids, n, qtok, qn, indptr, vals, FIRST_ROW, k_in))
    for q in range(4):
        assert np.array_equal(got[0][q], np.arange(k_in))
    assert not got[2][1:].any() and got[2][0, 0] != 0


def test_no_token_store(gpu):
    """tok_rows == 0 with NULL arrays: every score 0.0, the order kept; B == 0 launches nothing."""
    rng = np.random.default_rng(5)
    qtok = make_queries(rng, 3, 8, 8)
    ids, n = make_lists(rng, 3, 12, 10)
    got = run_dev(ids, n, qtok, [8, 8, 8], None, None, 0, 12)
    check(got, run_host(ids, n, qtok, [8, 8, 8], None, None, 0, 12))
    assert not got[2].any()
    nat.maxsim_rerank_dev(0, 0, 0, 12, 0, 0, 8, 8, 0, 0, 0, 0, 12, 0, 0, 0, 0)
    torch.cuda.synchronize()


def test_magnitudes(gpu):
    """+-60000 at dim 256 (sums near 1e12, far from fp32 overflow) and fp16 subnormals (every product a tiny normal fp32)."""
    rng = np.random.default_rng(6)
    dim = 256
    T = np.array([17, 1, 33, 16])
    indptr = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    big = (rng.choice([-60000.0, 60000.0, 59999.0, -123.0], (int(indptr[-1]), dim))).astype(np.float16)
    qbig = (rng.choice([-60000.0, 60000.0, 1.0], (2, 17, dim))).astype(np.float16)
    ids = np.tile(np.arange(4, dtype=np.int64) + FIRST_ROW, (2, 1))
    n = np.full(2, 4, dtype=np.int32)
    got = run_dev(ids, n, qbig, [17, 16], indptr, big, FIRST_ROW, 4)
    check(got, run_host(ids, n, qbig, [17, 16], indptr, big, FIRST_ROW, 4))
    assert np.isfinite(got[2]).all() and np.abs(got[2]).max() > 1e11
    shape = (int(indptr[-1]), dim)                  # magnitude bits below 2^10 = subnormal, either sign; half the store normal
    sub = (rng.integers(0, 1024, shape) | (rng.integers(0, 2, shape) << 15)).astype(np.uint16).view(np.float16)
    sub = np.where(rng.random(shape) < 0.5, sub, rng.standard_normal(shape).astype(np.float16))
    qsub = rng.integers(1, 1024, (2, 17, dim)).astype(np.uint16).view(np.float16)
    got = run_dev(ids, n, qsub, [17, 16], indptr, sub, FIRST_ROW, 4)
    check(got, run_host(ids, n, qsub, [17, 16], indptr, sub, FIRST_ROW, 4))
    assert got[2].any()


def test_refusals_leave_the_outputs_alone(gpu):
    rng = np.random.default_rng(7)
    B, k, dim, tq = 2, 8, 16, 8
    indptr, vals = make_store(rng, 16, dim)
    ids, n = make_lists(rng, B, k, 16)
    t = {"ids": torch.from_numpy(ids).cuda(), "n": torch.from_numpy(n).cuda(),
         "q": torch.from_numpy(make_queries(rng, B, tq, dim).view(np.int16)).cuda(),
         "qn": torch.full((B,), tq, dtype=torch.int32, device="cuda"), "ip": torch.from_numpy(indptr).cuda(),
         "v": torch.from_numpy(vals.view(np.int16)).cuda()}
    big = 3 * nat.HR_MAX_TOPK + 1
    out = {"pos": torch.full((B, big), SENT, dtype=torch.int32, device="cuda"),
           "ids": torch.full((B, big), SENT, dtype=torch.int64, device="cuda"),
           "sc": torch.full((B, big), float(SENT), dtype=torch.float64, device="cuda"),
           "n": torch.full((B,), SENT, dtype=torch.int32, device="cuda")}

    def call(**kw):
        a = dict(d_ids=t["ids"].data_ptr(), d_n=t["n"].data_ptr(), B=B, k_in=k, d_qtok=t["q"].data_ptr(), d_qn=t["qn"].data_ptr(),
                 tq_stride=tq, dim=dim, d_indptr=t["ip"].data_ptr(), d_tok=t["v"].data_ptr(), tok_rows=16, first_row=FIRST_ROW,
                 k_out=k, d_out_pos=out["pos"].data_ptr(), d_out_ids=out["ids"].data_ptr(), d_out_scores=out["sc"].data_ptr(),
                 d_out_n=out["n"].data_ptr())
        a.update(kw)
        nat.maxsim_rerank_dev(**a)

    bad = [dict(d_ids=0), dict(d_qtok=0), dict(d_qn=0), dict(d_out_pos=0), dict(d_out_ids=0), dict(d_out_scores=0),
           dict(d_out_n=0), dict(d_indptr=0), dict(d_tok=0), dict(dim=4), dict(dim=0), dict(dim=12), dict(dim=20),
           dict(d_qtok=t["q"].data_ptr() + 2), dict(d_tok=t["v"].data_ptr() + 8), dict(k_out=0), dict(k_out=k + 1), dict(k_in=0),
           dict(B=-1), dict(tok_rows=-1), dict(first_row=-1), dict(tq_stride=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(k_in=big, k_out=big), dict(tq_stride=nat.HR_MAX_QUERY_TOKENS + 1), dict(dim=264)):
        with pytest.raises(nat.HbmRagError) as e:      # HR_ELIMIT
            call(**kw)
        assert e.value.status == 5
    torch.cuda.synchronize()
    for o in out.values():
        assert bool((o == SENT).all())
    call()                                          # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert int(out["n"][0]) == int(n[0]) and int(out["n"][1]) == int(n[1])
