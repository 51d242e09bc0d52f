"""hr_decay_rerank_dev against the host restatement (advanced_rag/decay.py): positions, ids and counts equal, final scores
bit for bit, padding as the header states.  Refused calls launch nothing: sentinel-filled outputs stay as they were."""
import math

import numpy as np
import pytest

from advanced_rag import _native as nat
from advanced_rag import decay as D

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7
FIRST_ROW = 1000
COL_ROWS = 900
KINDS = {"i64": (nat.HR_COL_I64, np.int64), "f32": (nat.HR_COL_F32, np.float32), "f64": (nat.HR_COL_F64, np.float64)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_column(rng, kind):
    """COL_ROWS values around 500; the float kinds hold NaN (rows without a value) and one infinity."""
    if kind == "i64":
        return rng.integers(0, 1000, COL_ROWS).astype(np.int64)
    col = np.round(rng.uniform(0, 1000, COL_ROWS) * 4) / 4
    col[rng.choice(COL_ROWS, 60, replace=False)] = np.nan
    col[7] = np.inf
    return col.astype(KINDS[kind][1])


def make_params(rng, B, funcs):
    """One operand set per query; curves cycle through `funcs`."""
    p = np.zeros(B, dtype=nat.DECAY_QUERY_DTYPE)
    for q in range(B):
        func = funcs[q % len(funcs)]
        scale, decay, offset = float(rng.uniform(20, 300)), float(rng.uniform(0.1, 0.9)), float(rng.choice([0.0, 15.0]))
        coef = (math.log(decay) / (scale * scale) if func == 0 else math.log(decay) / scale if func == 1
                else (1.0 - decay) / scale)
        p[q] = (float(rng.uniform(300, 700)), offset, coef, func, 0)
    return p


def make_lists(rng, B, k_in, f64, norm):
    """ids [B, k_in] mostly inside the column, some below and above it; scores as a list with that norm code holds them.
    Query 0 is empty, query 1 short (when B >= 3); the last is full."""
    ids = np.stack([rng.choice(np.arange(FIRST_ROW - 40, FIRST_ROW + COL_ROWS + 40), k_in, replace=False) for _ in range(B)])
    if norm in (nat.HR_NORM_ATAN_DIST, nat.HR_NORM_MINMAX_DIST):
        s = np.sort(np.round(rng.uniform(0, 6, (B, k_in)) * 16) / 16, axis=1)
    elif norm == nat.HR_NORM_COSINE:
        s = -np.sort(-np.round(rng.uniform(-1, 1, (B, k_in)) * 64) / 64, axis=1)
    else:
        s = -np.sort(-np.round(rng.uniform(-20, 60, (B, k_in)) * 8) / 8, axis=1)
    if f64:
        s = s + rng.uniform(0, 1e-9, s.shape)      # not representable in fp32: a narrowing would show
    n = np.full(B, k_in, dtype=np.int32)
    if B >= 3:
        n[0] = 0
        n[1] = max(1, k_in // 3) if k_in > 1 else 0
    return ids.astype(np.int64), s.astype(np.float64 if f64 else np.float32), n


def run_dev(ids, scores, n, col, kind, first_row, params, norm, k_out, use_n=True, col_rows=None):
    B, k_in = ids.shape
    ids = ids.copy()
    if not use_n:                                   # the prefix ends at the first id < 0 instead
        for q in range(B):
            ids[q, n[q]:] = -1
    t_ids = torch.from_numpy(ids).cuda()
    t_sc = torch.from_numpy(np.ascontiguousarray(scores)).cuda()
    t_n = torch.from_numpy(np.ascontiguousarray(n)).cuda() if use_n else None
    t_col = torch.from_numpy(np.ascontiguousarray(col)).cuda() if col is not None and len(col) else None
    t_p = torch.from_numpy(params.view(np.uint8).reshape(B, -1).copy()).cuda()
    op = torch.full((B, k_out), SENT, dtype=torch.int32, device="cuda")
    oi = torch.full((B, k_out), SENT, dtype=torch.int64, device="cuda")
    os_ = torch.full((B, k_out), float(SENT), dtype=torch.float64, device="cuda")
    on = torch.full((B,), SENT, dtype=torch.int32, device="cuda")
    nat.decay_rerank_dev(t_ids.data_ptr(), t_sc.data_ptr(), scores.dtype == np.float64, t_n.data_ptr() if use_n else 0, B, k_in,
                         t_col.data_ptr() if t_col is not None else 0, KINDS[kind][0],
                         (len(col) if col is not None else 0) if col_rows is None else col_rows, first_row, t_p.data_ptr(),
                         norm, k_out, op.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return op.cpu().numpy(), oi.cpu().numpy(), os_.cpu().numpy(), on.cpu().numpy()


def run_host(ids, scores, n, col, first_row, params, norm, k_out):
    B = ids.shape[0]
    wp = np.full((B, k_out), -1, dtype=np.int32)
    wi = np.full((B, k_out), -1, dtype=np.int64)
    ws = np.zeros((B, k_out), dtype=np.float64)
    wn = np.zeros(B, dtype=np.int32)
    for q in range(B):
        lid = ids[q, :n[q]].tolist()
        vals = [float(col[i - first_row]) if col is not None and first_row <= i < first_row + len(col) else float("nan")
                for i in lid]
        ops = (float(params[q]["origin"]), float(params[q]["offset"]), float(params[q]["coef"]), int(params[q]["func"]))
        pos, oid, fin = D.decay_rerank(lid, [float(x) for x in scores[q, :n[q]]], vals, ops, norm, k_out)
        wp[q, :len(pos)], wi[q, :len(pos)], ws[q, :len(pos)], wn[q] = pos, oid, fin, len(pos)
    return wp, wi, ws, wn


def check(got, want):
    for g, w in zip((got[3], got[0], got[1]), (want[3], want[0], want[1])):
        assert np.array_equal(g, w)
    assert np.array_equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("kind", ["i64", "f32", "f64"])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("k_in", [1, 40, 257, 768])
def test_kernel_equals_the_restatement(gpu, k_in, f64, kind):
    """B = 3 (empty, short, full), the three curves in one launch, every norm code, both cuts, d_n given and NULL."""
    seed = k_in * 100 + f64 * 10 + list(KINDS).index(kind)
    rng = np.random.default_rng(seed)
    col = make_column(rng, kind)
    params = make_params(rng, 3, (2, 0, 1))
    for norm in (-1, 0, 1, 2, 3, 4):
        ids, scores, n = make_lists(rng, 3, k_in, f64, norm)
        for k_out in sorted({1, k_in}):
            want = run_host(ids, scores, n, col, FIRST_ROW, params, norm, k_out)
            check(run_dev(ids, scores, n, col, kind, FIRST_ROW, params, norm, k_out, use_n=(norm + k_out) % 2 == 0), want)
            if norm == 0:
                check(run_dev(ids, scores, n, col, kind, FIRST_ROW, params, norm, k_out, use_n=k_out != 1), want)


def test_ties_saturation_and_bad_function(gpu):
    """Equal values and equal scores tie (input order holds, also where every factor is zero); c * d * d below -708 gives
    0.0; a function code outside 0..2 gives factor 0 for that query; d_n beyond k_in is clamped."""
    k_in, B = 300, 5
    ids = np.tile(np.arange(FIRST_ROW, FIRST_ROW + k_in, dtype=np.int64), (B, 1))
    col = np.full(COL_ROWS, 500.0)
    col[:k_in:3] = 510.0                      # two values only: many finals tie
    col[k_in - 10:k_in] = 1e9                 # far away: the exponent saturates
    scores = np.full((B, k_in), 0.5, dtype=np.float32)
    scores[3] = -np.sort(-np.round(np.random.default_rng(5).uniform(-1, 1, k_in) * 4) / 4).astype(np.float32)
    params = np.zeros(B, dtype=nat.DECAY_QUERY_DTYPE)
    params[0] = (500.0, 0.0, math.log(0.5) / 100.0, 0, 0)
    params[1] = (500.0, 0.0, math.log(0.5) / 10.0, 1, 0)
    params[2] = (-1e6, 0.0, 0.5 / 10.0, 2, 0)         # linear, everything beyond the cut-off: all factors 0.0
    params[3] = (500.0, 20.0, math.log(0.5) / 100.0, 0, 0)  # everything near lies inside offset: factor 1.0
    params[4] = (500.0, 0.0, -1.0, 9, 0)              # unknown function
    n = np.array([k_in, k_in, k_in, k_in, k_in + 50], dtype=np.int32)
    nn = np.minimum(n, k_in)
    for norm in (-1, 0, 3):
        want = run_host(ids, scores, nn, col, FIRST_ROW, params, norm, k_in)
        got = run_dev(ids, scores, n, col, "f64", FIRST_ROW, params, norm, k_in)
        check(got, want)
        assert np.array_equal(got[0][2], np.arange(k_in)) and not got[2][2].any()      # all zero: the order is kept
        assert np.array_equal(got[0][4], np.arange(k_in)) and not got[2][4].any()
        sat = np.isin(got[1][0], ids[0, k_in - 10:])
        assert sat.sum() == 10 and not got[2][0][sat].any()


def test_empty_column_and_empty_batch(gpu):
    rng = np.random.default_rng(1)
    ids, scores, n = make_lists(rng, 3, 40, False, 0)
    params = make_params(rng, 3, (0, 1, 2))
    got = run_dev(ids, scores, n, None, "f64", 0, params, 0, 40)      # no column: d_col NULL, every factor 0
    check(got, run_host(ids, scores, n, None, 0, params, 0, 40))
    assert not got[2].any()
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    nat.decay_rerank_dev(0, 0, False, 0, 0, 40, 0, nat.HR_COL_F64, 0, 0, 0, 0, 40, 0, 0, 0, 0)      # B == 0: HR_OK, nothing read
    torch.cuda.synchronize()
    assert not z.any()


def test_refusals_leave_the_outputs_alone(gpu):
    rng = np.random.default_rng(2)
    B, k = 2, 8
    ids, scores, n = make_lists(rng, B, k, False, 0)
    col = make_column(rng, "f64")
    t = {"ids": torch.from_numpy(ids).cuda(), "sc": torch.from_numpy(scores).cuda(), "n": torch.from_numpy(n).cuda(),
         "col": torch.from_numpy(col).cuda(),
         "p": torch.from_numpy(make_params(rng, B, (0,)).view(np.uint8).reshape(B, -1).copy()).cuda()}
    big = 3 * nat.HR_MAX_TOPK + 1
    out = {"pos": torch.full((B, big), SENT, dtype=torch.int32, device="cuda"),
           "ids": torch.full((B, big), SENT, dtype=torch.int64, device="cuda"),
           "sc": torch.full((B, big), float(SENT), dtype=torch.float64, device="cuda"),
           "n": torch.full((B,), SENT, dtype=torch.int32, device="cuda")}

    def call(**kw):
        a = dict(d_ids=t["ids"].data_ptr(), d_scores=t["sc"].data_ptr(), score_is_f64=False, d_n=t["n"].data_ptr(), B=B, k_in=k,
                 d_col=t["col"].data_ptr(), col_kind=nat.HR_COL_F64, col_rows=COL_ROWS, first_row=FIRST_ROW,
                 d_params=t["p"].data_ptr(), norm=0, k_out=k, d_out_pos=out["pos"].data_ptr(), d_out_ids=out["ids"].data_ptr(),
                 d_out_scores=out["sc"].data_ptr(), d_out_n=out["n"].data_ptr())
        a.update(kw)
        nat.decay_rerank_dev(**a)

    bad = [dict(norm=-2), dict(norm=5), dict(col_kind=1), dict(col_kind=3), dict(col_kind=4), dict(col_kind=6),
           dict(d_ids=0), dict(d_scores=0), dict(d_params=0), dict(d_out_pos=0), dict(d_out_ids=0), dict(d_out_scores=0),
           dict(d_out_n=0), dict(d_col=0), dict(k_out=0), dict(k_out=k + 1), dict(k_in=0), dict(B=-1), dict(col_rows=-1),
           dict(first_row=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(nat.HbmRagError) as e:      # HR_ELIMIT
        call(k_in=big, k_out=big)
    assert e.value.status == 5
    torch.cuda.synchronize()
    for o in out.values():
        assert bool((o == SENT).all())
    call()                                          # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert int(out["n"][0]) == int(n[0]) and int(out["n"][1]) == int(n[1])


def test_filter_entry_points_still_refuse_the_f64_kind(gpu):
    """HR_COL_F64 is valid only in hr_decay_rerank_dev."""
    col = torch.zeros(64, dtype=torch.float64, device="cuda")
    mask = torch.full((8,), 0x55, dtype=torch.uint8, device="cuda")
    und = torch.full((8,), 0x55, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    leaf = nat.FilterLeaf()
    leaf.term.kind, leaf.term.op, leaf.term.col = nat.HR_COL_F64, nat.FILTER_OPS["=="], col.data_ptr()
    with pytest.raises(ValueError, match="bad filter term 0"):
        nat.filter_eval_expr_dev([leaf], [0], 64, 0, mask.data_ptr(), und.data_ptr(), counts.data_ptr())
    with pytest.raises(ValueError, match="bad filter term 0"):
        nat.filter_eval_dev([leaf.term], 64, 0, mask.data_ptr(), und.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    assert bool((mask == 0x55).all()) and bool((und == 0x55).all()) and bool((counts == SENT).all())
