"""hr_boost_rerank_dev against the host restatement (advanced_rag/boost.py): positions, ids, counts and matched bits equal,
final scores bit for bit, padding as the header states.  Refused calls launch nothing: sentinel-filled outputs stay as
they were."""
import numpy as np
import pytest

from advanced_rag import _native as nat
from advanced_rag import boost as BO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = -7
FIRST_ROW = 1000
MASK_ROWS = 899          # not a multiple of 8: the last byte's unused bits are set and must not match
KEY_ROWS = 700           # shorter than the masks: rows beyond it are keyed by their id
WEIGHTS = (3.0, 0.5, -2.0, 1.25, -0.75, 7.0, 1e-3, 0.0)
MODES = [(f, b, a) for f in (0, 1) for b in (0, 1) for a in (0, 1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def packed(keep):
    """bool [MASK_ROWS] -> the packed row mask, the unused bits of the last byte set to 1."""
    full = np.ones((MASK_ROWS + 7) // 8 * 8, dtype=bool)
    full[:MASK_ROWS] = keep
    return np.packbits(full, bitorder="little")


class Func:
    """One operand struct and its host view: keep = bool [MASK_ROWS] or None (NULL mask), keys = int64 [KEY_ROWS] or None."""

    def __init__(self, keep, weight, seed=None, keys=None, active=True):
        self.keep, self.weight, self.seed, self.keys, self.active = keep, float(weight), seed, keys, active

    def matches(self, i):
        r = i - FIRST_ROW
        return self.active and (self.keep is None or (0 <= r < MASK_ROWS and bool(self.keep[r])))

    def spec(self, lid):
        if self.seed is None:
            return self.weight
        keys = [int(self.keys[i - FIRST_ROW]) if self.keys is not None and 0 <= i - FIRST_ROW < len(self.keys) else i for i in lid]
        return (self.weight, self.seed, keys)


def make_funcs(rng, B, n_funcs):
    """[B][n_funcs] functions, different per query: random masks, a NULL mask, draws with and without a key column,
    negative and zero weights, and (from the second slot on) inactive padding slots that carry a match-all mask."""
    keys = rng.integers(-2 ** 62, 2 ** 62, KEY_ROWS).astype(np.int64)
    out = []
    for q in range(B):
        row = []
        for j in range(n_funcs):
            keep = None if (q + j) % 4 == 3 else rng.random(MASK_ROWS) < (0.1, 0.5, 0.9)[(q + j) % 3]
            draw = (q + 2 * j) % 3
            row.append(Func(keep, WEIGHTS[(3 * q + j) % len(WEIGHTS)],
                            seed=None if draw == 0 else int(rng.integers(0, 2 ** 64, dtype=np.uint64)),
                            keys=keys if draw == 2 else None, active=not (j >= 1 and (q + j) % 5 == 4)))
        out.append(row)
    return out


def make_lists(rng, B, k_in, f64, norm):
    """ids [B, k_in] mostly inside the masks, some below and above them; scores as a list with that norm code holds them.
    Query 0 is empty, query 1 short (when B >= 3); the last is full."""
    ids = np.stack([rng.choice(np.arange(FIRST_ROW - 40, FIRST_ROW + MASK_ROWS + 40), k_in, replace=False) for _ in range(B)])
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


def device_funcs(funcs):
    """-> (uint8 CUDA tensor [B, n_funcs * 56] of hr_boost_func records, the tensors they point into)."""
    B, F = len(funcs), len(funcs[0])
    rec = np.zeros((B, F), dtype=nat.BOOST_FUNC_DTYPE)
    keep_alive = {}
    for q in range(B):
        for j, f in enumerate(funcs[q]):
            m = k = None
            if f.keep is not None:
                m = keep_alive.setdefault(id(f.keep), torch.from_numpy(packed(f.keep)).cuda())
            if f.keys is not None:
                k = keep_alive.setdefault(id(f.keys), torch.from_numpy(f.keys).cuda())
            rec[q, j] = (m.data_ptr() if m is not None else 0, k.data_ptr() if k is not None else 0, MASK_ROWS,
                         len(f.keys) if f.keys is not None else 0, f.weight, f.seed or 0,
                         (nat.HR_BOOST_ACTIVE if f.active else 0) | (nat.HR_BOOST_RANDOM if f.seed is not None else 0), 0)
    return torch.from_numpy(rec.view(np.uint8).reshape(B, -1).copy()).cuda(), keep_alive


def run_dev(ids, scores, n, funcs, fmode, bmode, norm, asc, k_out, use_n=True):
    B, k_in = ids.shape
    ids = ids.copy()
    if not use_n:                                   # the prefix ends at the first id < 0 instead
        for q in range(B):
            ids[q, n[q]:] = -1
    t_ids = torch.from_numpy(ids).cuda()
    t_sc = torch.from_numpy(np.ascontiguousarray(scores)).cuda()
    t_n = torch.from_numpy(np.ascontiguousarray(n)).cuda() if use_n else None
    t_f, keep_alive = device_funcs(funcs)
    op = torch.full((B, k_out), SENT, dtype=torch.int32, device="cuda")
    oi = torch.full((B, k_out), SENT, dtype=torch.int64, device="cuda")
    os_ = torch.full((B, k_out), float(SENT), dtype=torch.float64, device="cuda")
    om = torch.full((B, k_out), SENT, dtype=torch.int32, device="cuda")
    on = torch.full((B,), SENT, dtype=torch.int32, device="cuda")
    nat.boost_rerank_dev(t_ids.data_ptr(), t_sc.data_ptr(), scores.dtype == np.float64, t_n.data_ptr() if use_n else 0, B, k_in,
                         t_f.data_ptr(), len(funcs[0]), FIRST_ROW, fmode, bmode, norm, bool(asc), k_out, op.data_ptr(),
                         oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep_alive
    return op.cpu().numpy(), oi.cpu().numpy(), os_.cpu().numpy(), on.cpu().numpy(), om.cpu().numpy()


def run_host(ids, scores, n, funcs, fmode, bmode, norm, asc, k_out):
    B = ids.shape[0]
    wp = np.full((B, k_out), -1, dtype=np.int32)
    wi = np.full((B, k_out), -1, dtype=np.int64)
    ws = np.zeros((B, k_out), dtype=np.float64)
    wm = np.zeros((B, k_out), dtype=np.int32)
    wn = np.zeros(B, dtype=np.int32)
    for q in range(B):
        lid = ids[q, :n[q]].tolist()
        pos, oid, fin, hit = BO.boost_rerank(lid, [float(x) for x in scores[q, :n[q]]],
                                             [[f.matches(i) for i in lid] for f in funcs[q]], [f.spec(lid) for f in funcs[q]],
                                             fmode, bmode, norm, bool(asc), k_out)
        wp[q, :len(pos)], wi[q, :len(pos)], ws[q, :len(pos)], wm[q, :len(pos)], wn[q] = pos, oid, fin, hit, len(pos)
    return wp, wi, ws, wn, wm


def check(got, want):
    for g, w in zip((got[3], got[0], got[1], got[4]), (want[3], want[0], want[1], want[4])):
        assert np.array_equal(g, w)
    assert np.array_equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("n_funcs", [1, 3, 8])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("k_in", [1, 40, 257, 768])
def test_kernel_equals_the_restatement(gpu, k_in, f64, n_funcs):
    """B = 3 (empty, short, full), different functions per query in one launch, every norm code, both cuts, both
    directions and all four mode pairs, d_n given and NULL."""
    rng = np.random.default_rng(k_in * 100 + f64 * 10 + n_funcs)
    funcs = make_funcs(rng, 3, n_funcs)
    turn = 0
    for norm in (-1, 0, 1, 2, 3, 4):
        ids, scores, n = make_lists(rng, 3, k_in, f64, norm)
        for k_out in sorted({1, k_in}):
            for fmode, bmode, asc in (MODES[turn % 8], MODES[(turn + 3) % 8]):
                want = run_host(ids, scores, n, funcs, fmode, bmode, norm, asc, k_out)
                check(run_dev(ids, scores, n, funcs, fmode, bmode, norm, asc, k_out, use_n=(norm + k_out + turn) % 2 == 0), want)
            turn += 1
    if k_in >= 40 and n_funcs > 1:      # the data holds what the case is about
        assert any(not f.active for row in funcs for f in row) and any(f.keep is None for row in funcs for f in row)


def test_mask_edges_and_key_ranges(gpu):
    """Bits 0 and 7 of a byte, the last row of a mask of 899 rows and the set bits behind it, ids below, inside and above
    the mask, a draw keyed by a column that ends before the mask does."""
    keep = np.zeros(MASK_ROWS, dtype=bool)
    keep[[40, 47, 0, MASK_ROWS - 1]] = True
    inside = [40, 47, 41, 46, 39, 48, 0, 1, 7, 8, MASK_ROWS - 1, MASK_ROWS - 2, KEY_ROWS - 1, KEY_ROWS, KEY_ROWS + 1]
    beyond = [MASK_ROWS, MASK_ROWS + 1, MASK_ROWS + 4, -1, -8, -1000, 5000, 2 ** 40]      # -1000: id 0
    ids = np.array([[FIRST_ROW + r for r in inside + beyond]], dtype=np.int64)
    k_in = ids.shape[1]
    scores = (1.0 - np.arange(k_in, dtype=np.float32) / 64)[None, :]
    n = np.array([k_in], dtype=np.int32)
    keys = np.arange(KEY_ROWS, dtype=np.int64) * -3
    every = np.ones(MASK_ROWS, dtype=bool)
    funcs = [[Func(keep, 4.0), Func(every, 2.0, seed=126, keys=keys), Func(None, 0.5, seed=2 ** 64 - 1)]]
    for fmode, bmode, asc in MODES:
        want = run_host(ids, scores, n, funcs, fmode, bmode, -1, asc, k_in)
        got = run_dev(ids, scores, n, funcs, fmode, bmode, -1, asc, k_in)
        check(got, want)
    hit = dict(zip(got[1][0].tolist(), got[4][0].tolist()))
    assert [r for r in inside + beyond if hit[FIRST_ROW + r] & 1] == [40, 47, 0, MASK_ROWS - 1]
    assert all((hit[FIRST_ROW + r] & 2) == 2 for r in inside) and not any(hit[FIRST_ROW + r] & 2 for r in beyond)
    assert all(hit[FIRST_ROW + r] & 4 for r in inside + beyond)      # the NULL mask matches every entry


def test_zero_weight_ties_nans_and_clamped_counts(gpu):
    """Weight 0 on a match-all function: every final is +-0.0, one tie, the input order holds in both directions.  A NaN
    final (inf x 0, or a NaN score) ranks last in either direction, NaNs in input order.  d_n beyond k_in is clamped."""
    k_in, B = 300, 3
    rng = np.random.default_rng(9)
    ids = np.tile(np.arange(FIRST_ROW, FIRST_ROW + k_in, dtype=np.int64), (B, 1))
    scores = -np.sort(-np.round(rng.uniform(-1, 1, (B, k_in)) * 4) / 4, axis=1).astype(np.float32)
    scores[1, [3, 77, 299]] = np.inf
    scores[1, [5, 256]] = np.nan
    scores[2, ::2] = scores[2, 0]                     # many equal finals
    half = np.arange(MASK_ROWS) % 3 == 0
    funcs = [[Func(None, 0.0)], [Func(None, 0.0)], [Func(half, -1.5)]]
    n = np.array([k_in, k_in, k_in + 50], dtype=np.int32)
    nn = np.minimum(n, k_in)
    for asc in (0, 1):
        want = run_host(ids, scores, nn, funcs, 0, 0, -1, asc, k_in)
        got = run_dev(ids, scores, n, funcs, 0, 0, -1, asc, k_in)
        check(got, want)
        assert np.array_equal(got[0][0], np.arange(k_in)) and not got[2][0].any()
        assert got[0][1][-5:].tolist() == [3, 5, 77, 256, 299] and np.isnan(got[2][1][-5:]).all()
        assert not np.isnan(got[2][1][:-5]).any()


def test_empty_batch_and_version(gpu):
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    nat.boost_rerank_dev(0, 0, False, 0, 0, 40, 0, 1, 0, 0, 0, -1, False, 40, 0, 0, 0, 0, 0)      # B == 0: HR_OK, nothing read
    torch.cuda.synchronize()
    assert not z.any()
    assert nat.load_library().hr_version() >= 12000


def test_refusals_leave_the_outputs_alone(gpu):
    rng = np.random.default_rng(2)
    B, k = 2, 8
    ids, scores, n = make_lists(rng, B, k, False, 0)
    funcs = make_funcs(rng, B, 3)
    t_f, keep_alive = device_funcs(funcs)
    t = {"ids": torch.from_numpy(ids).cuda(), "sc": torch.from_numpy(scores).cuda(), "n": torch.from_numpy(n).cuda()}
    big = 3 * nat.HR_MAX_TOPK + 1
    out = {"pos": torch.full((B, big), SENT, dtype=torch.int32, device="cuda"),
           "ids": torch.full((B, big), SENT, dtype=torch.int64, device="cuda"),
           "sc": torch.full((B, big), float(SENT), dtype=torch.float64, device="cuda"),
           "hit": torch.full((B, big), SENT, dtype=torch.int32, device="cuda"),
           "n": torch.full((B,), SENT, dtype=torch.int32, device="cuda")}

    def call(**kw):
        a = dict(d_ids=t["ids"].data_ptr(), d_scores=t["sc"].data_ptr(), score_is_f64=False, d_n=t["n"].data_ptr(), B=B, k_in=k,
                 d_funcs=t_f.data_ptr(), n_funcs=3, first_row=FIRST_ROW, function_mode=0, boost_mode=0, norm=0, ascending=False,
                 k_out=k, d_out_pos=out["pos"].data_ptr(), d_out_ids=out["ids"].data_ptr(), d_out_scores=out["sc"].data_ptr(),
                 d_out_matched=out["hit"].data_ptr(), d_out_n=out["n"].data_ptr())
        a.update(kw)
        nat.boost_rerank_dev(**a)

    bad = [dict(norm=-2), dict(norm=5), dict(function_mode=2), dict(function_mode=-1), dict(boost_mode=2), dict(boost_mode=-1),
           dict(d_ids=0), dict(d_scores=0), dict(d_funcs=0), dict(d_out_pos=0), dict(d_out_ids=0), dict(d_out_scores=0),
           dict(d_out_matched=0), dict(d_out_n=0), dict(k_out=0), dict(k_out=k + 1), dict(k_in=0), dict(B=-1), dict(n_funcs=0),
           dict(first_row=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(k_in=big, k_out=big), dict(n_funcs=nat.HR_MAX_BOOST_FUNCS + 1)):
        with pytest.raises(nat.HbmRagError) as e:      # HR_ELIMIT
            call(**kw)
        assert e.value.status == 5
    torch.cuda.synchronize()
    for o in out.values():
        assert bool((o == SENT).all())
    call()                                          # the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert int(out["n"][0]) == int(n[0]) and int(out["n"][1]) == int(n[1])
    del keep_alive
