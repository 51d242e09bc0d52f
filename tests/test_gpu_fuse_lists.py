"""Multi-list fusion on the device: hr_fuse_lists_dev against the two Python restatements of its contract
(retrieval.rrf_rank_lists, retrieval.score_fuse_lists) and, for the weighted mode, against the numpy arithmetic of
tests/score_fusion_ref.py generalised to L lists here.  Everything is compared bit for bit: ids, the float.hex() of every
fp64 score, the list masks, n_out and the padding.  For L <= 3 the outputs also equal hr_fuse_rrf_dev / hr_fuse_scores_dev.
Refused calls launch nothing: sentinel-filled outputs stay as they were."""
import ctypes
import json
import os

import numpy as np
import pytest

import score_fusion_ref as R
from advanced_rag import _native as nat
from advanced_rag.retrieval import rrf_rank_lists, score_fuse_lists

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RRF, WEIGHTED = 0, 1
ORDER_W1 = [1e16, 1.0, -1e16, 1.0]
ORDER_W2 = [1e16, -1e16, 1.0, 1.0]


def prefix_len(row):
    neg = np.nonzero(np.asarray(row) < 0)[0]
    return int(neg[0]) if len(neg) else len(row)


# ------------------------------------------------------------------------------------------------ the references
def ref_query(ids, scs, mode, norms, weights, rrf_k=60):
    """One query.  ids [L, k] (-1 ends a list), scs [L, k] fp32 or None -> [(id, fp64 score, mask)] in fused order.
    RRF: the restatement itself.  Weighted: score_fusion_ref's arithmetic (numpy float64, one rounded operation each)
    over L lists — the same visiting order, accumulation order and stable sort."""
    lists = [row[:prefix_len(row)] for row in ids]
    if mode == RRF:
        fused = rrf_rank_lists([l.tolist() for l in lists], [float(w) for w in weights], rrf_k)
        return [(i, s, sum(1 << l for l in ls)) for i, s, ls in fused]
    slot, order, score, mask = {}, [], [], []
    for li, (l, w) in enumerate(zip(lists, weights)):
        nv = R.normalise(scs[li][:len(l)], norms[li])
        for i, d in enumerate(l.tolist()):
            if d not in slot:
                slot[d] = len(order)
                order.append(d)
                score.append(np.float64(0.0))
                mask.append(0)
            score[slot[d]] = score[slot[d]] + nv[i] * np.float64(w)
            mask[slot[d]] |= 1 << li
    idx = sorted(range(len(order)), key=lambda j: score[j], reverse=True)
    return [(order[j], float(score[j]), mask[j]) for j in idx]


def ref_batch(ids, scs, mode, norms, weights, top_k, w_query=None, rrf_k=60):
    B = ids.shape[0]
    oi = np.full((B, top_k), -1, dtype=np.int64)
    os_ = np.zeros((B, top_k), dtype=np.float64)
    om = np.zeros((B, top_k), dtype=np.int32)
    on = np.zeros(B, dtype=np.int32)
    for q in range(B):
        w = w_query[q] if w_query is not None else weights
        fused = ref_query(ids[q], None if scs is None else scs[q], mode, norms, w, rrf_k)[:top_k]
        n = len(fused)
        oi[q, :n] = [f[0] for f in fused]
        os_[q, :n] = [f[1] for f in fused]
        om[q, :n] = [f[2] for f in fused]
        on[q] = n
    return oi, os_, om, on


# ------------------------------------------------------------------------------------------------ the device
def outs(B, top_k):
    return (torch.full((B, top_k), -7, dtype=torch.int64, device="cuda"), torch.full((B, top_k), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((B, top_k), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda"))


def run_dev(ids, scs, mode, norms, weights, top_k, w_query=None, rrf_k=60, raw=False):
    """ids [B, L, k] int64, scs [B, L, k] fp32 or None -> (ids, scores, masks, n) of hr_fuse_lists_dev."""
    B, L, k = ids.shape
    t_ids = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    t_sc = torch.from_numpy(np.ascontiguousarray(scs, dtype=np.float32)).cuda() if scs is not None else None
    wq = torch.from_numpy(np.ascontiguousarray(w_query, dtype=np.float64)).cuda() if w_query is not None else None
    o = outs(B, top_k)
    nat.fuse_lists_dev(t_ids.data_ptr(), t_sc.data_ptr() if t_sc is not None else 0, L, k, B, mode, rrf_k,
                       None if norms is None else list(norms), None if weights is None else list(weights),
                       wq.data_ptr() if wq is not None else 0, top_k, *[t.data_ptr() for t in o],
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if raw:
        return b"".join(t.cpu().numpy().tobytes() for t in o)
    return tuple(t.cpu().numpy() for t in o)


def check(got, want, what=""):
    gi, gs, gm, gn = got
    wi, ws, wm, wn = want
    assert np.array_equal(gn, wn), what
    assert np.array_equal(gi, wi), what
    assert [float(x).hex() for x in gs.ravel()] == [float(x).hex() for x in ws.ravel()], what
    assert np.array_equal(gm, wm), what


# ------------------------------------------------------------------------------------------------ cases
def make_scores(rng, code, B, k):
    """[B, k] fp32 scores as a list with that code holds them, quantised so that equal scores occur."""
    if code in (R.ATAN_DIST, R.MINMAX_DIST):
        s = np.sort(np.round(rng.uniform(0, 6, (B, k)) * 16) / 16, axis=1)
    elif code == R.COSINE:
        s = -np.sort(-np.round(rng.uniform(-1, 1, (B, k)) * 64) / 64, axis=1)
    else:
        s = -np.sort(-np.round(rng.uniform(-20, 60, (B, k)) * 8) / 8, axis=1)
    return s.astype(np.float32)


def make_case(seed, B, L, k):
    """Random lists over a shared pool (so ids recur across lists, and some appear once), with the edge rows of a batch."""
    rng = np.random.default_rng(seed)
    norms = [int(c) for c in rng.integers(0, 5, L)]
    pool = np.arange(2 * k + 2, dtype=np.int64) * 3 + 1
    ids = np.stack([np.stack([rng.permutation(pool)[:k] for _ in range(L)]) for _ in range(B)])
    scs = np.stack([make_scores(rng, norms[l], B, k) for l in range(L)], axis=1)
    if B >= 5:
        if L > 1:
            ids[1, 0, :] = -1                    # query 1: an empty first list
        ids[2, L - 1, 1:] = -1                   # query 2: a list of one entry
        scs[3, 0, :] = scs[3, 0, 0]              # query 3: a list of equal scores
        scs[4, :, :] = np.float32(0.5)           # query 4: every score equal
        if k >= 4:
            ids[0, 0, k - k // 4:] = -1          # query 0: a short list
    weights = [float(w) for w in np.round(rng.uniform(-0.5, 2.0, L) * 64) / 64]
    return ids, scs, norms, weights


@pytest.mark.parametrize("mode", [RRF, WEIGHTED])
@pytest.mark.parametrize("k", [1, 7, 64, 256])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 16])
def test_fuse_lists_equals_the_restatement(gpu, L, k, mode):
    B = 5
    seed = L * 1000 + k * 2 + mode
    ids, scs, norms, weights = make_case(seed, B, L, k)
    wq = np.round(np.random.default_rng(seed + 1).uniform(-1, 2, (B, L)) * 32) / 32     # per-query weights that differ
    distinct = max(len({int(i) for row in ids[q] for i in row[:prefix_len(row)]}) for q in range(B))
    sc = scs if mode == WEIGHTED else None
    for top_k in sorted({1, 20, 768, min(768, distinct + 3)}):
        want = ref_batch(ids, scs, mode, norms, weights, top_k)
        check(run_dev(ids, sc, mode, norms if mode == WEIGHTED else None, weights, top_k), want, f"top_k={top_k}")
    # per-query weights in one launch of 5 = five launches of 1 with those weights as host weights
    top_k = min(768, distinct + 3)
    want = ref_batch(ids, scs, mode, norms, None, top_k, wq)
    got = run_dev(ids, sc, mode, norms, weights, top_k, wq)
    check(got, want, "w_query")
    for q in range(B):
        one = run_dev(ids[q:q + 1], None if sc is None else sc[q:q + 1], mode, norms, list(wq[q]), top_k)
        check(one, tuple(a[q:q + 1] for a in got), f"launch of 1, query {q}")


def test_weighted_restatement_agrees_with_the_numpy_reference(gpu):
    """The two references of the weighted mode (Python floats, numpy float64) give the same bits, so the device is held to
    retrieval.score_fuse_lists as well."""
    ids, scs, norms, weights = make_case(77, 5, 6, 40)
    for q in range(5):
        lists = [(row[:prefix_len(row)].tolist(), scs[q, l][:prefix_len(row)]) for l, row in enumerate(ids[q])]
        a = [(i, float(s).hex(), sum(1 << l for l in ls)) for i, s, ls in score_fuse_lists(lists, weights, norms)]
        b = [(i, float(s).hex(), m) for i, s, m in ref_query(ids[q], scs[q], WEIGHTED, norms, weights)]
        assert a == b
    check(run_dev(ids, scs, WEIGHTED, norms, weights, 100), ref_batch(ids, scs, WEIGHTED, norms, weights, 100))


# ------------------------------------------------------------------------------------------------ L <= 3: the old kernels
def _three_list(ids, scs, mode, norms, weights, top_k):
    B, L, k = ids.shape
    t_i = [torch.from_numpy(np.ascontiguousarray(ids[:, l])).cuda() for l in range(L)]
    t_s = [torch.from_numpy(np.ascontiguousarray(scs[:, l])).cuda() for l in range(L)]
    o = outs(B, top_k)
    st = torch.cuda.current_stream().cuda_stream
    w = list(weights) + [0.0] * (3 - L)
    if mode == RRF:
        a = []
        for l in range(3):
            a += [t_i[l].data_ptr(), k] if l < L else [0, 0]
        nat.fuse_rrf_dev(*a, B, w[0], w[1], w[2], 60, top_k, *[t.data_ptr() for t in o], st)
    else:
        a = []
        for l in range(3):
            a += [t_i[l].data_ptr(), t_s[l].data_ptr(), k, norms[l]] if l < L else [0, 0, 0, 0]
        nat.fuse_scores_dev(*a, B, w[0], w[1], w[2], 0, top_k, *[t.data_ptr() for t in o], st)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in o)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_up_to_three_lists_equal_the_three_list_kernels(gpu, L):
    for code in range(5):                      # random lists, every norm code
        ids, scs, _, weights = make_case(500 + L * 10 + code, 5, L, 40)
        rng = np.random.default_rng(code)
        norms = [code] + [int(c) for c in rng.integers(0, 5, L - 1)]
        scs = np.stack([make_scores(rng, norms[l], 5, 40) for l in range(L)], axis=1)
        for top_k in (20, 130):
            check(run_dev(ids, scs, WEIGHTED, norms, weights, top_k), _three_list(ids, scs, WEIGHTED, norms, weights, top_k))
            check(run_dev(ids, None, RRF, None, weights, top_k), _three_list(ids, scs, RRF, norms, weights, top_k))


def test_g1_cases_equal_the_golden_scores_and_the_rrf_kernel(gpu):
    with open(os.path.join(os.path.dirname(__file__), "golden", "g1_fuse.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 20
    for c in cases:
        names = {}
        lists = [[names.setdefault(x, len(names)) for x in c[m]] for m in ("semantic", "sparse", "domain")]
        back = {v: k for k, v in names.items()}
        k = max(1, max(len(l) for l in lists))
        ids = np.full((1, 3, k), -1, dtype=np.int64)
        for l, lst in enumerate(lists):
            ids[0, l, :len(lst)] = lst
        w = [c["dense_weight"], c["sparse_weight"], 0.2]
        top_k = 3 * k
        gi, gs, gm, gn = run_dev(ids, None, RRF, None, w, top_k)
        n = int(gn[0])
        assert [back[int(i)] for i in gi[0, :n]] == c["ids"], c["label"]
        assert [float(s).hex() for s in gs[0, :n]] == c["scores"], c["label"]
        assert [sorted(m for b, m in enumerate(("semantic", "sparse", "domain")) if int(x) >> b & 1) for x in gm[0, :n]] == c["methods"]
        check((gi, gs, gm, gn), _three_list(ids, np.zeros(ids.shape, np.float32), RRF, None, w, top_k), c["label"])


# ------------------------------------------------------------------------------------------------ adversarial
def test_every_id_in_all_sixteen_lists_accumulates_in_list_order(gpu):
    """[1e16, 1, -1e16, 1] and [1e16, -1e16, 1, 1] repeated over 16 lists: the sum depends on the order of the additions,
    so a kernel that adds in any other order than list order gives other bits."""
    k = 64
    ids = np.stack([np.roll(np.arange(k, dtype=np.int64), l) for l in range(16)])[None]
    scs = np.full(ids.shape, 0.25, dtype=np.float32)
    for w4 in (ORDER_W1, ORDER_W2):
        w = w4 * 4
        for mode, norms in ((RRF, None), (WEIGHTED, [R.COSINE] * 16)):
            want = ref_batch(ids, scs, mode, norms, w, k + 2)
            assert want[3][0] == k and (want[2][0, :k] == 0xFFFF).all()
            check(run_dev(ids, scs if mode else None, mode, norms, w, k + 2), want)
    # the two single-entry cases of the host test, on the device
    one = np.zeros((1, 4, 1), dtype=np.int64)
    for w4, hexv in ((ORDER_W1, (0.047643442622950824).hex()), (ORDER_W2, (0.03278688524590164).hex())):
        got = run_dev(one, None, RRF, None, w4, 1)
        assert float(got[1][0, 0]).hex() == hexv and got[2][0, 0] == 15 and got[0][0, 0] == 0


def test_the_cap_sixteen_disjoint_lists_of_256_tie_in_list_order(gpu):
    ids = (np.arange(16, dtype=np.int64)[:, None] * 256 + np.arange(256, dtype=np.int64)[None, :])[None]
    got = run_dev(ids, None, RRF, None, [1.0] * 16, 768)
    want = ref_batch(ids, None, RRF, None, [1.0] * 16, 768)
    assert got[0][0, :18].tolist() == [l * 256 for l in range(16)] + [1, 257]
    assert len(set(want[1][0].tolist())) == 768 // 16
    check(got, want)
    scs = np.broadcast_to(np.linspace(1, -1, 256, dtype=np.float32), ids.shape)
    check(run_dev(ids, scs, WEIGHTED, [R.COSINE] * 16, [1.0] * 16, 768), ref_batch(ids, scs, WEIGHTED, [R.COSINE] * 16, [1.0] * 16, 768))


def test_list_edges(gpu):
    rng = np.random.default_rng(5)
    L, k = 6, 40
    ids = np.stack([rng.permutation(60)[:k] for _ in range(L)]).astype(np.int64)[None]
    ids[0, L - 1, :5] = [1000, 1001, 1002, 1003, 1004]      # ids that first appear in the last list, at its head
    ids[0, 2, :] = -1                                        # an empty list in the middle
    ids[0, 3, 7] = -1                                        # a -1 mid-list: what follows it is ignored
    ids[0, 3, 8:12] = [2000, 2001, 2002, 2003]
    scs = np.stack([make_scores(rng, R.ATAN, 1, k)[0] for _ in range(L)])[None]
    w = [0.5, 1.0, 3.0, 0.25, -0.75, 2.0]                    # a negative weight
    for mode, norms in ((RRF, None), (WEIGHTED, [3, 1, 0, 4, 3, 2])):
        want = ref_batch(ids, scs, mode, norms, w, 120)
        assert 1000 in want[0][0] and not (want[2][0] & 4).any()
        assert not set(want[0][0].tolist()) & {2000, 2001, 2002, 2003}     # the ignored ids appear nowhere else
        check(run_dev(ids, scs if mode else None, mode, norms, w, 120), want)
        check(run_dev(ids, scs if mode else None, mode, norms, None, 120, np.array([w])), want, "d_w_query only")


def test_wide_ids_and_table_collisions(gpu):
    k = 48
    base = np.arange(k, dtype=np.int64)
    lists = [base << 20,                                     # multiples of 2^20 (and the id 0)
             base << 40,                                     # multiples of 2^40
             (base << 32) | 5,                               # equal in their low 32 bits, above 2^32
             (base[::-1] << 32) | 5,
             base << 20,
             np.concatenate([(base[:k // 2] << 40), base[:k // 2] + (1 << 62)])]
    ids = np.stack(lists)[None]
    rng = np.random.default_rng(9)
    scs = rng.uniform(-1, 1, ids.shape).astype(np.float32)
    w = [1.0, 0.5, 0.25, 2.0, 1.5, 0.125]
    for mode, norms in ((RRF, None), (WEIGHTED, [0] * 6)):
        check(run_dev(ids, scs if mode else None, mode, norms, w, 300), ref_batch(ids, scs, mode, norms, w, 300))


def test_min_max_lists_of_equal_scores_and_of_one_entry(gpu):
    ids = np.full((1, 4, 8), -1, dtype=np.int64)
    ids[0, 0] = np.arange(8)
    ids[0, 1, 0] = 3                                         # one entry
    ids[0, 2] = np.arange(8)[::-1]
    ids[0, 3, :2] = [100, 0]
    scs = np.zeros(ids.shape, dtype=np.float32)
    scs[0, 0] = 2.5                                          # equal scores
    scs[0, 1, 0] = -4.0
    scs[0, 2] = np.linspace(9, 2, 8)
    scs[0, 3, :2] = [7.0, 7.0]
    for norms in ([3, 3, 3, 3], [4, 4, 4, 4], [3, 4, 4, 3]):
        w = [1.0, 0.5, 0.25, -2.0]
        check(run_dev(ids, scs, WEIGHTED, norms, w, 12), ref_batch(ids, scs, WEIGHTED, norms, w, 12))


def test_two_runs_give_identical_bytes(gpu):
    ids, scs, norms, weights = make_case(4242, 5, 16, 256)
    for mode in (RRF, WEIGHTED):
        a = run_dev(ids, scs, mode, norms, weights, 768, raw=True)
        assert a == run_dev(ids, scs, mode, norms, weights, 768, raw=True)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_status_and_write_nothing(gpu):
    lib = nat.load_library()
    assert lib.hr_version() >= 11900
    B, L, k, top_k = 2, 3, 8, 8
    ids = torch.arange(B * L * k, dtype=torch.int64, device="cuda")
    sc = torch.rand(B * L * k, dtype=torch.float32, device="cuda")
    wq = torch.ones(B * L + 1, dtype=torch.float64, device="cuda")
    big_i = torch.zeros(17 * 257, dtype=torch.int64, device="cuda")
    o = outs(B, top_k)
    OI, OS, OM, ON = [t.data_ptr() for t in o]
    I, S, WQ = ids.data_ptr(), sc.data_ptr(), wq.data_ptr()
    norms = (ctypes.c_int32 * 16)(*([0] * 16))
    w = (ctypes.c_double * 16)(*([1.0] * 16))
    p = lambda v: ctypes.c_void_p(v) if v else None
    addr = lambda a: ctypes.addressof(a)

    def call(d_ids=I, d_sc=S, n_lists=L, k_in=k, b=B, mode=WEIGHTED, rrf_k=60, nm=addr(norms), wt=addr(w), d_wq=0, top=top_k,
             oi=OI, os_=OS, om=OM, on=ON):
        return lib.hr_fuse_lists_dev(p(d_ids), p(d_sc), n_lists, k_in, b, mode, rrf_k, p(nm), p(wt), p(d_wq), top, p(oi),
                                     p(os_), p(om), p(on), None)

    EINVAL, ELIMIT = 1, 5
    for kw in (dict(n_lists=0), dict(k_in=0), dict(top=0), dict(b=-1), dict(n_lists=-3), dict(mode=2), dict(mode=-1),
               dict(d_ids=0), dict(oi=0), dict(os_=0), dict(om=0), dict(on=0), dict(wt=0), dict(d_sc=0), dict(nm=0),
               dict(d_ids=I + 4), dict(oi=OI + 4), dict(os_=OS + 4), dict(d_wq=WQ + 4), dict(wt=addr(w) + 4),
               dict(d_sc=S + 2), dict(om=OM + 2), dict(on=ON + 1), dict(nm=addr(norms) + 2)):
        assert call(**kw) == EINVAL, kw
    for bad in (5, -1):
        norms[1] = bad
        assert call() == EINVAL
        assert call(mode=RRF) == 0                     # norms are not read for RRF
        torch.cuda.synchronize()
        for t in o:
            t.fill_(-7)
    norms[1] = 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        w[2] = bad
        assert call() == EINVAL and call(mode=RRF) == EINVAL and call(d_wq=WQ) == EINVAL
    w[2] = 1.0
    for kw in (dict(d_ids=big_i.data_ptr(), n_lists=17), dict(d_ids=big_i.data_ptr(), k_in=257), dict(top=769)):
        assert call(**kw) == ELIMIT, kw
    assert b"" != lib.hr_last_error(None)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in o)
    assert call(b=0) == 0                              # B == 0: HR_OK, nothing launched
    assert call(b=0, d_sc=0, nm=0, mode=RRF) == 0
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in o)
    # the same arguments without a fault are served; RRF needs neither scores nor norms, d_w_query stands in for weights
    assert call() == 0 and call(mode=RRF, d_sc=0, nm=0) == 0 and call(wt=0, d_wq=WQ) == 0
    torch.cuda.synchronize()
    assert int(o[3][0]) == k
    with pytest.raises(ValueError):
        nat.fuse_lists_dev(I, S, L, k, B, 2, 60, [0] * L, [1.0] * L, 0, top_k, OI, OS, OM, ON)
    with pytest.raises(nat.HbmRagError):
        nat.fuse_lists_dev(I, S, L, k, B, 0, 60, None, [1.0] * L, 0, 769, OI, OS, OM, ON)


def test_duplicate_ids_inside_a_list_stay_in_bounds(gpu):
    """Outside the contract: only that the call returns, n_out is in range and the ids written are ids of the input."""
    ids = np.zeros((2, 16, 256), dtype=np.int64)
    ids[1] = np.arange(256)[None, :] // 4
    scs = np.ones(ids.shape, dtype=np.float32)
    for mode in (RRF, WEIGHTED):
        gi, gs, gm, gn = run_dev(ids, scs, mode, [3] * 16, [1.0] * 16, 768)
        assert 1 <= gn[0] <= 768 and 1 <= gn[1] <= 768
        assert set(gi[1, :gn[1]].tolist()) <= set(range(64)) and (gi[1, gn[1]:] == -1).all()
