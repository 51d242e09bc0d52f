"""Weighted score fusion on the device: hr_fuse_scores_dev, hr_fuse_scores (host form) and hr_post_lists_dev with
fusion = 1 against the numpy restatement of tests/score_fusion_ref.py, bit for bit: ids, fp64 scores, method masks, counts
and padding.  Refused calls launch nothing: sentinel-filled outputs stay as they were."""
import numpy as np
import pytest

import score_fusion_ref as R
from advanced_rag import _native as nat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NORM_SETS = [(0, 1, 0), (1, 1, 1), (2, 1, 2), (3, 3, 3), (4, 3, 4), (0, 3, 2), (1, 4, 3), (3, 0, 1)]
WEIGHT_SETS = [(0.7, 0.3, 0.2), (0.0, 1.0, 0.5), (-0.25, 0.5, 1.5), (1.0, 1.0, 1.0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def prefix_len(row):
    """Valid entries of one list: those before the first id < 0."""
    neg = np.nonzero(np.asarray(row) < 0)[0]
    return int(neg[0]) if len(neg) else len(row)


def make_scores(rng, code, B, k):
    """[B, k] fp32 scores as a list with that code holds them: L2 distances ascending, everything else descending; COSINE
    in [-1, 1], IP of both signs and beyond where atan saturates; quantised so that equal scores occur."""
    if code in (R.ATAN_DIST, R.MINMAX_DIST):
        s = np.sort(np.round(rng.uniform(0, 6, (B, k)) * 16) / 16, axis=1)
    elif code == R.COSINE:
        s = -np.sort(-np.round(rng.uniform(-1, 1, (B, k)) * 64) / 64, axis=1)
    else:
        s = -np.sort(-np.round(rng.uniform(-20, 60, (B, k)) * 8) / 8, axis=1)
    return s.astype(np.float32)


def make_case(seed, B, k, n_lists, overlap, norms):
    rng = np.random.default_rng(seed)
    ids, scs = [], []
    for l in range(n_lists):
        if overlap == "disjoint":
            pool = np.arange(l * 1000, l * 1000 + 2 * k)
        elif overlap == "partly":
            pool = np.arange(0, 2 * k + 2)
        else:
            pool = np.arange(k)          # every list holds the same ids, in another order
        ids.append(np.stack([rng.permutation(pool)[:k] for _ in range(B)]).astype(np.int64))
        scs.append(make_scores(rng, norms[l], B, k))
    if B >= 5:      # the edge rows
        if n_lists > 1:
            ids[0][1, :] = -1                    # query 1: an empty first list
        ids[-1][2, 1:] = -1                      # query 2: a list of one entry (min-max degenerate)
        scs[0][3, :] = scs[0][3, 0]              # query 3: a list of equal scores (min-max degenerate)
        for l in range(n_lists):                 # query 4: every score equal -> equal fused scores, first-seen order decides
            scs[l][4, :] = np.float32(0.5)
        if k >= 4:
            ids[0][0, k - k // 4:] = -1          # query 0: a short list
    return ids, scs


def run_dev(ids, scs, norms, weights, top_k, w_query=None):
    """-> (ids, scores, methods, n) of hr_fuse_scores_dev on sentinel-filled outputs."""
    B = ids[0].shape[0]
    t_ids = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in ids]
    t_sc = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in scs]
    oi = torch.full((B, top_k), -7, dtype=torch.int64, device="cuda")
    os_ = torch.full((B, top_k), -7.0, dtype=torch.float64, device="cuda")
    om = torch.full((B, top_k), -7, dtype=torch.int32, device="cuda")
    on = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    wq = torch.from_numpy(np.ascontiguousarray(w_query, dtype=np.float64)).cuda() if w_query is not None else None
    args = []
    for l in range(3):
        if l < len(ids):
            args += [t_ids[l].data_ptr(), t_sc[l].data_ptr(), ids[l].shape[1], norms[l]]
        else:
            args += [0, 0, 0, 0]
    nat.fuse_scores_dev(*args, B, weights[0], weights[1], weights[2], wq.data_ptr() if wq is not None else 0, top_k,
                        oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), os_.cpu().numpy(), om.cpu().numpy(), on.cpu().numpy()


def check(got, want):
    gi, gs, gm, gn = got
    wi, ws, wm, wn = want
    assert np.array_equal(gn, wn)
    assert np.array_equal(gi, wi)                      # ids and the -1 padding
    assert np.array_equal(bits(gs), bits(ws))          # fp64 scores bit for bit, 0.0 padding
    assert np.array_equal(gm, wm)


@pytest.fixture(scope="module")
def handle(gpu):
    h = nat.ShardHandle(8)
    yield h
    h.close()


@pytest.mark.parametrize("overlap", ["disjoint", "partly", "full"])
@pytest.mark.parametrize("n_lists", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 40, 256])
@pytest.mark.parametrize("B", [1, 5])
def test_fuse_scores_dev_equals_the_restatement(gpu, handle, B, k, n_lists, overlap):
    seed = B * 100000 + k * 100 + n_lists * 10 + ["disjoint", "partly", "full"].index(overlap)
    norms = NORM_SETS[seed % len(NORM_SETS)]
    weights = WEIGHT_SETS[(seed // 7) % len(WEIGHT_SETS)]
    ids, scs = make_case(seed, B, k, n_lists, overlap, norms)
    wq = None
    if B > 1 and n_lists == 2:       # per-query weights replace the three scalars
        wq = np.random.default_rng(seed).uniform(-1, 2, (B, 3))
        wq[4] = 1.0                  # (the equal-scores row keeps equal fused scores)
    distinct = max(len(set(np.concatenate([i[q][:prefix_len(i[q])] for i in ids]).tolist())) for q in range(B))
    for top_k in sorted({max(1, distinct // 2), distinct + 3}):      # below and above the number of distinct ids
        want = R.fuse_batch(ids + [None] * (3 - n_lists), scs + [None] * (3 - n_lists), weights, norms, top_k, wq)
        check(run_dev(ids, scs, norms, weights, top_k, wq), want)
    # the host form, one query at a time: the same fused list
    for q in sorted({0, B - 1, min(4, B - 1)}):
        lists = []
        for i, s in zip(ids, scs):
            lists.append((i[q][:prefix_len(i[q])], s[q][:prefix_len(i[q])]))
        w = wq[q] if wq is not None else weights
        fi, fs, fm = handle.fuse_scores(lists, norms[:n_lists], w)
        wi, ws, wm = R.fuse(lists, w, norms)
        assert np.array_equal(fi, wi) and np.array_equal(bits(fs), bits(ws)) and np.array_equal(fm, wm)


@pytest.mark.parametrize("code_a,code_b", [(0, 1), (1, 0), (2, 1), (3, 3), (4, 3), (1, 4), (2, 2)])
def test_every_norm_code_with_negative_scores_and_weights(gpu, code_a, code_b):
    rng = np.random.default_rng(code_a * 10 + code_b)
    B, k = 5, 40
    ids = [np.stack([rng.permutation(60)[:k] for _ in range(B)]).astype(np.int64) for _ in range(2)]
    scs = [make_scores(rng, code_a, B, k), make_scores(rng, code_b, B, k)]
    scs[1][0, :] = -np.abs(scs[1][0, :]) - 1      # an all-negative list
    scs[0][1, ::3] = 0.0
    for weights in ((0.7, 0.3, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 0.0)):
        want = R.fuse_batch(ids + [None], scs + [None], weights, (code_a, code_b, 0), 50)
        check(run_dev(ids, scs, (code_a, code_b, 0), weights, 50), want)


def test_the_arctangent_on_the_device_is_the_canonical_one(gpu):
    """One list, weight 1, code 1: fused score = 0.5 + catan(s) / PI for fp32 scores across the ranges (saturation
    beyond ~10, tiny values, both signs, infinities)."""
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.uniform(-1, 1, 100), rng.uniform(-60, 60, 100), 10.0 ** rng.uniform(-30, 30, 50),
                        [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf]]).astype(np.float32)
    ids = np.arange(len(s), dtype=np.int64).reshape(1, -1)
    got = run_dev([ids], [s.reshape(1, -1)], (1, 0, 0), (1.0, 0.0, 0.0), len(s))
    want = R.fuse_batch([ids, None, None], [s.reshape(1, -1), None, None], (1.0, 0.0, 0.0), (1, 0, 0), len(s))
    check(got, want)


# ---------------------------------------------------------------------------------------------- hr_post_lists_dev
def _outs(B, top_k, k_out, dev="cuda"):
    return (torch.full((B, top_k), -7, dtype=torch.int64, device=dev), torch.full((B, top_k), -7.0, dtype=torch.float64, device=dev),
            torch.full((B, top_k), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev),
            torch.full((B, k_out), -7, dtype=torch.int64, device=dev), torch.full((B, k_out), -7.0, dtype=torch.float64, device=dev),
            torch.full((B, k_out), -7.0, dtype=torch.float64, device=dev))


def _shard_lists(rng, W, B, k, ascending):
    """W per-shard lists of one modality: [W, B, k], each sorted as the search writes them, ids distinct across shards."""
    sc = np.round(rng.uniform(0, 6, (W, B, k)) * 16) / 16 if ascending else np.round(rng.uniform(-1, 1, (W, B, k)) * 64) / 64
    ids = np.stack([np.stack([rng.permutation(3 * k)[:k] * W + w for _ in range(B)]) for w in range(W)]).astype(np.int64)
    for w in range(W):
        for b in range(B):
            o = np.lexsort((ids[w, b], sc[w, b] if ascending else -sc[w, b]))
            ids[w, b], sc[w, b] = ids[w, b][o], sc[w, b][o]
    if W > 1:
        ids[W - 1, 0, k // 2:] = -1      # a short shard
    return ids, sc.astype(np.float32)


@pytest.mark.parametrize("rerank", [0, 1])
@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("norms", [(2, 1, 0), (4, 3, 0)])
def test_post_lists_weighted_equals_the_separate_launches(gpu, W, rerank, norms):
    """fusion = 1: one launch against merge (the semantic modality ascending, as an L2 collection's) -> hr_fuse_scores_dev
    -> hr_rerank_linear_dev, and against the restatement."""
    rng = np.random.default_rng(W * 10 + rerank)
    B, k, top_k, k_out = 5, 40, 20, 5
    st = torch.cuda.current_stream().cuda_stream
    mods = [_shard_lists(rng, W, B, k, True), _shard_lists(rng, W, B, k, False)]    # (both draw from the same ids: they overlap)
    t_ids = [torch.from_numpy(i).cuda() for i, _ in mods]
    t_sc = [torch.from_numpy(s).cuda() for _, s in mods]
    wq = torch.from_numpy(rng.uniform(0, 1, (B, 3))).cuda()
    # ---- the separate entry points
    m_ids, m_sc = [], []
    for m in range(2):
        if W > 1:
            mi = torch.empty((B, k), dtype=torch.int64, device="cuda")
            ms = torch.empty((B, k), dtype=torch.float32, device="cuda")
            nat.merge_topk_dev(t_sc[m].data_ptr(), t_ids[m].data_ptr(), W, B, k, k, mi.data_ptr(), ms.data_ptr(), st,
                               ascending=(m == 0))
        else:
            mi, ms = t_ids[m][0].contiguous(), t_sc[m][0].contiguous()
        m_ids.append(mi)
        m_sc.append(ms)
    w_fi, w_fs, w_fm, w_fn, w_ri, w_rs, w_ro = _outs(B, top_k, k_out)
    nat.fuse_scores_dev(m_ids[0].data_ptr(), m_sc[0].data_ptr(), k, norms[0], m_ids[1].data_ptr(), m_sc[1].data_ptr(), k,
                        norms[1], 0, 0, 0, 0, B, 0.0, 0.0, 0.0, wq.data_ptr(), top_k, w_fi.data_ptr(), w_fs.data_ptr(),
                        w_fm.data_ptr(), w_fn.data_ptr(), st)
    if rerank:
        nat.rerank_linear_dev(w_fi.data_ptr(), w_fs.data_ptr(), w_fm.data_ptr(), w_fn.data_ptr(), B, top_k, 1.0, 0.1, 0.0,
                              k_out, w_ri.data_ptr(), w_rs.data_ptr(), w_ro.data_ptr(), st)
    # ---- one launch
    g_fi, g_fs, g_fm, g_fn, g_ri, g_rs, g_ro = _outs(B, top_k, k_out)
    a = nat.PostArgs()
    got_m = []
    for m in range(2):
        a.ids[m], a.scores[m], a.k_in[m], a.k_fuse[m], a.norm[m] = t_ids[m].data_ptr(), t_sc[m].data_ptr(), k, k, norms[m]
        if W > 1:
            mi = torch.full((B, k), -9, dtype=torch.int64, device="cuda")
            ms = torch.full((B, k), -9.0, dtype=torch.float32, device="cuda")
            a.merged_ids[m], a.merged_scores[m] = mi.data_ptr(), ms.data_ptr()
            got_m.append((mi, ms))
    a.id_stride = a.score_stride = B * k
    a.n_lists, a.rrf_k, a.top_k, a.asc_mask, a.fusion = W, 60, top_k, 1, 1
    a.w_query = wq.data_ptr()
    a.fused_ids, a.fused_scores, a.fused_methods, a.fused_n = g_fi.data_ptr(), g_fs.data_ptr(), g_fm.data_ptr(), g_fn.data_ptr()
    a.rerank, a.base_w, a.method_bonus, a.recency_w, a.k_out = rerank, 1.0, 0.1, 0.0, k_out
    a.rr_ids, a.rr_scores, a.rr_orig = g_ri.data_ptr(), g_rs.data_ptr(), g_ro.data_ptr()
    nat.post_lists_dev(a, B, st)
    torch.cuda.synchronize()
    for (mi, ms), wi, ws in zip(got_m, m_ids, m_sc):
        assert torch.equal(mi, wi) and torch.equal(ms.view(torch.int32), ws.view(torch.int32))
    for g, w in ((g_fi, w_fi), (g_fm, w_fm), (g_fn, w_fn), (g_ri, w_ri)):
        assert torch.equal(g, w)
    for g, w in ((g_fs, w_fs), (g_rs, w_rs), (g_ro, w_ro)):
        assert torch.equal(g.view(torch.int64), w.view(torch.int64))
    want = R.fuse_batch([m_ids[0].cpu().numpy(), m_ids[1].cpu().numpy(), None],
                        [m_sc[0].cpu().numpy(), m_sc[1].cpu().numpy(), None], None, norms, top_k, wq.cpu().numpy())
    check((g_fi.cpu().numpy(), g_fs.cpu().numpy(), g_fm.cpu().numpy(), g_fn.cpu().numpy()), want)


def test_post_lists_with_fusion_0_equals_hr_fuse_rrf_dev(gpu):
    rng = np.random.default_rng(1)
    B, k, top_k = 5, 40, 20
    st = torch.cuda.current_stream().cuda_stream
    ids = [torch.from_numpy(np.stack([rng.permutation(60)[:k] for _ in range(B)]).astype(np.int64)).cuda() for _ in range(2)]
    w_fi, w_fs, w_fm, w_fn, _, _, _ = _outs(B, top_k, 1)
    nat.fuse_rrf_dev(ids[0].data_ptr(), k, ids[1].data_ptr(), k, 0, 0, B, 0.7, 0.3, 0.2, 60, top_k, w_fi.data_ptr(),
                     w_fs.data_ptr(), w_fm.data_ptr(), w_fn.data_ptr(), st)
    g_fi, g_fs, g_fm, g_fn, _, _, _ = _outs(B, top_k, 1)
    a = nat.PostArgs()
    for m in range(2):
        a.ids[m], a.k_in[m], a.k_fuse[m] = ids[m].data_ptr(), k, k       # no scores: RRF reads none
    a.n_lists, a.rrf_k, a.top_k, a.fusion = 1, 60, top_k, 0
    a.w[0], a.w[1], a.w[2] = 0.7, 0.3, 0.2
    a.fused_ids, a.fused_scores, a.fused_methods, a.fused_n = g_fi.data_ptr(), g_fs.data_ptr(), g_fm.data_ptr(), g_fn.data_ptr()
    nat.post_lists_dev(a, B, st)
    torch.cuda.synchronize()
    assert torch.equal(g_fi, w_fi) and torch.equal(g_fm, w_fm) and torch.equal(g_fn, w_fn)
    assert torch.equal(g_fs.view(torch.int64), w_fs.view(torch.int64))


# ---------------------------------------------------------------------------------------------- refusals
def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((o == -7).all()) for o in outs)


def test_refused_calls_launch_nothing(gpu):
    B, k, top_k = 3, 8, 8
    st = torch.cuda.current_stream().cuda_stream
    ids = torch.arange(B * k, dtype=torch.int64, device="cuda").view(B, k)
    sc = torch.rand((B, k), dtype=torch.float32, device="cuda")
    big_i = torch.arange(B * 257, dtype=torch.int64, device="cuda").view(B, 257)
    big_s = torch.rand((B, 257), dtype=torch.float32, device="cuda")
    outs = _outs(B, top_k, 2)
    o = [t.data_ptr() for t in outs[:4]]
    I, S = ids.data_ptr(), sc.data_ptr()

    def dev(*lists, top=top_k):
        nat.fuse_scores_dev(*lists, B, 0.5, 0.5, 0.5, 0, top, *o, st)

    for bad in ((I, 0, k, 0, 0, 0, 0, 0, 0, 0, 0, 0),            # NULL scores of a used list
                (I, S, k, 0, I, 0, k, 1, 0, 0, 0, 0),
                (I, S, k, 0, I, S, k, 1, I, 0, k, 0),
                (I, S, k, 5, 0, 0, 0, 0, 0, 0, 0, 0),            # a norm code outside 0..4
                (I, S, k, -1, 0, 0, 0, 0, 0, 0, 0, 0),
                (I, S, k, 0, I, S, k, 7, 0, 0, 0, 0),
                (0, S, k, 0, 0, 0, 0, 0, 0, 0, 0, 0)):           # NULL ids, as hr_fuse_rrf_dev refuses them
        with pytest.raises(ValueError):
            dev(*bad)
    with pytest.raises(ValueError):
        dev(I, S, k, 0, 0, 0, 0, 0, 0, 0, 0, 0, top=0)
    with pytest.raises(nat.HbmRagError):                          # HR_ELIMIT, as for RRF
        dev(big_i.data_ptr(), big_s.data_ptr(), 257, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert _untouched(outs)

    def post(**kw):
        a = nat.PostArgs()
        a.ids[0], a.scores[0], a.k_in[0], a.k_fuse[0] = I, S, k, k
        a.ids[1], a.scores[1], a.k_in[1], a.k_fuse[1], a.norm[1] = I, S, k, k, 1
        a.n_lists, a.rrf_k, a.top_k, a.fusion = 1, 60, top_k, 1
        a.fused_ids, a.fused_scores, a.fused_methods, a.fused_n = o
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, name)[v[0]] = v[1]
            else:
                setattr(a, name, v)
        nat.post_lists_dev(a, B, st)

    for bad in (dict(fusion=2), dict(fusion=-1), dict(scores=(0, None)), dict(scores=(1, None)), dict(norm=(0, 5)),
                dict(norm=(1, -1))):
        with pytest.raises(ValueError):
            post(**bad)
    assert _untouched(outs)
    post()                                   # the same arguments without the fault are served
    torch.cuda.synchronize()
    assert int(outs[3][0]) == k
    post(fusion=0, scores=(0, None))         # and RRF still needs no scores
    torch.cuda.synchronize()


def test_host_form_refusals_and_empty_input(gpu, handle):
    assert [len(x) for x in handle.fuse_scores([], [])] == [0, 0, 0]
    with pytest.raises(ValueError):
        handle.fuse_scores([([1, 2], [0.5, 0.25])], [5])
    with pytest.raises(ValueError):
        handle.fuse_scores([([1, 2], [0.5])], [0])
    with pytest.raises(nat.HbmRagError):
        handle.fuse_scores([(np.arange(257), np.zeros(257, np.float32))], [0])
