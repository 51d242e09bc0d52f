"""An L2 corpus cut into three shard handles on one GPU, held to the whole-corpus yardstick: the host merge (ShardSet),
the device merge (hr_merge_topk_asc_dev), hr_post_lists_dev with an ascending semantic modality, and a manager built
with semantic_metric="L2".  Equal distances lie on both sides of a cut and one shard holds fewer than k rows."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.shards import ShardSet

from l2_yardstick import bits, l2_search

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = (3000, 17, 2500)
D, V, NNZ, B, K = 80, 400, 8, 9, 40


def _corpus():
    rng = np.random.default_rng(42)
    n = sum(SIZES)
    X = rng.standard_normal((n, D)).astype(np.float16)
    X[3005] = X[2990]                      # equal distances on both sides of the first cut (and inside the small shard)
    X[3100] = X[2990]
    X[10] = X[5000]                        # ... and across the second one
    Q = rng.standard_normal((B, D)).astype(np.float32)
    Q[0] = X[2990].astype(np.float32)      # distance 0 three times, in three shards
    Q[1] = X[5000].astype(np.float32) + 0.5
    idx = np.stack([np.sort(rng.choice(V, NNZ, replace=False)) for _ in range(n)]).astype(np.int32).reshape(-1)
    val = np.abs(rng.standard_normal(n * NNZ)).astype(np.float32)
    ptr = np.arange(n + 1, dtype=np.int64) * NNZ
    SQ = [(np.sort(rng.choice(V, 12, replace=False)).astype(np.int32), np.abs(rng.standard_normal(12)).astype(np.float32))
          for _ in range(B)]
    return X, Q, ptr, idx, val, SQ


def _handles(X, ptr, idx, val, offsets):
    hs, lo = [], 0
    for sz in SIZES:
        hi = lo + sz
        h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_L2, V)
        if offsets:
            h.set_row_offset(lo)
        h.add_dense(X[lo:hi])
        h.add_sparse(ptr[lo:hi + 1] - ptr[lo], idx[ptr[lo]:ptr[hi]], val[ptr[lo]:ptr[hi]])
        h.finalize()
        hs.append(h)
        lo = hi
    return hs


def test_shardset_host_merge(gpu):
    X, Q, ptr, idx, val, _ = _corpus()
    hs = _handles(X, ptr, idx, val, offsets=False)
    s = ShardSet(hs)
    edges = np.concatenate([[0], np.cumsum(SIZES)])
    s.rows_of = [np.arange(edges[i], edges[i + 1], dtype=np.int64) for i in range(3)]
    s._n = int(edges[-1])
    for k in (K, 5):
        wi, ws = l2_search(X, Q, k)
        ids, sc = s.search_dense(Q, k)
        assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))
        assert ids[0, :3].tolist() == [2990, 3005, 3100] and (bits(sc[0, :3]) == 0).all()
    keep = np.random.default_rng(1).random(len(X)) < 0.4
    wi, ws = l2_search(X, Q, K, np.packbits(keep, bitorder="little"))
    ids, sc = s.search_dense(Q, K, keep)
    assert np.array_equal(ids, wi) and np.array_equal(bits(sc), bits(ws))
    for h in hs:
        h.close()


def test_device_merge_and_post_lists(gpu):
    X, Q, ptr, idx, val, SQ = _corpus()
    hs = _handles(X, ptr, idx, val, offsets=True)
    W = len(hs)
    g_ids = np.empty((2, W, B, K), np.int64)
    g_sc = np.empty((2, W, B, K), np.float32)
    for r, h in enumerate(hs):
        g_ids[0, r], g_sc[0, r] = h.search_dense(Q, K)
        g_ids[1, r], g_sc[1, r] = h.search_sparse(SQ, K, 0.2)
    assert (g_ids[0, 1, :, 17:] == -1).all()          # the 17-row shard pads its lists
    want_d = l2_search(X, Q, K)
    want_s = oracle.sparse_search(ptr, idx, val, SQ, K, 0.2)
    d_ids, d_sc = torch.from_numpy(g_ids).cuda(), torch.from_numpy(g_sc).cuda()
    st = torch.cuda.current_stream()

    # the merge entry point, narrower output included
    for k_out in (K, 7):
        oi = torch.empty((B, k_out), dtype=torch.int64, device="cuda")
        os_ = torch.empty((B, k_out), dtype=torch.float32, device="cuda")
        nat.merge_topk_dev(d_sc[0].data_ptr(), d_ids[0].data_ptr(), W, B, K, k_out, oi.data_ptr(), os_.data_ptr(),
                           st.cuda_stream, ascending=True)
        st.synchronize()
        assert np.array_equal(oi.cpu().numpy(), want_d[0][:, :k_out])
        assert np.array_equal(bits(os_.cpu().numpy()), bits(want_d[1][:, :k_out]))

    # merge of both modalities (semantic ascending, sparse descending) + RRF in one launch
    top_k = 2 * K
    m_ids = torch.empty((2, B, K), dtype=torch.int64, device="cuda")
    m_sc = torch.empty((2, B, K), dtype=torch.float32, device="cuda")
    f_ids = torch.empty((B, top_k), dtype=torch.int64, device="cuda")
    f_sc = torch.empty((B, top_k), dtype=torch.float64, device="cuda")
    f_m = torch.empty((B, top_k), dtype=torch.int32, device="cuda")
    f_n = torch.empty((B,), dtype=torch.int32, device="cuda")
    a = nat.PostArgs()
    for m in range(2):
        a.ids[m], a.scores[m] = d_ids[m].data_ptr(), d_sc[m].data_ptr()
        a.k_in[m], a.k_fuse[m] = K, K
        a.merged_ids[m], a.merged_scores[m] = m_ids[m].data_ptr(), m_sc[m].data_ptr()
    a.n_lists, a.rrf_k, a.top_k = W, 60, top_k
    a.id_stride = a.score_stride = B * K
    a.w[0], a.w[1], a.w[2] = 0.7, 0.3, 0.0
    a.fused_ids, a.fused_scores = f_ids.data_ptr(), f_sc.data_ptr()
    a.fused_methods, a.fused_n = f_m.data_ptr(), f_n.data_ptr()
    a.asc_mask = 1
    nat.post_lists_dev(a, B, st.cuda_stream)
    st.synchronize()
    for m, (wi, ws) in enumerate((want_d, want_s)):
        assert np.array_equal(m_ids[m].cpu().numpy(), wi), f"merged ids of modality {m}"
        assert np.array_equal(bits(m_sc[m].cpu().numpy()), bits(ws)), f"merged scores of modality {m}"
    for b in range(B):
        oi, os_, om = oracle.rrf(want_d[0][b][want_d[0][b] >= 0], want_s[0][b][want_s[0][b] >= 0], (), 0.7, 0.3, 0.0, 60)
        n = min(len(oi), top_k)
        assert int(f_n[b]) == n
        assert np.array_equal(f_ids[b, :n].cpu().numpy(), oi[:n])
        assert np.array_equal(f_sc[b, :n].cpu().numpy().view(np.uint64), os_[:n].view(np.uint64))
        assert np.array_equal(f_m[b, :n].cpu().numpy(), om[:n])
    for h in hs:
        h.close()


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
def test_manager_with_l2_semantic_collection(gpu, devices):
    from advanced_rag import MilvusIndexManager
    X, Q, ptr, idx, val, _ = _corpus()
    n = len(X)
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float16", enable_domain=False, devices=devices,
                             semantic_metric="L2")
    assert mgr.collections["semantic_index"].metric == "L2"
    lo = 0
    for step in (1000, 2017, n):
        hi = min(n, lo + step)
        mgr.add_rows(X[lo:hi].astype(np.float32), (ptr[lo:hi + 1], idx, val), ids=[f"c{r}" for r in range(lo, hi)],
                     contents=[f"text {r}" for r in range(lo, hi)], doc_id=[f"doc{r % 7}" for r in range(lo, hi)])
        lo = hi
    mgr.finalize()
    rows = np.arange(n)
    for flt, keep in ((None, None), ('doc_id == "doc3"', rows % 7 == 3)):
        m8 = None if keep is None else np.packbits(keep, bitorder="little")
        for b in (0, 1, 4):
            wi, ws = l2_search(X, Q[b][None], 20, m8)
            got = asyncio.run(mgr.search(Q[b], "semantic_index", 20, flt))
            assert [h["_row"] for h in got] == wi[0].tolist()
            sc = np.array([h["score"] for h in got], np.float32)
            assert np.array_equal(bits(sc), bits(ws[0]))
            assert (np.diff(sc) >= 0).all()                                   # distances, ascending
            got2 = asyncio.run(mgr.search(Q[b], "semantic_index", 20, flt, {"metric_type": "L2", "params": {"ef": 64}}))
            assert [h["_row"] for h in got2] == wi[0].tolist()
    with pytest.raises(ValueError):
        asyncio.run(mgr.search(Q[0], "semantic_index", 20, None, {"metric_type": "COSINE", "params": {"ef": 64}}))
    mgr.close() if hasattr(mgr, "close") else None
