"""Sharded hybrid search held to the oracle run on the WHOLE corpus, at the edges of the per-shard lists.

W real shard handles over contiguous, uneven row ranges (hr_set_row_offset) stand in for W ranks on one GPU.  Each rank
is a real HybridSearchEngine; only its all-gather (`_exchange`) is replaced by a copy of every rank's pack into the
rank's gathered buffer, so the lists, the flags, the post-exchange launch (merge -> RRF -> rerank, hr_post_lists_dev
with the engine's own PostArgs) and resolve_inexact are the product's.  Every expected answer comes from
oracle.dense_search / sparse_search over all rows (the global mask), oracle.rrf and the learned-rank formula, composed
as oracle_pipeline in test_gpu_engine.py does; ids, fp32 list scores and fp64 fused / reranked scores are compared bit
for bit.  The host-merge path (MilvusIndexManager(devices=[0] * W)) is held to the same oracle at the end."""
import asyncio

import numpy as np
import pytest

import oracle
from advanced_rag import _native as nat
from advanced_rag.engine import EngineConfig, HybridSearchEngine, ListPack, pack_sparse_queries

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HR_ELIMIT = 5
MERGE_LDS_MAX = 60 * 1024          # kMergeLdsMax of csrc/fuse.h
METRIC = {nat.HR_METRIC_COSINE: oracle.COSINE, nat.HR_METRIC_IP: oracle.IP}
DTYPE = {nat.HR_F16: np.float16, nat.HR_F32: np.float32}


def merge_lds_bytes(n_lists, k_in):
    return n_lists * k_in * 12 + n_lists * 4


# --------------------------------------------------------------------------- comparison
def same(got, want, what, ctx, bits=None):
    """Bit-exact equality; the failure names the case (layout, query) and the first differing position."""
    got, want = np.asarray(got), np.asarray(want)
    if bits is not None:
        got, want = got.view(bits), want.view(bits)
    if got.shape != want.shape:
        pytest.fail(f"{what} [{ctx}]: {got.shape[-1] if got.ndim else 0} entries, oracle {want.shape[-1] if want.ndim else 0}"
                    f" (got {got.tolist()}, oracle {want.tolist()})")
    bad = np.argwhere(got != want)
    if len(bad):
        pos = tuple(int(i) for i in bad[0])
        pytest.fail(f"{what} [{ctx}]: first difference at position {pos}: got {got[pos]!r}, oracle {want[pos]!r}")


# --------------------------------------------------------------------------- corpus
class Corpus:
    """Dense rows + CSR sparse rows over `sizes` contiguous shards.  The last `n_excl` terms of the vocabulary occur only
    in rows of shard `excl_shard` (one per row there)."""

    def __init__(self, sizes, d=48, V=300, nnz=6, seed=0, dtype=nat.HR_F16, signed_docs=False, excl_shard=None,
                 n_excl=8):
        rng = np.random.default_rng(seed)
        self.sizes = list(sizes)
        edges = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.bounds = [(int(edges[i]), int(edges[i + 1])) for i in range(len(self.sizes))]
        self.n, self.d, self.V, self.dtype = int(edges[-1]), d, V, dtype
        self.rng = rng
        self.X = rng.standard_normal((self.n, d)).astype(DTYPE[dtype])
        base = V - n_excl
        idx = np.sort(np.argpartition(rng.random((self.n, base)), nnz - 1, axis=1)[:, :nnz], axis=1).astype(np.int32)
        if excl_shard is not None:
            lo, hi = self.bounds[excl_shard]
            idx[lo:hi, -1] = base + rng.integers(0, n_excl, hi - lo)
        self.idx = idx.reshape(-1)
        val = rng.standard_normal(self.n * nnz).astype(np.float32)
        self.val = val if signed_docs else np.abs(val)
        self.ptr = np.arange(self.n + 1, dtype=np.int64) * nnz
        self.nnz = nnz

    def queries(self, B, q_nnz=12, signed=False, terms=None):
        rng = self.rng
        Q = rng.standard_normal((B, self.d)).astype(np.float32)
        SQ = []
        for _ in range(B):
            pool = np.arange(self.V) if terms is None else np.asarray(terms)
            qi = np.sort(rng.choice(pool, min(q_nnz, len(pool)), replace=False)).astype(np.int32)
            qv = rng.standard_normal(len(qi)).astype(np.float32)
            SQ.append((qi, qv if signed else np.abs(qv)))
        return Q, SQ

    def set_sparse_row(self, r, qi, qv):
        """Overwrite row r's sparse payload (same nnz)."""
        self.idx[self.ptr[r]:self.ptr[r + 1]] = qi
        self.val[self.ptr[r]:self.ptr[r + 1]] = qv

    def handles(self, metric=nat.HR_METRIC_COSINE, sparse=True):
        hs = []
        for lo, hi in self.bounds:
            h = nat.ShardHandle(self.d, self.dtype, metric, self.V if sparse else 0)
            h.set_row_offset(lo)
            if hi > lo:
                h.add_dense(self.X[lo:hi])
                if sparse:
                    p = self.ptr
                    h.add_sparse(p[lo:hi + 1] - p[lo], self.idx[p[lo]:p[hi]], self.val[p[lo]:p[hi]])
            h.finalize()
            hs.append(h)
        return hs


def packed_mask(keep):
    """Packed row mask, padded to whole 8-byte words (what device_filters hands the searches)."""
    m = np.packbits(np.asarray(keep, dtype=bool), bitorder="little")
    m = np.pad(m, (0, (-len(m)) % 8 + (8 if len(m) == 0 else 0)))
    return m


def omask(keep):
    """The oracle's row mask: packed like the product's (bit r % 8 of byte r // 8)."""
    return np.packbits(np.asarray(keep, dtype=bool), bitorder="little")


def shard_oracle(c, metric, Q, SQ, kp, drop, keep, r, modality, dom=None, Qd=None, k_dom=0):
    """The oracle's list of shard r alone (rows [lo, hi), global row numbers), kp wide like the pack."""
    lo, hi = c.bounds[r] if dom is None else dom.bounds[r]
    B = Q.shape[0]
    if hi == lo:
        return np.full((B, kp), -1, np.int64), np.zeros((B, kp), np.float32)
    m8 = None if keep is None else omask(keep[lo:hi])
    if modality == "dense":
        return oracle.dense_search(c.X[lo:hi], Q, kp, METRIC[metric], m8, row_offset=lo)
    if modality == "sparse":
        p = c.ptr
        return oracle.sparse_search(p[lo:hi + 1] - p[lo], c.idx[p[lo]:p[hi]], c.val[p[lo]:p[hi]], SQ, kp, drop, m8,
                                    row_offset=lo)
    ids, sc = oracle.dense_search(dom.X[lo:hi], Qd, k_dom, oracle.COSINE, row_offset=lo)
    return (np.pad(ids, ((0, 0), (0, kp - k_dom)), constant_values=-1), np.pad(sc, ((0, 0), (0, kp - k_dom))))


def expected(c, metric, cfg, Q, SQ, drop, keep=None, dom=None, Qd=None, weights=None):
    """Whole-corpus oracle: lists, fused top_k and reranked output, composed as test_gpu_engine.oracle_pipeline."""
    kp = 2 * cfg.top_k
    m8 = None if keep is None else omask(keep)
    lists = {"dense": oracle.dense_search(c.X, Q, kp, METRIC[metric], m8)}
    if cfg.use_sparse:
        lists["sparse"] = oracle.sparse_search(c.ptr, c.idx, c.val, SQ, kp, drop, m8)
    if Qd is not None:
        lists["domain"] = oracle.dense_search(dom.X, Qd, cfg.top_k, oracle.COSINE)
    fused, reranked = [], []
    for b in range(Q.shape[0]):
        w = (cfg.dense_weight, cfg.sparse_weight, cfg.domain_weight) if weights is None else tuple(weights[b])
        live = {k: v[0][b][v[0][b] >= 0] for k, v in lists.items()}
        fi, fs, fm = oracle.rrf(live["dense"], live.get("sparse", ()), live.get("domain", ()), w[0], w[1], w[2], cfg.rrf_k)
        fi, fs, fm = fi[:cfg.top_k], fs[:cfg.top_k], fm[:cfg.top_k]
        fused.append((fi, fs, fm))
        new = [cfg.base_weight * float(s) + cfg.method_bonus * float(bin(int(m)).count("1")) + cfg.recency_weight * 0.0
               for s, m in zip(fs, fm)]
        order = sorted(range(len(new)), key=lambda i: new[i], reverse=True)[:cfg.rerank_top_k]  # stable, like list.sort
        reranked.append((fi[order], np.array([new[i] for i in order], dtype=np.float64), fs[order]))
    return lists, fused, reranked


# --------------------------------------------------------------------------- W ranks on one process
class Rank(HybridSearchEngine):
    """One rank of a W-rank step: the all-gather is a copy of every rank's pack; everything else is the engine's."""
    peers = ()

    def _exchange(self, b):
        g = b["gathered"]
        for r, e in enumerate(self.peers):
            g[r].copy_(e._bufs[b["layout"].B]["pack"])
        return g


MODS = ("dense", "sparse", "domain")


def run_case(c, cfg, Q, SQ, drop=0.2, metric=nat.HR_METRIC_COSINE, keep=None, dom=None, Qd=None, weights=None,
             want_unproven=None, case=""):
    """Search on every rank, exchange, post; check flags and proven lists; repair; check everything against the
    whole-corpus oracle and the global merge form.  Returns the number of lists the ranks redid."""
    hs = c.handles(metric, sparse=cfg.use_sparse)
    hds = dom.handles(nat.HR_METRIC_COSINE, sparse=False) if dom is not None else [None] * len(hs)
    W, B, kp = len(hs), Q.shape[0], 2 * cfg.top_k
    ctx = f"{case} layout={c.sizes} metric={metric} dtype={c.dtype} top_k={cfg.top_k}"
    try:
        ranks = [Rank(h, cfg, simulate_ranks=W, domain_handle=hd) for h, hd in zip(hs, hds)]
        for e in ranks:
            e.peers = ranks
            e._buffers(Q.shape[0])
        dq = torch.from_numpy(Q).cuda()
        sq = ranks[0].upload_sparse(pack_sparse_queries(SQ, drop)) if cfg.use_sparse else None
        dqd = torch.from_numpy(np.ascontiguousarray(Qd)).cuda() if Qd is not None else None
        wq = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).cuda() if weights is not None else None
        dmasks = [None if keep is None else torch.from_numpy(packed_mask(keep[lo:hi])).cuda() for lo, hi in c.bounds]
        for e, dm in zip(ranks, dmasks):
            e.search(dq, sq, dqd, rowmask=dm, weights=wq)
        st = torch.cuda.current_stream().cuda_stream
        for e in ranks:  # every rank's lists are in every gathered buffer now: the step as W ranks run it
            e._post_lists(e._bufs[B], B, st)
        torch.cuda.synchronize()

        lists, fused, reranked = expected(c, metric, cfg, Q, SQ, drop, keep, dom, Qd, weights)
        mods = [m for m in MODS if m in lists]
        slot = {"dense": 0, "sparse": 1, "domain": ranks[0]._bufs[B]["n_mod"] - 1}
        own = np.stack([e._bufs[B]["flags"].cpu().numpy() for e in ranks])           # [W, n_mod, B]
        for r, e in enumerate(ranks):
            agg = e._bufs[B]["agg_flags"].cpu().numpy()
            same(agg, own.min(axis=0), f"aggregate flags of rank {r} (min over the ranks)", ctx)
        kdom = cfg.top_k

        def check_lists(proven_only):
            b0 = ranks[0]._bufs[B]
            agg = b0["agg_flags"].cpu().numpy()
            for m in mods:
                s = slot[m]
                for r in range(W):   # each rank's own list against the oracle on its rows
                    ids, sc = ListPack(b0["n_mod"], B, kp).views(b0["gathered"][r])
                    wi, ws = shard_oracle(c, metric, Q, SQ, kp, drop, keep, r, m, dom, Qd, kdom)
                    for q in range(B):
                        if proven_only and not own[r, s, q]:
                            continue
                        same(ids[s, q].cpu().numpy(), wi[q], f"{m} list of shard {r}", f"{ctx} query={q}")
                        same(sc[s, q].cpu().numpy(), ws[q], f"{m} scores of shard {r}", f"{ctx} query={q}", np.uint32)
                mi, ms = (b0["m_dom_ids"], b0["m_dom_scores"]) if m == "domain" else (b0["m_ids"][s], b0["m_scores"][s])
                mi, ms = mi.cpu().numpy(), ms.cpu().numpy()
                wi, ws = lists[m]
                for q in range(B):
                    if proven_only and not agg[s, q]:
                        continue
                    same(mi[q], wi[q], f"merged {m} list", f"{ctx} query={q}")
                    same(ms[q], ws[q], f"merged {m} scores", f"{ctx} query={q}", np.uint32)

        check_lists(proven_only=True)
        if want_unproven is not None:
            assert (own == 0).any() == want_unproven, f"[{ctx}] expected {'an' if want_unproven else 'no'} unproven list"
        Qd_host = None if Qd is None else np.ascontiguousarray(Qd)
        redone = sum(e.resolve_inexact(e._bufs[B], Q, SQ, drop, Qd_host) for e in ranks)
        torch.cuda.synchronize()
        for e in ranks:  # every rank's repairs reach every rank
            e._post_lists(e._bufs[B], B, st)
        torch.cuda.synchronize()
        own = np.stack([e._bufs[B]["flags"].cpu().numpy() for e in ranks])
        assert own.min() == 1, f"[{ctx}] a list is still unproven after resolve_inexact"
        check_lists(proven_only=False)

        for r, e in enumerate(ranks):
            b = e._bufs[B]
            for q in range(B):
                qctx = f"{ctx} rank={r} query={q}"
                fi, fs, fm = fused[q]
                nf = int(b["fused_n"][q])
                same(b["fused_ids"][q, :nf].cpu().numpy(), fi, "fused ids", qctx)
                same(b["fused_scores"][q, :nf].cpu().numpy(), fs, "fused scores", qctx, np.uint64)
                same(b["fused_methods"][q, :nf].cpu().numpy(), fm, "fused methods", qctx)
                same(b["fused_ids"][q, nf:].cpu().numpy(), np.full(cfg.top_k - nf, -1), "fused padding", qctx)
                ri, rs, ro = reranked[q]
                nr = len(ri)
                same(b["rr_ids"][q, :nr].cpu().numpy(), ri, "reranked ids", qctx)
                same(b["rr_scores"][q, :nr].cpu().numpy(), rs, "reranked scores", qctx, np.uint64)
                same(b["rr_orig"][q, :nr].cpu().numpy(), ro, "reranked fused scores", qctx, np.uint64)
                same(b["rr_ids"][q, nr:].cpu().numpy(), np.full(cfg.rerank_top_k - nr, -1), "rerank padding", qctx)

        # the global form of the merge (hr_merge_topk_dev) over the same gathered buffer
        b0 = ranks[0]._bufs[B]
        g = b0["gathered"]
        for m in mods:
            k_out = kdom if m == "domain" else kp
            oi = torch.empty((B, k_out), dtype=torch.int64, device="cuda")
            os_ = torch.empty((B, k_out), dtype=torch.float32, device="cuda")
            sc_off, id_off, sc_stride, id_stride = b0["layout"].merge_args(slot[m])
            nat.merge_topk_dev(g.data_ptr() + sc_off, g.data_ptr() + id_off, W, B, kp, k_out, oi.data_ptr(),
                               os_.data_ptr(), st, score_stride=sc_stride, id_stride=id_stride)
            torch.cuda.synchronize()
            same(oi.cpu().numpy(), lists[m][0], f"{m} list of merge_topk_dev", ctx)
            same(os_.cpu().numpy(), lists[m][1], f"{m} scores of merge_topk_dev", ctx, np.uint32)
        return redone
    finally:
        for h in list(hs) + [hd for hd in hds if hd is not None]:
            h.close()


# --------------------------------------------------------------------------- 1. shard layouts
LAYOUTS = {                     # top_k = 20 -> k' = 40
    "w2_short_and_long": [37, 1500],
    "w3_one_row_exact_kp": [1, 40, 2100],
    "w8_ragged_with_empty": [300, 1, 40, 39, 0, 900, 57, 610],
    "w3_total_below_kp": [7, 1, 17],
    "w8_total_below_kp": [3, 0, 5, 1, 9, 2, 0, 4],
}
STORAGE = {"cosine_f16": (nat.HR_METRIC_COSINE, nat.HR_F16), "ip_f32": (nat.HR_METRIC_IP, nat.HR_F32),
           "ip_f16": (nat.HR_METRIC_IP, nat.HR_F16), "cosine_f32": (nat.HR_METRIC_COSINE, nat.HR_F32)}


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_match_whole_corpus_oracle(gpu, layout, storage):
    metric, dtype = STORAGE[storage]
    c = Corpus(LAYOUTS[layout], dtype=dtype, seed=len(layout) * 7 + metric)
    Q, SQ = c.queries(6)
    Q[0] = c.X[-1].astype(np.float32)            # a query that is a row of the last shard
    run_case(c, EngineConfig(top_k=20), Q, SQ, metric=metric, case=f"{layout}/{storage}")


def test_zero_row_shard_is_served_empty_and_proven(gpu):
    """The library accepts a shard without rows (no HbmRagError): its lists are all padding and flagged proven."""
    c = Corpus([0, 50])
    hs = c.handles()
    h = hs[0]
    try:
        ids, sc = h.search_dense(np.ones((2, c.d), np.float32), 40)
        assert (ids == -1).all() and (sc == 0).all()
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        oi = torch.empty((2, 40), dtype=torch.int64, device="cuda")
        os_ = torch.empty((2, 40), dtype=torch.float32, device="cuda")
        h.search_dense_dev(torch.ones((2, c.d), device="cuda").data_ptr(), 2, 40, oi.data_ptr(), os_.data_ptr(),
                           flags.data_ptr())
        torch.cuda.synchronize()
        assert (oi == -1).all().item() and flags.min().item() == 1
    finally:
        for x in hs:
            x.close()


# --------------------------------------------------------------------------- 2. masks and tombstones
@pytest.mark.parametrize("layout", ["w3_one_row_exact_kp", "w8_ragged_with_empty"])
def test_mask_empties_a_shard_and_thins_the_rest(gpu, layout):
    c = Corpus(LAYOUTS[layout], seed=11)
    Q, SQ = c.queries(5, q_nnz=40)
    keep = np.zeros(c.n, dtype=bool)
    big = int(np.argmax(c.sizes))
    for r, (lo, hi) in enumerate(c.bounds):   # shard `big` loses every row; the others keep fewer than k' rows
        if r != big:
            keep[lo:hi] = np.arange(hi - lo) % 3 != 1
            keep[lo + 30:hi] = False
    run_case(c, EngineConfig(top_k=20), Q, SQ, keep=keep, case=f"mask/{layout}")


# --------------------------------------------------------------------------- 3. short or empty sparse lists
@pytest.mark.parametrize("drop", [0.0, 0.2], ids=["drop0", "drop02"])
@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
def test_sparse_lists_short_or_empty_on_some_ranks(gpu, signed, drop):
    sizes = [200, 30, 700, 1]
    c = Corpus(sizes, V=300, nnz=5, seed=3, signed_docs=signed, excl_shard=1)
    B = 6
    Q, SQ = c.queries(B, q_nnz=10, signed=signed)
    excl = np.arange(c.V - 8, c.V)
    for q in (0, 1):        # only terms that occur in shard 1: every other rank's sparse list is empty
        qi = np.sort(c.rng.choice(excl, 5, replace=False)).astype(np.int32)
        qv = c.rng.standard_normal(5).astype(np.float32)
        SQ[q] = (qi, qv if signed else np.abs(qv))
    SQ[2] = (np.array([c.V - 1], np.int32), np.array([-1.0 if signed else 1.0], np.float32))
    run_case(c, EngineConfig(top_k=20), Q, SQ, drop=drop, case=f"sparse/{'signed' if signed else 'unsigned'}/{drop}")


# --------------------------------------------------------------------------- 4. ties
def test_identical_rows_across_shards_at_the_merged_cut(gpu):
    """15 copies of one row in each of three shards (45 > k' = 40, none at a shard's own cut): the lowest global rows
    win the cut.  Equal sparse rows across shards tie the same way."""
    c = Corpus([500, 333, 800], seed=21)
    proto = c.X[0].copy()
    sp_i, sp_v = c.idx[:c.nnz].copy(), c.val[:c.nnz].copy()
    copies = []
    for lo, hi in c.bounds:
        rows = lo + np.sort(c.rng.choice(hi - lo, 15, replace=False))
        copies += rows.tolist()
    for r in copies:
        c.X[r] = proto
        c.set_sparse_row(r, sp_i, sp_v)
    Q, SQ = c.queries(4)
    Q[0] = proto.astype(np.float32)
    SQ[0] = (sp_i, sp_v)
    Q[1] = proto.astype(np.float32) + 0.01 * c.rng.standard_normal(c.d).astype(np.float32)
    run_case(c, EngineConfig(top_k=20), Q, SQ, drop=0.0, case="ties/across")


def test_tie_at_one_shards_cut_is_flagged_then_repaired(gpu):
    """5000 copies of one row inside shard 1: that shard cannot prove its list, the aggregate flag says so on every
    rank, resolve_inexact repairs it, and lists, fusion and rerank then equal the oracle."""
    c = Corpus([1500, 5200, 90], seed=31)
    lo, _ = c.bounds[1]
    c.X[lo + 100:lo + 5100] = c.X[lo + 7]
    Q, SQ = c.queries(4)
    Q[0] = c.X[lo + 7].astype(np.float32)
    redone = run_case(c, EngineConfig(top_k=20), Q, SQ, want_unproven=True, case="ties/one-shard-cut")
    assert redone >= 1


def test_tie_at_cut_under_a_row_mask_is_repaired_with_the_mask(gpu):
    """The same unproven list under a row mask: the repair must search the masked rows, not the whole shard."""
    c = Corpus([900, 5200], seed=33)
    lo, _ = c.bounds[1]
    c.X[lo + 100:lo + 5100] = c.X[lo + 7]
    keep = np.ones(c.n, dtype=bool)
    keep[lo + 100:lo + 2000:2] = False
    keep[:900:3] = False
    Q, SQ = c.queries(3)
    Q[0] = c.X[lo + 7].astype(np.float32)
    run_case(c, EngineConfig(top_k=20), Q, SQ, keep=keep, want_unproven=True, case="ties/masked-cut")


# --------------------------------------------------------------------------- 6 and 7. fusion and rerank after the merge
FUSION = ["dense_sparse", "dense_sparse_domain", "dense_only", "dense_sparse_wquery", "dense_sparse_domain_wquery",
          "dense_only_wquery"]


@pytest.mark.parametrize("fusion", FUSION)
def test_fusion_after_merge(gpu, fusion):
    sizes = [120, 1, 41, 800, 0, 230]
    c = Corpus(sizes, seed=41)
    B = 7
    Q, SQ = c.queries(B)
    cfg = EngineConfig(top_k=20, use_sparse="sparse" in fusion)
    dom = Qd = weights = None
    if "domain" in fusion:
        dom = Corpus(sizes, d=32, seed=42)
        Qd = dom.queries(B)[0]
    if "wquery" in fusion:
        rng = np.random.default_rng(43)
        weights = rng.random((B, 3))
        weights[1] = 0.0                                  # every fused score 0: the rerank order is the method bonus
        weights[2] = (0.5, 0.5, 0.5)                      # equal weights: rank ties across the lists
        weights[3] = (0.7, 0.0, 0.2)
    run_case(c, cfg, Q, SQ, dom=dom, Qd=Qd, weights=weights, case=f"fusion/{fusion}")


@pytest.mark.parametrize("fusion", ["dense_sparse", "dense_sparse_domain"])
def test_top_k_beyond_distinct_fused_ids(gpu, fusion):
    """12 rows in all, top_k = 20: every list is padded and fewer ids than top_k survive the fusion."""
    sizes = [5, 0, 1, 6]
    c = Corpus(sizes, seed=51)
    B = 4
    Q, SQ = c.queries(B)
    dom = Corpus(sizes, d=32, seed=52) if "domain" in fusion else None
    Qd = dom.queries(B)[0] if dom is not None else None
    run_case(c, EngineConfig(top_k=20, rerank_top_k=8), Q, SQ, dom=dom, Qd=Qd, case=f"top_k>ids/{fusion}")


def test_rerank_ties_from_the_method_bonus(gpu):
    """Weights that make fused scores collide and let the method bonus decide: the stable list.sort order."""
    sizes = [60, 3, 90]
    c = Corpus(sizes, seed=61)
    B = 4
    Q, SQ = c.queries(B, q_nnz=30)
    weights = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.1, 0.1, 0.1], [1.0, 1.0, 0.0]])
    cfg = EngineConfig(top_k=20, rerank_top_k=20, method_bonus=0.1)
    run_case(c, cfg, Q, SQ, weights=weights, case="rerank/bonus-ties")


# --------------------------------------------------------------------------- 8. size limits
def test_kprime_max_with_eight_lists(gpu):
    """k' = HR_MAX_TOPK (top_k = 128) over 8 lists: 8 * 256 entries fit the merge's LDS staging."""
    assert merge_lds_bytes(8, nat.HR_MAX_TOPK) <= MERGE_LDS_MAX
    sizes = [600, 255, 256, 1, 0, 900, 257, 40]
    c = Corpus(sizes, seed=71)
    Q, SQ = c.queries(5, q_nnz=40)
    run_case(c, EngineConfig(top_k=nat.HR_MAX_TOPK // 2, rerank_top_k=10), Q, SQ, case="kp=256/8 lists")


@pytest.mark.parametrize("short", [False, True], ids=["full_lists", "short_lists"])
def test_merge_beyond_lds_is_refused_then_global_form(gpu, short):
    """32 lists of k' = 256 exceed kMergeLdsMax: hr_post_lists_dev refuses with HR_ELIMIT (the engine's own PostArgs);
    hr_merge_topk_dev takes merge_topk_big_kernel and yields the oracle's list — also when the lists are short and
    padding sits in the middle of the gathered buffer."""
    W, kp, B = 32, nat.HR_MAX_TOPK, 3
    assert merge_lds_bytes(W, kp) > MERGE_LDS_MAX
    rng = np.random.default_rng(81)
    sizes = (rng.integers(0, 60, W) if short else rng.integers(200, 330, W)).tolist()
    sizes[3], sizes[4], sizes[9] = 0, 1, 256
    c = Corpus(sizes, d=32, V=200, nnz=4, seed=82)
    Q, SQ = c.queries(B, q_nnz=20)
    keep = None
    if short:
        keep = rng.random(c.n) < 0.7
        lo, hi = c.bounds[10]
        keep[lo:hi] = False
    hs = c.handles()
    try:
        layout = ListPack(2, B, kp)
        gathered = torch.zeros((W, layout.nbytes), dtype=torch.uint8, device="cuda")
        dq = torch.from_numpy(Q).cuda()
        p, i_, v_, mx = pack_sparse_queries(SQ, 0.2)
        dp, di_, dv_ = torch.from_numpy(p).cuda(), torch.from_numpy(i_).cuda(), torch.from_numpy(v_).cuda()
        st = torch.cuda.current_stream().cuda_stream
        masks = []
        for r, h in enumerate(hs):
            lo, hi = c.bounds[r]
            dm = None if keep is None else torch.from_numpy(packed_mask(keep[lo:hi])).cuda()
            masks.append(dm)
            ids, scores = layout.views(gathered[r])
            fl = layout.flags_view(gathered[r])
            ptr = dm.data_ptr() if dm is not None else 0
            h.search_dense_dev(dq.data_ptr(), B, kp, ids[0].data_ptr(), scores[0].data_ptr(), fl[0].data_ptr(), ptr, st)
            h.search_sparse_dev(dp.data_ptr(), di_.data_ptr(), dv_.data_ptr(), B, len(i_), mx, kp, ids[1].data_ptr(),
                                scores[1].data_ptr(), fl[1].data_ptr(), ptr, st)
        torch.cuda.synchronize()
        for r, h in enumerate(hs):   # lists a shard could not prove: the host form, as resolve_inexact does
            ids, scores = layout.views(gathered[r])
            fl = layout.flags_view(gathered[r]).cpu().numpy()
            ptr = masks[r].data_ptr() if masks[r] is not None else 0
            for m in range(2):
                bad = np.nonzero(fl[m] == 0)[0]
                if len(bad):
                    hi_, hs_ = (h.search_dense(Q[bad], kp, None, ptr) if m == 0 else
                                h.search_sparse([SQ[i] for i in bad], kp, 0.2, None, ptr))
                    sel = torch.from_numpy(bad).cuda()
                    ids[m].index_copy_(0, sel, torch.from_numpy(hi_).cuda())
                    scores[m].index_copy_(0, sel, torch.from_numpy(hs_).cuda())
        eng = HybridSearchEngine(hs[0], EngineConfig(top_k=kp // 2), simulate_ranks=W)
        b = eng._buffers(B)
        a = eng._post_args(b, B, W, gathered)
        with pytest.raises(nat.HbmRagError) as err:
            nat.post_lists_dev(a, B, st)
        assert err.value.status == HR_ELIMIT
        m8 = None if keep is None else omask(keep)
        want = (oracle.dense_search(c.X, Q, kp, oracle.COSINE, m8), oracle.sparse_search(c.ptr, c.idx, c.val, SQ, kp, 0.2, m8))
        for m, (wi, ws) in enumerate(want):
            for k_out in (kp, 40):
                oi = torch.empty((B, k_out), dtype=torch.int64, device="cuda")
                os_ = torch.empty((B, k_out), dtype=torch.float32, device="cuda")
                sc_off, id_off, sc_stride, id_stride = layout.merge_args(m)
                nat.merge_topk_dev(gathered.data_ptr() + sc_off, gathered.data_ptr() + id_off, W, B, kp, k_out,
                                   oi.data_ptr(), os_.data_ptr(), st, score_stride=sc_stride, id_stride=id_stride)
                torch.cuda.synchronize()
                ctx = f"32 lists short={short} layout={sizes} modality={m} k_out={k_out}"
                same(oi.cpu().numpy(), wi[:, :k_out], "merge_topk_dev ids", ctx)
                same(os_.cpu().numpy(), ws[:, :k_out], "merge_topk_dev scores", ctx, np.uint32)
    finally:
        for h in hs:
            h.close()


# --------------------------------------------------------------------------- the host-merge path
def _manager(W, X16, csr, batches, V):
    from advanced_rag import MilvusIndexManager
    n = X16.shape[0]
    mgr = MilvusIndexManager(semantic_dim=X16.shape[1], sparse_dim=V, dtype="float16", enable_domain=False,
                             devices=[0] * W)
    ptr, idx, val = csr
    lo = 0
    for b in batches:  # ragged appends
        hi = min(n, lo + b)
        mgr.add_rows(X16[lo:hi].astype(np.float32), (ptr[lo:hi + 1], idx, val), ids=[f"c{r}" for r in range(lo, hi)],
                     contents=[f"text {r}" for r in range(lo, hi)], doc_id=[f"doc{r % 7}" for r in range(lo, hi)],
                     entropy=[(r % 10) / 10 for r in range(lo, hi)])
        lo = hi
    assert lo == n
    mgr.finalize()
    return mgr


HOST_CASES = {   # (W, appends, copies of one row placed in every shard)
    "w2_ragged": (2, [37, 1, 400, 13], 0),
    "w3_below_kp": (3, [5, 1, 3, 7], 0),
    "w8_one_row_shards": (8, [3, 2, 4], 0),
    "w3_ties_at_cut": (3, [300, 11, 290], 15),
}


@pytest.fixture()
def long_timeout():
    from advanced_rag.constants import RetrievalConstants
    old = RetrievalConstants.TIMEOUT_SECONDS
    RetrievalConstants.TIMEOUT_SECONDS = 60.0
    yield
    RetrievalConstants.TIMEOUT_SECONDS = old


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_host_merge_manager_matches_whole_corpus_oracle(gpu, long_timeout, case):
    from advanced_rag import HybridRetriever, RetrievalConfig
    from advanced_rag.embedding_cache import initialize_caches
    W, batches, n_copies = HOST_CASES[case]
    n, d, V, nnz = sum(batches), 48, 300, 6
    c = Corpus([n], d=d, V=V, nnz=nnz, seed=91 + W)
    X16 = c.X
    if n_copies:
        rows = np.sort(c.rng.choice(n, 3 * n_copies, replace=False))
        X16[rows] = X16[rows[0]]
        for r in rows:
            c.set_sparse_row(r, c.idx[c.ptr[rows[0]]:c.ptr[rows[0] + 1]].copy(), c.val[c.ptr[rows[0]]:c.ptr[rows[0] + 1]].copy())
    csr = (c.ptr, c.idx, c.val)
    mgr = _manager(W, X16, csr, batches, V)
    try:
        assert mgr._main.n_shards == W
        cols = {"doc_id": np.array([f"doc{r % 7}" for r in range(n)]), "chunk_id": np.array([f"c{r}" for r in range(n)]),
                "entropy": np.array([(r % 10) / 10 for r in range(n)], dtype=np.float32)}
        dead = np.zeros(n, dtype=bool)
        # tombstones: the first 25 rows of shard 0 (all of them where the shard is that small)
        for r in mgr._main.rows_of[0][:25].tolist():
            asyncio.run(mgr.delete_by_filter("semantic_index", f'chunk_id == "c{r}"'))
            dead[r] = True
        sp = {"metric_type": "IP", "params": {"drop_ratio_search": 0.2}}
        rng = np.random.default_rng(7)
        for trial in range(3):
            q = X16[int(rows[0]) if n_copies and trial == 0 else int(rng.integers(n))].astype(np.float32)
            qi = np.sort(rng.choice(V, 20, replace=False)).astype(np.int32)
            qv = np.abs(rng.standard_normal(20)).astype(np.float32)
            for flt in (None, 'doc_id == "doc3"', 'entropy >= 0.5 and doc_id != "doc1"'):
                keep = ~dead if flt is None else (oracle.filter_mask(flt, cols, n) & ~dead)
                m8 = omask(keep)
                for k in (40, 7):
                    wi, ws = oracle.dense_search(X16, q[None], k, oracle.COSINE, m8)
                    got = asyncio.run(mgr.search(q, "semantic_index", k, flt))
                    ctx = f"host/{case} layout={[len(r) for r in mgr._main.rows_of]} trial={trial} filter={flt!r} k={k}"
                    live = wi[0][wi[0] >= 0]
                    same(np.array([h["_row"] for h in got], np.int64), live, "dense rows", ctx)
                    same(np.array([h["score"] for h in got], np.float32), ws[0][:len(live)], "dense scores", ctx, np.uint32)
                    assert [h["id"] for h in got] == [f"c{r}" for r in live], ctx
                    wi, ws = oracle.sparse_search(c.ptr, c.idx, c.val, [(qi, qv)], k, 0.2, m8)
                    got = asyncio.run(mgr.search({"indices": qi.tolist(), "values": qv.tolist()}, "sparse_index", k, flt, sp))
                    live = wi[0][wi[0] >= 0]
                    same(np.array([h["_row"] for h in got], np.int64), live, "sparse rows", ctx)
                    same(np.array([h["score"] for h in got], np.float32), ws[0][:len(live)], "sparse scores", ctx, np.uint32)

        class Gen:
            def encode_semantic(self, text):
                return X16[int(text)].astype(np.float32)

            def encode_sparse(self, text):
                r = int(text)
                return {"indices": c.idx[c.ptr[r]:c.ptr[r + 1]].tolist(), "values": c.val[c.ptr[r]:c.ptr[r + 1]].tolist()}

        initialize_caches()
        mgr.embedding_generator = Gen()
        top_k = 10
        for row in (int(rows[0]) if n_copies else 0, n - 1):
            for filters, flt in ((None, None), ({"doc_id": "doc3"}, 'doc_id == "doc3"')):
                out = asyncio.run(HybridRetriever(mgr, RetrievalConfig(top_k=top_k)).retrieve(str(row), filters=filters,
                                                                                               profile_hint="default"))
                keep = ~dead if flt is None else (oracle.filter_mask(flt, cols, n) & ~dead)
                m8 = omask(keep)
                di, _ = oracle.dense_search(X16, X16[row][None].astype(np.float32), 2 * top_k, oracle.COSINE, m8)
                sq = (c.idx[c.ptr[row]:c.ptr[row + 1]], c.val[c.ptr[row]:c.ptr[row + 1]])
                si, _ = oracle.sparse_search(c.ptr, c.idx, c.val, [sq], 2 * top_k, 0.2, m8)
                fi, fs, fm = oracle.rrf(di[0][di[0] >= 0], si[0][si[0] >= 0], (), 0.7, 0.3, 0.2, 60)
                ctx = f"host retrieve/{case} row={row} filter={flt!r}"
                assert [o["id"] for o in out] == [f"c{r}" for r in fi[:top_k]], ctx
                same(np.array([o["score"] for o in out], np.float64), fs[:top_k], "retrieve scores", ctx, np.uint64)
                names = {1: "semantic", 2: "sparse"}
                assert [sorted(o["retrieval_methods"]) for o in out] == \
                    [sorted(v for bit, v in names.items() if m & bit) for m in fm[:top_k]], ctx
    finally:
        asyncio.run(mgr.close())
