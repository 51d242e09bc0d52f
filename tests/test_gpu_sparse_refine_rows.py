"""The sparse refine (refine_sparse_chain, csrc/sparse.h) held to the oracle where its own control flow can go wrong:
rows of 0 .. 2500 entries with the matches at the edges of its 64-entry segments, scores that depend on the order of the
fp64 additions, vocabularies wide enough for the 32768-bit membership filter to alias, and rows as the BM25 encoder makes
them.  The cases and the reasoning behind them are in tests/refine_rows_data.py; tests/test_refine_rows_data.py shows on
the CPU that each of them can fail.

Every case goes through the C ABI twice: the host form (every list: ids and score bits equal to the oracle's) and the
device form.  The constructed cases use non-negative weights and keep 1 % between consecutive distinct scores, far
above the scan's bound, so the device form must PROVE every list (flag 1) and every list is compared; only the one signed
query of case C and the BM25 lists of case D (real scores may tie) are held to "flag 1 implies equal".  Each case is
repeated under the debug settings of test_gpu_proof_edges.VARIANTS (one test per case and setting), with batches of 63
and 64 queries: the sizes on either side of the fused finishing kernel's default threshold (finish_fused_ok,
csrc/hbmrag.hip; tests/test_refine_rows_data.py reads the threshold from that file).  The oracle's lists are computed once
per (case, batch, k) and shared by every variant and batch size."""
import numpy as np
import pytest

import oracle
import refine_rows_data as R
from advanced_rag import _native as nat
from advanced_rag.engine import EngineConfig, HybridSearchEngine, pack_sparse_queries
from test_gpu_proof_edges import DEBUG_KEYS, VARIANTS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VARIANT_IDS = ["default", "finish_chain", "finish_fused", "no_trim", "group_16", "group_64_fused"]
assert len(VARIANT_IDS) == len(VARIANTS)
each_variant = pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)

_cases = {}
_oracle = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = (R.case_a() if name == "A" else R.case_a(masked=True) if name == "A_masked" else R.case_b()
                        if name == "B" else R.case_d() if name == "D" else R.case_c(int(name[2:])))
    return _cases[name]


def oracle_lists(case, batch, k):
    """The oracle's lists of the batch's distinct queries: computed once per (case, batch, k), shared by every variant."""
    key = (case.name, batch.name, k)
    if key not in _oracle:
        ids, sc = oracle.sparse_search(case.indptr, case.idx, case.val, batch.queries, k, 0.0, case.mask)
        ids.setflags(write=False)
        sc.setflags(write=False)
        _oracle[key] = (ids, sc)
    return _oracle[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def options():
    def set_(settings):
        for key in DEBUG_KEYS:
            nat.debug_option(key, 0)
        for key, value in settings:
            nat.debug_option(key, value)
    yield set_
    for key in DEBUG_KEYS:
        nat.debug_option(key, 0)


def sparse_dev(h, queries, k, d_mask):
    ptr, qi, qv, mx = pack_sparse_queries(queries, 0.0, h.sparse_dim)
    B = len(queries)
    dev = torch.device("cuda:0")
    tp, ti, tv = (torch.from_numpy(a).to(dev) for a in (ptr, qi, qv))
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    sc = torch.empty((B, k), dtype=torch.float32, device=dev)
    fl = torch.full((B,), 7, dtype=torch.int32, device=dev)
    h.search_sparse_dev(tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), B, int(ptr[-1]), mx, k, ids.data_ptr(), sc.data_ptr(),
                        fl.data_ptr(), d_mask.data_ptr() if d_mask is not None else 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()


def check_batch(h, case, batch, k, B, d_mask, must_prove):
    queries, pick = R.batch_of(batch, B)
    o_ids, o_sc = oracle_lists(case, batch, k)
    o_ids, o_sc = o_ids[pick], o_sc[pick]
    where = f"{case.name} / {batch.name} / k={k} / B={B}"
    ids, sc = h.search_sparse(queries, k, 0.0, rowmask=case.mask)
    bad = np.nonzero((ids != o_ids).any(axis=1) | (bits(sc) != bits(o_sc)).any(axis=1))[0]
    assert bad.size == 0, f"{where}: host form, queries {bad[:6]} (distinct {[pick[b] for b in bad[:6]]}): " \
                          f"{ids[bad[0]][:6]} {sc[bad[0]][:6]} vs oracle {o_ids[bad[0]][:6]} {o_sc[bad[0]][:6]}"
    d_ids, d_sc, fl = sparse_dev(h, queries, k, d_mask)
    assert set(np.unique(fl)) <= {0, 1}, fl
    if must_prove:
        held = np.array([pick[b] not in batch.signed for b in range(B)])
        assert fl[held].min() == 1, f"{where}: device form left queries {np.nonzero(held & (fl == 0))[0][:8]} unproven"
    ok = fl == 1
    bad = np.nonzero(ok & ((d_ids != o_ids).any(axis=1) | (bits(d_sc) != bits(o_sc)).any(axis=1)))[0]
    assert bad.size == 0, f"{where}: device form, queries {bad[:6]} flagged exact: {d_ids[bad[0]][:6]} {d_sc[bad[0]][:6]} " \
                          f"vs oracle {o_ids[bad[0]][:6]} {o_sc[bad[0]][:6]}"


def run_case(options, variant, case, sizes=R.BATCH_SIZES, must_prove=True):
    d_mask = torch.from_numpy(case.mask).cuda() if case.mask is not None else None
    options(variant)
    h = nat.ShardHandle(0, sparse_dim=case.V)     # HR_DEBUG_GROUP_ROWS applies to handles created afterwards
    try:
        h.add_sparse(case.indptr, case.idx, case.val)
        h.finalize()
        for batch in case.batches:
            for k in batch.ks:
                for B in sizes or (len(batch.queries),):
                    check_batch(h, case, batch, k, B, d_mask, must_prove)
    finally:
        h.close()


@each_variant
def test_a_row_lengths_and_placements(gpu, options, variant):
    run_case(options, variant, get_case("A"))


@each_variant
def test_a_with_a_row_mask(gpu, options, variant):
    run_case(options, variant, get_case("A_masked"))


@each_variant
def test_b_entry_order(gpu, options, variant):
    run_case(options, variant, get_case("B"))


@each_variant
@pytest.mark.parametrize("V", R.C_VOCABS)
def test_c_wide_vocabularies(gpu, options, variant, V):
    run_case(options, variant, get_case(f"C_{V}"))


@each_variant
def test_d_bm25_rows(gpu, options, variant):
    run_case(options, variant, get_case("D"), sizes=None, must_prove=False)


@pytest.mark.parametrize("B", [7, 35], ids=["chain", "fused_pair"])
def test_d_bm25_rows_beside_a_dense_collection(gpu, B):
    """The same rows through HybridSearchEngine: 35 queries of two modalities take the fused finishing kernel, 7 the
    multi-launch chain; either way the sparse modality's list is the oracle's, ids and score bits: every list flagged
    exact as it comes back, and every list after resolve_inexact."""
    case = get_case("D")
    batch = case.batches[0]
    n, d = R.D_DOCS, 32
    rng = np.random.default_rng(43)
    X = rng.standard_normal((n, d)).astype(np.float16)
    SQ = [batch.queries[i % len(batch.queries)] for i in range(B)]
    Q = rng.standard_normal((B, d)).astype(np.float32)
    h = nat.ShardHandle(d, nat.HR_F16, nat.HR_METRIC_COSINE, case.V)
    try:
        h.add_dense(X)
        h.add_sparse(case.indptr, case.idx, case.val)
        h.finalize()
        cfg = EngineConfig(top_k=20)
        eng = HybridSearchEngine(h, cfg)
        out = eng.search(torch.from_numpy(Q).cuda(), eng.upload_sparse(pack_sparse_queries(SQ, 0.0, case.V)))
        torch.cuda.synchronize()
        o_ids, o_sc = oracle_lists(case, batch, 2 * cfg.top_k)
        pick = [i % len(batch.queries) for i in range(B)]
        o_ids, o_sc = o_ids[pick], o_sc[pick]

        def unequal():     # the queries whose sparse list differs from the oracle's in an id or in a score bit
            si, ss = out["ids"][1].cpu().numpy(), out["scores"][1].cpu().numpy()
            return (si != o_ids).any(axis=1) | (bits(ss) != bits(o_sc)).any(axis=1)

        flags = out["flags"].cpu().numpy()
        assert set(np.unique(flags)) <= {0, 1}, flags
        bad = np.nonzero((flags[1] == 1) & unequal())[0]
        assert bad.size == 0, f"queries {bad[:6]} flagged exact: {out['ids'][1][bad[0]][:6]} {out['scores'][1][bad[0]][:6]} " \
                              f"vs oracle {o_ids[bad[0]][:6]} {o_sc[bad[0]][:6]}"
        eng.resolve_inexact(out, Q, SQ, 0.0)
        torch.cuda.synchronize()
        bad = np.nonzero(unequal())[0]
        assert bad.size == 0, f"queries {bad[:6]} after resolve_inexact: {out['ids'][1][bad[0]][:6]} " \
                              f"{out['scores'][1][bad[0]][:6]} vs oracle {o_ids[bad[0]][:6]} {o_sc[bad[0]][:6]}"
    finally:
        h.close()
