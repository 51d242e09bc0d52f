"""Which profiling phase every launch of a search is booked under (hr_last_kernel_ms): bench.py's roofline reads
dense_scan / sparse_scan at level 1, the probes read the finishing phases at level 2.  Launch counts per entry point, for
the multi-launch finishing chain, the fused finishing kernel and the scans-only level."""
import pytest

from advanced_rag import _native as nat
from advanced_rag.engine import pack_sparse_queries
from test_gpu_engine import corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, V, NNZ, B, K = 20000, 128, 1000, 12, 9, 40

DENSE_SCAN = {"prep": 1, "dense_scan": 1}
SPARSE_SCAN = {"sparse_scan": 1}          # the sparse query prep books nothing
DENSE_CHAIN = {"group_select": 1, "refine": 1, "topk": 1}
SPARSE_CHAIN = {"sparse_select": 1, "sparse_refine": 1, "sparse_topk": 1}
# both modalities in one finish: the merged launches on the dense phases, each refine on its own
PAIR_CHAIN = {"group_select": 1, "refine": 1, "sparse_refine": 1, "topk": 1}


def _sum(*parts):
    out = {}
    for p in parts:
        for name, c in p.items():
            out[name] = out.get(name, 0) + c
    return out


def _fused(n):
    return {"finish_fused": n}


# (profiling level, HR_DEBUG_FINISH_MODE) -> entry point -> launches per phase; phases not named are 0
EXPECTED = {
    (2, 1): {"dense": _sum(DENSE_SCAN, DENSE_CHAIN),
             "sparse": _sum(SPARSE_SCAN, SPARSE_CHAIN),
             "two_phase": _sum(DENSE_SCAN, SPARSE_SCAN, PAIR_CHAIN),
             "hybrid": _sum(DENSE_SCAN, DENSE_CHAIN, SPARSE_SCAN, SPARSE_CHAIN)},
    (2, 2): {"dense": _sum(DENSE_SCAN, _fused(1)),
             "sparse": _sum(SPARSE_SCAN, _fused(1)),
             "two_phase": _sum(DENSE_SCAN, SPARSE_SCAN, _fused(1)),   # one launch for both sides
             "hybrid": _sum(DENSE_SCAN, SPARSE_SCAN, _fused(2))},
}
SCANS_ONLY = {"dense": {"dense_scan": 1}, "sparse": {"sparse_scan": 1},
              "two_phase": {"dense_scan": 1, "sparse_scan": 1}, "hybrid": {"dense_scan": 1, "sparse_scan": 1}}
for mode in (0, 1, 2):
    EXPECTED[(1, mode)] = SCANS_ONLY


@pytest.fixture(scope="module")
def shard(gpu):
    X, ptr, idx, val, Q, SQ = corpus(N, D, V, NNZ, B, seed=N + B)
    h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    h.add_dense(X)
    h.add_sparse(ptr, idx, val)
    h.finalize()
    p, i_, v_, mx = pack_sparse_queries(SQ, 0.2)
    dev = dict(q=torch.from_numpy(Q).cuda(), p=torch.from_numpy(p).cuda(), i=torch.from_numpy(i_).cuda(),
               v=torch.from_numpy(v_).cuda(), nnz=len(i_), mx=mx,
               ids=torch.empty((2, B, K), dtype=torch.int64, device="cuda"),
               sc=torch.empty((2, B, K), dtype=torch.float32, device="cuda"),
               fl=torch.empty((2, B), dtype=torch.int32, device="cuda"))
    yield h, dev
    h.close()


def _calls(h, t):
    st = torch.cuda.current_stream().cuda_stream
    q, sp = t["q"].data_ptr(), (t["p"].data_ptr(), t["i"].data_ptr(), t["v"].data_ptr())
    out = (t["ids"].data_ptr(), t["sc"].data_ptr(), t["fl"].data_ptr())

    def two_phase():
        h.hybrid_scan_dev(q, *sp, B, t["nnz"], t["mx"], K, 0, st)      # the slot is not prepared: prep + scans
        h.hybrid_finish_dev(q, *sp, B, t["mx"], K, 0, *out, st)

    return {"dense": lambda: h.search_dense_dev(q, B, K, *out, 0, st),
            "sparse": lambda: h.search_sparse_dev(*sp, B, t["nnz"], t["mx"], K, *out, 0, st),
            "two_phase": two_phase,
            "hybrid": lambda: h.search_hybrid_dev(q, *sp, B, t["nnz"], t["mx"], K, *out, 0, st)}


@pytest.mark.parametrize("level,mode", sorted(EXPECTED))
def test_launches_are_booked_under_their_phases(shard, level, mode):
    h, t = shard
    try:
        h.set_profiling(level)
        nat.debug_option(nat.HR_DEBUG_FINISH_MODE, mode)
        for name, call in _calls(h, t).items():
            h.kernel_ms()                      # clears the spans
            call()
            torch.cuda.synchronize()
            got = {phase: n for phase, (_, n) in h.kernel_ms().items()}
            want = {phase: EXPECTED[(level, mode)][name].get(phase, 0) for phase in nat.PHASE_NAMES}
            assert got == want, (name, level, mode)
    finally:
        nat.debug_option(nat.HR_DEBUG_FINISH_MODE, 0)
        h.set_profiling(0)
