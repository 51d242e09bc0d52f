"""Ad-hoc measurement (not a test): what the boost ranker costs (csrc/boost.h, advanced_rag/boost.py).

One MI355X.

  (a) hr_boost_rerank_dev alone at B = 128, k_in = 40 / 256 / 768, with 1 and with 8 functions per query, with and without
      draws (fp64 scores, identity norm, whole list out, masks over 1M rows, different masks per function), alternating
      with hr_decay_rerank_dev (linear curve) on the same lists in the same windows: the same counting sort with one
      column load per entry instead of up to eight scattered byte loads.  One launch between two device events; the ratio
      of the medians is reported.
  (b) end to end on a one-shard manager (--rows x --dim), 64 requests in flight: search(ranker=FunctionScore(...,
      candidates=80)) against the plain search(top_k=80); retrieve() with and without RetrievalConfig(boost=...).

The contenders alternate, window after window, in one process; a warm-up, then --repeats windows each; the median, the
spread (max - min) and the minimum are reported.

  python tests/probes/boost_probe.py --out profiles/boost_ranker.json [--commit ID]
"""
import argparse
import asyncio
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=101)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--mask-rows", type=int, default=1_000_000)
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--in-flight", type=int, default=64)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402
from advanced_rag.boost import BoostRanker, FunctionScore   # noqa: E402
from advanced_rag.constants import RetrievalConstants   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("boost_probe needs a GPU: a CPU run says nothing about these numbers")

device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
B = args.batch
rng = np.random.default_rng(args.seed)
result = {"command": " ".join(sys.argv), "commit": args.commit, "hr_version": nat.load_library().hr_version(), "B": B,
          "repeats": args.repeats}


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "min": round(float(min(xs)), 3)}


def launch_us(fns):
    """Device-event time of one call of each of `fns`, alternating between them: {name: median / spread / min} in us."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    cs.synchronize()
    out = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.repeats):
        for name, fn in fns.items():
            e0.record(cs)
            fn()
            e1.record(cs)
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: spread(v) for k, v in out.items()}


# ---- (a) the kernel alone --------------------------------------------------------------------------------------------------
st = cs.cuda_stream
M = args.mask_rows
masks = [torch.from_numpy(rng.integers(0, 256, (M + 7) // 8, dtype=np.uint8)).to(device) for _ in range(nat.HR_MAX_BOOST_FUNCS)]
keys = torch.from_numpy(rng.integers(0, M // 10, M).astype(np.int64)).to(device)
col = torch.from_numpy(rng.uniform(0, 60 * 86400.0, M)).to(device)
result["kernel_unit"] = "microseconds per launch, between device events"
result["mask_rows"] = M
for k in (40, 256, 768):
    ids = torch.from_numpy(np.stack([rng.choice(M, k, replace=False) for _ in range(B)]).astype(np.int64)).to(device)
    sc = torch.from_numpy(-np.sort(-rng.uniform(0, 0.03, (B, k)), axis=1)).to(device)
    n = torch.full((B,), k, dtype=torch.int32, device=device)
    pos = torch.empty((B, k), dtype=torch.int32, device=device)
    oi = torch.empty((B, k), dtype=torch.int64, device=device)
    os_ = torch.empty((B, k), dtype=torch.float64, device=device)
    om = torch.empty((B, k), dtype=torch.int32, device=device)
    on = torch.empty((B,), dtype=torch.int32, device=device)
    fns, keep = {}, []
    for n_funcs in (1, 8):
        for draws in (False, True):
            rec = np.zeros((B, n_funcs), dtype=nat.BOOST_FUNC_DTYPE)
            for q in range(B):
                for j in range(n_funcs):
                    rec[q, j] = (masks[(q + j) % len(masks)].data_ptr(), keys.data_ptr() if draws and j % 2 == 0 else 0, M,
                                 M if draws and j % 2 == 0 else 0, 0.5 + 0.25 * j, 1000 * q + j,
                                 nat.HR_BOOST_ACTIVE | (nat.HR_BOOST_RANDOM if draws else 0), 0)
            d_f = torch.from_numpy(rec.view(np.uint8).reshape(B, -1)).to(device)
            keep.append(d_f)
            fns[f"boost_{n_funcs}f" + ("_draws" if draws else "")] = (lambda d_f=d_f, n_funcs=n_funcs: nat.boost_rerank_dev(
                ids.data_ptr(), sc.data_ptr(), True, n.data_ptr(), B, k, d_f.data_ptr(), n_funcs, 0, 1, 0, -1, False, k,
                pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), st))
    p = np.zeros(B, dtype=nat.DECAY_QUERY_DTYPE)
    for q in range(B):
        p[q] = (float(rng.uniform(0, 60 * 86400.0)), 3600.0, 0.5 / (10 * 86400.0), nat.HR_DECAY_LINEAR, 0)
    d_p = torch.from_numpy(p.view(np.uint8).reshape(B, -1)).to(device)
    fns["decay_linear"] = lambda: nat.decay_rerank_dev(
        ids.data_ptr(), sc.data_ptr(), True, n.data_ptr(), B, k, col.data_ptr(), nat.HR_COL_F64, M, 0, d_p.data_ptr(), -1, k,
        pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(), st)
    got = launch_us(fns)
    base = got["decay_linear"]["median"]
    got["ratio_to_decay_linear"] = {name: round(v["median"] / base, 3) for name, v in got.items() if name != "decay_linear"}
    result[f"kernel_k{k}"] = got

# ---- (b) end to end --------------------------------------------------------------------------------------------------------
N, D, V, TOP_K, W, IN_FLIGHT = args.rows, args.dim, 2048, 20, 80, args.in_flight
X = rng.standard_normal((N, D)).astype(np.float16)
nnz = 8
idx = np.sort(rng.integers(0, V, (N, nnz)), axis=1).astype(np.int32)
idx += np.arange(nnz, dtype=np.int32)[None, :]          # strictly ascending within a row
val = (np.abs(rng.standard_normal((N, nnz))) + 0.1).astype(np.float32)
csr = (np.arange(N + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
Q = rng.standard_normal((IN_FLIGHT, D)).astype(np.float32)
SQ = [(np.sort(rng.choice(V, 30, replace=False)).astype(np.int32), (np.abs(rng.standard_normal(30)) + 0.5).astype(np.float32))
      for _ in range(IN_FLIGHT)]


class Gen:
    run_inline = True

    def encode_semantic(self, text):
        return Q[int(text.rsplit("q", 1)[1])]

    def encode_sparse(self, text):
        qi, qv = SQ[int(text.rsplit("q", 1)[1])]
        return {"indices": qi.tolist(), "values": qv.astype(float).tolist()}

    def encode_domain(self, text, domain=None):
        return np.zeros(8, np.float32)


mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V + nnz, enable_domain=False)
mgr.add_rows(X, csr, contents=[("manual " if r % 4 == 0 else "forum ") + f"error{r % 50}" for r in range(N)],
             token_count=[int(t) for t in rng.integers(10, 400, N)])
mgr.finalize()
mgr.embedding_generator = Gen()
RetrievalConstants.TIMEOUT_SECONDS = 60.0
spec = FunctionScore(BoostRanker('TEXT_MATCH(content, "manual")', 1.5), BoostRanker("token_count < 30", 0.5),
                     BoostRanker('TEXT_MATCH(content, "error7")', 2.0), BoostRanker("chunk_index in [0, 1]", 1.1),
                     BoostRanker(None, 0.1, {"seed": 42, "field": "doc_id"}), function_mode="sum", candidates=W)
retr_plain = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K))
retr_boost = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, boost=spec))


async def burst(make):
    return await asyncio.gather(*(make(i) for i in range(IN_FLIGHT)))


contenders = {
    "search_plain_topk_W": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", W))),
    "search_ranker": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", TOP_K, ranker=spec))),
    "retrieve_plain": lambda: asyncio.run(burst(lambda i: retr_plain.retrieve(f"plain statement q{i}", profile_hint="default"))),
    "retrieve_boost": lambda: asyncio.run(burst(lambda i: retr_boost.retrieve(f"plain statement q{i}", profile_hint="default"))),
}
t0 = time.perf_counter()
contenders["search_ranker"]()          # the first use: four masks are evaluated, the doc_id keys are built and mirrored
first = time.perf_counter() - t0
for fn in contenders.values():
    fn()
times = {k: [] for k in contenders}
for _ in range(args.rounds):
    for name, fn in contenders.items():
        t0 = time.perf_counter()
        fn()
        times[name].append((time.perf_counter() - t0) * 1e3)
result["end_to_end"] = {"unit": f"milliseconds per burst of {IN_FLIGHT} concurrent requests, wall clock", "rows": N, "dim": D,
                        "top_k": TOP_K, "W": W, "functions": len(spec.functions), "rounds": args.rounds,
                        **{k: spread(v) for k, v in times.items()}}
result["first_use"] = {"first_ranked_burst_seconds": round(first, 3), "rows": N, "group_key_bytes": mgr._group_keys_on_device().nbytes}
result["front_stats"] = {k: v for k, v in mgr._front.stats.items() if k.endswith("launches") or k == "requests"}
asyncio.run(mgr.close())

print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
