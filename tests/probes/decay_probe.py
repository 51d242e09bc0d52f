"""Ad-hoc measurement (not a test): what the decay ranker costs (csrc/decay.h, advanced_rag/decay.py).

One MI355X.

  (a) hr_decay_rerank_dev alone at B = 128, k_in = 40 / 256 / 768, for each curve (fp64 scores, float64 column, identity
      norm, whole list out), alternating with hr_rerank_linear_dev on the same lists where that kernel takes them
      (k_in <= HR_MAX_TOPK): the same counting sort without the decay arithmetic.  One launch between two device events.
  (b) end to end on a one-shard manager (--rows x --dim, timestamps over 60 days), 64 requests in flight:
      search(ranker=...) against the plain search(top_k=W); retrieve() with and without RetrievalConfig(decay=...); and the
      reference-style host recency parse (20 datetime.fromisoformat calls per request) that a freshness ranking on the
      host costs, on one thread.
  (c) first use: seconds of host parsing per 1M rows of the epoch column, and the bytes of its HBM mirror.

The contenders alternate, window after window, in one process; a warm-up, then --repeats windows each; the median and the
spread (max - min) are reported.

  python tests/probes/decay_probe.py --out profiles/decay_ranker.json [--commit ID]
"""
import argparse
import asyncio
import json
import math
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=101)
ap.add_argument("--batch", type=int, default=128)
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
from advanced_rag.columns import PayloadColumns   # noqa: E402
from advanced_rag.constants import RetrievalConstants   # noqa: E402
from advanced_rag.decay import DecayRanker   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("decay_probe needs a GPU: a CPU run says nothing about these numbers")

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
n_col = 100_000
col = torch.from_numpy(rng.uniform(0, 60 * 86400.0, n_col)).to(device)
result["kernel_unit"] = "microseconds per launch, between device events"
for k in (40, 256, 768):
    ids = torch.from_numpy(np.stack([rng.choice(n_col, k, replace=False) for _ in range(B)]).astype(np.int64)).to(device)
    sc = torch.from_numpy(-np.sort(-rng.uniform(0, 0.03, (B, k)), axis=1)).to(device)
    n = torch.full((B,), k, dtype=torch.int32, device=device)
    meth = torch.ones((B, k), dtype=torch.int32, device=device)
    pos = torch.empty((B, k), dtype=torch.int32, device=device)
    oi = torch.empty((B, k), dtype=torch.int64, device=device)
    os_, oo = torch.empty((B, k), dtype=torch.float64, device=device), torch.empty((B, k), dtype=torch.float64, device=device)
    on = torch.empty((B,), dtype=torch.int32, device=device)
    fns = {}
    keep = []
    for func, name in enumerate(("gauss", "exp", "linear")):
        p = np.zeros(B, dtype=nat.DECAY_QUERY_DTYPE)
        scale = 10 * 86400.0
        coef = (math.log(0.5) / (scale * scale), math.log(0.5) / scale, 0.5 / scale)[func]
        for q in range(B):
            p[q] = (float(rng.uniform(0, 60 * 86400.0)), 3600.0, coef, func, 0)
        d_p = torch.from_numpy(p.view(np.uint8).reshape(B, -1)).to(device)
        keep.append(d_p)
        fns["decay_" + name] = (lambda d_p=d_p: nat.decay_rerank_dev(
            ids.data_ptr(), sc.data_ptr(), True, n.data_ptr(), B, k, col.data_ptr(), nat.HR_COL_F64, n_col, 0, d_p.data_ptr(), -1, k,
            pos.data_ptr(), oi.data_ptr(), os_.data_ptr(), on.data_ptr(), st))
    if k <= nat.HR_MAX_TOPK:
        L = nat.load_library()
        vp = nat._vp
        fns["rerank_linear"] = lambda: L.hr_rerank_linear_dev(vp(ids.data_ptr()), vp(sc.data_ptr()), vp(meth.data_ptr()), vp(n.data_ptr()),
                                                              None, B, k, 1.0, 0.01, 0.0, k, vp(oi.data_ptr()), vp(os_.data_ptr()),
                                                              vp(oo.data_ptr()), vp(st))
    result[f"kernel_k{k}"] = launch_us(fns)
    if k > nat.HR_MAX_TOPK:
        result[f"kernel_k{k}"]["rerank_linear"] = "not taken: hr_rerank_linear_dev stops at HR_MAX_TOPK"

# ---- (c) first use of the epoch column (host) ---------------------------------------------------------------------------------
T0 = datetime(2024, 5, 1)
n_parse = 1_000_000
stamps_1m = [(T0 - timedelta(seconds=int(s))).isoformat() for s in rng.integers(0, 60 * 86400, n_parse)]
cols = PayloadColumns()
cols["timestamp"].extend(stamps_1m)
t0 = time.perf_counter()
cols.epoch_seconds()
result["first_use"] = {"host_parse_seconds_per_1M_rows": round(time.perf_counter() - t0, 3), "mirror_bytes_per_row": 8}
del cols

# ---- (b) end to end --------------------------------------------------------------------------------------------------------
N, D, V, TOP_K, W, IN_FLIGHT = args.rows, args.dim, 2048, 20, 80, args.in_flight
X = rng.standard_normal((N, D)).astype(np.float16)
nnz = 8
idx = np.sort(rng.integers(0, V, (N, nnz)), axis=1).astype(np.int32)
idx += np.arange(nnz, dtype=np.int32)[None, :]          # strictly ascending within a row
val = (np.abs(rng.standard_normal((N, nnz))) + 0.1).astype(np.float32)
csr = (np.arange(N + 1, dtype=np.int64) * nnz, idx.reshape(-1), val.reshape(-1))
stamps = stamps_1m[:N]
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
mgr.add_rows(X, csr, timestamp=stamps)
mgr.finalize()
mgr.embedding_generator = Gen()
RetrievalConstants.TIMEOUT_SECONDS = 60.0
ranker = DecayRanker("timestamp", "gauss", (T0 - timedelta(days=7)).isoformat(), 10 * 86400.0, 3600.0, candidates=W)
retr_plain = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K))
retr_decay = HybridRetriever(mgr, RetrievalConfig(top_k=TOP_K, decay=ranker))


def host_recency_parse():
    """The reference-style recency of a request's 20 hits: datetime.fromisoformat per hit, on one thread."""
    now = datetime.utcnow()
    for i in range(IN_FLIGHT):
        for s in stamps[20 * i:20 * i + 20]:
            1.0 / (1.0 + max(0.0, (now - datetime.fromisoformat(s)).total_seconds() / 86400.0))


async def burst(make):
    return await asyncio.gather(*(make(i) for i in range(IN_FLIGHT)))


contenders = {
    "search_plain_topk_W": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", W))),
    "search_ranker": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", TOP_K, ranker=ranker))),
    "retrieve_plain": lambda: asyncio.run(burst(lambda i: retr_plain.retrieve(f"plain statement q{i}", profile_hint="default"))),
    "retrieve_decay": lambda: asyncio.run(burst(lambda i: retr_decay.retrieve(f"plain statement q{i}", profile_hint="default"))),
    "host_recency_parse_20_hits": host_recency_parse,
}
t0 = time.perf_counter()
contenders["search_ranker"]()          # the first use: the epoch column is parsed and mirrored
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
                        "top_k": TOP_K, "W": W, "rounds": args.rounds, **{k: spread(v) for k, v in times.items()}}
result["first_use"].update(first_ranked_burst_seconds=round(first, 3), rows=N,
                           mirror_bytes=mgr._decay_columns_on_device().nbytes,
                           host_build_s=round(mgr._decay_columns_on_device().stats["host_build_s"], 3))
result["front_stats"] = {k: v for k, v in mgr._front.stats.items() if k.endswith("launches") or k == "requests"}
asyncio.run(mgr.close())

print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
