"""Ad-hoc measurement (not a test): what the multi-list fusion (csrc/fuse_lists.h, hr_fuse_lists_dev) costs.

One MI355X.

  (a) kernel: B = 128 queries, lists whose ids overlap by about a half.  The new kernel at L = 2, k = 40 and at L = 3,
      k = 256 beside hr_fuse_rrf_dev / hr_fuse_scores_dev on the same lists; the new kernel alone at L = 8, k = 40 and at
      L = 16, k = 256, both modes.  One launch between two device events; the contenders alternate, window after window, in
      one process; a warm-up, then --repeats windows each; median and spread (max - min) in microseconds.
  (b) end to end: --rows x 384 fp16 rows on one shard, 64 requests in flight.  multi_search of 4 wordings (limit 40 each,
      fused to 20) against the caller's alternative without it: 4 search() calls and retrieval.rrf_rank_lists over the
      formatted hits.  The two alternate, round after round; requests/s and the p50 of a request's latency.

  python tests/probes/multi_fusion_probe.py --out profiles/multi_fusion.json [--commit ID] [--rows 1000000]
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
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("multi_fusion_probe needs a GPU: a CPU run says nothing about these numbers")

device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
B = args.batch
result = {"command": " ".join(sys.argv), "commit": args.commit, "hr_version": nat.load_library().hr_version(), "B": B,
          "repeats": args.repeats, "unit": "microseconds per launch, between device events"}


def spread(xs):
    return {"median": round(float(np.median(xs)), 2), "spread": round(float(max(xs) - min(xs)), 2),
            "min": round(float(min(xs)), 2)}


def launch_us(fns):
    """Device-event time of one call of each of `fns`, alternating between them: {name: median / spread / min}."""
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


def write():
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


rng = np.random.default_rng(args.seed)
st = cs.cuda_stream
for L, k, old in ((2, 40, True), (3, 256, True), (8, 40, False), (16, 256, False)):
    pool = L * k // 2 + k
    ids = np.stack([np.stack([rng.permutation(pool)[:k] for _ in range(L)]) for _ in range(B)]).astype(np.int64)
    sc = -np.sort(-rng.uniform(-1, 1, (B, L, k)), axis=2).astype(np.float32)
    d_ids, d_sc = torch.from_numpy(ids).to(device), torch.from_numpy(sc).to(device)
    l_ids = [d_ids[:, l].contiguous() for l in range(L)]
    l_sc = [d_sc[:, l].contiguous() for l in range(L)]
    top_k = min(L * k, 768)
    oi = torch.empty((B, top_k), dtype=torch.int64, device=device)
    os_ = torch.empty((B, top_k), dtype=torch.float64, device=device)
    om = torch.empty((B, top_k), dtype=torch.int32, device=device)
    on = torch.empty((B,), dtype=torch.int32, device=device)
    outs = (oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), st)
    w = [0.7, 0.3, 0.2][:L] if L <= 3 else [1.0] * L

    def new(mode, code=0):
        return lambda: nat.fuse_lists_dev(d_ids.data_ptr(), d_sc.data_ptr(), L, k, B, mode, 60, [code] * L, w, 0, top_k, *outs)

    fns = {"lists_rrf": new(0), "lists_weighted_code0": new(1, 0), "lists_weighted_code3": new(1, 3)}
    if old:
        w3 = w + [0.0] * (3 - L)
        a = []
        for l in range(3):
            a += [l_ids[l].data_ptr(), k] if l < L else [0, 0]
        fns["three_list_rrf"] = lambda a=a, w3=w3: nat.fuse_rrf_dev(*a, B, w3[0], w3[1], w3[2], 60, top_k, *outs)

        def scores(code):
            b = []
            for l in range(3):
                b += [l_ids[l].data_ptr(), l_sc[l].data_ptr(), k, code] if l < L else [0, 0, 0, 0]
            return lambda: nat.fuse_scores_dev(*b, B, w3[0], w3[1], w3[2], 0, top_k, *outs)
        fns["three_list_scores_code0"] = scores(0)
        fns["three_list_scores_code3"] = scores(3)
    result[f"kernel_L{L}_k{k}"] = launch_us(fns)
    print(f"kernel_L{L}_k{k}", json.dumps(result[f"kernel_L{L}_k{k}"]), flush=True)
    write()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def end_to_end():
    from advanced_rag import MilvusIndexManager
    from advanced_rag.multi_search import RRFRanker, SearchRequest
    from advanced_rag.retrieval import rrf_rank_lists
    n, d, W, flight = args.rows, 384, 4, 64
    mgr = MilvusIndexManager(semantic_dim=d, sparse_dim=512, enable_domain=False)
    step = 1 << 17
    for lo in range(0, n, step):
        mgr.add_rows_synthetic(rng.standard_normal((min(step, n - lo), d), dtype=np.float32).astype(np.float16))
    mgr.finalize()
    Q = rng.standard_normal((flight, W, d), dtype=np.float32)

    async def fused(i):
        t0 = time.perf_counter()
        hits = await mgr.multi_search([SearchRequest(Q[i, j], "semantic_index", 40) for j in range(W)], RRFRanker(), 20)
        return time.perf_counter() - t0, [h["id"] for h in hits]

    async def by_hand(i):
        t0 = time.perf_counter()
        lists = await asyncio.gather(*[mgr.search(Q[i, j], "semantic_index", 40) for j in range(W)])
        ranked = rrf_rank_lists([[h["id"] for h in hits] for hits in lists], [1.0] * W, 60)[:20]
        return time.perf_counter() - t0, [r[0] for r in ranked]

    async def round_of(fn):
        t0 = time.perf_counter()
        out = await asyncio.gather(*[fn(i) for i in range(flight)])
        return time.perf_counter() - t0, [o[0] for o in out], [o[1] for o in out]

    async def run():
        stats = {"multi_search": ([], []), "four_searches_and_host_rrf": ([], [])}
        fns = {"multi_search": fused, "four_searches_and_host_rrf": by_hand}
        same = None
        for r in range(args.rounds + 2):
            answers = {}
            for name, fn in fns.items():
                wall, lat, ids = await round_of(fn)
                answers[name] = ids
                if r >= 2:             # two warm-up rounds
                    stats[name][0].append(wall)
                    stats[name][1].extend(lat)
            same = answers["multi_search"] == answers["four_searches_and_host_rrf"]
        return stats, same

    stats, same = asyncio.run(run())
    out = {"rows": n, "dim": d, "wordings": W, "in_flight": flight, "rounds": args.rounds, "same_ids": bool(same)}
    for name, (walls, lat) in stats.items():
        out[name] = {"requests_per_s": round(flight * len(walls) / sum(walls), 1),
                     "round_ms": spread([w * 1e3 for w in walls]), "p50_ms": round(float(np.percentile(lat, 50)) * 1e3, 3),
                     "p95_ms": round(float(np.percentile(lat, 95)) * 1e3, 3)}
    out["front"] = {k: v for k, v in mgr._front.stats.items() if k.endswith("launches") or k in ("rounds", "requests")}
    asyncio.run(mgr.close())
    return out


try:
    result["end_to_end"] = end_to_end()
except Exception as e:      # the kernel figures above stand on their own
    result["end_to_end"] = {"error": f"{type(e).__name__}: {e}"}
print(json.dumps(result, indent=1))
write()
