"""Ad-hoc measurement (not a test): what the late-interaction rerank costs (csrc/maxsim.h, advanced_rag/maxsim.py).

One MI355X.

  (a) hr_maxsim_rerank_dev alone at B = 128, k_in = 80 / 256, Tq = 32, rows of 64 tokens, dim = 64 / 128, whole list out;
      one launch between two device events.  Beside every figure its two floors for the same call: the gathered token
      bytes (B * k_in * T_r * dim * 2) at the float4 copy rate (6.29 TB/s) and 2 * B * k_in * Tq * T_r * dim FLOP at the
      measured fp32 matrix rate (155 TFLOP/s), and the ratio of the measured time to the larger floor.  The store is far
      larger than the Infinity Cache and the ids of a list are drawn without repetition.
  (b) end to end on a one-shard manager (--rows x --dim, --tokens token vectors of --token-dim per row), 64 requests in
      flight: search(ranker=MaxSimRanker(candidates=80)) beside the plain search(top_k=80).
  (c) the HBM the mirror holds: by construction 2 * token_dim bytes per token plus 8 per row.

The contenders alternate, window after window, in one process; a warm-up, then --repeats windows each; the median and the
spread (max - min) are reported.

  python tests/probes/maxsim_probe.py --out profiles/maxsim.json [--commit ID]
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
ap.add_argument("--repeats", type=int, default=51)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=384)
ap.add_argument("--tokens", type=int, default=8)
ap.add_argument("--token-dim", type=int, default=64)
ap.add_argument("--in-flight", type=int, default=64)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import MilvusIndexManager   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402
from advanced_rag.maxsim import MaxSimRanker   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("maxsim_probe needs a GPU: a CPU run says nothing about these numbers")

COPY_BYTES_PER_S, F32_MATRIX_FLOPS = 6.29e12, 155e12
device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
B = args.batch
rng = np.random.default_rng(args.seed)
result = {"command": " ".join(sys.argv), "commit": args.commit, "hr_version": nat.load_library().hr_version(), "B": B,
          "repeats": args.repeats, "floors": {"copy_bytes_per_s": COPY_BYTES_PER_S, "f32_matrix_flops": F32_MATRIX_FLOPS}}


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "min": round(float(min(xs)), 3)}


def launch_us(fns):
    """Device-event time of one call of each of `fns`, alternating between them: {name: median / spread / min} in us."""
    for fn in fns.values():
        for _ in range(3):
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
TQ, TR, STORE_ROWS = 32, 64, 100_000
result["kernel_unit"] = "microseconds per launch, between device events"
fns, keep, shapes = {}, [], {}
for dim in (64, 128):
    tok = (torch.randn((STORE_ROWS * TR, dim), device=device, dtype=torch.float32)).to(torch.float16)      # finite by construction
    indptr = torch.arange(STORE_ROWS + 1, dtype=torch.int64, device=device) * TR
    qt = torch.randn((B, TQ, dim), device=device, dtype=torch.float32).to(torch.float16)
    qn = torch.full((B,), TQ, dtype=torch.int32, device=device)
    for k in (80, 256):
        ids = torch.from_numpy(np.stack([rng.choice(STORE_ROWS, k, replace=False) for _ in range(B)]).astype(np.int64)).to(device)
        n = torch.full((B,), k, dtype=torch.int32, device=device)
        pos = torch.empty((B, k), dtype=torch.int32, device=device)
        oi = torch.empty((B, k), dtype=torch.int64, device=device)
        os_ = torch.empty((B, k), dtype=torch.float64, device=device)
        on = torch.empty((B,), dtype=torch.int32, device=device)
        keep.append((tok, indptr, qt, qn, ids, n, pos, oi, os_, on))
        name = f"dim{dim}_k{k}"
        fns[name] = (lambda ids=ids, n=n, qt=qt, qn=qn, indptr=indptr, tok=tok, pos=pos, oi=oi, os_=os_, on=on, k=k, dim=dim:
                     nat.maxsim_rerank_dev(ids.data_ptr(), n.data_ptr(), B, k, qt.data_ptr(), qn.data_ptr(), TQ, dim, indptr.data_ptr(),
                                           tok.data_ptr(), STORE_ROWS, 0, k, pos.data_ptr(), oi.data_ptr(), os_.data_ptr(),
                                           on.data_ptr(), st))
        shapes[name] = (k, dim)
timed = launch_us(fns)
result["kernel"] = {"Tq": TQ, "T_r": TR, "store_rows": STORE_ROWS}
for name, (k, dim) in shapes.items():
    bytes_floor = B * k * TR * dim * 2 / COPY_BYTES_PER_S * 1e6
    flop_floor = 2.0 * B * k * TQ * TR * dim / F32_MATRIX_FLOPS * 1e6
    result["kernel"][name] = {**timed[name], "floor_token_bytes_us": round(bytes_floor, 2), "floor_f32_matrix_us": round(flop_floor, 2),
                              "median_over_larger_floor": round(timed[name]["median"] / max(bytes_floor, flop_floor), 2)}
del keep, fns
torch.cuda.empty_cache()

# ---- (b) end to end --------------------------------------------------------------------------------------------------------
N, D, TD, T, W, TOP_K, IN_FLIGHT = args.rows, args.dim, args.token_dim, args.tokens, 80, 20, args.in_flight
mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, enable_domain=False, token_dim=TD)
step = 100_000
for lo in range(0, N, step):
    hi = min(N, lo + step)
    X = rng.standard_normal((hi - lo, D), dtype=np.float32).astype(np.float16)
    tv = rng.standard_normal(((hi - lo) * T, TD), dtype=np.float32).astype(np.float16)
    mgr.add_rows(X, None, token_vectors=(np.arange(hi - lo + 1, dtype=np.int64) * T, tv))
mgr.finalize()
Q = rng.standard_normal((IN_FLIGHT, D)).astype(np.float32)
rankers = [MaxSimRanker(rng.standard_normal((32, TD)).astype(np.float32), candidates=W) for _ in range(IN_FLIGHT)]


async def burst(make):
    return await asyncio.gather(*(make(i) for i in range(IN_FLIGHT)))


contenders = {
    "search_plain_topk_W": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", W))),
    "search_ranker": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", TOP_K, ranker=rankers[i]))),
}
t0 = time.perf_counter()
contenders["search_ranker"]()          # the first use: the token vectors are mirrored
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
                        "tokens_per_row": T, "token_dim": TD, "Tq": 32, "top_k": TOP_K, "W": W, "rounds": args.rounds,
                        **{k: spread(v) for k, v in times.items()}}
mirror = mgr._token_vectors_on_device()
result["mirror"] = {"first_ranked_burst_seconds": round(first, 3), "bytes_held": mirror.nbytes, "uploaded_bytes": mirror.stats["uploaded_bytes"],
                    "by_construction_bytes": 2 * TD * N * T + 8 * (N + 1),
                    "at_1M_rows_of_32_tokens_dim_128_GB": round((2 * 128 * 32 * 1_000_000 + 8 * 1_000_001) / 1e9, 2)}
result["front_stats"] = {k: v for k, v in mgr._front.stats.items() if k.endswith("launches") or k == "requests"}
asyncio.run(mgr.close())

print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
