"""Ad-hoc measurement (not a test): what MaxSim as a first-stage search costs (hr_maxsim_scan_dev, csrc/maxsim.h;
manager.maxsim_search).

One MI355X.

  (a) hr_maxsim_scan_dev alone over a store of 100 000 rows x 32 tokens, dim = 64 / 128, Tq = 32, B = 1 / 16, under no mask
      and under a mask that passes 1 % of the rows; one launch between two device events.  Beside every figure its two
      floors for the same call: the token bytes actually gathered (B * passing rows * T_r * dim * 2) at the float4 copy
      rate (6.29 TB/s) and 2 * B * passing rows * Tq * T_r * dim FLOP at the measured fp32 matrix rate (155 TFLOP/s).  In the
      same windows hr_maxsim_rerank_dev scores the same number of (query, row) pairs as lists of up to 768 ids drawn
      without repetition: the ratio scan / rerank says whether the scan fills the machine as well as the rerank does.
  (b) end to end on a one-shard manager (--rows x --dim, --tokens token vectors of --token-dim per row), ONE caller:
      maxsim_search(top_k=20) beside search(ranker=MaxSimRanker(candidates=80)), wall clock per call.

The contenders alternate, window after window, in one process; a warm-up, then --repeats windows each (--rounds for (b));
the median, the spread (max - min) and the minimum are reported.

  python tests/probes/maxsim_search_probe.py --out profiles/maxsim_search.json [--commit ID]
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
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--tokens", type=int, default=8)
ap.add_argument("--token-dim", type=int, default=64)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--store-rows", type=int, default=100_000)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--skip-end-to-end", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import MilvusIndexManager   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402
from advanced_rag.maxsim import MaxSimRanker   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("maxsim_search_probe needs a GPU: a CPU run says nothing about these numbers")

COPY_BYTES_PER_S, F32_MATRIX_FLOPS = 6.29e12, 155e12
device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
rng = np.random.default_rng(args.seed)
result = {"command": " ".join(sys.argv), "commit": args.commit, "hr_version": nat.load_library().hr_version(),
          "repeats": args.repeats, "floors": {"copy_bytes_per_s": COPY_BYTES_PER_S, "f32_matrix_flops": F32_MATRIX_FLOPS}}


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "min": round(float(min(xs)), 3)}


def launch_us(fns):
    """Device-event time of one call of each of `fns`, alternating between them: {name: median / spread / min} in us."""
    for fn in fns.values():
        for _ in range(2):
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


# ---- (a) the scan alone, the rerank over as many pairs beside it -----------------------------------------------------------
st = cs.cuda_stream
TQ, TR, STORE_ROWS, K_MAX = 32, 32, args.store_rows, 3 * nat.HR_MAX_TOPK
result["kernel_unit"] = "microseconds per launch, between device events"
result["kernel"] = {"Tq": TQ, "T_r": TR, "store_rows": STORE_ROWS}
for dim in (64, 128):
    tok = torch.randn((STORE_ROWS * TR, dim), device=device, dtype=torch.float32).to(torch.float16)      # finite by construction
    indptr = torch.arange(STORE_ROWS + 1, dtype=torch.int64, device=device) * TR
    bits = {"all": None, "1pct": rng.random(STORE_ROWS) < 0.01}
    fns, keep, shapes = {}, [], {}
    for B in (1, 16):
        qt = torch.randn((B, TQ, dim), device=device, dtype=torch.float32).to(torch.float16)
        qn = torch.full((B,), TQ, dtype=torch.int32, device=device)
        sc = torch.empty((B, STORE_ROWS), dtype=torch.float32, device=device)
        rw = torch.empty((B, STORE_ROWS), dtype=torch.int32, device=device)
        for mname, m in bits.items():
            passing = STORE_ROWS if m is None else int(m.sum())
            d_m = torch.from_numpy(np.packbits(m.astype(np.uint8), bitorder="little")).to(device) if m is not None else None
            name = f"dim{dim}_B{B}_{mname}"
            fns["scan_" + name] = (lambda qt=qt, qn=qn, B=B, dim=dim, d_m=d_m, sc=sc, rw=rw:
                                   nat.maxsim_scan_dev(qt.data_ptr(), qn.data_ptr(), B, TQ, dim, indptr.data_ptr(), tok.data_ptr(),
                                                       STORE_ROWS, STORE_ROWS, d_m.data_ptr() if d_m is not None else 0,
                                                       sc.data_ptr(), rw.data_ptr(), st))
            # the rerank over the same number of (query, row) pairs
            pairs = B * passing
            k = min(K_MAX, pairs)
            Br = -(-pairs // k)
            ids = torch.from_numpy(np.stack([rng.choice(STORE_ROWS, k, replace=False) for _ in range(Br)]).astype(np.int64)).to(device)
            n = torch.full((Br,), k, dtype=torch.int32, device=device)
            rqt = torch.randn((Br, TQ, dim), device=device, dtype=torch.float32).to(torch.float16)
            rqn = torch.full((Br,), TQ, dtype=torch.int32, device=device)
            pos = torch.empty((Br, k), dtype=torch.int32, device=device)
            oi = torch.empty((Br, k), dtype=torch.int64, device=device)
            os_ = torch.empty((Br, k), dtype=torch.float64, device=device)
            on = torch.empty((Br,), dtype=torch.int32, device=device)
            keep.append((d_m, ids, n, rqt, rqn, pos, oi, os_, on))
            fns["rerank_" + name] = (lambda ids=ids, n=n, rqt=rqt, rqn=rqn, pos=pos, oi=oi, os_=os_, on=on, k=k, Br=Br, dim=dim:
                                     nat.maxsim_rerank_dev(ids.data_ptr(), n.data_ptr(), Br, k, rqt.data_ptr(), rqn.data_ptr(), TQ, dim,
                                                           indptr.data_ptr(), tok.data_ptr(), STORE_ROWS, 0, k, pos.data_ptr(),
                                                           oi.data_ptr(), os_.data_ptr(), on.data_ptr(), st))
            shapes[name] = (B, passing, Br, k)
    timed = launch_us(fns)
    for name, (B, passing, Br, k) in shapes.items():
        bytes_floor = B * passing * TR * dim * 2 / COPY_BYTES_PER_S * 1e6
        flop_floor = 2.0 * B * passing * TQ * TR * dim / F32_MATRIX_FLOPS * 1e6
        s, r = timed["scan_" + name], timed["rerank_" + name]
        result["kernel"][name] = {"scan": s, "passing_rows": passing, "floor_token_bytes_us": round(bytes_floor, 2),
                                  "floor_f32_matrix_us": round(flop_floor, 2),
                                  "scan_median_over_larger_floor": round(s["median"] / max(bytes_floor, flop_floor), 2),
                                  "rerank_same_pairs": {**r, "lists": Br, "k_in": k, "pairs": Br * k},
                                  "rerank_median_over_larger_floor": round(r["median"] * (B * passing) / (Br * k) / max(bytes_floor, flop_floor), 2),
                                  "scan_over_rerank_per_pair": round(s["median"] / (r["median"] * (B * passing) / (Br * k)), 3)}
    del keep, fns, tok, indptr
    torch.cuda.empty_cache()

# ---- (b) end to end, one caller ----------------------------------------------------------------------------------------------
if not args.skip_end_to_end:
    N, D, TD, T, W, TOP_K = args.rows, args.dim, args.token_dim, args.tokens, 80, 20
    mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, enable_domain=False, token_dim=TD)
    step = 100_000
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        X = rng.standard_normal((hi - lo, D), dtype=np.float32).astype(np.float16)
        tv = rng.standard_normal(((hi - lo) * T, TD), dtype=np.float32).astype(np.float16)
        mgr.add_rows(X, None, token_vectors=(np.arange(hi - lo + 1, dtype=np.int64) * T, tv))
    mgr.finalize()
    NQ = 8
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    QT = [rng.standard_normal((32, TD)).astype(np.float32) for _ in range(NQ)]
    rankers = [MaxSimRanker(qt, candidates=W) for qt in QT]
    contenders = {
        "maxsim_search_top20": lambda i: asyncio.run(mgr.maxsim_search(QT[i % NQ], TOP_K)),
        "search_ranker_candidates80": lambda i: asyncio.run(mgr.search(Q[i % NQ], "semantic_index", TOP_K, ranker=rankers[i % NQ])),
        "maxsim_search_top20_filter_10pct": lambda i: asyncio.run(mgr.maxsim_search(QT[i % NQ], TOP_K, "chunk_index == 3")),
    }
    t0 = time.perf_counter()
    contenders["maxsim_search_top20"](0)          # the first use: the token vectors are mirrored
    first = time.perf_counter() - t0
    for fn in contenders.values():
        for i in range(2):
            fn(i)
    times = {k: [] for k in contenders}
    for r in range(args.rounds):
        for name, fn in contenders.items():
            t0 = time.perf_counter()
            fn(r)
            times[name].append((time.perf_counter() - t0) * 1e3)
    result["end_to_end"] = {"unit": "milliseconds per call, one caller, wall clock", "rows": N, "dim": D, "tokens_per_row": T,
                            "token_dim": TD, "Tq": 32, "top_k": TOP_K, "W": W, "rounds": args.rounds,
                            "first_maxsim_search_seconds": round(first, 3), **{k: spread(v) for k, v in times.items()},
                            "stats": {k: v for k, v in mgr.stats.items() if k.startswith("maxsim")}}
    asyncio.run(mgr.close())

print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
