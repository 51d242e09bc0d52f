"""Ad-hoc measurement (not a test): what Collection.query costs on the device path, and what a stored-row fetch moves.

One MI355X, one collection of 10,000,000 x 768 fp16 rows (drawn on the device) with payload columns (documents of 10
chunks: doc_id = "doc" + 7 digits, chunk_index = row % 10).  In ONE process:

  (a) query(expr, limit=100) and query(expr, ["count(*)"]) through the device path (cached packed mask in HBM ->
      hr_mask_rows_dev -> two counts and <= 100 ids read back) against the host restatement a caller had before: mask
      read-back + unpackbits + flatnonzero — for a selective expression (`doc_id in [64 ids]`) and one that passes half
      the rows (`chunk_index < 5`).  The mask of either is evaluated once before the clock starts (both ways use the same
      cached mask).  Wall time, the two ways alternating window by window; hr_mask_rows_dev alone between device events.
  (b) hr_get_dense_rows_dev for 16,384 contiguous and 16,384 random rows (fp16 out and fp32 out), between device events:
      GB/s of useful bytes (rows * dim * stored element size read + the output written) beside the float4 copy rate
      measured in the same call (a 1 GiB device-to-device copy, bytes read + written).

Every timing: a warm-up, then --repeats windows; the median and the spread (max - min) between windows are reported.

  python tests/probes/query_probe.py --out profiles/query_fetch.json [--rows N] [--commit ID]
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
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import MilvusIndexManager   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("query_probe needs a GPU: a CPU run says nothing about these numbers")

N, D, FETCH = args.rows, args.dim, 16384
device = torch.device("cuda", 0)
rng = np.random.default_rng(args.seed)
t0 = time.perf_counter()
mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, dtype="float16", enable_domain=False)
mgr.collections.pop("sparse_index", None)
mgr._main.first.reserve(N)
step = 1 << 19
gen = torch.Generator(device=device)
gen.manual_seed(args.seed)
for lo in range(0, N, step):
    hi = min(N, lo + step)
    m = hi - lo
    rows = torch.randn((m, D), generator=gen, device=device, dtype=torch.float32).to(torch.float16)
    torch.cuda.synchronize(device)
    r = np.arange(lo, hi)
    zeros = np.zeros(m, np.float32)
    mgr.add_rows(rows, None, ids=[f"c{x:08d}" for x in range(lo, hi)], contents=[""] * m,
                 doc_id=[f"doc{x // 10:07d}" for x in range(lo, hi)], chunk_index=r % 10, token_count=r % 2000,
                 entropy=zeros, redundancy=zeros, domain_density=zeros, timestamp=[""] * m, metadata_json=[""] * m)
mgr.finalize()
n_docs = (N + 9) // 10
result = {"command": " ".join(sys.argv), "commit": args.commit, "rows": N, "dim": D, "dtype": "float16", "repeats": args.repeats,
          "corpus_build_s": round(time.perf_counter() - t0, 1)}
print(f"collection built in {result['corpus_build_s']} s", file=sys.stderr, flush=True)
cs = torch.cuda.current_stream(device)
h = mgr._main.first


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "spread": round(float(max(xs) - min(xs)), 4), "all": [round(x, 4) for x in xs]}


def wall_ms(fns, inner=5):
    """Wall time per call of each of `fns`, alternating between them window by window: {name: [ms per window]}."""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize(device)
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            out[name].append((time.perf_counter() - t) * 1e3 / inner)
    return out


def event_us(fns, inner=10):
    """Device-event time per launch of each of `fns`, alternating between them: {name: [us per window]}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    cs.synchronize()
    out = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.repeats):
        for name, fn in fns.items():
            e0.record(cs)
            for _ in range(inner):
                fn()
            e1.record(cs)
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / inner * 1e3)
    return out


# ---- (a) query and count(*) against the host restatement ---------------------------------------------------------------------
docs64 = [f"doc{(i * (n_docs // 65)) % n_docs:07d}" for i in range(64)]
EXPRS = {"selective_in_64_docs": "doc_id in [" + ", ".join(f'"{d}"' for d in docs64) + "]", "half_the_rows": "chunk_index < 5"}
q = lambda *a, **kw: asyncio.run(mgr.query("semantic_index", *a, **kw))
result["a_query"] = {}
for name, expr in EXPRS.items():
    mask = mgr._global_device_mask(expr)           # evaluated once, cached: both ways below start from it

    def host_rows(limit=100):
        keep = np.unpackbits(mask.cpu().numpy(), bitorder="little")[:N].astype(bool)
        return np.flatnonzero(keep)[:limit]

    def host_count():
        return int(np.unpackbits(mask.cpu().numpy(), bitorder="little")[:N].sum())

    got = q(expr, limit=100)
    want = host_rows()
    count = q(expr, ["count(*)"])[0]["count(*)"]
    w = wall_ms({"query_limit_100": lambda: q(expr, limit=100), "host_flatnonzero_100": host_rows,
                 "query_count": lambda: q(expr, ["count(*)"]), "host_count": host_count})
    d_rows = torch.empty(100, dtype=torch.int64, device=device)
    d_counts = torch.empty(2, dtype=torch.int64, device=device)
    scratch = torch.empty(nat.mask_rows_scratch_bytes(N), dtype=torch.uint8, device=device)
    k = event_us({"hr_mask_rows_dev": lambda: nat.mask_rows_dev(mask.data_ptr(), N, 0, 0, 100, d_rows.data_ptr(), d_counts.data_ptr(),
                                                                scratch.data_ptr(), cs.cuda_stream)})
    result["a_query"][name] = {
        "expr": expr if len(expr) < 80 else expr[:77] + "...", "rows_passing": count, "mask_bytes": int(mask.numel()),
        "answers_equal": bool([x["id"] for x in got] == [f"c{r:08d}" for r in want] and count == host_count()),
        "query_limit_100_ms": spread(w["query_limit_100"]), "host_flatnonzero_100_ms": spread(w["host_flatnonzero_100"]),
        "query_count_ms": spread(w["query_count"]), "host_count_ms": spread(w["host_count"]),
        "host_over_query": round(float(np.median(w["host_flatnonzero_100"]) / np.median(w["query_limit_100"])), 1),
        "mask_rows_kernels_us": spread(k["hr_mask_rows_dev"])}
result["stats"] = dict(mgr.stats)

# ---- (b) stored rows out of the tiles against the copy rate ----------------------------------------------------------------
src = torch.empty(1 << 28, dtype=torch.float32, device=device)       # 1 GiB
dst = torch.empty_like(src)
copy = event_us({"copy": lambda: dst.copy_(src)}, inner=4)
copy_rate = 2 * src.numel() * 4 / (float(np.median(copy["copy"])) * 1e-6)
del src, dst
result["b_fetch"] = {"rows_fetched": FETCH, "copy_rate_bytes_per_s": round(copy_rate, 0), "copy_us": spread(copy["copy"])}
id_sets = {"contiguous": np.arange(N // 2, N // 2 + FETCH, dtype=np.int64), "random": rng.choice(N, FETCH, replace=False).astype(np.int64)}
missing = torch.zeros(1, dtype=torch.int32, device=device)
for out_name, out_dtype, t_dtype, out_size in (("fp16_out", nat.HR_F16, torch.float16, 2), ("fp32_out", nat.HR_F32, torch.float32, 4)):
    out = torch.empty((FETCH, D), dtype=t_dtype, device=device)
    for name, ids in id_sets.items():
        d_ids = torch.from_numpy(ids).to(device)
        us = event_us({"get": lambda: h.get_dense_rows_dev(d_ids.data_ptr(), FETCH, out_dtype, out.data_ptr(), D, missing.data_ptr(),
                                                           cs.cuda_stream)})
        useful = FETCH * D * (2 + out_size)          # stored bytes read + output bytes written
        rate = useful / (float(np.median(us["get"])) * 1e-6)
        result["b_fetch"][f"{name}_{out_name}"] = {"us": spread(us["get"]), "useful_bytes": useful, "useful_bytes_per_s": round(rate, 0),
                                                   "fraction_of_copy_rate": round(rate / copy_rate, 3), "missing": int(missing.item())}
check = h.get_dense_rows(id_sets["random"][:64])
d_ids = torch.from_numpy(id_sets["random"][:64].copy()).to(device)
out = torch.empty((64, D), dtype=torch.float32, device=device)
h.get_dense_rows_dev(d_ids.data_ptr(), 64, nat.HR_F32, out.data_ptr(), D, 0, cs.cuda_stream)
cs.synchronize()
result["b_fetch"]["host_and_device_forms_equal"] = bool(np.array_equal(check, out.cpu().numpy()))

asyncio.run(mgr.close())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
