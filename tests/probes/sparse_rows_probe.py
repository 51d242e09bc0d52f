"""Ad-hoc measurement (not a test): what reading stored sparse rows back costs.

One MI355X, one sparse shard of 10,000,000 rows with 20 entries each over 10,000 dimensions (bulk-ingested without
payload columns: ids and chunk_index = row % 10 are derived from the row number).  In ONE process:

  (a) hr_get_sparse_rows_dev for 16,384 contiguous and 16,384 random rows between device events — the whole call (three
      scan launches + the gather, cap = the total) and the count pass alone (cap = 0) — as GB/s of useful bytes (8 bytes
      per entry read + 8 written, 8 per id read, 8 per row pointer written) beside the float4 copy rate measured in the
      same call (a 1 GiB device-to-device copy, bytes read + written).  The two id sets alternate window by window.
  (b) query("sparse_index", "chunk_index == 3", limit=100, output_fields=["embedding"]) end to end, wall time, beside the
      same query without the embedding.

Repeated fetches of the same ids may be served from the Infinity Cache: these are rates of the kernel, not of cold HBM.
Every timing: a warm-up, then --repeats windows; the median and the spread (max - min) between windows are reported.

  python tests/probes/sparse_rows_probe.py --out profiles/sparse_rows.json [--rows N] [--commit ID]
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
ap.add_argument("--nnz", type=int, default=20)
ap.add_argument("--sparse-dim", type=int, default=10_000)
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
    sys.exit("sparse_rows_probe needs a GPU: a CPU run says nothing about these numbers")

N, NNZ, V, D, FETCH = args.rows, args.nnz, args.sparse_dim, 8, 16384
device = torch.device("cuda", 0)
rng = np.random.default_rng(args.seed)
t0 = time.perf_counter()
mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=V, dtype="float16", enable_domain=False)
step, stride = 1 << 20, V // NNZ
for lo in range(0, N, step):
    m = min(N, lo + step) - lo
    # one index per stride of the vocabulary: ascending and distinct within a row
    idx = (np.arange(NNZ, dtype=np.int32) * stride + rng.integers(0, stride, size=(m, NNZ), dtype=np.int32)).reshape(-1)
    val = (rng.random(m * NNZ, dtype=np.float32) + np.float32(0.25))
    dense = rng.standard_normal((m, D), dtype=np.float32).astype(np.float16)
    mgr.add_rows_synthetic(dense, (np.arange(m + 1, dtype=np.int64) * NNZ, idx, val))
    print(f"{lo + m} rows staged", file=sys.stderr, flush=True)
mgr.finalize()
result = {"command": " ".join(sys.argv), "commit": args.commit, "rows": N, "nnz_per_row": NNZ, "sparse_dim": V, "repeats": args.repeats,
          "corpus_build_s": round(time.perf_counter() - t0, 1)}
print(f"collection built in {result['corpus_build_s']} s", file=sys.stderr, flush=True)
cs = torch.cuda.current_stream(device)
h = mgr._main.first


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "spread": round(float(max(xs) - min(xs)), 4), "all": [round(x, 4) for x in xs]}


def event_us(fns, inner=10):
    """Device-event time per call of each of `fns`, alternating between them window by window: {name: [us per window]}."""
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


def wall_ms(fns, inner=5):
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


# ---- (a) the gather against the copy rate ------------------------------------------------------------------------------------
src = torch.empty(1 << 28, dtype=torch.float32, device=device)       # 1 GiB
dst = torch.empty_like(src)
copy = event_us({"copy": lambda: dst.copy_(src)}, inner=4)
copy_rate = 2 * src.numel() * 4 / (float(np.median(copy["copy"])) * 1e-6)
del src, dst
result["a_fetch"] = {"rows_fetched": FETCH, "copy_rate_bytes_per_s": round(copy_rate, 0), "copy_us": spread(copy["copy"])}
id_sets = {"contiguous": np.arange(N // 2, N // 2 + FETCH, dtype=np.int64),
           "random": rng.choice(N, min(FETCH, N), replace=False).astype(np.int64)}
cap = FETCH * NNZ
indptr = torch.empty(FETCH + 1, dtype=torch.int64, device=device)
counts = torch.zeros(2, dtype=torch.int64, device=device)
scratch = torch.empty(nat.get_sparse_rows_scratch_bytes(FETCH), dtype=torch.uint8, device=device)
o_idx = torch.empty(cap, dtype=torch.int32, device=device)
o_val = torch.empty(cap, dtype=torch.float32, device=device)
d_ids = {name: torch.from_numpy(ids).to(device) for name, ids in id_sets.items()}


def fetch(name, with_entries=True):
    n = int(d_ids[name].numel())
    h.get_sparse_rows_dev(d_ids[name].data_ptr(), n, indptr.data_ptr(), o_idx.data_ptr() if with_entries else 0,
                          o_val.data_ptr() if with_entries else 0, cap if with_entries else 0, counts.data_ptr(), scratch.data_ptr(),
                          cs.cuda_stream)


us = event_us({"contiguous": lambda: fetch("contiguous"), "random": lambda: fetch("random"),
               "contiguous_count_pass": lambda: fetch("contiguous", False), "random_count_pass": lambda: fetch("random", False)})
for name in id_sets:
    n = int(d_ids[name].numel())
    useful = n * NNZ * 16 + n * 16
    rate = useful / (float(np.median(us[name])) * 1e-6)
    result["a_fetch"][name] = {"us": spread(us[name]), "count_pass_us": spread(us[name + "_count_pass"]), "useful_bytes": useful,
                               "useful_bytes_per_s": round(rate, 0), "fraction_of_copy_rate": round(rate / copy_rate, 4)}
fetch("random")
cs.synchronize()
ptr, idx, val = h.get_sparse_rows(id_sets["random"][:64])
n64 = int(ptr[-1])
result["a_fetch"]["counts"] = counts.cpu().tolist()
result["a_fetch"]["host_and_device_forms_equal"] = bool(np.array_equal(indptr[:65].cpu().numpy(), ptr) and
                                                        np.array_equal(o_idx[:n64].cpu().numpy(), idx) and
                                                        np.array_equal(o_val[:n64].cpu().numpy(), val))

# ---- (b) query with the payloads, end to end ---------------------------------------------------------------------------------
q = lambda fields: asyncio.run(mgr.query("sparse_index", "chunk_index == 3", fields, limit=100))
got = q(["embedding"])
w = wall_ms({"query_100_with_embedding": lambda: q(["embedding"]), "query_100_ids_only": lambda: q([])})
result["b_query"] = {"entities": len(got), "entries_per_entity": int(got[0]["embedding"]["indices"].shape[0]),
                     "query_100_with_embedding_ms": spread(w["query_100_with_embedding"]),
                     "query_100_ids_only_ms": spread(w["query_100_ids_only"]), "stats": dict(mgr.stats)}

asyncio.run(mgr.close())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
