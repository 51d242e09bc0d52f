"""Ad-hoc measurement (not a test): what a deep search (offset + top_k > HR_MAX_TOPK) costs on one MI355X.

  python tests/probes/deep_search_probe.py --out profiles/deep_search.json [--commit ID] [--part select,dense,sparse]
                                           [--kernel-stats FILE] [--ab-parent MS --ab-new MS --ab-spread MS]

Single query, W in {257, 1000, 4096, 16384}, alternating windows within one call: every figure is the median over the windows
and the spread (max - min) between them.

  select   hr_deep_topk_dev alone at n = --rows candidates (device events around the whole call), and the same at n = W (the
           passes and the gather have next to nothing to read there: launch overheads + the sort).
  dense    one shard of --rows x --dim fp16 COSINE rows: the whole hr_search_dense_deep call (host clock, the call is
           synchronous) beside a plain hr_search_dense at top_k = 256 of the same shard in the same windows — the floor a
           paging caller would multiply by ceil(W / 256); the full-shard refine and the selection by the library's own device
           events (hr_set_profiling), the refine as bytes read over time beside the rate of a device-to-device copy of 1 GiB
           measured in the same call.
  sparse   the same for a sparse shard of --rows docs x 20 entries.

--kernel-stats: a rocprofv3 --kernel-trace --stats kernel table (CSV) of a run of `--part select` on its own; the rows of the
deep_* kernels are copied into the JSON (the split of the selection into passes, gather and sort).  The --ab-* figures are the
ms_per_step of the default bench.py line, parent library against this one alternating on one box, copied as given.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--part", default="select,dense,sparse")
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--ab-parent", type=float, default=None)
ap.add_argument("--ab-new", type=float, default=None)
ap.add_argument("--ab-spread", type=float, default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

N, D = args.rows, args.dim
WS = [257, 1000, 4096, 16384]
parts = set(args.part.split(","))
dev = torch.device("cuda", 0)
rng = np.random.default_rng(args.seed)
stream = torch.cuda.current_stream(dev)


def summary(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "windows": len(xs)}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def wall_ms(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def copy_rate():
    """GB/s (read + written) of a device-to-device copy of 1 GiB."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    ms = [device_ms(lambda: dst.copy_(src), 5) for _ in range(args.windows)]
    del src, dst
    return summary([2 * (1 << 30) / (m * 1e-3) / 1e9 for m in ms])


result = {"commit": args.commit, "rows": N, "dim": D, "windows": args.windows, "steps_per_window": args.steps,
          "device": torch.cuda.get_device_name(0)}

if "select" in parts:
    scores = torch.randn(N, device=dev)                     # distinct scores for the most part: the usual case
    rows = torch.randperm(N, device=dev, dtype=torch.int32) if N < 2**31 else None
    ids = torch.empty(16384, dtype=torch.int64, device=dev)
    sc = torch.empty(16384, dtype=torch.float32, device=dev)
    scratch = torch.empty(nat.deep_topk_scratch_bytes(N, 1, 16384), dtype=torch.uint8, device=dev)

    def select(n, W):
        nat.deep_topk_dev(scores.data_ptr(), rows.data_ptr(), n, 1, W, 0, False, 0, ids.data_ptr(), sc.data_ptr(),
                          scratch.data_ptr(), stream.cuda_stream)

    for W in WS:                                            # warm-up: code objects, the sort's LDS attribute
        select(N, W)
        select(W, W)
    stream.synchronize()
    full = {W: [] for W in WS}
    tiny = {W: [] for W in WS}
    for _ in range(args.windows):
        for W in WS:
            full[W].append(device_ms(lambda: select(N, W), 10))
            tiny[W].append(device_ms(lambda: select(W, W), 10))
    result["select"] = {"n": N, "bytes_per_pass": 8 * N,
                        "ms_at_n": {str(W): summary(full[W]) for W in WS},
                        "ms_at_n_equal_W": {str(W): summary(tiny[W]) for W in WS}}
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            result["select"]["kernel_trace"] = [r for r in csv.DictReader(f) if "deep_" in (r.get("Name") or r.get("KernelName") or "")]
    del scores, rows, scratch


def windows_of(h, deep, plain, refine_phase, topk_phase, bytes_read):
    """Alternating windows of the deep calls (every W) and the plain top_k = 256 call: wall ms per call, and the refine /
    selection device ms of the deep calls from the library's spans."""
    for W in WS:
        deep(W)
    plain()
    wall = {W: [] for W in WS}
    ref = {W: [] for W in WS}
    sel = {W: [] for W in WS}
    floor = []
    for _ in range(args.windows):
        for W in WS:
            h.set_profiling(0)
            wall[W].append(wall_ms(lambda: deep(W), args.steps))
            h.set_profiling(2)
            h.kernel_ms()
            for _ in range(args.steps):
                deep(W)
            ms = h.kernel_ms()
            ref[W].append(ms[refine_phase][0])
            sel[W].append(ms[topk_phase][0])
        h.set_profiling(0)
        floor.append(wall_ms(plain, args.steps))
    out = {"plain_top256_call_ms": summary(floor), "refine_bytes_read": bytes_read, "deep": {}}
    for W in WS:
        r = summary(ref[W])
        out["deep"][str(W)] = {"call_ms": summary(wall[W]), "refine_ms": r, "selection_ms": summary(sel[W]),
                               "refine_GBps": bytes_read / (r["median"] * 1e-3) / 1e9,
                               "paged_floor_ms": -(-W // 256) * statistics.median(floor)}
    return out


if "dense" in parts or "sparse" in parts:
    result["copy_GBps"] = copy_rate()

if "dense" in parts:
    h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, 0)
    h.reserve(N)
    t0 = time.perf_counter()
    step = 1 << 18
    for lo in range(0, N, step):
        X = torch.randn((min(step, N - lo), D), device=dev, dtype=torch.float32)
        X = (X / X.norm(dim=1, keepdim=True)).half().contiguous()
        stream.synchronize()
        h.add_dense_dev(X.data_ptr(), X.shape[0])
    h.finalize()
    q = rng.standard_normal((1, D)).astype(np.float32)
    out = windows_of(h, lambda W: h.search_dense_deep(q, W), lambda: h.search_dense(q, 256), "refine", "topk", h.dense_scan_bytes)
    out["ingest_s"] = time.perf_counter() - t0
    ids, _ = h.search_dense_deep(q, 300)
    pids, _ = h.search_dense(q, 256)
    out["head_equals_plain_list"] = bool(np.array_equal(ids[:, :256], pids))
    result["dense"] = out
    h.close()

if "sparse" in parts:
    V, L = 30_011, 20                                       # a prime vocabulary: any stride gives distinct terms in a row
    h = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    step = 1 << 20
    nnz = 0
    for lo in range(0, N, step):
        n = min(step, N - lo)
        start = rng.integers(0, V, (n, 1))
        stride = rng.integers(1, V, (n, 1))
        idx = np.sort((start + stride * np.arange(L)) % V, axis=1).astype(np.int32)
        val = rng.random((n, L), dtype=np.float32) + 0.05
        h.add_sparse(np.arange(n + 1, dtype=np.int64) * L, idx.reshape(-1), val.reshape(-1))
        nnz += n * L
    h.finalize()
    terms = np.sort(rng.permutation(V)[:32]).astype(np.int32)
    query = [(terms, np.ones(32, np.float32))]
    out = windows_of(h, lambda W: h.search_sparse_deep(query, W), lambda: h.search_sparse(query, 256), "sparse_refine",
                     "sparse_topk", nnz * 8 + (N + 1) * 8)
    ids, _ = h.search_sparse_deep(query, 300)
    pids, _ = h.search_sparse(query, 256)
    out["head_equals_plain_list"] = bool(np.array_equal(ids[:, :256], pids))
    out["query_terms"] = 32
    result["sparse"] = out
    h.close()

if args.ab_parent is not None:
    result["bench_default_line"] = {"parent_ms_per_step": args.ab_parent, "this_ms_per_step": args.ab_new,
                                    "parent_window_spread_ms": args.ab_spread}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
