"""Ad-hoc measurement (not a test): what a page of the search iterator costs on one MI355X beside a deep call.

  python tests/probes/search_iterator_probe.py --out profiles/search_iterator.json [--commit ID] [--part dense,sparse]
                                               [--parent-json FILE] [--ab-parent MS --ab-new MS --ab-spread MS]

Single query, k in {1000, 16384}, alternating windows within one call: every figure is the median over the windows and the
spread (max - min) between them, wall clock around the synchronous call.

  dense    one shard of --rows x --dim fp16 COSINE rows: hr_search_dense_deep_after with a cursor in the middle of the ranking
           (score 0, row --rows / 2: half of the rows of random unit vectors follow it) beside hr_search_dense_deep at the same
           k and offset 0, from the same library in the same windows.
  sparse   the sparse shard of tests/probes/deep_search_probe.py (--rows docs x 20 entries, 32 query terms): the cursor is the
           last hit of the fourth 16 384-row page.

--parent-json: the output of a run of this script with --deep-only in a process of its own that loaded the parent commit's
libhbmrag.so (HBMRAG_LIB=... python tests/probes/search_iterator_probe.py --deep-only --out FILE): the deep calls alone on
the same shards from the same seeds.  Two processes one after the other on one box, not alternating windows.
The --ab-* figures are the ms_per_step of the default bench.py line, parent checkout against this tree alternating on one
box, copied as given.
"""
import argparse
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
ap.add_argument("--part", default="dense,sparse")
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--parent-json", default=None)
ap.add_argument("--deep-only", action="store_true", help="a library without the cursor forms: the deep calls alone")
ap.add_argument("--ab-parent", type=float, default=None)
ap.add_argument("--ab-new", type=float, default=None)
ap.add_argument("--ab-spread", type=float, default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

if args.deep_only:      # the parent's library does not export them
    for name in ("hr_search_dense_deep_after", "hr_search_sparse_deep_after", "hr_deep_topk_window_dev"):
        nat._SIGNATURES.pop(name)

N, D = args.rows, args.dim
KS = [1000, 16384]
parts = set(args.part.split(","))
dev = torch.device("cuda", 0)
rng = np.random.default_rng(args.seed)
stream = torch.cuda.current_stream(dev)


def summary(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "windows": len(xs)}


def wall_ms(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def windows_of(deep, page):
    """Alternating windows: for every k the deep call at offset 0, then (unless --deep-only) the page behind the cursor."""
    for k in KS:
        deep(k)
        if page:
            page(k)
    d, p = {k: [] for k in KS}, {k: [] for k in KS}
    for _ in range(args.windows):
        for k in KS:
            d[k].append(wall_ms(lambda: deep(k), args.steps))
            if page:
                p[k].append(wall_ms(lambda: page(k), args.steps))
    out = {}
    for k in KS:
        out[str(k)] = {"deep_offset0_call_ms": summary(d[k])}
        if page:
            out[str(k)]["page_after_cursor_call_ms"] = summary(p[k])
            out[str(k)]["page_minus_deep_ms"] = out[str(k)]["page_after_cursor_call_ms"]["median"] - out[str(k)]["deep_offset0_call_ms"]["median"]
    return out


result = {"commit": args.commit, "hr_version": nat.load_library().hr_version(), "rows": N, "dim": D, "windows": args.windows,
          "steps_per_window": args.steps, "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv)}

if "dense" in parts:
    h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, 0)
    h.reserve(N)
    torch.manual_seed(args.seed)
    step = 1 << 18
    for lo in range(0, N, step):
        X = torch.randn((min(step, N - lo), D), device=dev, dtype=torch.float32)
        X = (X / X.norm(dim=1, keepdim=True)).half().contiguous()
        stream.synchronize()
        h.add_dense_dev(X.data_ptr(), X.shape[0])
    h.finalize()
    q = rng.standard_normal((1, D)).astype(np.float32)
    cursor = (np.zeros(1, np.float32), np.array([N // 2], np.int64))
    page = None if args.deep_only else (lambda k: h.search_dense_deep_after(q, k, cursor))
    out = {"by_k": windows_of(lambda k: h.search_dense_deep(q, k), page), "cursor": "score 0.0, row rows / 2"}
    if page:
        ids, sc = h.search_dense_deep_after(q, 16384, cursor)
        out["page_full"] = bool((ids >= 0).all())
        out["page_first_score"] = float(sc[0, 0])
        a = h.search_dense_deep_after(q, 1000)
        b = h.search_dense_deep(q, 1000)
        out["page0_equals_deep_list"] = bool(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes())
    result["dense"] = out
    h.close()
    torch.cuda.empty_cache()

if "sparse" in parts:
    V, L = 30_011, 20                                       # a prime vocabulary: any stride gives distinct terms in a row
    h = nat.ShardHandle(0, nat.HR_F16, nat.HR_METRIC_COSINE, V)
    step = 1 << 20
    for lo in range(0, N, step):
        n = min(step, N - lo)
        start = rng.integers(0, V, (n, 1))
        stride = rng.integers(1, V, (n, 1))
        idx = np.sort((start + stride * np.arange(L)) % V, axis=1).astype(np.int32)
        val = rng.random((n, L), dtype=np.float32) + 0.05
        h.add_sparse(np.arange(n + 1, dtype=np.int64) * L, idx.reshape(-1), val.reshape(-1))
    h.finalize()
    terms = np.sort(rng.permutation(V)[:32]).astype(np.int32)
    query = [(terms, np.ones(32, np.float32))]
    page, out = None, {}
    if not args.deep_only:
        cursor = None
        for _ in range(4):
            ids, sc = h.search_sparse_deep_after(query, 16384, cursor)
            m = int((ids[0] >= 0).sum())
            cursor = (sc[:, m - 1].copy(), ids[:, m - 1].copy())
        out["cursor"] = f"the last hit of the fourth 16 384-row page (score {float(cursor[0][0])!r}), {m} hits on that page"
        page = lambda k: h.search_sparse_deep_after(query, k, cursor)   # noqa: E731
    out["by_k"] = windows_of(lambda k: h.search_sparse_deep(query, k), page)
    out["query_terms"] = 32
    result["sparse"] = out
    h.close()

if args.parent_json:
    with open(args.parent_json) as f:
        result["parent_library"] = json.load(f)

if args.ab_parent is not None:
    result["bench_default_line"] = {"parent_ms_per_step": args.ab_parent, "this_ms_per_step": args.ab_new,
                                    "parent_window_spread_ms": args.ab_spread}
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
