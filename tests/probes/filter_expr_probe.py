"""Ad-hoc measurement (not a test): what the expression evaluator (hr_filter_eval_expr_dev, csrc/filter.h) costs.

One MI355X, one collection of 10,000,000 rows (documents of 10 chunks: doc_id = "doc" + 7 digits, chunk_index = row % 10,
entropy and token_count random; dense rows of 8 fp16 values, no sparse rows: only the payload matters here).

  (a) a three-term conjunction through hr_filter_eval_dev and the same tree through hr_filter_eval_expr_dev: both stream the
      same columns (8 + 4 + 8 bytes per row); kernel time by device events, the two entry points alternating.
  (b) `doc_id in [N ids]` for N = 1, 64, 4096: kernel time against the floor of reading the 16-byte key column once at the
      float4 copy rate DESIGN section 5 records (6.29 TB/s moved).
  (c) today's workaround for such a list: N separate `doc_id == ...` evaluations (DeviceFilters.evaluate, end to end: launch,
      count read-back), timed at N = 64 and extrapolated linearly from there, beside one evaluate of the list.
  (d) delete_by_filter of 64 documents: one `in` expression against 64 calls (end to end, distinct documents per repeat).

Every timing: a warm-up, then REPEATS windows; the median and the spread (max - min) between windows are reported, and a
difference counts only if it exceeds the spread.

  python tests/probes/filter_expr_probe.py --out profiles/filter_expr.json [--commit ID]
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
    sys.exit("filter_expr_probe needs a GPU: a CPU run says nothing about these numbers")

N, D, COPY_RATE = args.rows, 8, 6.29e12
rng = np.random.default_rng(args.seed)
t0 = time.perf_counter()
mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, dtype="float16", enable_domain=False)
mgr.collections.pop("sparse_index", None)
step = 1 << 19
for lo in range(0, N, step):
    hi = min(N, lo + step)
    mgr.add_rows(rng.standard_normal((hi - lo, D)).astype(np.float16), None,
                 doc_id=[f"doc{r // 10:07d}" for r in range(lo, hi)], chunk_index=(np.arange(lo, hi) % 10).tolist(),
                 entropy=rng.random(hi - lo).astype(np.float32).tolist(), token_count=rng.integers(0, 2000, hi - lo).tolist())
mgr.finalize()
n_docs = (N + 9) // 10
result = {"command": " ".join(sys.argv), "commit": args.commit, "rows": N, "documents": n_docs, "repeats": args.repeats,
          "corpus_build_s": round(time.perf_counter() - t0, 1), "copy_rate_bytes_per_s": COPY_RATE}
dev = mgr._filters_on_device()
device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
mask = torch.empty(8 * ((N + 63) // 64), dtype=torch.uint8, device=device)
und = torch.empty_like(mask)
counts = torch.zeros(2, dtype=torch.int32, device=device)


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "all": [round(x, 3) for x in xs]}


def kernel_us(fns, inner=20):
    """Device-event time per launch of each of `fns`, alternating between them: {name: [us per window]}."""
    for fn in fns.values():
        for _ in range(10):
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


def docs(n, first=0):
    """n document ids spread over the collection."""
    return [f"doc{(first + i * (n_docs // (n + 1))) % n_docs:07d}" for i in range(n)]


def in_list(ids):
    return "doc_id in [" + ", ".join(f'"{d}"' for d in ids) + "]"


# ---- (a) the conjunction: old kernel against new ---------------------------------------------------------------------------------
CONJ = "chunk_index < 5 and entropy > 0.2 and token_count >= 100"
terms, _ = dev._terms(CONJ, N)
leaves = []
for t in terms:
    leaf = nat.FilterLeaf()
    leaf.term = t
    leaves.append(leaf)
program = [0, 1, nat.HR_FILTER_AND, 2, nat.HR_FILTER_AND]
ptrs = (0, mask.data_ptr(), und.data_ptr(), counts.data_ptr(), cs.cuda_stream)
a = kernel_us({"hr_filter_eval_dev": lambda: nat.filter_eval_dev(terms, N, *ptrs),
               "hr_filter_eval_expr_dev": lambda: nat.filter_eval_expr_dev(leaves, program, N, *ptrs)})
nat.filter_eval_dev(terms, N, *ptrs)
old = (mask.clone(), und.clone(), counts.clone())
nat.filter_eval_expr_dev(leaves, program, N, *ptrs)
cs.synchronize()
bytes_a = N * (8 + 4 + 8)
result["a_conjunction"] = {
    "expr": CONJ, "column_bytes": bytes_a, "outputs_equal": bool(torch.equal(old[0], mask) and torch.equal(old[1], und)
                                                                 and torch.equal(old[2], counts)),
    "old_us": spread(a["hr_filter_eval_dev"]), "new_us": spread(a["hr_filter_eval_expr_dev"]),
    "new_over_old": round(float(np.median(a["hr_filter_eval_expr_dev"]) / np.median(a["hr_filter_eval_dev"])), 3),
    "old_bytes_per_s": round(bytes_a / (float(np.median(a["hr_filter_eval_dev"])) * 1e-6), 0),
    "new_bytes_per_s": round(bytes_a / (float(np.median(a["hr_filter_eval_expr_dev"])) * 1e-6), 0)}

# ---- (b) a list against the column-read floor -----------------------------------------------------------------------------------------
floor_us = 16 * N / COPY_RATE * 1e6
result["b_list_vs_floor"] = {"key_column_bytes": 16 * N, "floor_us": round(floor_us, 2), "lists": {}}
eq_terms, _ = dev._terms('doc_id == "doc0000042"', N)
for n in (1, 64, 4096):
    lv, prog = dev._terms(in_list(docs(n)), N)
    us = kernel_us({"in": lambda: nat.filter_eval_expr_dev(lv, prog.codes, N, *ptrs),
                    "eq": lambda: nat.filter_eval_dev(eq_terms, N, *ptrs)})
    cs.synchronize()
    result["b_list_vs_floor"]["lists"][str(n)] = {
        "in_us": spread(us["in"]), "one_equality_us": spread(us["eq"]),
        "in_over_floor": round(float(np.median(us["in"])) / floor_us, 2), "set_bytes": 16 * n}
    nat.filter_eval_expr_dev(lv, prog.codes, N, *ptrs)
    # a string leaf never says "true" by itself: the matches are the undecided rows the host settles ((c) includes that)
    result["b_list_vs_floor"]["lists"][str(n)]["rows_undecided"] = int(counts.cpu()[1])


# ---- (c) against N separate equality evaluations, end to end ------------------------------------------------------------------------------
def wall_ms(fn):
    fn()
    out = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


ids64 = docs(64)
separate = wall_ms(lambda: [dev.evaluate(f'doc_id == "{d}"', N) for d in ids64])
result["c_workaround"] = {"separate_64_ms": spread(separate), "per_equality_ms": round(float(np.median(separate)) / 64, 4), "one_list_ms": {}}
for n in (1, 64, 4096):
    expr = in_list(docs(n))
    one = wall_ms(lambda: dev.evaluate(expr, N))
    result["c_workaround"]["one_list_ms"][str(n)] = {
        **spread(one), "separate_extrapolated_ms": round(float(np.median(separate)) / 64 * n, 2),
        "separate_over_list": round(float(np.median(separate)) / 64 * n / float(np.median(one)), 1)}

# ---- (d) batched delete -------------------------------------------------------------------------------------------------------------------
batched, single = [], []
for rep in range(args.repeats + 1):            # the first pair is the warm-up
    ids_a, ids_b = docs(64, first=1000 * (2 * rep) + 1), docs(64, first=1000 * (2 * rep + 1) + 1)
    t = time.perf_counter()
    asyncio.run(mgr.delete_by_filter("semantic_index", in_list(ids_a)))
    batched.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    for d in ids_b:
        asyncio.run(mgr.delete_by_filter("semantic_index", f'doc_id == "{d}"'))
    single.append((time.perf_counter() - t) * 1e3)
result["d_delete_64_documents"] = {"one_in_expression_ms": spread(batched[1:]), "sixty_four_calls_ms": spread(single[1:]),
                                   "calls_over_expression": round(float(np.median(single[1:]) / np.median(batched[1:])), 1),
                                   "rows_tombstoned": int(mgr._deleted.sum())}
result["filter_stats"] = dict(dev.stats)

asyncio.run(mgr.close())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
