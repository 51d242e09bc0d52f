"""Ad-hoc measurement (not a test): what the keyword leaf of hr_filter_eval_expr_dev (TEXT_MATCH, csrc/filter.h) costs.

One MI355X.  Rows of ~40 words (30 .. 50, uniform) from a vocabulary of 50 000.

  (a) the kernel, on a word CSR of --rows rows generated on the device (ids uniform, not sorted within a row: the kernel's
      work per entry does not depend on the order): a one-word and a 1 000-word leaf between device events, alternating in
      the same call with a device-to-device copy (torch's vectorised copy_) of a buffer of the CSR's size,
      4 * entries + 8 * rows bytes — the copy reads AND writes that many bytes, the leaf only reads them.
  (b) `doc_id in [64 ids]` (no keyword leaf: filter_expr_kernel<false>) over a synthetic key column of --rows rows through
      this tree's library and through --parent-lib (the parent checkout's build of the same entry point; the structs are
      the same), alternating windows in one process on one box.  Skipped without --parent-lib.
  (c) end to end on a collection of --e2e-rows rows with real `content`: the host build of the word sets (first use), the
      first search(filters=TEXT_MATCH...) (upload + kernel + search), the cached one, and the HBM the mirror holds.

Every timing: a warm-up, then REPEATS windows; the median and the spread (max - min) between windows are reported.

  python tests/probes/text_match_probe.py --out profiles/text_match.json [--parent-lib PATH] [--commit ID]
"""
import argparse
import asyncio
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--e2e-rows", type=int, default=10_000_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import MilvusIndexManager   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("text_match_probe needs a GPU: a CPU run says nothing about these numbers")

N, VOCAB = args.rows, 50_000
device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
result = {"command": " ".join(sys.argv), "commit": args.commit, "rows": N, "vocabulary": VOCAB, "repeats": args.repeats}


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "all": [round(x, 3) for x in xs]}


def kernel_us(fns, inner=5):
    """Device-event time per call of each of `fns`, alternating between them: {name: [us per window]}."""
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


mask = torch.empty(8 * ((N + 63) // 64), dtype=torch.uint8, device=device)
und = torch.empty_like(mask)
counts = torch.zeros(2, dtype=torch.int32, device=device)
ptrs = (0, mask.data_ptr(), und.data_ptr(), counts.data_ptr(), cs.cuda_stream)

# ---- (a) the keyword leaf against a copy of the CSR's size -------------------------------------------------------------------------
gen = torch.Generator(device=device)
gen.manual_seed(args.seed)
lens = torch.randint(30, 51, (N,), generator=gen, device=device, dtype=torch.int64)
indptr = torch.zeros(N + 1, dtype=torch.int64, device=device)
torch.cumsum(lens, 0, out=indptr[1:])
entries = int(indptr[-1])
words = torch.randint(0, VOCAB, (entries,), generator=gen, device=device, dtype=torch.int32)
csr_bytes = 4 * entries + 8 * N
src = torch.empty(csr_bytes // 4, dtype=torch.float32, device=device).normal_()
dst = torch.empty_like(src)


def match_leaf(n_words):
    ids = torch.arange(0, n_words, dtype=torch.int32, device=device) * (VOCAB // max(n_words, 1))     # ascending, distinct
    leaf = nat.FilterLeaf()
    t = leaf.term
    t.kind, t.op, t.col, t.ival = nat.HR_COL_TOKENS, nat.HR_OP_MATCH, indptr.data_ptr(), 1
    t.key[0], t.key[1] = words.data_ptr(), N
    leaf.set, leaf.n_set = ids.data_ptr(), n_words
    return leaf, ids


result["a_keyword_leaf"] = {"entries": entries, "csr_bytes": csr_bytes, "leaves": {}}
for n_words in (1, 1000):
    leaf, keep_alive = match_leaf(n_words)
    us = kernel_us({"leaf": lambda: nat.filter_eval_expr_dev([leaf], [0], N, *ptrs), "copy": lambda: dst.copy_(src)})
    nat.filter_eval_expr_dev([leaf], [0], N, *ptrs)
    kept = int(counts.cpu()[0])
    lm, cm = float(np.median(us["leaf"])), float(np.median(us["copy"]))
    result["a_keyword_leaf"]["leaves"][str(n_words)] = {
        "leaf_us": spread(us["leaf"]), "copy_us": spread(us["copy"]), "leaf_over_copy": round(lm / cm, 3),
        "leaf_read_bytes_per_s": round(csr_bytes / (lm * 1e-6), 0), "copy_moved_bytes_per_s": round(2 * csr_bytes / (cm * 1e-6), 0),
        "rows_kept": kept}
del src, dst, words, indptr, lens

# ---- (b) an `in` list without a keyword leaf: this tree against the parent -----------------------------------------------------------
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    parent.hr_filter_eval_expr_dev.restype = ctypes.c_int
    parent.hr_filter_eval_expr_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64] + \
        [ctypes.c_void_p] * 5
    parent.hr_version.restype = ctypes.c_int
    keys = torch.randint(0, 1 << 62, (N, 2), generator=gen, device=device, dtype=torch.int64)
    picked = keys[torch.arange(64, device=device) * (N // 64)].cpu().numpy()
    picked = picked[np.lexsort((picked[:, 1], picked[:, 0]))]          # non-negative: signed order is the unsigned one
    d_set = torch.from_numpy(np.ascontiguousarray(picked)).to(device)
    leaf = nat.FilterLeaf()
    leaf.term.kind, leaf.term.op, leaf.term.col = nat.HR_COL_STR16, nat.HR_OP_IN, keys.data_ptr()
    leaf.set, leaf.n_set = d_set.data_ptr(), 64
    arr = (nat.FilterLeaf * 1)(leaf)
    prog = (ctypes.c_int32 * 1)(0)

    def via_parent():
        rc = parent.hr_filter_eval_expr_dev(ctypes.byref(arr), 1, ctypes.byref(prog), 1, N, None, mask.data_ptr(), und.data_ptr(),
                                            counts.data_ptr(), cs.cuda_stream)
        assert rc == 0, rc

    us = kernel_us({"this_tree": lambda: nat.filter_eval_expr_dev([leaf], [0], N, *ptrs), "parent": via_parent}, inner=20)
    nat.filter_eval_expr_dev([leaf], [0], N, *ptrs)
    mine = (und.clone(), counts.clone())
    via_parent()
    cs.synchronize()
    result["b_in_list_vs_parent"] = {
        "parent_hr_version": parent.hr_version(), "this_hr_version": nat.load_library().hr_version(), "key_column_bytes": 16 * N,
        "this_tree_us": spread(us["this_tree"]), "parent_us": spread(us["parent"]),
        "this_over_parent": round(float(np.median(us["this_tree"]) / np.median(us["parent"])), 4),
        "outputs_equal": bool(torch.equal(mine[0], und) and torch.equal(mine[1], counts)), "rows_undecided": int(counts.cpu()[1])}
    del keys

# ---- (c) end to end ---------------------------------------------------------------------------------------------------------------------
E, D = args.e2e_rows, 8
rng = np.random.default_rng(args.seed)
vocab = np.asarray([f"w{i}" for i in range(VOCAB)])
t0 = time.perf_counter()
mgr = MilvusIndexManager(semantic_dim=D, sparse_dim=0, dtype="float16", enable_domain=False)
mgr.collections.pop("sparse_index", None)
step = 1 << 18
for lo in range(0, E, step):
    hi = min(E, lo + step)
    k = rng.integers(30, 51, hi - lo)
    flat = vocab[rng.integers(0, VOCAB, int(k.sum()))]
    cuts = np.cumsum(k)[:-1]
    contents = [", ".join(part) + "." for part in np.split(flat, cuts)]          # punctuation glued to the words
    mgr.add_rows(rng.standard_normal((hi - lo, D)).astype(np.float16), None, contents=contents)
mgr.finalize()
build_s = time.perf_counter() - t0
t0 = time.perf_counter()
ws = mgr._cols.word_sets()                    # what a server does before serving: the host tokenises every row once
word_sets_s = time.perf_counter() - t0
q = rng.standard_normal(D).astype(np.float32)
expr = 'TEXT_MATCH(content, "w17 w4242 w31337", minimum_should_match=1)'
asyncio.run(mgr.search(q, "semantic_index", 10))         # the unfiltered path is warm
t0 = time.perf_counter()
hits = asyncio.run(mgr.search(q, "semantic_index", 10, expr))
first_ms = (time.perf_counter() - t0) * 1e3
cached = []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    asyncio.run(mgr.search(q, "semantic_index", 10, expr))
    cached.append((time.perf_counter() - t0) * 1e3)
dev = mgr._filters_on_device()
other = 'TEXT_MATCH(content, "w99 w12345")'
new_expr = []
for i in range(args.repeats):                  # a NEW expression once the mirror is in HBM: lookup + kernel + count read-back
    t0 = time.perf_counter()
    dev.evaluate(other.replace("w99", f"w{100 + i}"), E)
    new_expr.append((time.perf_counter() - t0) * 1e3)
result["c_end_to_end"] = {
    "rows": E, "corpus_build_s": round(build_s, 1), "word_sets_host_build_s": round(word_sets_s, 2),
    "word_sets_host_build_s_per_million_rows": round(word_sets_s / (E / 1e6), 2), "distinct_words": len(ws.ids),
    "host_word_set_bytes": ws.nbytes, "hbm_mirror_bytes": dev.word_mirror_bytes, "first_search_ms": round(first_ms, 2),
    "cached_search_ms": spread(cached), "new_expression_evaluate_ms": spread(new_expr), "hits": len(hits),
    "filter_stats": dict(dev.stats)}
asyncio.run(mgr.close())
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
