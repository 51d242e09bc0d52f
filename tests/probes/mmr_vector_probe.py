"""Ad-hoc measurement (not a test): what vector MMR costs (csrc/mmr.h mmr_select_vec_kernel, advanced_rag/mmr.py).

One MI355X.

  (a) hr_mmr_select_vec_dev alone (its gather included) at B = 128, k_out = 20, k_in = 80 / 256, dim = 384 / 768, fp16 rows,
      alternating with hr_mmr_select_dev (token Jaccard, 40-token rows) on lists of the same shape.  One call between two
      device events.
  (b) end to end on a one-shard manager (--rows x --dim, 40-word contents), --in-flight requests in flight:
      search(ranker=MMRRanker(candidates=80)) against the plain search(top_k=80); retrieve() of the troubleshooting profile
      with mmr_similarity="embedding" against "tokens" on a manager with mmr_on_device off and on; and the token-set build
      (host tokenisation of every row, once) that the embedding form never makes.

The contenders alternate, window after window, in one process; a warm-up, then --repeats windows each; the median and the
spread (max - min) are reported.

  python tests/probes/mmr_vector_probe.py --out profiles/mmr_vector.json [--commit ID]
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
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=384)
ap.add_argument("--in-flight", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--skip-end-to-end", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402
from advanced_rag.constants import RetrievalConstants   # noqa: E402
from advanced_rag.mmr import MMRRanker   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("mmr_vector_probe needs a GPU: a CPU run says nothing about these numbers")

device = torch.device("cuda", 0)
cs = torch.cuda.current_stream(device)
st = cs.cuda_stream
B, K_OUT = args.batch, 20
rng = np.random.default_rng(args.seed)
result = {"command": " ".join(sys.argv), "commit": args.commit, "hr_version": nat.load_library().hr_version(), "B": B,
          "k_out": K_OUT, "repeats": args.repeats}


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "min": round(float(min(xs)), 3)}


def write_out():
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


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
result["kernel_unit"] = "microseconds per call (gather + selection), between device events"
n_shard, n_tok = 100_000, 40
tok = np.sort(rng.integers(0, 5000, (n_shard, n_tok)), axis=1).astype(np.int32)
tok += np.arange(n_tok, dtype=np.int32)[None, :]          # strictly ascending within a row
d_tok = torch.from_numpy(tok.reshape(-1)).to(device)
d_indptr = torch.from_numpy(np.arange(n_shard + 1, dtype=np.int64) * n_tok).to(device)
for dim in (384, 768):
    h = nat.ShardHandle(dim, nat.HR_F16, nat.HR_METRIC_COSINE)
    h.add_dense(rng.standard_normal((n_shard, dim)).astype(np.float16))
    h.finalize()
    for k in (80, 256):
        ids = torch.from_numpy(np.stack([rng.choice(n_shard, k, replace=False) for _ in range(B)]).astype(np.int64)).to(device)
        sc32 = torch.from_numpy(-np.sort(-rng.uniform(0.2, 0.9, (B, k)), axis=1).astype(np.float32)).to(device)
        sc64 = sc32.double()
        n = torch.full((B,), k, dtype=torch.int32, device=device)
        lam = torch.full((B,), 0.5, dtype=torch.float64, device=device)
        pos = torch.empty((B, K_OUT), dtype=torch.int32, device=device)
        val = torch.empty((B, K_OUT), dtype=torch.float64, device=device)
        on = torch.empty((B,), dtype=torch.int32, device=device)
        scratch = torch.empty(h.mmr_vec_scratch_bytes(B, k), dtype=torch.uint8, device=device)
        fns = {
            "vector": lambda: h.mmr_select_vec_dev(ids.data_ptr(), sc32.data_ptr(), False, nat.HR_NORM_NONE, n.data_ptr(), B, k,
                                                   lam.data_ptr(), K_OUT, scratch.data_ptr(), pos.data_ptr(), val.data_ptr(),
                                                   on.data_ptr(), st),
            "jaccard_40_tokens": lambda: nat.mmr_select_dev(ids.data_ptr(), sc64.data_ptr(), n.data_ptr(), B, k, d_indptr.data_ptr(),
                                                            d_tok.data_ptr(), n_shard, 0, lam.data_ptr(), K_OUT, pos.data_ptr(),
                                                            on.data_ptr(), st),
        }
        result[f"kernel_dim{dim}_k{k}"] = {**launch_us(fns), "scratch_bytes": int(scratch.numel())}
        cs.synchronize()
    h.close()
write_out()

# ---- (b) end to end --------------------------------------------------------------------------------------------------------
if not args.skip_end_to_end:
    N, D, V, W, IN_FLIGHT = args.rows, args.dim, 2048, 80, args.in_flight
    X = rng.standard_normal((N, D), dtype=np.float32).astype(np.float16)
    nnz = 8
    idx = np.sort(rng.integers(0, V, (N, nnz)), axis=1).astype(np.int32)
    idx += np.arange(nnz, dtype=np.int32)[None, :]
    sval = (np.abs(rng.standard_normal((N, nnz))) + 0.1).astype(np.float32)
    csr = (np.arange(N + 1, dtype=np.int64) * nnz, idx.reshape(-1), sval.reshape(-1))
    words = rng.integers(0, 5000, (N, 40))
    contents = [" ".join(f"w{t}" for t in row) for row in words]
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

    RetrievalConstants.TIMEOUT_SECONDS = 120.0
    mgrs = {}
    for on_device in (False, True):
        m = MilvusIndexManager(semantic_dim=D, sparse_dim=V + nnz, enable_domain=False, mmr_on_device=on_device)
        m.add_rows(X, csr, contents=contents)
        m.finalize()
        m.embedding_generator = Gen()
        mgrs[on_device] = m
    mgr = mgrs[False]
    ranker = MMRRanker(0.5, candidates=W)
    retr = {(sim, dev): HybridRetriever(mgrs[dev], RetrievalConfig(top_k=20, mmr_similarity=sim))
            for sim in ("tokens", "embedding") for dev in (False, True)}

    async def burst(make):
        return await asyncio.gather(*(make(i) for i in range(IN_FLIGHT)))

    contenders = {
        "search_plain_topk_W": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", W))),
        "search_mmr_ranker": lambda: asyncio.run(burst(lambda i: mgr.search(Q[i], "semantic_index", 20, ranker=ranker))),
    }
    for (sim, dev), r in retr.items():
        contenders[f"retrieve_troubleshooting_{sim}_mmr_on_device_{'on' if dev else 'off'}"] = \
            lambda r=r: asyncio.run(burst(lambda i: r.retrieve(f"plain statement q{i}", profile_hint="troubleshooting")))
    contenders["search_mmr_ranker"]()
    for name in ("retrieve_troubleshooting_embedding_mmr_on_device_off", "retrieve_troubleshooting_embedding_mmr_on_device_on"):
        contenders[name]()
    built = {str(dev): mgrs[dev]._cols._token_sets is not None for dev in (False, True)}      # still unbuilt: embedding only so far
    t0 = time.perf_counter()
    mgr._cols.token_sets()
    build_s = time.perf_counter() - t0
    for fn in contenders.values():
        fn()
    times = {k: [] for k in contenders}
    for _ in range(args.rounds):
        for name, fn in contenders.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result["end_to_end"] = {"unit": f"milliseconds per burst of {IN_FLIGHT} concurrent requests, wall clock", "rows": N, "dim": D,
                            "top_k": 20, "W": W, "rounds": args.rounds, **{k: spread(v) for k, v in times.items()}}
    result["token_set_build"] = {"host_seconds": round(build_s, 3), "rows": N, "words_per_row": 40,
                                 "built_before_the_tokens_form_ran": built}
    result["front_stats"] = {str(dev): {k: v for k, v in mgrs[dev]._front.stats.items() if k.endswith("launches") or k == "requests"}
                             for dev in (False, True)}
    for m in mgrs.values():
        asyncio.run(m.close())

print(json.dumps(result, indent=1))
write_out()
