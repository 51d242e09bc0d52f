"""Ad-hoc measurement (not a test): what the weighted score fusion costs beside reciprocal-rank fusion (csrc/fuse.h).

One MI355X.  B = 128 queries, two lists per query whose ids overlap by about a half.

  (a) hr_fuse_scores_dev with norm codes 0 / 1 / 3 on both lists against hr_fuse_rrf_dev, at k = 40 and at k = 256;
  (b) hr_post_lists_dev (one list per modality, no merge, no rerank) with fusion = 0 and with fusion = 1 (codes 0 and 1).

Every timing is one launch between two device events; the contenders alternate, window after window, in one process; a
warm-up, then --repeats windows each; the median and the spread (max - min) are reported in microseconds.

  python tests/probes/score_fusion_probe.py --out profiles/score_fusion.json [--commit ID]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=101)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("score_fusion_probe needs a GPU: a CPU run says nothing about these numbers")

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


def lists(k, rng):
    ids = [np.stack([rng.permutation(3 * k // 2 + 1)[:k] for _ in range(B)]).astype(np.int64) for _ in range(2)]
    sc = [-np.sort(-rng.uniform(-1, 1, (B, k)), axis=1).astype(np.float32),
          -np.sort(-rng.uniform(0, 30, (B, k)), axis=1).astype(np.float32)]
    return [torch.from_numpy(a).to(device) for a in ids], [torch.from_numpy(a).to(device) for a in sc]


rng = np.random.default_rng(args.seed)
st = cs.cuda_stream
for k in (40, 256):
    ids, sc = lists(k, rng)
    top_k = 2 * k
    oi = torch.empty((B, top_k), dtype=torch.int64, device=device)
    os_ = torch.empty((B, top_k), dtype=torch.float64, device=device)
    om = torch.empty((B, top_k), dtype=torch.int32, device=device)
    on = torch.empty((B,), dtype=torch.int32, device=device)
    outs = (oi.data_ptr(), os_.data_ptr(), om.data_ptr(), on.data_ptr(), st)

    def rrf():
        nat.fuse_rrf_dev(ids[0].data_ptr(), k, ids[1].data_ptr(), k, 0, 0, B, 0.7, 0.3, 0.2, 60, top_k, *outs)

    def scores(code):
        return lambda: nat.fuse_scores_dev(ids[0].data_ptr(), sc[0].data_ptr(), k, code, ids[1].data_ptr(), sc[1].data_ptr(), k,
                                           code, 0, 0, 0, 0, B, 0.7, 0.3, 0.2, 0, top_k, *outs)

    result[f"fuse_k{k}"] = launch_us({"rrf": rrf, "scores_code0": scores(0), "scores_code1": scores(1), "scores_code3": scores(3)})

    if k == 40:
        def post(fusion):
            a = nat.PostArgs()
            for m in range(2):
                a.ids[m], a.scores[m], a.k_in[m], a.k_fuse[m], a.norm[m] = ids[m].data_ptr(), sc[m].data_ptr(), k, k, m
            a.n_lists, a.rrf_k, a.top_k, a.fusion = 1, 60, 20, fusion
            a.w[0], a.w[1], a.w[2] = 0.7, 0.3, 0.2
            a.fused_ids, a.fused_scores, a.fused_methods, a.fused_n = outs[:4]
            return lambda: nat.post_lists_dev(a, B, st)

        result["post_lists_k40_top20"] = launch_us({"fusion0_rrf": post(0), "fusion1_weighted": post(1)})

print(json.dumps(result, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
