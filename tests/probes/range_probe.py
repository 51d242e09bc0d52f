"""Ad-hoc measurement (not a test): what a range search (hr_search_dense_range_dev) costs beside the plain one.

One shard (default 10,000,000 x 768 fp16, COSINE), B = 128 queries, top_k = 20 (half of the 40 rows a query has in range), the device forms on one stream.

1. Plain steps (hr_search_dense_dev) against ranged steps with wide-open bounds (hr_search_dense_range_dev, radius = -2,
   range_filter = +2: every row in range, finite ceilings, the ranged scan instantiation), in alternating windows of one
   call: per window the dense scan time by the library's own device events (hr_set_profiling) and the wall time per step;
   the spread between the windows of one form is reported beside the difference between the forms — a difference counts
   only if it exceeds that spread.
2. An annulus workload: `--planted` rows per query planted above range_filter (cosine 0.95 .. 0.999) and 40 inside the
   range (0.6 .. 0.8), bounds 0.5 / 0.9: the share of device lists proven and the time per step with the clamp on and
   off (HR_DEBUG_NO_RANGE_CLAMP), plus the time of the host form with the clamp on.

  python tests/probes/range_probe.py --out profiles/range_search.json [--commit ID] [--ab-parent MS --ab-new MS --ab-spread MS]

The --ab-* figures are the `ms_per_step` of the default bench.py line from tests/probes/ab_many.sh (parent library
against this one on one box) and the parent's own window-to-window spread; they are copied into the JSON as given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--top-k", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--planted", type=int, default=1500)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--ab-parent", type=float, default=None)
ap.add_argument("--ab-new", type=float, default=None)
ap.add_argument("--ab-spread", type=float, default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))

import torch   # noqa: E402
from advanced_rag import _native as nat   # noqa: E402

N, D, B, K = args.rows, args.dim, args.batch, args.top_k
rng = np.random.default_rng(args.seed)
dev = torch.device("cuda", 0)
Qh, _ = np.linalg.qr(rng.standard_normal((D, B)))
Qh = np.ascontiguousarray(Qh.T, dtype=np.float32)                # orthonormal queries, one per ROW (C order: the device reads it raw)

# the corpus: random unit rows; per query `planted` rows above the range and 40 inside it, at random row numbers
h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, 0)
per_q = args.planted + 40
special = rng.permutation(N)[:B * per_q]
owner = np.full(N, -1, np.int32)
owner[special] = np.repeat(np.arange(B, dtype=np.int32), per_q)
cosine = np.zeros(N, np.float32)
cosine[special] = np.tile(np.concatenate([np.linspace(0.6, 0.8, 40), rng.uniform(0.95, 0.999, args.planted)]), B)
t0 = time.perf_counter()
step = 1 << 17
for lo in range(0, N, step):
    hi = min(N, lo + step)
    X = rng.standard_normal((hi - lo, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    own = np.flatnonzero(owner[lo:hi] >= 0)
    if own.size:
        q = Qh[owner[lo:hi][own]]
        noise = X[own] - (X[own] * q).sum(axis=1, keepdims=True) * q
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        c = cosine[lo:hi][own][:, None]
        X[own] = c * q + np.sqrt(1.0 - c * c) * noise
    h.add_dense(X)
h.finalize()
ingest_s = time.perf_counter() - t0

d_q = torch.from_numpy(Qh).to(dev)
ids = torch.empty((B, K), dtype=torch.int64, device=dev)
sc = torch.empty((B, K), dtype=torch.float32, device=dev)
fl = torch.empty((B,), dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(dev)
SCAN_PHASE = nat.PHASE_NAMES[1]                                  # PH_SCAN: the dense scan launches


def bounds(radius, range_filter):
    return (torch.full((B,), radius, dtype=torch.float64, device=dev), torch.full((B,), range_filter, dtype=torch.float64, device=dev))


def run(form, steps):
    """-> (wall ms per step, dense scan ms per step from the library's device events, flags of the last step)."""
    h.set_profiling(1)
    h.kernel_ms()                                                # drop what was recorded before
    stream.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        if form is None:
            h.search_dense_dev(d_q.data_ptr(), B, K, ids.data_ptr(), sc.data_ptr(), fl.data_ptr(), 0, stream.cuda_stream)
        else:
            h.search_dense_range_dev(d_q.data_ptr(), B, K, form[0].data_ptr(), form[1].data_ptr(), ids.data_ptr(),
                                     sc.data_ptr(), fl.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    wall = (time.perf_counter() - t) * 1e3 / steps
    mean_ms, launches = h.kernel_ms()[SCAN_PHASE]
    h.set_profiling(0)
    return wall, mean_ms * launches / steps, fl.cpu().numpy().copy()


def spread(v):
    return float(max(v) - min(v)) if v else 0.0


out = {"commit": args.commit, "rows": N, "dim": D, "batch": B, "top_k": K, "ingest_s": round(ingest_s, 1)}
wide = bounds(-2.0, 2.0)
run(None, 5), run(wide, 5)                                        # warm-up
plain, ranged = [], []
for _ in range(args.windows):
    plain.append(run(None, args.steps)[:2])
    ranged.append(run(wide, args.steps)[:2])
out["wide_open"] = {
    "plain_scan_ms": [round(s, 4) for _, s in plain], "ranged_scan_ms": [round(s, 4) for _, s in ranged],
    "plain_step_ms": [round(w, 4) for w, _ in plain], "ranged_step_ms": [round(w, 4) for w, _ in ranged],
    "plain_scan_spread_ms": round(spread([s for _, s in plain]), 4),
    "ranged_minus_plain_scan_ms": round(float(np.median([s for _, s in ranged]) - np.median([s for _, s in plain])), 4)}

annulus = bounds(0.5, 0.9)
res = {}
for name, off in (("clamp_on", 0), ("clamp_off", 1)):
    nat.debug_option(nat.HR_DEBUG_NO_RANGE_CLAMP, off)
    run(annulus, 3)
    w = [run(annulus, args.steps) for _ in range(args.windows)]
    dev_ids = ids.cpu().numpy().copy()
    res[name] = {"step_ms": [round(x[0], 4) for x in w], "proven_share": float(np.mean(w[-1][2] == 1)),
                 "hits_per_device_list": float((dev_ids >= 0).sum(axis=1).mean())}
    if not off:      # (without the clamp the host form escalates every query to a refine of the whole shard: not timed)
        t = time.perf_counter()
        host_ids, _ = h.search_dense_range(Qh, K, 0.5, 0.9)
        res[name]["host_form_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        res[name]["hits_per_host_list"] = float((host_ids >= 0).sum(axis=1).mean())
        res[name]["device_lists_equal_host"] = bool(np.array_equal(dev_ids, host_ids))
nat.debug_option(nat.HR_DEBUG_NO_RANGE_CLAMP, 0)
out["annulus"] = dict(res, planted_above_per_query=args.planted, in_range_per_query=40)
if args.ab_parent is not None:
    out["bench_ab"] = {"parent_ms_per_step": args.ab_parent, "new_ms_per_step": args.ab_new,
                       "parent_window_spread_ms": args.ab_spread}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
h.close()
