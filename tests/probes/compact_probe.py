"""Ad-hoc measurement (not a test): what hr_compact costs and what it buys.

One hybrid shard (default 10,000,000 x 768 fp16 + 20 sparse entries per row, V = 10,000; rows drawn on the device from
seeds), 30 % of the rows tombstoned at random.  In ONE process:

  cost   hr_compact wall time, compact_tiles_kernel between HIP events (hr_last_compact_ms), the bytes that kernel must
         move (old tiles read + new tiles written) and the rate that makes, as a fraction of the float4 copy rate of the
         device (6.29 TB/s); beside it the only alternative without hr_compact: a NEW handle filled with the survivors —
         hr_add_dense_raw_dev from rows already in HBM + hr_add_sparse + hr_finalize (producing the survivors' rows is
         not counted: a lower bound of that way);
  gain   dense / sparse scan time of a 128-query hybrid step (hr_set_profiling(1)) on the tombstoned shard with its row
         mask, and on the compacted shard; hr_device_bytes before and after.

The compacted handle and the rebuilt one must answer alike; the probe reports what it found (`checked`).

  python tests/probes/compact_probe.py --out profiles/compact_probe.json [--rows N] [--commit ID]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "advanced-rag-milvus_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--drop", type=float, default=0.3)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--out", default=None)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()

import torch                                              # noqa: E402
from advanced_rag import _native as nat                   # noqa: E402
from advanced_rag.engine import pack_sparse_queries       # noqa: E402

COPY_RATE = 6.29e12      # float4 copy, bytes/s moved (read + written)
N, D, V, NNZ, B, K, CHUNK = args.rows, args.dim, 10000, 20, 128, 40, 500_000
dev = torch.device("cuda", 0)
rng = np.random.default_rng(args.seed)
keep = rng.random(N) >= args.drop
d_keep_bool = torch.from_numpy(keep).to(dev)


def chunk_rows(c):
    """Rows [c * CHUNK, ...) of the corpus, fp16 in HBM, from the chunk's own seed."""
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed * 1000 + c)
    m = min(CHUNK, N - c * CHUNK)
    return torch.randn((m, D), generator=g, device=dev, dtype=torch.float32).to(torch.float16)


def fill(only_kept):
    st = torch.cuda.current_stream(dev)
    for c in range((N + CHUNK - 1) // CHUNK):
        rows = chunk_rows(c)
        if only_kept:
            rows = rows[d_keep_bool[c * CHUNK: c * CHUNK + rows.shape[0]]].contiguous()
        # torch's default stream has the handle 0, which the library reads as "use the ingest stream": the rows must be
        # complete before the append is enqueued there
        torch.cuda.synchronize(dev)
        yield rows, st


t0 = time.perf_counter()
idx = (np.arange(NNZ, dtype=np.int32)[None, :] * (V // NNZ) + rng.integers(0, V // NNZ, size=(N, NNZ), dtype=np.int32)).reshape(-1)
val = (np.abs(rng.standard_normal(N * NNZ, dtype=np.float32)) + 0.01).astype(np.float32)
ptr = np.arange(N + 1, dtype=np.int64) * NNZ
h = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, V)
h.reserve(N)
for rows, st in fill(False):
    h.add_dense_dev(rows.data_ptr(), rows.shape[0], st.cuda_stream)
h.add_sparse(ptr, idx, val)
h.finalize()
build_s = time.perf_counter() - t0
print(f"shard built in {build_s:.1f} s", file=sys.stderr, flush=True)

Q = rng.standard_normal((B, D)).astype(np.float32)
SQ = [((np.arange(40, dtype=np.int32) * (V // 40) + rng.integers(0, V // 40, size=40, dtype=np.int32)),
       (np.abs(rng.standard_normal(40)) + 0.01).astype(np.float32)) for _ in range(B)]
p, qi, qv, mx = pack_sparse_queries(SQ, 0.0)
dq, dp, di, dv = (torch.from_numpy(a).to(dev) for a in (Q, p, qi, qv))
ids = torch.empty((2, B, K), dtype=torch.int64, device=dev)
sc = torch.empty((2, B, K), dtype=torch.float32, device=dev)
fl = torch.zeros((2, B), dtype=torch.int32, device=dev)
mask_bytes = np.zeros(8 * ((N + 63) // 64), np.uint8)
packed = np.packbits(keep, bitorder="little")
mask_bytes[: packed.size] = packed
d_mask = torch.from_numpy(mask_bytes).to(dev)


def step_ms(handle, d_rowmask):
    """Mean dense / sparse scan ms of a 128-query hybrid step (one warm-up step, then --steps of them)."""
    st = torch.cuda.current_stream(dev)
    handle.set_profiling(1)
    for i in range(args.steps + 1):
        handle.search_hybrid_dev(dq.data_ptr(), dp.data_ptr(), di.data_ptr(), dv.data_ptr(), B, len(qi), mx, K, ids.data_ptr(),
                                 sc.data_ptr(), fl.data_ptr(), d_rowmask, st.cuda_stream)
        st.synchronize()
        if i == 0:
            handle.kernel_ms()
    ms = handle.kernel_ms()
    handle.set_profiling(0)
    return {"dense_scan_ms": ms["dense_scan"][0], "sparse_scan_ms": ms["sparse_scan"][0], "launches": ms["dense_scan"][1]}


out = {"commit": args.commit, "rows": N, "dim": D, "dtype": "float16", "sparse_dim": V, "nnz_per_row": NNZ,
       "dropped_fraction": float(1.0 - keep.mean()), "survivors": int(keep.sum()), "build_s": build_s}
out["before"] = dict(step_ms(h, d_mask.data_ptr()), device_bytes=h.device_bytes, scan_bytes=h.dense_scan_bytes)
lists_before = (ids.cpu().numpy().copy(), fl.cpu().numpy().copy())

# ---- the alternative a user has without hr_compact: a new handle from the survivors
torch.cuda.synchronize(dev)
t0 = time.perf_counter()
rp = np.concatenate([[0], np.cumsum(np.full(N, NNZ, np.int64)[keep])]).astype(np.int64)
e_keep = np.repeat(keep, NNZ)
s_idx, s_val = idx[e_keep], val[e_keep]
csr_s = time.perf_counter() - t0
alt = nat.ShardHandle(D, nat.HR_F16, nat.HR_METRIC_COSINE, V)
t_dense = 0.0
t1 = time.perf_counter()
alt.reserve(int(keep.sum()))
t_dense += time.perf_counter() - t1
for rows, st in fill(True):
    t1 = time.perf_counter()
    alt.add_dense_dev(rows.data_ptr(), rows.shape[0], st.cuda_stream)      # synchronises before it returns
    t_dense += time.perf_counter() - t1
t1 = time.perf_counter()
alt.add_sparse(rp, s_idx, s_val)
t_sparse = time.perf_counter() - t1
t1 = time.perf_counter()
alt.finalize()
t_fin = time.perf_counter() - t1
out["rebuild"] = {"add_dense_raw_dev_ms": t_dense * 1e3, "add_sparse_ms": t_sparse * 1e3, "finalize_ms": t_fin * 1e3,
                  "total_ms": (t_dense + t_sparse + t_fin) * 1e3, "host_csr_gather_ms_not_counted": csr_s * 1e3}

print("rebuilt from the survivors", out["rebuild"], file=sys.stderr, flush=True)

# ---- hr_compact
h.set_profiling(1)
torch.cuda.synchronize(dev)
t0 = time.perf_counter()
kept = h.compact(d_keep=d_mask.data_ptr())
wall = (time.perf_counter() - t0) * 1e3
cms = h.compact_ms()
h.set_profiling(0)
assert kept == (int(keep.sum()), int(keep.sum()))
row_bytes = h.dense_scan_bytes // kept[0] - 4             # tile bytes per row (padded dimension); the scan also reads 4 B of scale
moved = row_bytes * (N + kept[0])        # every old tile read (16-byte pieces share sectors with dropped neighbours) + new tiles written
must = row_bytes * 2 * kept[0]           # the survivors alone, read + written
out["compact"] = {"wall_ms": wall, "library_call_ms": cms["call"], "tile_gather_ms": cms["tile_gather"],
                  "posting_rebuild_ms": cms["posting_rebuild"], "tile_bytes_old_read_plus_new_written": moved,
                  "tile_bytes_survivors_read_plus_written": must,
                  "tile_gather_TBps_old_plus_new": moved / (cms["tile_gather"] * 1e-3) / 1e12,
                  "tile_gather_TBps_survivors_only": must / (cms["tile_gather"] * 1e-3) / 1e12,
                  "fraction_of_copy_rate_old_plus_new": moved / (cms["tile_gather"] * 1e-3) / COPY_RATE,
                  "fraction_of_copy_rate_survivors_only": must / (cms["tile_gather"] * 1e-3) / COPY_RATE}
out["after"] = dict(step_ms(h, 0), device_bytes=h.device_bytes, scan_bytes=h.dense_scan_bytes)
lists_after = (ids.cpu().numpy().copy(), fl.cpu().numpy().copy())
out["rebuilt_handle"] = dict(step_ms(alt, 0), device_bytes=alt.device_bytes)
lists_alt = (ids.cpu().numpy().copy(), fl.cpu().numpy().copy())

# the compacted and the rebuilt handle must answer alike: the host forms (exact lists) on a few queries, and the device
# form list by list; against the tombstoned shard only the row numbers may have moved
hd, hs = h.search_dense(Q[:4], K), h.search_sparse(SQ[:4], K, 0.0)
ad, as_ = alt.search_dense(Q[:4], K), alt.search_sparse(SQ[:4], K, 0.0)
host_equal = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(hd + hs, ad + as_))
flags_equal = bool(np.array_equal(lists_after[1], lists_alt[1]))
differing = [(m, int(b), int(lists_after[1][m, b]), int(lists_alt[1][m, b])) for m in range(2) for b in range(B)
             if not np.array_equal(lists_after[0][m, b], lists_alt[0][m, b])]
new_of = np.cumsum(keep) - 1
both = (lists_before[1] == 1) & (lists_after[1] == 1)
moved_only = all(np.array_equal(np.where(lists_before[0][m, b] >= 0, new_of[np.maximum(lists_before[0][m, b], 0)], -1),
                                lists_after[0][m, b]) for m in range(2) for b in np.nonzero(both[m])[0])
out["checked"] = {"host_forms_equal_rebuilt": host_equal, "device_flags_equal_rebuilt": flags_equal,
                  "device_lists_differing_from_rebuilt (modality, query, flag, flag)": differing[:16],
                  "n_device_lists_differing": len(differing), "proven_lists_equal_masked_shard_renumbered": bool(moved_only),
                  "proven_lists_compared": int(both.sum()), "proven_after": lists_after[1].sum(axis=1).tolist()}
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
