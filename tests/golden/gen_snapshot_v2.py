"""Records tests/golden/snapshot_v2.json: the length, SHA-256 and header bytes of the snapshot hr_save writes for three
small shards built from fixed seeds.  The fixture pins the version-2 file format byte for byte; it was recorded with the
library of the commit before the shard store's buffers became owning (same hr_version, 10501), and a library that writes
anything else has changed the format.

Needs a GPU and a built library (HBMRAG_LIB selects another build):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_snapshot_v2.py > tests/golden/snapshot_v2.json

tests/test_gpu_store_lifecycle.py runs this file for CASES, build_case and describe, so the shards of the test are the
shards of the fixture.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HEADER_BYTES = 96
# name -> seed, dense (dim, dtype, metric, rows) or None, sparse (V, rows, entries per row, the empty row) or None
CASES = {
    "A_f16_cosine_hybrid": dict(seed=101, dense=(32, "f16", "cosine", 70), sparse=(50, 70, 3, 41)),
    "B_f32_l2_one_row": dict(seed=102, dense=(40, "f32", "l2", 1), sparse=None),
    "C_sparse_only": dict(seed=103, dense=None, sparse=(50, 70, 3, None)),
}


def build_case(nat, name):
    """The finalized shard of CASES[name]."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    dim, dtype, metric = 0, nat.HR_F16, nat.HR_METRIC_COSINE
    if c["dense"]:
        dim, dt, me, n = c["dense"]
        dtype = {"f16": nat.HR_F16, "f32": nat.HR_F32}[dt]
        metric = {"cosine": nat.HR_METRIC_COSINE, "l2": nat.HR_METRIC_L2}[me]
        X = rng.standard_normal((n, dim)).astype(np.float16 if dt == "f16" else np.float32)
    h = nat.ShardHandle(dim, dtype, metric, c["sparse"][0] if c["sparse"] else 0)
    if c["dense"]:
        h.add_dense(X)
    if c["sparse"]:
        V, n, nnz, empty = c["sparse"]
        counts = np.full(n, nnz, dtype=np.int64)
        if empty is not None:
            counts[empty] = 0
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        idx = np.concatenate([np.sort(rng.choice(V, int(m), replace=False)) for m in counts]).astype(np.int32)
        val = (np.abs(rng.standard_normal(idx.size)) + 0.01).astype(np.float32)
        h.add_sparse(ptr, idx, val)
    h.finalize()
    return h


def describe(blob):
    return dict(length=len(blob), sha256=hashlib.sha256(blob).hexdigest(), header_hex=blob[:HEADER_BYTES].hex())


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "advanced-rag-milvus_amd"))
    from advanced_rag import _native as nat

    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CASES.items():
            h = build_case(nat, name)
            path = os.path.join(tmp, name + ".hbmrag")
            h.save(path)
            h.close()
            with open(path, "rb") as f:
                out.append(dict(case=name, seed=c["seed"], **describe(f.read())))
    json.dump(dict(hr_version=nat.load_library().hr_version(), snapshots=out), sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
